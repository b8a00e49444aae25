"""Cost of checkpoint evaluation on one MI355X: the SSIM / squared-error kernel (acg_frame_metrics) and Trainer.rollout_metrics
against Trainer.test_sequence.

  python tools/bench_eval.py [--launches 200] [--batch 32] [--reps 10]

Kernel: fp32 frames, 224 frames (config 2's eval: B = 32 x 7 steps) of 64x64x3 and of 128x128x3.  Timed two ways over
``--launches`` back-to-back launches between two events: captured into one HIP graph and replayed (the device time of the
launches, host overhead excluded), and as plain eager calls from Python (what a caller pays, ctypes included).
Rollout: the DNA generator at ``--batch`` sequences of 8 frames (7 steps), f32; the two calls alternate, frames/s of each.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from action_conditioned_gans_amd import _lib  # noqa: E402
from action_conditioned_gans_amd import graph as G  # noqa: E402
from action_conditioned_gans_amd import metrics as M  # noqa: E402
from action_conditioned_gans_amd import train as T  # noqa: E402


def kernel_times(n, s, launches):
    lib = _lib.get()
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.uniform(-1, 1, (n, s, s, 3)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.uniform(-1, 1, (n, s, s, 3)).astype(np.float32)).cuda()
    ssim = torch.empty(n, device='cuda')
    sq = torch.empty(n, device='cuda')
    wsb = lib.frame_metrics_workspace_bytes(n, s, s)
    ws = torch.empty(wsb, dtype=torch.uint8, device='cuda')
    P = ctypes.c_void_p
    args = [P(x.data_ptr()), P(y.data_ptr()), P(ssim.data_ptr()), P(sq.data_ptr()), n, s, s, 3, 3, _lib.ACG_F32, 2.0, M.K1, M.K2,
            P(ws.data_ptr()), wsb]

    def launch():
        lib.frame_metrics(*args, P(torch.cuda.current_stream().cuda_stream))

    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        launch()
    e1.record()
    torch.cuda.synchronize()
    eager_us = e0.elapsed_time(e1) * 1e3 / launches
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for _ in range(launches):
                launch()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(5):
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / launches)
    return best, eager_us


def rollout_rates(batch, reps):
    G.reset_default_graph()
    sess = G.Session(device='cuda:0')
    tr = T.Trainer(sess, False, 'bce', 'adam', True, batch_size=batch, img_size=64)
    sess.run(G.global_variables_initializer())
    rng = np.random.default_rng(1)
    frames = rng.uniform(-1, 1, (batch, 8, 64, 64, 3)).astype(np.float32)
    acts = rng.standard_normal((batch, 8, 10)).astype(np.float32)
    for _ in range(3):
        tr.test_sequence(frames, frames, acts)
        tr.rollout_metrics(frames, acts)
    t_seq, t_met = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.test_sequence(frames, frames, acts)
        t1 = time.perf_counter()
        tr.rollout_metrics(frames, acts)            # returns host arrays: synchronised
        t2 = time.perf_counter()
        t_seq.append(t1 - t0)
        t_met.append(t2 - t1)
    sess.close()
    n = batch * 7
    return n / np.median(t_seq), n / np.median(t_met)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=10)
    a = ap.parse_args()
    print('device: %s' % torch.cuda.get_device_name(0))
    for s, target in ((64, 30.0), (128, 100.0)):
        graph_us, eager_us = kernel_times(224, s, a.launches)
        print('frame_metrics 224 x %dx%dx3 fp32: %.1f us/launch (HIP graph, %d launches; target <= %.0f us: %s), %.1f us eager from Python'
              % (s, s, graph_us, a.launches, target, 'met' if graph_us <= target else 'NOT met', eager_us))
    seq, met = rollout_rates(a.batch, a.reps)
    print('DNA generator, batch %d, 7 steps: test_sequence %.0f frames/s, rollout_metrics (+ model and identity SSIM) %.0f frames/s, '
          'ratio %.3f (target >= 0.95: %s)' % (a.batch, seq, met, met / seq, 'met' if met / seq >= 0.95 else 'NOT met'))


if __name__ == '__main__':
    main()
