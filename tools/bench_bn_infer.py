#!/usr/bin/env python
"""BatchNorm with stored statistics on one MI355X: the apply kernel per generator layer, and the rollout rate of the two modes.

  python tools/bench_bn_infer.py [--dtype bf16] [--batches 1,32] [--reps 12] [--stream-probe build/stream_probe] [--skip-rollout]

Per layer (the BatchNorm layers of the DNA generator at 64 x 64, batch 1 and 32): acg_bn_act_infer beside acg_bn_act_fwd on the
same tensors - each timed the way a program runs it, N launches captured into a HIP graph and replayed between two events, the
tensors where the previous launch left them (cache-warm, as the step finds them behind the producing conv) - and beside what
tools/micro/stream_probe.hip gives for a two-pass stream (one read, one write) of the same bytes, when its binary is there:
  hipcc -O3 --offload-arch=gfx950 -o build/stream_probe tools/micro/stream_probe.hip
(float32 tensors only; without the binary the column says so).  "of peak": algorithmic bytes (x in, y out) over the kernel time,
as a fraction of the 8 TB/s HBM peak - no threshold is set on it: tensors of a few KB to 16 MB are bound by launch and round-trip
latency, not by bytes.

Rollout: Trainer.rollout_metrics of the DNA generator at batch 32, 7 steps, bn='stored' against bn='batch', alternating in one
process; frames/s per repetition, medians, and the run-to-run spread (max - min) of the batch-statistics rate."""
import argparse
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from action_conditioned_gans_amd import _lib   # noqa: E402
from action_conditioned_gans_amd import graph as G   # noqa: E402
from action_conditioned_gans_amd import train as T   # noqa: E402

# (label, output height = width at 64 x 64, channels)
LAYERS = [('g/conv1', 32, 32), ('g/conv2', 16, 64), ('g/conv3', 8, 128), ('g/conv4', 4, 256), ('g/tconv1', 8, 128),
          ('g/tconv2', 16, 128), ('g/sconv3', 8, 32), ('g/sconv4', 4, 16), ('g/tconv3', 32, 128)]
HBM_PEAK = 8.0e12      # bytes / s (MI355X)


def timed(fn, n_graph=40, reps=5):
    """fn(stream pointer); -> microseconds per launch (best of ``reps`` replays of a graph of ``n_graph`` launches)."""
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for _ in range(n_graph):
            fn(sp)
    gr.replay()
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / n_graph)
    return best


def stream_probe(path, sizes):
    """{(rows, C): (stream us, stream-with-parameters us)} from the probe binary, or {} when it is not there."""
    if not path or not os.path.exists(path):
        return {}
    args = [path, 'ew'] + [str(v) for rc in sizes for v in rc]
    out = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, check=True).stdout.decode()
    got = {}
    for line in out.splitlines():
        f = line.split()
        if len(f) == 7 and f[0] == 'ew' and f[3] == 'stream_us':
            got[(int(f[1]), int(f[2]))] = (float(f[4]), float(f[6]))
    return got


def kernels(dtype, batches, probe_path):
    lib, dev = _lib.get(), torch.device('cuda:0')
    half = dtype == 'bf16'
    tdt, es, code = (torch.bfloat16, 2, _lib.ACG_BF16) if half else (torch.float32, 4, _lib.ACG_F32)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    sizes = [(b * hw * hw, c) for b in batches for _, hw, c in LAYERS]
    # the probe runs in a process of its own, before this one touches the device
    probe = {} if half else stream_probe(probe_path, sizes)
    torch.cuda.init()
    print('# %s; us per launch (HIP graph of 40 launches, best of 5 replays); bytes = x in + y out' % dtype)
    print('# %-10s %3s %7s %4s %9s | %9s %8s | %9s | %11s %11s' % ('layer', 'B', 'rows', 'C', 'KB', 'infer us', 'of peak', 'bn_fwd us',
                                                                   'stream us', '+params us'))
    tot = {}
    for b in batches:
        for label, hw, c in LAYERS:
            rows = b * hw * hw
            g = torch.Generator(device=dev).manual_seed(rows + c)
            x = (torch.randn(rows, c, device=dev, generator=g) * 1.5 + 0.3).to(tdt)
            beta = torch.randn(c, device=dev, generator=g) * 0.1
            mean, var = torch.randn(c, device=dev, generator=g), torch.rand(c, device=dev, generator=g) + 0.5
            y, y2 = torch.empty_like(x), torch.empty_like(x)
            smean, srstd = torch.empty(c, device=dev), torch.empty(c, device=dev)
            nb = lib.bn_workspace_bytes(rows, c, 1)
            ws = torch.zeros(max(nb, 16), dtype=torch.uint8, device=dev)
            t_inf = timed(lambda s: lib.bn_act_infer(p(x), p(beta), p(mean), p(var), p(y), rows, c, 0, 0, 1e-3, _lib.ACT_RELU, 0.0, code, s))
            t_fwd = timed(lambda s: lib.bn_act_fwd(p(x), p(beta), p(y2), p(smean), p(srstd), rows, c, 0, 0, 1, 1e-3, _lib.ACT_RELU, 0.0, code,
                                                   0, p(ws), nb, s))
            nbytes = 2.0 * rows * c * es
            pr = probe.get((rows, c))
            print('%-12s %3d %7d %4d %9.1f | %9.2f %7.2f%% | %9.2f | %11s %11s' % (
                label, b, rows, c, nbytes / 1024, t_inf, 100.0 * nbytes / (t_inf * 1e-6) / HBM_PEAK, t_fwd,
                '%.2f' % pr[0] if pr else 'not built', ('%.2f' % pr[1] if pr[1] > 0 else '-') if pr else 'not built'))
            acc = tot.setdefault(b, [0.0, 0.0, 0.0])
            acc[0] += t_inf
            acc[1] += t_fwd
            acc[2] += pr[0] if pr else 0.0
    for b, (a, f, s) in tot.items():
        print('# batch %d, nine layers: infer %.1f us, bn_act_fwd %.1f us%s' % (b, a, f, ', stream %.1f us' % s if probe else ''))


def rollout(batch, reps):
    G.reset_default_graph()
    sess = G.Session(device='cuda:0')
    tr = T.Trainer(sess, False, 'bce', 'adam', True, batch_size=batch, img_size=64, lookahead=False, bn_inference=True)
    sess.run(G.global_variables_initializer())
    rng = np.random.default_rng(1)
    frames = rng.uniform(-1, 1, (batch, 8, 64, 64, 3)).astype(np.float32)
    acts = rng.standard_normal((batch, 8, 10)).astype(np.float32)
    for t in range(4):
        tr.calibrate_bn(frames[:, t], acts[:, t])
    for _ in range(3):
        tr.rollout_metrics(frames, acts, bn='stored')
        tr.rollout_metrics(frames, acts, bn='batch')
    rate = {'stored': [], 'batch': []}
    n = batch * 7
    for _ in range(reps):
        for mode in ('stored', 'batch'):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.rollout_metrics(frames, acts, bn=mode)           # returns host arrays: synchronised
            rate[mode].append(n / (time.perf_counter() - t0))
    sess.close()
    print('# rollout_metrics, DNA generator, batch %d, 7 steps, %d alternating repetitions; frames/s' % (batch, reps))
    for mode in ('stored', 'batch'):
        print('%-7s %s' % (mode, ' '.join('%.0f' % r for r in rate[mode])))
    ms, mb = float(np.median(rate['stored'])), float(np.median(rate['batch']))
    spread = float(max(rate['batch']) - min(rate['batch']))
    print('median: stored %.0f, batch %.0f frames/s (ratio %.3f); run-to-run spread of the batch rate (max - min) %.0f, stdev %.0f'
          % (ms, mb, ms / mb, spread, float(np.std(rate['batch']))))
    print('stored is not below batch by more than that spread: %s' % ('met' if ms >= mb - spread else 'NOT met'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'])
    ap.add_argument('--batches', default='1,32')
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--stream-probe', default=os.path.join(ROOT, 'build', 'stream_probe'))
    ap.add_argument('--skip-rollout', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_bn_infer.py measures on a GPU: none is visible')
    kernels(a.dtype, [int(v) for v in a.batches.split(',')], a.stream_probe)
    print('device: %s' % torch.cuda.get_device_name(0))
    if not a.skip_rollout:
        rollout(32, a.reps)


if __name__ == '__main__':
    main()
