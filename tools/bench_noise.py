#!/usr/bin/env python
"""What the generator's noise input costs on one MI355X (profiles/noise/).

  python tools/bench_noise.py [--steps 200] [--reps 5] [--out profiles/noise/bench_noise.txt]

(a) acg_noise_concat alone at (B, A, Z) = (32, 10, 8) - config 2's batch - and (64, 10, 64), the largest draw: N calls captured
    back to back into a HIP graph and replayed, wall time / N, beside the launch floor measured the same way in the same process
    (tools/launch_floor.py's method: N one-thread acg_step_inc kernels).  The call is one block; what it costs over the floor is
    its arithmetic - up to 8 Philox blocks and 32 logf / cosf / sinf per thread.
(b) steps per second of a config-2 trainer (batch 32, 64^2, DNA k = 5, bce, Adam, float32; one D step + one G step, device-resident
    inputs, replayed HIP graphs) with noise_dim = 8 against the same tree with noise_dim = 0 and lookahead=False - the call path a
    noise_dim > 0 trainer takes.  Both sessions live in one process and take turns: --reps rounds of --steps iterations each.
No threshold is set: the figures are written out."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from action_conditioned_gans_amd import _lib, graph as G, optim, train as T   # noqa: E402

N_GRAPH = 100
LINES = []


def say(line=''):
    print(line, flush=True)
    LINES.append(line)


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def graph_us_per_call(call, reps):
    """-> [us per call of each replay] of a graph of N_GRAPH calls."""
    call(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for _ in range(N_GRAPH):
            call(sp)
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    got = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(10):
            gr.replay()
        torch.cuda.synchronize()
        got.append((time.perf_counter() - t0) * 1e6 / (10 * N_GRAPH))
    return got


def entry_times(reps):
    lib, dev = _lib.get(), torch.device('cuda:0')
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    floor = graph_us_per_call(lambda s: lib.step_inc(p(cnt), s), reps)
    say('%-34s %s   median %.2f us per kernel' % ('launch floor (step_inc, 1 thread)', ' '.join('%.2f' % v for v in floor), float(np.median(floor))))
    for b, a, z in ((32, 10, 8), (64, 10, 64)):
        actions = torch.randn(b, a, device=dev)
        state = torch.tensor([7, 0], dtype=torch.int64, device=dev)
        scale = torch.ones(1, device=dev)
        out = torch.zeros(b, a + z, device=dev)
        t = graph_us_per_call(lambda s: lib.noise_concat(p(actions), p(state), p(scale), p(out), b, a, z, 0, s), reps)
        say('%-34s %s   median %.2f us per call = floor + %.2f us' % ('noise_concat B=%d A=%d Z=%d' % (b, a, z), ' '.join('%.2f' % v for v in t),
                                                                     float(np.median(t)), float(np.median(t)) - float(np.median(floor))))


def step_rates(steps, reps):
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(32, 64, 64, 3, device=dev, generator=gen) * 2 - 1
    y = torch.rand(32, 64, 64, 3, device=dev, generator=gen) * 2 - 1
    a = torch.randn(32, 10, device=dev, generator=gen)
    s = a[:, 5:].contiguous()
    live = []
    for label, kw in (('noise_dim 0, lookahead off', {}), ('noise_dim 8', dict(noise_dim=8))):
        G.reset_default_graph()
        optim.set_data_parallel(1)
        sess = G.Session(device='cuda:0')
        tr = T.Trainer(sess, True, 'bce', 'adam', True, batch_size=32, img_size=64, ksize=5, lookahead=False, **kw)
        sess.run(G.global_variables_initializer())

        def run(tr=tr):
            tr.train_d(x, y, a)
            tr.train_g(x, y, a, s, device_fetch=True)
        for _ in range(5):                                   # eager, capture, replays
            run()
        live.append((label, sess, run))
    torch.cuda.synchronize()
    out = {label: [] for label, _, _ in live}
    for _ in range(reps):
        for label, sess, run in live:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                run()
            torch.cuda.synchronize()
            out[label].append(steps / (time.perf_counter() - t0))
    for label, sess, run in live:
        sess.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'noise', 'bench_noise.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_noise.py measures on a GPU: none is visible')
    say('device: %s' % torch.cuda.get_device_name(0))
    say('# (a) us per kernel in a HIP graph of %d back-to-back calls, one column per block of 10 replays' % N_GRAPH)
    entry_times(args.reps)
    say('# (b) iterations (one D step + one G step) per second, config 2, plain call path; %d rounds of %d iterations, sessions taking turns'
        % (args.reps, args.steps))
    rates = step_rates(args.steps, args.reps)
    for label, v in rates.items():
        say('%-28s %s   median %.1f steps/s = %.1f us per iteration' % (label, ' '.join('%.1f' % r for r in v), float(np.median(v)),
                                                                        1e6 / float(np.median(v))))
    off, on = (float(np.median(v)) for v in rates.values())
    say('noise_dim 8 costs %.1f us per iteration (%.2f %%); spread of the noise_dim 0 rounds (max - min): %.1f us'
        % (1e6 / on - 1e6 / off, 100 * (off / on - 1), 1e6 / min(rates['noise_dim 0, lookahead off']) - 1e6 / max(rates['noise_dim 0, lookahead off'])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
