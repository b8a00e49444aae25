#!/usr/bin/env python
"""What the latent posterior costs on one MI355X (profiles/latent/).

  python tools/bench_latent.py [--steps 200] [--reps 5] [--parent DIR] [--out profiles/latent/bench_latent.txt]

(a) acg_latent_fwd (with its KL sum) and acg_latent_bwd alone at (B, A, Z) = (32, 10, 8) - config 2's batch - and (128, 10, 64), the
    largest draw: N calls captured back to back into a HIP graph and replayed, wall time / N, beside the launch floor measured
    the same way in the same process (N one-thread acg_step_inc kernels) and acg_noise_concat, whose draw the forward shares.
(b) one D step and one G step of a config-2 trainer (batch 32, 64^2, DNA k = 5, bce, Adam, float32; device-resident inputs,
    replayed HIP graphs) with noise_dim = 8, with and without ``posterior``.  Both sessions live in one process and take turns:
    --reps rounds of --steps steps each.  The encoder is four conv 5x5/2 + BatchNorm layers and a head on a [B, 64, 64, 6] input -
    about a second, narrower discriminator pass - forward in both steps and backward in the G step: its cost is the feature's.
(c) with --parent DIR, a built tree of the parent commit: `bench.py --gpus 1` of that tree and of this one, the feature off,
    taking turns (--bench-rounds rounds, a fresh process each), steps/s side by side, and the generated frames of the last
    timed step (bench.py --dump-outputs) compared bit for bit.
No threshold is set: the figures are written out."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
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
    """-> [us per call of each block of 10 replays] of a graph of N_GRAPH calls."""
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
    floor = float(np.median(graph_us_per_call(lambda s: lib.step_inc(p(cnt), s), reps)))
    say('%-40s median %.2f us per kernel' % ('launch floor (step_inc, 1 thread)', floor))
    for b, a, z in ((32, 10, 8), (128, 10, 64)):
        actions, stats = torch.randn(b, a, device=dev), torch.cat([torch.randn(b, z, device=dev), torch.randn(b, z, device=dev) - 1.0], dim=1)
        state = torch.tensor([7, 0], dtype=torch.int64, device=dev)
        mode, scale = torch.ones(2, device=dev), torch.ones(1, device=dev)
        out, kl = torch.zeros(b, a + z, device=dev), torch.zeros(1, device=dev)
        dout, dstats = torch.randn(b, a + z, device=dev), torch.zeros(b, 2 * z, device=dev)
        calls = (('noise_concat', lambda s: lib.noise_concat(p(actions), p(state), p(scale), p(out), b, a, z, 0, s)),
                 ('latent_fwd (posterior, kl)', lambda s: lib.latent_fwd(p(actions), p(stats), p(state), p(mode), p(out), p(kl), b, a, z, 0, s)),
                 ('latent_fwd (posterior, no kl)', lambda s: lib.latent_fwd(p(actions), p(stats), p(state), p(mode), p(out), None, b, a, z, 0, s)),
                 ('latent_bwd', lambda s: lib.latent_bwd(p(dout), p(out), p(stats), p(mode), 0.5, p(dstats), None, b, a, z, s)))
        for label, call in calls:
            t = float(np.median(graph_us_per_call(call, reps)))
            say('%-40s median %.2f us per call = floor + %.2f us' % ('%s B=%d A=%d Z=%d' % (label, b, a, z), t, t - floor))


def step_rates(steps, reps):
    """-> {(label, step): [steps/s per round]} of the D step and the G step of two config-2 trainers taking turns."""
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(32, 64, 64, 3, device=dev, generator=gen) * 2 - 1
    y = torch.rand(32, 64, 64, 3, device=dev, generator=gen) * 2 - 1
    a = torch.randn(32, 10, device=dev, generator=gen)
    s = a[:, 5:].contiguous()
    live = []
    for label, kw in (('noise_dim 8', {}), ('noise_dim 8, posterior', dict(posterior=True))):
        G.reset_default_graph()
        optim.set_data_parallel(1)
        sess = G.Session(device='cuda:0')
        tr = T.Trainer(sess, True, 'bce', 'adam', True, batch_size=32, img_size=64, ksize=5, lookahead=False, noise_dim=8, **kw)
        sess.run(G.global_variables_initializer())
        runs = {'D step': lambda tr=tr: tr.train_d(x, y, a), 'G step': lambda tr=tr: tr.train_g(x, y, a, s, device_fetch=True)}
        for _ in range(5):                                   # eager, capture, replays
            for run in runs.values():
                run()
        live.append((label, sess, runs))
    torch.cuda.synchronize()
    out = {(label, step): [] for label, _, runs in live for step in runs}
    for _ in range(reps):
        for label, sess, runs in live:
            for step, run in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    run()
                torch.cuda.synchronize()
                out[(label, step)].append(steps / (time.perf_counter() - t0))
    for label, sess, runs in live:
        sess.close()
    return out


def bench_turns(parent, rounds, steps, warmup):
    """bench.py of the parent tree and of this one, taking turns, a fresh process each: -> {label: [steps/s]}, frames identical."""
    trees = (('parent', os.path.abspath(parent)), ('this tree', ROOT))
    rates, frames = {label: [] for label, _ in trees}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(rounds):
            for label, tree in trees:
                dump = os.path.join(tmp, '%s_%d' % (label.split()[0], r))
                res = subprocess.run([sys.executable, os.path.join(tree, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                                      '--no-cpu-baseline', '--dump-outputs', dump], cwd=tree, stdout=subprocess.PIPE, check=True, timeout=600)
                line = json.loads([ln for ln in res.stdout.decode().splitlines() if ln.startswith('{')][-1])
                rates[label].append(float(line['value']))
                frames.setdefault(label, []).append(np.load(os.path.join(dump, 'generated_frames.npy')))
    first = frames['parent'][0]
    same = all(np.array_equal(f.view(np.uint32), first.view(np.uint32)) for fs in frames.values() for f in fs)
    return rates, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--parent', default=None, metavar='DIR', help='a built tree of the parent commit: also run (c)')
    ap.add_argument('--bench-rounds', type=int, default=3)
    ap.add_argument('--bench-steps', type=int, default=200)
    ap.add_argument('--bench-warmup', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'latent', 'bench_latent.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_latent.py measures on a GPU: none is visible')
    say('device: %s' % torch.cuda.get_device_name(0))
    say('# (a) us per kernel in a HIP graph of %d back-to-back calls, median over %d blocks of 10 replays' % (N_GRAPH, args.reps))
    entry_times(args.reps)
    say('# (b) steps per second, config 2, plain call path; %d rounds of %d steps, sessions and steps taking turns' % (args.reps, args.steps))
    rates = step_rates(args.steps, args.reps)
    med = {k: float(np.median(v)) for k, v in rates.items()}
    for (label, step), v in rates.items():
        say('%-24s %-7s %s   median %.1f steps/s = %.1f us per step' % (label, step, ' '.join('%.1f' % r for r in v), med[(label, step)],
                                                                      1e6 / med[(label, step)]))
    for step in ('D step', 'G step'):
        off, on = med[('noise_dim 8', step)], med[('noise_dim 8, posterior', step)]
        base = rates[('noise_dim 8', step)]
        say('posterior costs %.1f us per %s (%.2f %%); spread of the rounds without it (max - min): %.1f us'
            % (1e6 / on - 1e6 / off, step, 100 * (off / on - 1), 1e6 / min(base) - 1e6 / max(base)))
    if args.parent:
        say('# (c) bench.py --gpus 1 --steps %d --warmup %d, the feature off: the parent commit and this tree taking turns, %d rounds'
            % (args.bench_steps, args.bench_warmup, args.bench_rounds))
        turns, same = bench_turns(args.parent, args.bench_rounds, args.bench_steps, args.bench_warmup)
        for label, v in turns.items():
            say('%-12s %s   median %.2f steps/s' % (label, ' '.join('%.2f' % r for r in v), float(np.median(v))))
        say('generated frames of the last timed step, all %d runs: %s' % (2 * args.bench_rounds, 'bit-identical' if same else 'DIFFERENT'))
        if not same:
            raise SystemExit('the generated frames differ between the parent commit and this tree')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
