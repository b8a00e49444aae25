#!/usr/bin/env python
"""What differentiable augmentation of the discriminator's inputs costs on one MI355X (profiles/d_augment/).

  python tools/bench_d_augment.py [--steps 100] [--reps 3] [--parent DIR] [--out profiles/d_augment/bench_d_augment.txt]
  python tools/bench_d_augment.py --trace-steps 20        (the workload of a `rocprofv3 --kernel-trace --stats` run: nothing is timed)

(a) acg_d_augment_fwd and acg_d_augment_bwd alone at config 2's D(both) input - [64, 64, 64, 8] float32, 2 frames of 3 channels -
    and at [64, 128, 128, 8]: device events around N back-to-back calls, after warm-up, time / N; in the same process
    acg_inst_noise_add at sigma = 0 on the same tensor, a pure copy of the same bytes.  The yardstick: forward and backward each
    at most 3 x that copy (two passes over the input, a reduction and a barrier per block).  A miss is reported, not tuned away.
(b) one training iteration (D step + G step) of a config-2 trainer (batch 32, 64^2, DNA k = 5, bce, Adam, float32; device-resident
    inputs, replayed HIP graphs), lookahead=False, with d_augment='color,translation,cutout' and without.  Both sessions live in
    one process and take turns: --reps rounds of --steps iterations each.  No threshold.
(c) with --parent DIR, a built tree of the parent commit: `bench.py --gpus 1` of that tree and of this one, the feature off,
    taking turns (--reps rounds, a fresh process each), steps/s side by side, and the generated frames of the last timed step
    (bench.py --dump-outputs) compared bit for bit; written to bench_parent_vs_pr.txt beside --out."""
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

N_CALLS = 200
POLICY = 'color,translation,cutout'
LINES = []


def say(line=''):
    print(line, flush=True)
    LINES.append(line)


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def event_us_per_call(call, reps):
    """-> [us per call of each round]: device events around N_CALLS back-to-back calls on the current stream, after warm-up."""
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(20):
        call(s)
    torch.cuda.synchronize()
    got = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N_CALLS):
            call(s)
        e1.record()
        torch.cuda.synchronize()
        got.append(e0.elapsed_time(e1) * 1e3 / N_CALLS)
    return got


def entry_times(reps):
    lib, dev = _lib.get(), torch.device('cuda:0')
    misses = []
    for rows, side in ((64, 64), (64, 128)):
        pitch = 8
        x = torch.randn(rows, side, side, pitch, device=dev)
        y = torch.empty_like(x)
        state = torch.tensor([7, 0], dtype=torch.int64, device=dev)
        params = torch.zeros(rows, 8, device=dev)
        lib.d_augment_draw(p(state), p(params), rows, side, side, 7, 2, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        nbytes = lib.d_augment_workspace_bytes(rows, side, side, 2, 3)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        key, sigma = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(1, device=dev)
        pixels = rows * side * side
        moved = 2 * x.numel() * 4
        say('# [%d, %d, %d, %d] float32: %.1f MB read + written by a copy' % (rows, side, side, pitch, moved / 1e6))
        copy = event_us_per_call(lambda s: lib.inst_noise_add(p(x), p(y), p(key), p(sigma), pixels, 6, pitch, 3, 3, _lib.code(torch.float32), 2, s), reps)
        cmed = float(np.median(copy))
        say('%-34s %s   median %.2f us per call, %.2f TB/s' % ('inst_noise_add sigma 0 (copy)', ' '.join('%.2f' % v for v in copy), cmed, moved / cmed / 1e6))
        for name, fn in (('d_augment_fwd', lib.d_augment_fwd), ('d_augment_bwd', lib.d_augment_bwd)):
            t = event_us_per_call(lambda s: fn(p(x), p(params), p(y), rows, side, side, pitch, 2, 3, p(ws), nbytes, s), reps)
            med = float(np.median(t))
            ok = med <= 3 * cmed
            say('%-34s %s   median %.2f us per call (two launches) = %.2f x the copy: yardstick 3 x %s'
                % (name, ' '.join('%.2f' % v for v in t), med, med / cmed, 'met' if ok else 'MISSED'))
            if not ok:
                misses.append((name, side))
    return misses


def _sessions():
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(32, 64, 64, 3, device=dev, generator=gen) * 2 - 1
    y = torch.rand(32, 64, 64, 3, device=dev, generator=gen) * 2 - 1
    a = torch.randn(32, 10, device=dev, generator=gen)
    s = torch.randn(32, 5, device=dev, generator=gen)
    live = []
    for label, kw in (('d_augment off, lookahead off', {}), ('d_augment ' + POLICY, dict(d_augment=POLICY))):
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
    return live


def step_rates(steps, reps):
    live = _sessions()
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


def trace_workload(steps):
    """Iterations of the augmented trainer alone, for a kernel trace: the d_augment_* kernels of `steps` D + G steps."""
    label, sess, run = _sessions()[1]
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    print('ran %d more iterations of %s' % (steps, label))


def bench_turns(parent, reps, steps, warmup):
    """bench.py of the parent tree and of this one, taking turns, a fresh process each: -> {label: [steps/s]}, frames identical."""
    trees = (('parent', os.path.abspath(parent)), ('this tree', ROOT))
    rates, frames = {label: [] for label, _ in trees}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(reps):
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
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--parent', default=None, metavar='DIR', help='a built tree of the parent commit: also run (c)')
    ap.add_argument('--bench-steps', type=int, default=200)
    ap.add_argument('--bench-warmup', type=int, default=20)
    ap.add_argument('--trace-steps', type=int, default=0, metavar='N', help='run N augmented iterations and exit (for a kernel trace)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'd_augment', 'bench_d_augment.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_d_augment.py measures on a GPU: none is visible')
    if args.trace_steps:
        return trace_workload(args.trace_steps)
    say('device: %s' % torch.cuda.get_device_name(0))
    say('# (a) us per call: device events around %d back-to-back calls, one column per round' % N_CALLS)
    misses = entry_times(max(args.reps, 5))
    say('# (b) training iterations (D step + G step) per second, config 2, plain call path; %d rounds of %d iterations, sessions taking turns'
        % (args.reps, args.steps))
    rates = step_rates(args.steps, args.reps)
    for label, v in rates.items():
        say('%-44s %s   median %.1f it/s = %.1f us per iteration' % (label, ' '.join('%.1f' % r for r in v), float(np.median(v)),
                                                                     1e6 / float(np.median(v))))
    off, on = (float(np.median(v)) for v in rates.values())
    say('ratio on / off %.4f: the augmentation costs %.1f us per iteration (%.2f %%)' % (on / off, 1e6 / on - 1e6 / off, 100 * (off / on - 1)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(LINES) + '\n')
    if args.parent:
        del LINES[:]
        say('# bench.py --gpus 1 --steps %d --warmup %d, the feature off: the parent commit and this tree taking turns, %d rounds'
            % (args.bench_steps, args.bench_warmup, args.reps))
        turns, same = bench_turns(args.parent, args.reps, args.bench_steps, args.bench_warmup)
        for label, v in turns.items():
            say('%-12s %s   median %.2f steps/s' % (label, ' '.join('%.2f' % r for r in v), float(np.median(v))))
        say('generated frames of the last timed step, all %d runs: %s' % (2 * args.reps, 'bit-identical' if same else 'DIFFERENT'))
        with open(os.path.join(os.path.dirname(os.path.abspath(args.out)), 'bench_parent_vs_pr.txt'), 'w') as f:
            f.write('\n'.join(LINES) + '\n')
        if not same:
            raise SystemExit('the generated frames differ between the parent commit and this tree')
    if misses:
        say('yardstick missed: %s' % ', '.join('%s at %d^2' % m for m in misses))


if __name__ == '__main__':
    main()
