#!/usr/bin/env python
"""What instance noise on the discriminator's inputs costs on one MI355X (profiles/d_noise/).

  python tools/bench_d_noise.py [--steps 200] [--reps 5] [--parent DIR] [--out profiles/d_noise/bench_d_noise.txt]

(a) acg_inst_noise_prepare and acg_inst_noise_add alone at config 2's shape - the D step's [2 B, 64, 64, 8] input, B = 32: 262 144
    pixels, 6 channels at a pitch of 8, noise on channels 3..5 - in float32 and bf16: N calls captured back to back into a HIP
    graph and replayed, wall time / N, beside the launch floor measured the same way in the same process (N one-thread
    acg_step_inc kernels), and the bytes the add moves over its time.
(b) one D step of a config-2 trainer (batch 32, 64^2, DNA k = 5, bce, Adam, float32; device-resident inputs, replayed HIP graph)
    with d_noise = 0.5 against the same tree with d_noise = 0 and lookahead=False - the call path a d_noise > 0 trainer takes.
    Both sessions live in one process and take turns: --reps rounds of --steps D steps each.
(c) with --parent DIR, a built tree of the parent commit: `bench.py --gpus 1` of that tree and of this one, the feature off,
    taking turns (--reps rounds, a fresh process each), steps/s side by side, and the generated frames of the last timed step
    (bench.py --dump-outputs) compared bit for bit.
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
    floor = graph_us_per_call(lambda s: lib.step_inc(p(cnt), s), reps)
    med = float(np.median(floor))
    say('%-40s %s   median %.2f us per kernel' % ('launch floor (step_inc, 1 thread)', ' '.join('%.2f' % v for v in floor), med))
    state = torch.tensor([7, 0], dtype=torch.int64, device=dev)
    updates = torch.zeros(1, dtype=torch.int64, device=dev)
    key, sigma = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(1, device=dev)
    t = graph_us_per_call(lambda s: lib.inst_noise_prepare(p(state), p(updates), p(key), p(sigma), 0.5, 0.05, 0, 10 ** 6, 1, s), reps)
    say('%-40s %s   median %.2f us per call = floor + %.2f us' % ('inst_noise_prepare', ' '.join('%.2f' % v for v in t), float(np.median(t)),
                                                                 float(np.median(t)) - med))
    pixels, pitch = 2 * 32 * 64 * 64, 8
    for name, dtype in (('float32', torch.float32), ('bf16', torch.bfloat16)):
        x = torch.randn(pixels, pitch, device=dev).to(dtype)
        y = torch.empty_like(x)
        t = graph_us_per_call(lambda s: lib.inst_noise_add(p(x), p(y), p(key), p(sigma), pixels, 6, pitch, 3, 3, _lib.code(dtype), 2, s), reps)
        moved = 2 * x.numel() * x.element_size()
        say('%-40s %s   median %.2f us per call: %.1f MB read + written, %.2f TB/s'
            % ('inst_noise_add %s [%d, %d]' % (name, pixels, pitch), ' '.join('%.2f' % v for v in t), float(np.median(t)), moved / 1e6,
               moved / float(np.median(t)) / 1e6))


def d_step_rates(steps, reps):
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(32, 64, 64, 3, device=dev, generator=gen) * 2 - 1
    y = torch.rand(32, 64, 64, 3, device=dev, generator=gen) * 2 - 1
    a = torch.randn(32, 10, device=dev, generator=gen)
    live = []
    for label, kw in (('d_noise 0, lookahead off', {}), ('d_noise 0.5', dict(d_noise=0.5, d_noise_final=0.05, d_noise_decay_steps=10 ** 6))):
        G.reset_default_graph()
        optim.set_data_parallel(1)
        sess = G.Session(device='cuda:0')
        tr = T.Trainer(sess, True, 'bce', 'adam', True, batch_size=32, img_size=64, ksize=5, lookahead=False, **kw)
        sess.run(G.global_variables_initializer())

        def run(tr=tr):
            tr.train_d(x, y, a)
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
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--parent', default=None, metavar='DIR', help='a built tree of the parent commit: also run (c)')
    ap.add_argument('--bench-steps', type=int, default=200)
    ap.add_argument('--bench-warmup', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'd_noise', 'bench_d_noise.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_d_noise.py measures on a GPU: none is visible')
    say('device: %s' % torch.cuda.get_device_name(0))
    say('# (a) us per kernel in a HIP graph of %d back-to-back calls, one column per block of 10 replays' % N_GRAPH)
    entry_times(args.reps)
    say('# (b) D steps per second, config 2, plain call path; %d rounds of %d steps, sessions taking turns' % (args.reps, args.steps))
    rates = d_step_rates(args.steps, args.reps)
    for label, v in rates.items():
        say('%-28s %s   median %.1f steps/s = %.1f us per D step' % (label, ' '.join('%.1f' % r for r in v), float(np.median(v)),
                                                                     1e6 / float(np.median(v))))
    off, on = (float(np.median(v)) for v in rates.values())
    say('d_noise 0.5 costs %.1f us per D step (%.2f %%); spread of the d_noise 0 rounds (max - min): %.1f us'
        % (1e6 / on - 1e6 / off, 100 * (off / on - 1), 1e6 / min(rates['d_noise 0, lookahead off']) - 1e6 / max(rates['d_noise 0, lookahead off'])))
    if args.parent:
        say('# (c) bench.py --gpus 1 --steps %d --warmup %d, the feature off: the parent commit and this tree taking turns, %d rounds'
            % (args.bench_steps, args.bench_warmup, args.reps))
        turns, same = bench_turns(args.parent, args.reps, args.bench_steps, args.bench_warmup)
        for label, v in turns.items():
            say('%-12s %s   median %.2f steps/s' % (label, ' '.join('%.2f' % r for r in v), float(np.median(v))))
        say('generated frames of the last timed step, all %d runs: %s' % (2 * args.reps, 'bit-identical' if same else 'DIFFERENT'))
        if not same:
            raise SystemExit('the generated frames differ between the parent commit and this tree')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
