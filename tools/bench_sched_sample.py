#!/usr/bin/env python
"""What scheduled sampling costs a K-step G step on one MI355X (DESIGN section 7 "Scheduled sampling", profiles/sched_sample/).

  python tools/bench_sched_sample.py [--parent PATH] [--rounds 4] [--steps 400] [--out profiles/sched_sample/bench_sched_sample.txt]

Times ``Trainer.train_g_rollout`` at B = 32, K = 3, the DNA generator, bce / Adam, replayed from its HIP graph, device-resident
inputs: three cases taking turns inside every round - ``parent`` (the package of another checkout, built there: the commit before
scheduled sampling existed; left out without --parent), ``off`` (this tree, ``sched_sampling='off'``: the same program) and ``on``
(``'constant'`` at p = 0.5: 1 + 2 (K - 1) launches more).  Every case of every round is a fresh child process (one GPU process at
a time), so a round's cases see the same clocks and no case inherits another's allocator or graph state.  Reports milliseconds per
step, the medians, the differences and the spread (max - min) each case shows over the rounds.  No threshold."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINES = []


def say(line=''):
    print(line, flush=True)
    LINES.append(line)


def worker(args):
    """One case in this process: -> one JSON line {'ms_per_step', 'launches'}."""
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch
    from action_conditioned_gans_amd import graph as G, optim, train as T
    B, K = args.batch, args.rollout_steps
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cuda:0')
    kw = dict(sched_sampling='constant', ss_start=0.5, ss_seed=1) if args.mode == 'on' else {}
    tr = T.Trainer(sess, True, 'bce', 'adam', True, batch_size=B, img_size=64, ksize=5, lookahead=False, rollout_steps=K, **kw)
    sess.run(G.global_variables_initializer())
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.uniform(-1, 1, (B, K + 1, 64, 64, 3)).astype(np.float32)).cuda()
    a = torch.from_numpy(rng.standard_normal((B, K, 10)).astype(np.float32)).cuda()
    s = torch.from_numpy(rng.standard_normal((B, K, 5)).astype(np.float32)).cuda()
    for _ in range(args.warmup):                 # eager, capture, replays
        tr.train_g_rollout(x, a, s, device_fetch=True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        tr.train_g_rollout(x, a, s, device_fetch=True)
    e1.record()
    torch.cuda.synchronize()
    prog = [p for p in sess._programs.values() if p is not None and p.graphs is not None]
    launches = sum(len(seg) for p in prog for kind, seg in p.segments if kind == 'dev')
    sess.close()
    print(json.dumps({'ms_per_step': e0.elapsed_time(e1) / args.steps, 'launches': launches}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a checkout of the commit to compare with, its library built')
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--rollout_steps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sched_sample', 'bench_sched_sample.txt'))
    ap.add_argument('--worker', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--root', default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument('--mode', default='off', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    import numpy as np
    cases = ([('parent', args.parent, 'off')] if args.parent else []) + [('off', ROOT, 'off'), ('on', ROOT, 'on')]
    say('train_g_rollout, B = %d, K = %d, DNA, bce / Adam, HIP-graph replay, device-resident inputs; %d steps after %d warm-up steps; '
        '%d rounds, the cases taking turns in every round, one fresh process each' % (args.batch, args.rollout_steps, args.steps, args.warmup, args.rounds))
    times, launches = {label: [] for label, _, _ in cases}, {}
    for _ in range(args.rounds):
        for label, root, mode in cases:
            cmd = [sys.executable, os.path.abspath(__file__), '--worker', '--root', root, '--mode', mode, '--steps', str(args.steps),
                   '--warmup', str(args.warmup), '--batch', str(args.batch), '--rollout_steps', str(args.rollout_steps)]
            out = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=300).stdout.decode()
            res = json.loads([l for l in out.splitlines() if l.startswith('{')][-1])
            times[label].append(res['ms_per_step'])
            launches[label] = res['launches']
    say('# ms per step, one column per round')
    for label, v in times.items():
        say('%-7s %s   median %.3f   spread (max - min) %.3f   ops that launch in the captured program: %d'
            % (label, ' '.join('%.3f' % t for t in v), float(np.median(v)), max(v) - min(v), launches[label]))
    med = {label: float(np.median(v)) for label, v in times.items()}
    if 'parent' in med:
        say('off - parent: %+.3f ms' % (med['off'] - med['parent']))
    say('on - off: %+.3f ms (%+d ops that launch, one launch each)' % (med['on'] - med['off'], launches['on'] - launches['off']))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
