#!/usr/bin/env python
"""What a learning-rate schedule costs in the optimizer launch on one MI355X (DESIGN section "Learning rates", profiles/lr_schedule/).

  python tools/bench_lr_schedule.py [--parent-lib PATH/libacgan_hip.so] [--reps 9] [--out profiles/lr_schedule/bench_lr_schedule.txt]

Hot kernel time of acg_adam_step_lr / acg_rmsprop_step_lr (cosine, with a warmup) beside acg_adam_step / acg_rmsprop_step over
flat buffers of config 2's generator and discriminator sizes (batch 32, 64^2, DNA k = 5): N launches of one entry captured into a
HIP graph and replayed between two events, the variants taking turns inside every round; microseconds per launch, medians, and
the run-to-run spread (max - min) of the plain entry.  --parent-lib: the same two plain entries of another build of the library
(the commit before the schedule existed), loaded beside this one, as the baseline the issue asks for.  No threshold: the
buffers (4 or 3 passes of 10 - 30 MB) live in the caches, so this is the hot relaunch, not the in-situ time of a training step."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from action_conditioned_gans_amd import _lib, graph as G, optim, train as T   # noqa: E402

LINES = []


def say(line=''):
    print(line, flush=True)
    LINES.append(line)


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def sizes():
    """Config 2's flat-buffer sizes (G, D), from the graph itself."""
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cuda:0')
    T.Trainer(sess, True, 'bce', 'adam', True, batch_size=32, img_size=64, ksize=5)
    out = sess.graph.layout('g')[1], sess.graph.layout('d')[1]
    sess.close()
    return out


def graph_of(fn, n_graph):
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for _ in range(n_graph):
            fn(sp)
    gr.replay()
    torch.cuda.synchronize()
    return gr


def once(gr, n_graph):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    gr.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n_graph


def parent_entries(path):
    """acg_adam_step / acg_rmsprop_step of another build, bound by this build's table (their signatures are ABI)."""
    cdll = ctypes.CDLL(path)
    out = {}
    for name in ('acg_adam_step', 'acg_rmsprop_step'):
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = ctypes.c_int32, _lib.SIGNATURES[name][1]
        out[name[4:]] = fn
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lr_schedule', 'bench_lr_schedule.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_lr_schedule.py measures on a GPU: none is visible')
    lib, dev = _lib.get(), torch.device('cuda:0')
    parent = parent_entries(args.parent_lib) if args.parent_lib else {}
    say('device: %s; HIP graphs of %d launches, %d rounds, the variants taking turns in every round' % (torch.cuda.get_device_name(0), args.launches, args.reps))
    f = lambda v: float(np.float32(v))       # noqa: E731
    sched = _lib.LrSched(_lib.LrSched.KINDS.index('cosine'), 100, 10 ** 6, f(0.1))
    for scope, n in zip(('G', 'D'), sizes()):
        prm, grd, s1, s2 = (torch.randn(n, device=dev) * 0.02 for _ in range(4))
        s1.abs_()
        s2.abs_()
        step = torch.ones(1, dtype=torch.int32, device=dev)
        count, word, out = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, device=dev)
        adam = (p(prm), p(grd), p(s1), p(s2), p(step), n, f(1e-3), f(0.9), f(0.999), f(1e-8), 1.0, 0, 0.0, 0.0)
        rms = (p(prm), p(grd), p(s1), n, f(5e-5), f(0.9), f(1e-10), 1.0, 0, 0.0, 0.0)
        tail = (ctypes.byref(sched), p(count), p(word), p(out), None, 0.0, None, None)
        variants = [('adam_step', lambda s: lib.adam_step(*adam, s)), ('adam_step_lr', lambda s: lib.adam_step_lr(*adam, *tail, s)),
                    ('rmsprop_step', lambda s: lib.rmsprop_step(*rms, s)), ('rmsprop_step_lr', lambda s: lib.rmsprop_step_lr(*rms, *tail, s))]
        if parent:
            variants += [('adam_step (parent)', lambda s: parent['adam_step'](*adam, s)),
                         ('rmsprop_step (parent)', lambda s: parent['rmsprop_step'](*rms, s))]
        graphs = [(label, graph_of(fn, args.launches)) for label, fn in variants]
        times = {label: [] for label, _ in graphs}
        for _ in range(args.reps):
            for label, gr in graphs:
                times[label].append(once(gr, args.launches))
        say('# %s: %d floats (%.1f MB per buffer); us per launch, one column per round' % (scope, n, n * 4 / 1e6))
        for label, v in times.items():
            say('%-24s %s   median %.2f' % (label, ' '.join('%.2f' % t for t in v), float(np.median(v))))
        for kind in ('adam', 'rmsprop'):
            base = kind + ('_step (parent)' if parent else '_step')
            spread = max(times[base]) - min(times[base])
            delta = float(np.median(times[kind + '_step_lr'])) - float(np.median(times[base]))
            say('%s_step_lr - %s: %+.2f us (spread of the baseline, max - min: %.2f us)' % (kind, base, delta, spread))
        if int(count.item()) != 2 * (1 + args.reps) * args.launches:
            raise SystemExit('%d updates counted' % int(count.item()))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
