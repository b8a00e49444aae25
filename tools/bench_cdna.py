#!/usr/bin/env python
"""CDNA generator measurements (profiles/cdna/).

(a) acg_cdna_composite_fwd / _bwd against the unfused acg_cdna_fwd / _bwd (M pieces written to HBM) at (32, 64^2), (256, 64^2)
    and (32, 128^2), M = 10, k = 5: device events around back-to-back launches (warm-up first; at least --reps launches and
    at least 1 s per block), algorithmic bytes and FLOPs, and the share of the bound that applies;
(b) training steps/s at batch 32, 64^2, bce, Adam, look-ahead call path, device-resident inputs (as bench.py), CDNA against
    DNA config 2, in one process, alternating, --repeats each;
(c) Trainer.rollout_metrics frames/s, CDNA against DNA;
(d) the painted canvas (profiles/canvas/): acg_cdna_composite_canvas_fwd / _bwd among the rows of (a), in the
    same process as the entries they extend, and training steps/s of CDNA with the canvas against CDNA without, as (b).
--only picks the blocks.  --trace N: only N replayed CDNA training steps (the workload of a `rocprofv3 --kernel-trace --stats` run
of its own), with --canvas those of the generator with the canvas."""
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

HBM = 8.0e12          # B/s, spec (MI355X_MICROARCH: 6.29 TB/s measured copy)
FP32 = 157.3e12       # FLOP/s vector, spec
DEV = torch.device('cuda:0')


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def timed(fn, reps, min_s=1.0):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    n, total = 0, 0.0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while n < reps or total < min_s * 1e3:
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1)
        n += reps
    return total * 1e3 / n        # us per launch


def kernels(reps):
    lib, st = _lib.get(), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    M, k, C, sh = 10, 5, 3, 1e-12
    for B, S in ((32, 64), (256, 64), (32, 128)):
        px = B * S * S
        par = torch.randn(B, k * k * M, device=DEV)
        img = torch.rand(B, S, S, C, device=DEV) * 2 - 1
        z = torch.randn(B, S, S, M + 1, device=DEV)
        bias = torch.randn(M + 1, device=DEV)
        out, dout = torch.empty_like(img), torch.randn_like(img)
        kn, dpar, dz, db = torch.empty_like(par), torch.empty_like(par), torch.empty_like(z), torch.zeros(M + 1, device=DEV)
        nb = lib.cdna_composite_workspace_bytes(B, S, S, C, M, k)
        ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
        pieces, dpieces = torch.empty(M, B, S, S, C, device=DEV), torch.randn(M, B, S, S, C, device=DEV)
        dimg = torch.empty_like(img)
        zc, dzc = torch.randn(B, S, S, M + 2, device=DEV), torch.empty(B, S, S, M + 2, device=DEV)
        biasc, dbc = torch.randn(M + 2, device=DEV), torch.zeros(M + 2, device=DEV)
        canvas, dcanvas = torch.rand_like(img) * 2 - 1, torch.empty_like(img)
        nbc = lib.cdna_composite_canvas_workspace_bytes(B, S, S, C, M, k)
        wsc = torch.zeros(nbc, dtype=torch.uint8, device=DEV)
        nbu = lib.cdna_workspace_bytes(B, S, S, C, M, k)
        wsu = torch.zeros(nbu, dtype=torch.uint8, device=DEV)
        # algorithmic: forward reads image + M+1 logits, writes the frame; backward reads image, logits, dout, writes dlogits.
        # FLOPs: C*M*k*k FMAs per pixel (x2) for the transform, once forward and twice backward (recompute + kernel gradient)
        fl = 2.0 * px * C * M * k * k
        rows = (('composite_fwd', lambda: lib.cdna_composite_fwd(p(par), p(z), p(bias), p(img), 0, p(out), p(kn), B, S, S, C, M, k, sh, st),
                 px * 4 * (2 * C + M + 1), fl),
                ('composite_bwd', lambda: lib.cdna_composite_bwd(p(par), p(kn), p(z), p(bias), p(img), 0, p(dout), p(dpar), p(dz), p(db), 0.0,
                                                                 B, S, S, C, M, k, sh, p(ws), nb, st),
                 px * 4 * (2 * C + 2 * (M + 1)), 2 * fl),
                # the canvas: one more logit and the canvas read; backward also dcanvas written and one more dlogit
                ('canvas_fwd', lambda: lib.cdna_composite_canvas_fwd(p(par), p(zc), p(biasc), p(img), 0, p(canvas), p(out), p(kn), B, S, S, C,
                                                                     M, k, sh, st),
                 px * 4 * (3 * C + M + 2), fl),
                ('canvas_bwd', lambda: lib.cdna_composite_canvas_bwd(p(par), p(kn), p(zc), p(biasc), p(img), 0, p(canvas), p(dout), p(dpar),
                                                                     p(dzc), p(dbc), 0.0, p(dcanvas), B, S, S, C, M, k, sh, p(wsc), nbc, st),
                 px * 4 * (4 * C + 2 * (M + 2)), 2 * fl),
                ('unfused cdna_fwd', lambda: lib.cdna_fwd(p(par), p(img), p(pieces), p(kn), B, S, S, C, M, k, sh, 0, st),
                 px * 4 * C * (1 + M), fl),
                ('unfused cdna_bwd', lambda: lib.cdna_bwd(p(par), p(kn), p(img), p(dpieces), p(dpar), p(dimg), B, S, S, C, M, k, sh, 0, p(wsu), nbu, st),
                 px * 4 * C * (2 + M), 2 * fl))
        for name, fn, nbytes, flops in rows:
            us = timed(fn, reps)
            tb, tf = nbytes / HBM * 1e6, flops / FP32 * 1e6
            bound = 'HBM' if tb >= tf else 'FP32'
            print('%-17s B=%-4d %3dx%-3d %8.2f us  %7.2f MB %8.2f GFLOP  %6.0f GB/s  bound %s: %.1f%%' % (
                name, B, S, S, us, nbytes / 1e6, flops / 1e9, nbytes / us / 1e3, bound, 100 * max(tb, tf) / us), flush=True)


def _trainer(model, B=32, **kw):
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cuda:0')
    tr = T.Trainer(sess, True, 'bce', 'adam', model, batch_size=B, img_size=64, ksize=5, **kw)
    sess.run(G.global_variables_initializer())
    rng = np.random.default_rng(7)
    x = rng.uniform(-1, 1, (B, 64, 64, 3)).astype(np.float32)
    a = rng.standard_normal((B, 10)).astype(np.float32)
    s = rng.standard_normal((B, 5)).astype(np.float32)
    dev = [sess.upload(v) for v in (x, np.roll(x, 1, axis=2), a, s)]
    return sess, tr, dev


def _steps(tr, dev, n):
    x, y, a, s = dev
    for _ in range(n):
        tr.train_d(x, y, a, next_g=(x, a))
        tr.train_g(x, y, a, s, device_fetch=True)
    torch.cuda.synchronize()


def steps(repeats, n):
    runs = {m: _trainer(m) for m in ('cdna', True)}
    for sess, tr, dev in runs.values():
        _steps(tr, dev, 10)                               # eager, capture, replay
    rates = {'cdna': [], True: []}
    for _ in range(repeats):
        for m, (sess, tr, dev) in runs.items():
            t0 = time.perf_counter()
            _steps(tr, dev, n)
            rates[m].append(n / (time.perf_counter() - t0))
    for m, name in (('cdna', 'CDNA'), (True, 'DNA config 2')):
        print('train steps/s %-13s %s  median %.1f' % (name, ' '.join('%.1f' % r for r in rates[m]), float(np.median(rates[m]))))
    print('CDNA / DNA step rate: %.3f' % (np.median(rates['cdna']) / np.median(rates[True])))
    for sess, _, _ in runs.values():
        sess.close()


def steps_canvas(repeats, n):
    """CDNA with the canvas against CDNA without it: one process, alternating."""
    runs = {name: _trainer('cdna', **kw) for name, kw in (('canvas', {'canvas': True}), ('plain', {}))}
    for sess, tr, dev in runs.values():
        _steps(tr, dev, 10)
    rates = {name: [] for name in runs}
    for _ in range(repeats):
        for name, (sess, tr, dev) in runs.items():
            t0 = time.perf_counter()
            _steps(tr, dev, n)
            rates[name].append(n / (time.perf_counter() - t0))
    for name in runs:
        print('train steps/s CDNA %-7s %s  median %.1f' % (name, ' '.join('%.1f' % r for r in rates[name]), float(np.median(rates[name]))))
    print('CDNA canvas / CDNA step rate: %.3f' % (np.median(rates['canvas']) / np.median(rates['plain'])))
    for sess, _, _ in runs.values():
        sess.close()


def rollout(repeats, B=32, Tn=8):
    rng = np.random.default_rng(11)
    frames = rng.uniform(-1, 1, (B, Tn, 64, 64, 3)).astype(np.float32)
    acts = rng.standard_normal((B, Tn, 10)).astype(np.float32)
    res = {}
    for m, name in (('cdna', 'CDNA'), (True, 'DNA')):
        sess, tr, _ = _trainer(m)
        for _ in range(3):
            tr.rollout_metrics(frames, acts)
        best = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for _ in range(10):
                tr.rollout_metrics(frames, acts)
            best.append(10 * B * (Tn - 1) / (time.perf_counter() - t0))
        res[name] = float(np.median(best))
        print('rollout_metrics frames/s %-5s %s  median %.0f' % (name, ' '.join('%.0f' % r for r in best), res[name]))
        sess.close()
    print('CDNA / DNA rollout rate: %.3f' % (res['CDNA'] / res['DNA']))


BLOCKS = ['kernels', 'steps', 'rollout', 'canvas_steps']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--trace', type=int, default=0, help='only this many replayed CDNA steps (for rocprofv3)')
    ap.add_argument('--canvas', action='store_true', help='--trace: the generator with the painted canvas')
    ap.add_argument('--only', nargs='+', choices=BLOCKS, default=BLOCKS, help='the blocks to run (default: all)')
    args = ap.parse_args()
    if args.trace:
        sess, tr, dev = _trainer('cdna', **({'canvas': True} if args.canvas else {}))
        _steps(tr, dev, 10 + args.trace)
        sess.close()
        return
    if 'kernels' in args.only:
        kernels(args.reps)
    if 'steps' in args.only:
        steps(args.repeats, args.steps)
    if 'rollout' in args.only:
        rollout(args.repeats)
    if 'canvas_steps' in args.only:
        steps_canvas(args.repeats, args.steps)


if __name__ == '__main__':
    main()
