#!/usr/bin/env python
"""Affine (STP) generator measurements.

(a) acg_affine_composite_fwd / _bwd at (32, 64^2) and (32, 128^2), M = 10, C = 3, beside acg_cdna_composite_fwd / _bwd at k = 5
    in the same process: device events around back-to-back launches (warm-up first; at least --reps launches and at least
    --min_s per block) and the algorithmic bytes.  The transforms are drawn as the tests draw them: 'near' the identity (the trained
    case) and 'wide' (8 x the spread: scattered taps, many of them - and some whole masks - outside the image);
(b) with --steps N > 0: training steps/s at batch 32, 64^2, bce, Adam, look-ahead call path, device-resident inputs, the affine
    generator against the CDNA generator, alternating, --repeats each;
(c) the painted canvas (profiles/canvas/): acg_affine_composite_canvas_fwd / _bwd and acg_cdna_composite_canvas_fwd / _bwd among
    the rows of (a), and with --canvas_steps N > 0 training steps/s of the affine generator with the canvas against the one without.
--trace N: only N replayed affine training steps with the canvas (the workload of a `rocprofv3 --kernel-trace --stats` run)."""
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

DEV = torch.device('cuda:0')
PARAM_SCALE = (.15, .15, .25, .15, .15, .25)


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def timed(fn, reps, min_s):
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


def kernels(reps, min_s):
    lib, st = _lib.get(), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    M, k, C, sh = 10, 5, 3, 1e-12
    gen = torch.Generator().manual_seed(0)
    for B, S in ((32, 64), (32, 128)):
        px = B * S * S
        theta = torch.randn(B, M, 6, generator=gen) * torch.tensor(PARAM_SCALE)
        near, wide = theta.reshape(B, M * 6).to(DEV), (8 * theta).reshape(B, M * 6).to(DEV)
        par = torch.randn(B, k * k * M, device=DEV)
        img = torch.rand(B, S, S, C, device=DEV) * 2 - 1
        z = torch.randn(B, S, S, M + 1, device=DEV)
        bias = torch.randn(M + 1, device=DEV)
        out, dout = torch.empty_like(img), torch.randn_like(img)
        kn, dpar, dz, db = torch.empty_like(par), torch.empty_like(par), torch.empty_like(z), torch.zeros(M + 1, device=DEV)
        dth = torch.empty_like(near)
        nb = lib.cdna_composite_workspace_bytes(B, S, S, C, M, k)
        ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
        nba = lib.affine_composite_workspace_bytes(B, S, S, C, M)
        wsa = torch.zeros(nba, dtype=torch.uint8, device=DEV)
        zc, dzc = torch.randn(B, S, S, M + 2, device=DEV), torch.empty(B, S, S, M + 2, device=DEV)
        biasc, dbc = torch.randn(M + 2, device=DEV), torch.zeros(M + 2, device=DEV)
        canvas, dcanvas = torch.rand_like(img) * 2 - 1, torch.empty_like(img)
        nbc = lib.cdna_composite_canvas_workspace_bytes(B, S, S, C, M, k)
        wsc = torch.zeros(nbc, dtype=torch.uint8, device=DEV)
        nbac = lib.affine_composite_canvas_workspace_bytes(B, S, S, C, M)
        wsac = torch.zeros(nbac, dtype=torch.uint8, device=DEV)
        # algorithmic bytes: forward reads image + M+1 logits, writes the frame; backward reads image, logits, dout, writes dlogits;
        # the canvas adds one logit and the canvas read, backward also dcanvas and one more dlogit
        fb, bb = px * 4 * (2 * C + M + 1), px * 4 * (2 * C + 2 * (M + 1))
        fbc, bbc = px * 4 * (3 * C + M + 2), px * 4 * (4 * C + 2 * (M + 2))
        lib.cdna_composite_fwd(p(par), p(z), p(bias), p(img), 0, p(out), p(kn), B, S, S, C, M, k, sh, st)
        rows = [('cdna_composite_fwd k=5', lambda: lib.cdna_composite_fwd(p(par), p(z), p(bias), p(img), 0, p(out), p(kn), B, S, S, C, M, k, sh, st), fb),
                ('cdna_composite_bwd k=5', lambda: lib.cdna_composite_bwd(p(par), p(kn), p(z), p(bias), p(img), 0, p(dout), p(dpar), p(dz), p(db), 0.0,
                                                                          B, S, S, C, M, k, sh, p(ws), nb, st), bb),
                ('cdna_canvas_fwd k=5', lambda: lib.cdna_composite_canvas_fwd(p(par), p(zc), p(biasc), p(img), 0, p(canvas), p(out), p(kn),
                                                                              B, S, S, C, M, k, sh, st), fbc),
                ('cdna_canvas_bwd k=5', lambda: lib.cdna_composite_canvas_bwd(p(par), p(kn), p(zc), p(biasc), p(img), 0, p(canvas), p(dout),
                                                                              p(dpar), p(dzc), p(dbc), 0.0, p(dcanvas), B, S, S, C, M, k, sh,
                                                                              p(wsc), nbc, st), bbc)]
        for name, th in (('near', near), ('wide', wide)):
            rows += [('affine_composite_fwd %s' % name,
                      lambda th=th: lib.affine_composite_fwd(p(th), p(z), p(bias), p(img), 0, p(out), B, S, S, C, M, st), fb),
                     ('affine_composite_bwd %s' % name,
                      lambda th=th: lib.affine_composite_bwd(p(th), p(z), p(bias), p(img), 0, p(dout), p(dth), p(dz), p(db), 0.0, B, S, S, C, M,
                                                             p(wsa), nba, st), bb),
                     ('affine_canvas_fwd %s' % name,
                      lambda th=th: lib.affine_composite_canvas_fwd(p(th), p(zc), p(biasc), p(img), 0, p(canvas), p(out), B, S, S, C, M, st), fbc),
                     ('affine_canvas_bwd %s' % name,
                      lambda th=th: lib.affine_composite_canvas_bwd(p(th), p(zc), p(biasc), p(img), 0, p(canvas), p(dout), p(dth), p(dzc), p(dbc),
                                                                    0.0, p(dcanvas), B, S, S, C, M, p(wsac), nbac, st), bbc)]
        for name, fn, nbytes in rows:
            us = timed(fn, reps, min_s)
            print('%-26s B=%-3d %3dx%-3d %8.2f us  %7.2f MB  %6.0f GB/s' % (name, B, S, S, us, nbytes / 1e6, nbytes / us / 1e3), flush=True)


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


def steps(repeats, n, canvas=False):
    """affine against CDNA; ``canvas``: affine with the canvas against affine without."""
    if canvas:
        runs = {'affine canvas': _trainer('affine', canvas=True), 'affine': _trainer('affine')}
    else:
        runs = {m: _trainer(m) for m in ('affine', 'cdna')}
    for sess, tr, dev in runs.values():
        _steps(tr, dev, 10)                               # eager, capture, replay
    rates = {m: [] for m in runs}
    for _ in range(repeats):
        for m, (sess, tr, dev) in runs.items():
            t0 = time.perf_counter()
            _steps(tr, dev, n)
            rates[m].append(n / (time.perf_counter() - t0))
    for m in runs:
        print('train steps/s %-13s %s  median %.1f' % (m, ' '.join('%.1f' % r for r in rates[m]), float(np.median(rates[m]))))
    first, second = list(runs)
    print('%s / %s step rate: %.3f' % (first, 'CDNA' if second == 'cdna' else second, np.median(rates[first]) / np.median(rates[second])))
    for sess, _, _ in runs.values():
        sess.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--min_s', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--steps', type=int, default=0, help='also time this many training steps per repeat (0: kernels only)')
    ap.add_argument('--canvas_steps', type=int, default=0, help='also time this many steps per repeat with and without the canvas')
    ap.add_argument('--no_kernels', action='store_true', help='skip the kernel block')
    ap.add_argument('--trace', type=int, default=0, help='only this many replayed affine steps with the canvas (for rocprofv3)')
    args = ap.parse_args()
    if args.trace:
        sess, tr, dev = _trainer('affine', canvas=True)
        _steps(tr, dev, 10 + args.trace)
        sess.close()
        return
    if not args.no_kernels:
        kernels(args.reps, args.min_s)
    if args.steps:
        steps(args.repeats, args.steps)
    if args.canvas_steps:
        steps(args.repeats, args.canvas_steps, canvas=True)


if __name__ == '__main__':
    main()
