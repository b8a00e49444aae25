#!/usr/bin/env python
"""Measurements of training through K-step rollouts (profiles/rollout/).

(a) acg_dna_bwd_image at (32, 64^2, k=5) and (32, 128^2, k=11), next to acg_dna_bwd (dlogits + dbias) at the same shapes: device
    events around back-to-back launches (warm-up first; at least --reps launches and at least 1 s per block), algorithmic bytes
    and the fraction of the HBM peak;
(b) G-step time at config 2's shape (batch 32, 64^2, DNA k = 5, bce, Adam, float32) for K = 1..4: K = 1 is Trainer.train_g on
    the plain call path, K > 1 Trainer.train_g_rollout; host inputs, --steps replayed steps after warm-up, one process."""
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
    C = 3
    for B, S, k in ((32, 64, 5), (32, 128, 11)):
        kk, px = k * k, B * S * S
        z = torch.randn(B, S, S, kk, device=DEV)
        bias = torch.randn(kk, device=DEV)
        img, dout = torch.rand(B, S, S, C, device=DEV), torch.randn(B, S, S, C, device=DEV)
        dimg, dz, db = torch.empty_like(img), torch.empty_like(z), torch.zeros(kk, device=DEV)
        wsb = lib.dna_workspace_bytes(B, S, S, k)
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        t_img = timed(lambda: lib.dna_bwd_image(p(z), p(bias), p(dout), None, 0, 0, 0, p(dimg), 0.0, B, S, S, C, k, _lib.ACG_F32, st), reps)
        t_bwd = timed(lambda: lib.dna_bwd(p(z), p(bias), p(img), p(dout), None, 0, 0, 0, p(dz), p(db), 0.0, B, S, S, C, k, _lib.ACG_F32,
                                          p(ws), wsb, st), reps)
        by_img = px * (kk + 2 * C) * 4               # logits once, dout, dimage
        by_bwd = px * (2 * kk + 2 * C) * 4           # logits, dlogits, image, dout
        print('(%d, %d^2, k=%d)  dna_bwd_image %8.1f us  %6.1f MB  %5.2f TB/s = %4.1f %% of HBM peak   |   dna_bwd %8.1f us  %6.1f MB  '
              '%5.2f TB/s = %4.1f %%' % (B, S, k, t_img, by_img / 1e6, by_img / t_img / 1e6, 100 * by_img / t_img / 1e6 / (HBM / 1e12),
                                          t_bwd, by_bwd / 1e6, by_bwd / t_bwd / 1e6, 100 * by_bwd / t_bwd / 1e6 / (HBM / 1e12)), flush=True)


def g_steps(steps, warmup, ks):
    B, S = 32, 64
    rng = np.random.default_rng(0)
    base = {}
    for K in ks:
        G.reset_default_graph()
        optim.set_data_parallel(1)
        sess = G.Session(device='cuda:0')
        tr = T.Trainer(sess, True, 'bce', 'adam', True, batch_size=B, img_size=S, ksize=5, lookahead=False, rollout_steps=K)
        sess.run(G.global_variables_initializer())
        x = rng.uniform(-1, 1, (B, K + 1, S, S, 3)).astype(np.float32)
        a = rng.standard_normal((B, K, 10)).astype(np.float32)
        s = rng.standard_normal((B, K, 5)).astype(np.float32)
        xs, xn, a0, s0 = np.ascontiguousarray(x[:, 0]), np.ascontiguousarray(x[:, 1]), np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(s[:, 0])
        step = (lambda: tr.train_g(xs, xn, a0, s0, device_fetch=True)) if K == 1 else (lambda: tr.train_g_rollout(x, a, s, device_fetch=True))
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        base.setdefault(1, ms)
        print('K=%d  G step %7.3f ms  = %.2f x the K=1 step (K x: %.2f)' % (K, ms, ms / base[1], ms / base[1] / K), flush=True)
        sess.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--ks', type=str, default='1,2,3,4')
    args = ap.parse_args()
    print('MI355X, %s' % torch.cuda.get_device_name(0), flush=True)
    kernels(args.reps)
    g_steps(args.steps, args.warmup, [int(v) for v in args.ks.split(',')])


if __name__ == '__main__':
    main()
