#!/usr/bin/env python
"""acg_frame_metrics and acg_ssim_loss of two builds of the library in ONE process: the same plans, the same bits, the same speed.

  python tools/ssim_ab.py --parent-lib PATH/libacgan_hip.so [--rounds 9] [--out profiles/ssim_window/parent_vs_pr.txt]

PATH is the library of the commit to compare against, built in a worktree of its own; the other side is this tree's library.
(1) plans: both workspace queries agree at every shape of tests/test_gpu_eval.py::SHAPES and tests/test_gpu_ssim_loss.py::SHAPES.
(2) bits: at those shapes acg_frame_metrics on 'uniform' and 'noise' inputs in f32, bf16 and both mixed storages, at pitch C and
    pitch 4, and acg_ssim_loss value-only, gradient-only and both on 'uniform' and 'near_identical' inputs: every output tensor
    torch.equal.  No tolerance.
(3) speed: each launch captured N times into a HIP graph (as tools/bench_ssim_loss.py does it); the two libraries' graphs take
    turns inside every round, in alternating order; medians per library.  REQUIREMENT: this tree's median exceeds the parent's by
    no more than the spread (max - min) of the parent's own rounds in this run.
Exit status 1 if a check fails; the report is written either way."""
import argparse
import ctypes
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from action_conditioned_gans_amd import _lib, metrics as M   # noqa: E402
from action_conditioned_gans_amd.ops import SSIM_DATA_RANGE, SSIM_K1, SSIM_K2   # noqa: E402

DEV = 'cuda:0'
LINES = []
SPEED_CASES = [('acg_frame_metrics', (224, 64, 64, 3)), ('acg_frame_metrics', (224, 128, 128, 3)),
               ('acg_ssim_loss grad', (32, 64, 64, 3)), ('acg_ssim_loss grad', (32, 128, 128, 3))]


def say(line=''):
    print(line, flush=True)
    LINES.append(line)


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ssim_loss(lib, x, y, value, grad, stream=None):
    """One acg_ssim_loss call on NaN-filled outputs -> (value or None, dpred or None)."""
    n, h, w, c = x.shape
    nb = lib.ssim_loss_workspace_bytes(n, h, w, c)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    val = torch.full((1,), float('nan'), device=DEV) if value else None
    dp = torch.full_like(x, float('nan')) if grad else None
    lib.ssim_loss(p(x), p(y), p(val), p(dp), 1.0, n, h, w, c, SSIM_DATA_RANGE, SSIM_K1, SSIM_K2, p(ws), nb,
                  stream or ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return val, dp


def same_plans(libs, shapes):
    bad = 0
    for n, h, w, c in shapes:
        got = [(lib.frame_metrics_workspace_bytes(n, h, w), lib.ssim_loss_workspace_bytes(n, h, w, c)) for lib in libs]
        bad += got[0] != got[1]
        say('%-20s frame_metrics %9d / %9d   ssim_loss %10d / %10d   %s' % ((n, h, w, c), got[0][0], got[1][0], got[0][1], got[1][1],
                                                                             'equal' if got[0] == got[1] else 'DIFFERENT'))
    return bad


def same_bits(libs, shapes):
    import ssim_loss_ref as R
    import test_gpu_eval as K
    cases = bad = 0

    def compare(tag, outs):
        nonlocal cases, bad
        cases += 1
        torch.cuda.synchronize()
        if not all(torch.equal(a, b) for a, b in zip(*outs)):
            bad += 1
            say('DIFFERENT: %s' % (tag,))

    for shape in shapes:
        c = shape[-1]
        for kind in ('uniform', 'noise'):
            x, y = K._inputs(kind, shape, np.random.default_rng(zlib.crc32(repr((shape, kind)).encode())))
            for storage, (ta, tb) in K.STORAGE.items():
                a, b = K._stored(x, ta), K._stored(y, tb)
                for pitch in sorted({c, 4}):
                    pad = lambda t: torch.cat([t, torch.zeros(t.shape[:-1] + (pitch - c,), dtype=t.dtype, device=t.device)], dim=-1).contiguous()   # noqa: E731
                    compare(('frame_metrics', shape, kind, storage, pitch), [M.frame_metrics(pad(a), pad(b), channels=c, lib=lib) for lib in libs])
        for kind in ('uniform', 'near_identical'):
            xh, yh = R.case(kind, shape, seed=sum(shape))
            x, y = torch.from_numpy(np.ascontiguousarray(xh)).to(DEV), torch.from_numpy(np.ascontiguousarray(yh)).to(DEV)
            for call, (value, grad) in (('value', (True, False)), ('gradient', (False, True)), ('both', (True, True))):
                compare(('ssim_loss', shape, kind, call), [[t for t in ssim_loss(lib, x, y, value, grad) if t is not None] for lib in libs])
    say('%d cases, %d different' % (cases, bad))
    return bad


def graph_of(fn, n_graph):
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for _ in range(n_graph):
            fn(sp)
    gr.replay()
    torch.cuda.synchronize()
    return gr


def same_speed(libs, rounds, n_graph):
    bad = 0
    for entry, shape in SPEED_CASES:
        n, h, w, c = shape
        g = torch.Generator(device=DEV).manual_seed(0)
        x = torch.rand(*shape, device=DEV, generator=g) * 2 - 1
        y = (x + 0.1 * torch.randn(*shape, device=DEV, generator=g)).clamp(-1, 1)
        graphs, keep = {}, []
        for label, lib in zip(('parent', 'pr'), libs):
            if entry == 'acg_frame_metrics':
                nb = lib.frame_metrics_workspace_bytes(n, h, w)
                ws, ssim, sq = torch.zeros(nb, dtype=torch.uint8, device=DEV), torch.empty(n, device=DEV), torch.empty(n, device=DEV)
                fn = lambda s, lib=lib, ws=ws, ssim=ssim, sq=sq, nb=nb: lib.frame_metrics(   # noqa: E731
                    p(x), p(y), p(ssim), p(sq), n, h, w, c, 0, _lib.ACG_F32, SSIM_DATA_RANGE, SSIM_K1, SSIM_K2, p(ws), nb, s)
            else:
                nb = lib.ssim_loss_workspace_bytes(n, h, w, c)
                ws, dp = torch.zeros(nb, dtype=torch.uint8, device=DEV), torch.empty_like(x)
                fn = lambda s, lib=lib, ws=ws, dp=dp, nb=nb: lib.ssim_loss(   # noqa: E731
                    p(x), p(y), None, p(dp), 1.0, n, h, w, c, SSIM_DATA_RANGE, SSIM_K1, SSIM_K2, p(ws), nb, s)
            keep.append((ws, fn))
            graphs[label] = graph_of(fn, n_graph)
        times = {k: [] for k in graphs}
        for r in range(-1, rounds):                       # round -1 warms both graphs up and is not kept
            for label in (('parent', 'pr') if r % 2 == 0 else ('pr', 'parent')):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graphs[label].replay()
                e1.record()
                torch.cuda.synchronize()
                if r >= 0:
                    times[label].append(e0.elapsed_time(e1) * 1e3 / n_graph)
        med = {k: float(np.median(v)) for k, v in times.items()}
        spread = max(times['parent']) - min(times['parent'])
        ok = med['pr'] <= med['parent'] + spread
        bad += not ok
        say('# %s %s; us per call (HIP graph of %d calls), one column per round' % (entry, shape, n_graph))
        for label in ('parent', 'pr'):
            say('%-8s %s   median %.3f' % (label, ' '.join('%.3f' % t for t in times[label]), med[label]))
        say('REQUIREMENT pr median <= parent median + parent spread: %.3f <= %.3f + %.3f: %s' % (med['pr'], med['parent'], spread, 'met' if ok else 'NOT met'))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', required=True, metavar='PATH', help="the parent commit's libacgan_hip.so")
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--n-graph', type=int, default=200, help='launches captured into one graph')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ssim_window', 'parent_vs_pr.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ssim_ab.py compares on a GPU: none is visible')
    if args.rounds < 7:
        raise SystemExit('at least 7 rounds')
    import test_gpu_eval
    import test_gpu_ssim_loss
    shapes = list(dict.fromkeys(test_gpu_eval.SHAPES + test_gpu_ssim_loss.SHAPES))
    libs = [_lib.Library(args.parent_lib, require=tuple(_lib.EXTENSIONS)), _lib.get()]
    say('device: %s; parent / pr = %s / %s' % (torch.cuda.get_device_name(0), os.path.basename(args.parent_lib), os.path.basename(libs[1].path)))
    say('## plans: workspace bytes, parent / pr')
    bad = same_plans(libs, shapes)
    say('## bits: every output tensor torch.equal between the two libraries')
    bad += same_bits(libs, shapes)
    say('## speed: %d rounds, the two graphs taking turns' % args.rounds)
    bad += same_speed(libs, args.rounds, args.n_graph)
    say('%s' % ('all checks met' if not bad else '%d checks NOT met' % bad))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(LINES) + '\n')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
