#!/usr/bin/env python
"""The six CDNA entries of two builds of the library in ONE process: the same workspaces, the same bits, the same speed.

  python tools/cdna_ab.py --parent-lib PATH/libacgan_hip.so [--rounds 9] [--out profiles/cdna_common/parent_vs_pr.txt]

PATH is the library of the commit to compare against, built in a worktree of its own; the other side is this tree's library
(the protocol of tools/ssim_ab.py).
(1) plans: acg_cdna_workspace_bytes and acg_cdna_composite_workspace_bytes agree at every shape of tests/test_gpu_cdna.py::SHAPES
    and at the unfused mask-chunk shape of tests/test_gpu_ops.py::test_cdna.
(2) bits: at those shapes, on inputs seeded on the CPU and outputs pre-filled with NaN: acg_cdna_fwd (pieces, kern_norm),
    acg_cdna_bwd (dparams, dimage), acg_cdna_composite_fwd (frame, kern_norm), acg_cdna_composite_bwd (dparams, dlogits, dbias
    with accumulate 0 and then 1): every tensor torch.equal.  No tolerance.
(3) speed: the kernel cases of tools/bench_cdna.py, each entry captured N times into a HIP graph; the two libraries' graphs
    take turns inside every round, in alternating order; medians per library.  REQUIREMENT: this tree's median exceeds the
    parent's by no more than the spread (max - min) of the parent's own rounds in this run.
Exit status 1 if a check fails; the report is written either way."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from action_conditioned_gans_amd import _lib   # noqa: E402

DEV = 'cuda:0'
SHIFT = 1e-12
CHUNKED = (2, 17, 33, 4, 29, 7)                # the unfused backward's mask chunks with a remainder
SPEED_SHAPES = [(32, 64, 64, 3, 10, 5), (256, 64, 64, 3, 10, 5), (32, 128, 128, 3, 10, 5)]
LINES = []


def say(line=''):
    print(line, flush=True)
    LINES.append(line)


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def nan(*shape):
    return torch.full(shape, float('nan'), device=DEV)


def entries(lib, shape, params, z, bias, img, dout, dpieces):
    """name -> (call(stream), outputs) of the four launching entries on NaN-filled outputs of this library's own."""
    b, h, w, c, m, k = shape
    nbu, nbc = lib.cdna_workspace_bytes(b, h, w, c, m, k), lib.cdna_composite_workspace_bytes(b, h, w, c, m, k)
    wsu, wsc = torch.zeros(nbu, dtype=torch.uint8, device=DEV), torch.zeros(nbc, dtype=torch.uint8, device=DEV)
    pieces, knu, dparu, dimg = nan(m, b, h, w, c), nan(b, k * k * m), nan(b, k * k * m), nan(b, h, w, c)
    frame, knc, dparc, dz, db = nan(b, h, w, c), nan(b, k * k * m), nan(b, k * k * m), nan(b, h, w, m + 1), nan(m + 1)
    return {
        'cdna_fwd': (lambda st: lib.cdna_fwd(p(params), p(img), p(pieces), p(knu), b, h, w, c, m, k, SHIFT, _lib.ACG_F32, st),
                     {'pieces': pieces, 'kern_norm': knu}),
        'cdna_bwd': (lambda st: lib.cdna_bwd(p(params), p(knu), p(img), p(dpieces), p(dparu), p(dimg), b, h, w, c, m, k, SHIFT,
                                          _lib.ACG_F32, p(wsu), nbu, st),
                     {'dparams': dparu, 'dimage': dimg}),
        'cdna_composite_fwd': (lambda st: lib.cdna_composite_fwd(p(params), p(z), p(bias), p(img), 0, p(frame), p(knc), b, h, w, c, m, k, SHIFT, st),
                               {'frame': frame, 'kern_norm': knc}),
        'cdna_composite_bwd': (lambda st, acc=0.0: lib.cdna_composite_bwd(p(params), p(knc), p(z), p(bias), p(img), 0, p(dout), p(dparc), p(dz), p(db),
                                                                      acc, b, h, w, c, m, k, SHIFT, p(wsc), nbc, st),
                               {'dparams': dparc, 'dlogits': dz, 'dbias': db}),
    }


def same_plans(libs, shapes):
    bad = 0
    for s in shapes:
        got = [(lib.cdna_workspace_bytes(*s), lib.cdna_composite_workspace_bytes(*s)) for lib in libs]
        bad += got[0] != got[1]
        say('%-26s cdna %9d / %9d   cdna_composite %9d / %9d   %s' % (s, got[0][0], got[1][0], got[0][1], got[1][1],
                                                                    'equal' if got[0] == got[1] else 'DIFFERENT'))
    return bad


def same_bits(libs, shapes):
    import test_gpu_cdna as K
    cases = bad = 0
    for shape in shapes:
        b, h, w, c, m, k = shape
        params, z, bias, img, dout = (t.to(DEV) for t in K._case(shape, seed=1))
        dpieces = torch.randn(m, b, h, w, c, generator=torch.Generator().manual_seed(2)).to(DEV)
        sides = [entries(lib, shape, params, z, bias, img, dout, dpieces) for lib in libs]
        for name in sides[0]:
            for acc in ((0.0, 1.0) if name == 'cdna_composite_bwd' else (None,)):
                for side in sides:
                    side[name][0](stream()) if acc is None else side[name][0](stream(), acc)
                torch.cuda.synchronize()
                for out in sides[0][name][1]:
                    cases += 1
                    if not torch.equal(sides[0][name][1][out], sides[1][name][1][out]):
                        bad += 1
                        say('DIFFERENT: %s %s %s%s' % (shape, name, out, '' if acc is None else ' accumulate %g' % acc))
    say('%d tensors at %d shapes, %d different' % (cases, len(shapes), bad))
    return bad


def graph_of(fn, n_graph):
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        st = stream()
        for _ in range(n_graph):
            fn(st)
    gr.replay()
    torch.cuda.synchronize()
    return gr


def same_speed(libs, rounds, n_graph):
    bad = 0
    for shape in SPEED_SHAPES:
        b, h, w, c, m, k = shape
        g = torch.Generator(device=DEV).manual_seed(0)
        params = torch.randn(b, k * k * m, device=DEV, generator=g)
        img = torch.rand(b, h, w, c, device=DEV, generator=g) * 2 - 1
        z, bias = torch.randn(b, h, w, m + 1, device=DEV, generator=g), torch.randn(m + 1, device=DEV, generator=g)
        dout, dpieces = torch.randn(b, h, w, c, device=DEV, generator=g), torch.randn(m, b, h, w, c, device=DEV, generator=g)
        sides = {label: entries(lib, shape, params, z, bias, img, dout, dpieces) for label, lib in zip(('parent', 'pr'), libs)}
        for name in sides['pr']:                      # forwards first: they leave the kern_norm the backwards read
            graphs = {label: graph_of(side[name][0], n_graph) for label, side in sides.items()}
            times = {label: [] for label in graphs}
            for r in range(-1, rounds):               # round -1 warms both graphs up and is not kept
                for label in (('parent', 'pr') if r % 2 == 0 else ('pr', 'parent')):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    graphs[label].replay()
                    e1.record()
                    torch.cuda.synchronize()
                    if r >= 0:
                        times[label].append(e0.elapsed_time(e1) * 1e3 / n_graph)
            med = {label: float(np.median(v)) for label, v in times.items()}
            spread = max(times['parent']) - min(times['parent'])
            ok = med['pr'] <= med['parent'] + spread
            bad += not ok
            say('# acg_%s %s; us per call (HIP graph of %d calls), one column per round' % (name, shape, n_graph))
            for label in ('parent', 'pr'):
                say('%-8s %s   median %.3f' % (label, ' '.join('%.3f' % t for t in times[label]), med[label]))
            say('REQUIREMENT pr median <= parent median + parent spread: %.3f <= %.3f + %.3f: %s' % (
                med['pr'], med['parent'], spread, 'met' if ok else 'NOT met'))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', required=True, metavar='PATH', help="the parent commit's libacgan_hip.so")
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--n-graph', type=int, default=100, help='launches captured into one graph')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cdna_common', 'parent_vs_pr.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('cdna_ab.py compares on a GPU: none is visible')
    if args.rounds < 7:
        raise SystemExit('at least 7 rounds')
    import test_gpu_cdna
    shapes = test_gpu_cdna.SHAPES + [CHUNKED]
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
