#!/usr/bin/env python
"""The convolution entries of two builds of the library in ONE process: the same plans, the same bits.

  python tools/conv_ab.py --parent-lib PATH/libacgan_hip.so [--out profiles/conv_tile/parent_vs_pr.txt]

PATH is the library of the commit to compare against, built in a worktree of its own; the other side is this tree's library.
(1) plans: acg_conv2d_workspace_bytes, _splits, _tile, _slab_layouts and _stats_layout agree for every descriptor used below, for
    the three contractions and both storages.
(2) bits: (a) every entry tests/conv_inventory.py records for c2, c3, c4, c5 and plain, replayed as tests/test_gpu_conv_inventory.py
    replays it (same seeded operands, same ABI entry, flags and accumulate value) through both libraries; (b) the conv cases of
    tests/op_cases.py at the shape lists of tests/test_gpu_ops.py (small maps, the wide kernel, the merged input gradient, pitched
    tensors, dgrad_c, the bias + activation epilogue, epilogue statistics, both slab layouts, the paired launch), run once per
    library.  Every tensor an entry leaves - outputs, statistics partials, slab workspaces with their canaries, the BatchNorm
    results computed from them - is compared byte for byte.  No tolerance: nothing that differs between the two builds touches a
    floating-point operation or the order of a sum.
Exit status 1 if anything differs; the report is written either way."""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from action_conditioned_gans_amd import _lib as L, graph as G   # noqa: E402

LINES = []


def say(line=''):
    print(line, flush=True)
    LINES.append(line)


def same_bytes(a, b):
    a, b = a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)
    return a.shape == b.shape and bool(torch.equal(a, b))


def tensors(v):
    if isinstance(v, torch.Tensor):
        return [v]
    if isinstance(v, (tuple, list)):
        return [t for x in v for t in tensors(x)]
    return []


def compare(tag, recs, tally):
    """recs: per library a list of (label, tensor)"""
    a, b = recs
    tally[0] += 1
    bad = len(a) != len(b) or any(la != lb or not same_bytes(ta, tb) for (la, ta), (lb, tb) in zip(a, b))
    if bad:
        tally[1] += 1
        where = [la for (la, ta), (lb, tb) in zip(a, b) if la != lb or not same_bytes(ta, tb)]
        say('DIFFERENT: %s: %d / %d tensors; first at %s' % (tag, len(a), len(b), where[:1]))
    return len(a)


# ---- plans
def plan_of(lib, d, which, dtype):
    rows, cols, brows, rrows = (ctypes.c_int32(0) for _ in range(4))
    out = [lib.conv2d_workspace_bytes(ctypes.byref(d), which, dtype), lib.conv2d_splits(ctypes.byref(d), which, dtype),
           lib.conv2d_tile(ctypes.byref(d), which, dtype, ctypes.byref(rows), ctypes.byref(cols)), rows.value, cols.value,
           lib.conv2d_slab_layouts(ctypes.byref(d), which, dtype) if which != L.CONV_WGRAD else 0]
    for groups in (1, 2):
        out += [lib.conv2d_stats_layout(ctypes.byref(d), which, dtype, groups, ctypes.byref(brows), ctypes.byref(rrows)), brows.value, rrows.value]
    return out


def same_plans(libs, descs):
    bad = 0
    for key in descs:
        for which in (L.CONV_FWD, L.CONV_DGRAD, L.CONV_WGRAD):
            for dtype in (L.ACG_F32, L.ACG_BF16):
                d = L.ConvDesc(*key)
                if dtype == L.ACG_BF16:
                    d.in_pitch = d.out_pitch = 0
                got = [plan_of(lib, d, which, dtype) for lib in libs]
                if got[0] != got[1]:
                    bad += 1
                    say('DIFFERENT plan: %s which %d dtype %d: %s / %s' % (key, which, dtype, got[0], got[1]))
    say('%d descriptors x 3 contractions x 2 storages: %d plans different' % (len(descs), bad))
    return bad


# ---- (a) the inventory of the benchmark's programs
def inventory_bits(libs, descs, tally):
    import pytest
    import conv_inventory as CI
    import test_gpu_conv_inventory as K
    from abi_call import Abi

    current = []

    class Recorder(K.Replay):
        """Replay with every check replaced by a record of the tensors it would have looked at."""

        def __init__(self, abi, inv):
            super().__init__(abi, inv)
            self.rec = []
            stats = abi.fwd_stats_d

            def fwd_stats_d(*a, **k):
                got = stats(*a, **k)
                self.rec += [('statistics partials', t) for t in tensors(got)]
                return got
            abi.fwd_stats_d = fwd_stats_d

        def keep(self, *ws):
            self.rec += [('workspace', w._acg_canary if hasattr(w, '_acg_canary') else w) for w in ws if w is not None]
            super().keep(*ws)

        def check_out(self, got, ref, c, n, tag, tol=None):
            self.rec.append((tag, got))

        def bitwise(self, a, b, tag):
            self.rec += [(tag, a), (tag, b)]

        def bn_fwd_ref(self, conv, bn, beta, tag, y, mean, rstd):
            self.rec += [(tag + ' bn', t) for t in (conv, y, mean, rstd)]

        def check_dw(self, dw, lay, dw0, acc, tag):
            self.rec.append((tag, dw))

    K.close = lambda got, ref, tol, tag: current[0].rec.append((tag, got))      # the module's float64 comparisons: record what was compared
    done = set()
    for cfg in CI.CONFIGS:
        mp = pytest.MonkeyPatch()
        inv, sess, tr = CI.record(mp, lambda **kw: G.Session(device='cuda:0', **kw), cfg)
        mp.undo()
        recs = [Recorder(Abi(lib, 'cuda:0', conv_dtype=inv.conv_dtype), inv) for lib in libs]
        recs[1].layers = recs[0].layers          # one set of seeded operands for both
        ran = n = 0
        for key, e in inv.entries.items():
            descs.setdefault(tuple(e['desc']))
            if key in done:
                continue
            done.add(key)
            for r in recs:
                current[:] = [r]
                r.rec = []
                r.run(e)
            torch.cuda.synchronize()
            n += compare('%s (%s)' % (CI.describe(e), cfg), [r.rec for r in recs], tally)
            ran += 1
        for program, items in inv.reduces:
            for r in recs:
                current[:] = [r]
                r.rec = []
                r.reduce_list(program, items)
            torch.cuda.synchronize()
            n += compare('%s reduce list %s' % (cfg, program), [r.rec for r in recs], tally)
        say('%-5s %3d entries (%3d replayed here), %d reduce lists, %5d tensors compared; path kinds: %s' % (
            cfg, len(inv.entries), ran, len(inv.reduces), n, ' '.join(sorted(inv.kinds()))))
        sess.close()
        del recs, sess, tr, inv
        torch.cuda.empty_cache()


# ---- (b) the conv cases of the op tests
def case_bits(libs, descs, tally):
    import op_cases as C
    import test_gpu_ops as T
    from abi_call import Abi

    plumbing = {'stream', 'empty', 'ws', 'bn_ws', 'desc', 'sync', 'to16', 'from16', 'prep_weights', 'canary_intact', 'no_timeout', 'half', 'lib',
                'device', 'conv_dtype', 'bn_flags', 'record'}

    class RecAbi(Abi):
        """Every tensor a call wrapper of tests/abi_call.py returns."""

        def __getattribute__(self, name):
            v = object.__getattribute__(self, name)
            if name.startswith('_') or name in plumbing or not callable(v):
                if name == 'desc':
                    def desc(*a, **k):
                        d = v(*a, **k)
                        descs.setdefault(tuple(d.key()))
                        return d
                    return desc
                return v

            def call(*a, **k):
                out = v(*a, **k)
                object.__getattribute__(self, 'record').extend((name, t) for t in tensors(out))
                return out
            return call

    wide = [((48, 64, 64, 64, 128, 5, 2, 'SAME'), False), ((52, 62, 62, 56, 96, 5, 2, 'SAME'), False), ((12, 64, 64, 128, 160, 5, 2, 'SAME'), False),
            ((13, 63, 61, 96, 160, 5, 2, 'SAME'), False), ((48, 32, 32, 160, 128, 3, 1, 'SAME'), False), ((12, 32, 32, 160, 128, 5, 2), True),
            ((12, 32, 32, 160, 121, 5, 2), True)]
    small = [(64, 4, 4, 256, 512, 5, 2, 'SAME'), (12, 4, 4, 24, 40, 5, 2, 'SAME'), (9, 3, 4, 16, 8, 3, 2, 'SAME'), (16, 4, 4, 6, 32, 5, 2, 'SAME'),
             (8, 2, 2, 64, 16, 3, 1, 'SAME')]
    f32 = [('conv %s' % (s,), lambda a, s=s: C.case_conv(a, s, T.TOL_CONV)) for s in C.CONV_SHAPES + small + [(32, 16, 16, 128, 128, 5, 2, 'SAME')]]
    f32 += [('deconv %s' % (s,), lambda a, s=s: C.case_deconv(a, s, T.TOL_CONV)) for s in C.DECONV_SHAPES + [(32, 2, 2, 64, 32, 5, 2), (8, 2, 1, 16, 12, 5, 2)]]
    f32 += [('merged input gradient', lambda a: C.case_merged_dgrad(a, T.TOL_CONV)), ('dgrad_c', lambda a: C.case_dgrad_channel_limit(a, T.TOL_CONV)),
            ('dgrad_c, split', lambda a: C.case_dgrad_limit_split_reduction(a, T.TOL_CONV)), ('conv pitched', lambda a: C.case_conv_pitched(a, T.TOL_CONV)),
            ('deconv pitched', lambda a: C.case_deconv_pitched(a, T.TOL_CONV)), ('bias + activation epilogue', lambda a: C.case_deconv_bias_act(a, T.TOL_CONV)),
            ('epilogue statistics', lambda a: C.case_conv_bn_stats(a, T.TOL_CONV, 1e-4, min_fused=4)), ('slab hand-off layouts', lambda a: C.case_slab_handoff(a, 2e-5))]
    b16 = [('conv %s' % (s,), lambda a, s=s: C.case_conv_bf16(a, s, T.TOL_BF16, T.TOL_CONV)) for s in C.CONV_SHAPES + [(32, 64, 64, 64, 128, 5, 2, 'SAME')]]
    b16 += [('deconv %s' % (s,), lambda a, s=s: C.case_conv_bf16(a, s, T.TOL_BF16, T.TOL_CONV, transposed=True)) for s in C.DECONV_SHAPES]
    b16 += [('wide kernel %s' % (s,), lambda a, s=s, t=t: C.case_conv_bf16(a, s, T.TOL_BF16, T.TOL_CONV, transposed=t)) for s, t in wide]
    b16 += [('merged input gradient', lambda a: C.case_merged_dgrad(a, T.TOL_BF16)), ('dgrad_c', lambda a: C.case_dgrad_channel_limit(a, T.TOL_BF16)),
            ('dgrad_c, split', lambda a: C.case_dgrad_limit_split_reduction(a, T.TOL_BF16)), ('bias + activation epilogue', lambda a: C.case_deconv_bias_act(a, T.TOL_CONV)),
            ('epilogue statistics', lambda a: C.case_conv_bn_stats(a, T.TOL_BF16, 2e-3, min_fused=4)),
            ('epilogue statistics, wide kernel', lambda a: C.case_conv_bn_stats(a, T.TOL_BF16, 2e-3, min_fused=3, layers=C.STATS_LAYERS_WIDE)),
            ('slab hand-off layouts', lambda a: C.case_slab_handoff(a, 2e-5, min_rows=1)), ('paired launch', lambda a: C.case_bwd_pair_bf16(a, T.TOL_BF16, T.TOL_CONV)),
            ('float32 head', lambda a: C.case_head_f32_in_bf16_network(a, T.TOL_CONV, 6e-3))]
    for storage, dtype, cases in (('f32', L.ACG_F32, f32), ('bf16', L.ACG_BF16, b16)):
        n = 0
        for tag, fn in cases:
            recs = []
            for lib in libs:
                abi = RecAbi(lib, 'cuda:0', conv_dtype=dtype)
                object.__setattr__(abi, 'record', [])
                fn(abi)
                torch.cuda.synchronize()
                recs.append(abi.record)
            n += compare('%s %s' % (storage, tag), recs, tally)
            del recs
            torch.cuda.empty_cache()
        say('%-5s %3d cases of tests/op_cases.py, %5d tensors compared' % (storage, len(cases), n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', required=True, metavar='PATH', help="the parent commit's libacgan_hip.so")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_tile', 'parent_vs_pr.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('conv_ab.py compares on a GPU: none is visible')
    libs = [L.Library(args.parent_lib, require=tuple(L.EXTENSIONS)), L.get()]
    say('device: %s; parent / pr = %s / %s' % (torch.cuda.get_device_name(0), os.path.basename(args.parent_lib) + ' of the parent commit', os.path.relpath(libs[1].path, ROOT)))
    descs, tally = {}, [0, 0]
    say('## bits: every tensor byte-identical between the two libraries')
    inventory_bits(libs, descs, tally)
    case_bits(libs, descs, tally)
    say('%d comparisons, %d different' % tuple(tally))
    say('## plans: workspace bytes, splits, tile, slab layouts, statistics layout')
    bad = tally[1] + same_plans(libs, descs)
    say('%s' % ('all checks met' if not bad else '%d checks NOT met' % bad))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(LINES) + '\n')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
