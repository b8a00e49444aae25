"""GPU checks of the transposed LDS stores of the fp32 MFMA convolution (conv_f32_kernel.h: put_part).

A 64-wide tile stores a transposed half quad with one two-dword LDS write issued from inline assembly, which the compiler's wait
counting does not see; an explicit wait orders those stores before the barrier that publishes the buffer.  The stores put the same
values into the same slots as before, so every case holds, for each contraction it lists and with the uniform_k / uniform_w
loaders switched on and off (the generic, LIN, UK, UW and ragged instantiations all store through put_part):
  * its premise out of acg_conv2d_path / acg_conv2d_pair_path - tile, LIN, ragged, compact, splits, the variant - as a failure,
    never a skip (conv_path_cases.HOW says what to do when the planner has moved a shape);
  * the result against the float64 reference of tests/conv_path_cases.py at the project's bar TOL_CONV, as it is;
  * TWO runs of the same launch into sentinel-filled outputs, bit for bit, workspace (split-K slabs) included: a store that
    is not ordered before the barrier shows up as a run-to-run difference;
  * for the paired launch: bit-equal to the separate entries (conv_path_cases.Runner.pair), and two runs bit for bit.

Shapes are the smallest that reach each instantiation; most are the cases of test_gpu_conv_wgrad_uniform.py / test_gpu_conv_uniform_k.py.
The 128x32 weight gradient (whole-quad stores on its gathered side, single dwords on its dense side) is here as the neighbour
whose stores did not change."""
import collections
import ctypes

import pytest
import torch

import conv_path_cases as P
from action_conditioned_gans_amd import _lib as L

pytestmark = pytest.mark.gpu

# expect: contraction -> (tile, path-string words that must be present, uniform_k, uniform_w) with the variants ON; with them off
# the plan must be the same and both variants 0.  pair: (tile of A, uniform_k of A) or None.
Case = collections.namedtuple('Case', 'name why desc transposed expect pair')


def case(name, why, desc, expect, transposed=False, pair=None):
    return Case(name, why, desc, transposed, expect, pair)


W64, N128 = (64, 64), (128, 32)

CASES = [
    case('wgrad_14_steps', '14 x 64 x 64 pixels, 4 -> 36 channels, 2 x 2: one 64x64 tile, 1792 K-steps over 128 splits = 14 per split: every unrolled copy, '
         'both row-table halves, dead steps in the last round; 16 of the 64 rows and 36 of the 64 columns exist',
         P._sq(14, 64, 64, 4, 36, 2, 1), dict(wgrad=(W64, (), 0, 1))),
    case('wgrad_13_steps_narrow', '13 x 64 x 64 pixels, 4 -> 24 channels, 3 x 3: one 128x32 tile, 13 K-steps per split (the unchanged neighbour)',
         P._sq(13, 64, 64, 4, 24, 3, 1), dict(wgrad=(N128, (), 0, 1))),
    case('partial_tiles', '126 pixels, 32 -> 40 channels: N = 40 < 64 (masked columns on the dense side of both contractions), 288 rows = 4.5 row tiles of the '
         'weight gradient, 126 rows = 2 partial row tiles of the forward; FWD LIN with uniform_k on and off',
         P._sq(2, 9, 7, 32, 40, 3, 1), dict(fwd=(W64, ('lin',), 1, 0), wgrad=(W64, (), 0, 1))),
    case('ragged_25', '25 gathered channels: the ragged 64x64 instantiations of the forward and of the weight gradient (quads at the end of a tap are partial)',
         P._sq(2, 9, 7, 25, 40, 3, 1), dict(fwd=(W64, ('ragged',), 0, 0), wgrad=(W64, ('ragged',), 0, 0))),
    case('channels_36_pair', '36 gathered channels, a multiple of 4 and not of 32: FWD LIN whose uniform_k rule declines; DGRAD + WGRAD pair, both 64x64, generic A',
         P._sq(2, 9, 7, 36, 40, 3, 1), dict(fwd=(W64, ('lin',), 0, 0), wgrad=(W64, (), 0, 1)), pair=(W64, 0)),
    case('compact_not_lin_pair', 'batch 8, 2 x 2 outputs: the forward runs compacted taps, so it is not LIN (filter rows by (tap, channel) state); '
         'DGRAD + WGRAD pair with a uniform_k compact A; the weight gradient is ONE K-step (two dead stages)',
         P._sq(8, 4, 4, 64, 64, 5, 2), dict(fwd=(W64, ('compact',), 0, 0), wgrad=(W64, (), 0, 1)), pair=(W64, 1)),
    case('transposed_fwd_pair', 'a transposed layer on the adjoint descriptor: FWD LIN (uniform_k) as A + WGRAD pair, both 64x64',
         P._sq(2, 13, 11, 32, 128, 5, 2), dict(wgrad=(W64, (), 0, 1)), transposed=True, pair=(W64, 1)),
]

def variants(lib, on):
    """Both switches for a block (conv_path_cases.switches, shared with the other variant tests and the random sweep)."""
    return P.switches(lib, uk=on, uw=on)


def row_of(c):
    return P.row(c.name, c.why, c.desc, {}, transposed=c.transposed)


def premise(lib, c, r):
    """The paths the case is there for, with the variants on and off: {contraction: path with the variants on}."""
    out = {}
    for contraction, (tile, words, uk, uw) in c.expect.items():
        with variants(lib, 1):
            on = P.query(lib, r, contraction)
        with variants(lib, 0):
            off = P.query(lib, r, contraction)
        s = P.path_str(on)
        assert on.family == L.ConvPath.FAMILIES.index('mfma_f32'), '%s %s: not on the fp32 MFMA kernels (%s).  %s' % (c.name, contraction, s, P.HOW)
        assert (on.tile_rows, on.tile_cols) == tile and on.nvec == 1, '%s %s: %s, the case is there for the %dx%d tile with 16-byte dense rows.  %s' % (
            (c.name, contraction, s) + tile + (P.HOW,))
        for w in ('lin', 'ragged', 'compact'):
            assert (w in s.split()) == (w in words), '%s %s: %s, the case is there for %s.  %s' % (c.name, contraction, s, words or 'the plain path', P.HOW)
        assert (on.uniform_k, on.uniform_w) == (uk, uw), '%s %s: uniform_k %d uniform_w %d, the case is there for %d %d (%s).  %s' % (
            c.name, contraction, on.uniform_k, on.uniform_w, uk, uw, s, P.HOW)
        assert (off.uniform_k, off.uniform_w) == (0, 0), '%s %s: a variant is reported with the switches off' % (c.name, contraction)
        P.same_plan(on, off, '%s %s' % (c.name, contraction))
        out[contraction] = on
    if c.pair is not None:
        d = P.desc_of(r)
        kind = L.PAIR_KINDS[lib.conv2d_pair_path(ctypes.byref(d), 1 if c.transposed else 0, L.ACG_F32, 0)]
        assert kind == 'conv_pair_f32', '%s: the pair entry answers %s.  %s' % (c.name, kind, P.HOW)
        with variants(lib, 1):
            pa = P.query(lib, r, 'dgrad', True)
        assert ((pa.tile_rows, pa.tile_cols), pa.uniform_k) == c.pair, '%s: contraction A of the pair is %s uniform_k %d.  %s' % (c.name, P.path_str(pa), pa.uniform_k, P.HOW)
        assert pa.lin == (1 if c.transposed else 0), '%s: contraction A of the pair is %s.  %s' % (c.name, P.path_str(pa), P.HOW)
    return out


def run_fwd(run):
    x, ref, side = run.fwd_io()
    y = run.output(side)
    ws = run.abi.fwd_d(run.d, run.r.transposed, x, run.lay.w, y)
    run.keep(ws)
    run.done()
    run.check_out(y, ref, ref.shape[-1], ref.shape[-1], 'fwd')
    return dict(y=y, ws=ws)


def run_wgrad(run):
    """Accumulate mode 0 into a sentinel-filled dw: the launch owns every bit of the result."""
    x, dy = run.wgrad_io()
    dw = torch.full(run.lay.w.shape, P.SENTINEL, device=run.abi.device)
    ws = run.abi.wgrad_d(run.d, run.r.transposed, x, dy, dw, 0.0)
    run.keep(ws)
    run.done()
    run.close(dw, run.lay.dW.to(dw.device), P.TOL_CONV, 'wgrad')
    return dict(dw=dw, ws=ws)


def run_pair(run):
    abi, d, t = run.abi, run.d, run.r.transposed
    dy, ref, side, c, n = run.dgrad_io()
    x, dyw = run.wgrad_io()
    dx, dw = run.output(side), torch.full(run.lay.w.shape, P.SENTINEL, device=abi.device)
    wsd, wsw = abi.bwd_pair_d(d, t, dy, run.lay.w, x, dx, dw, 0.0, 0)
    run.keep(wsd, wsw)
    run.done()
    run.check_out(dx, ref, c, n, 'pair dx')
    run.close(dw, run.lay.dW.to(dw.device), P.TOL_CONV, 'pair dw')
    return dict(dx=dx, dw=dw, ws_dx=wsd, ws_dw=wsw)


def twice(name, what, fn):
    a, b = fn(), fn()
    P.same_bits(a, b, '%s %s' % (name, what), 'of two runs of the same launch')
    return a


RUN = dict(fwd=run_fwd, wgrad=run_wgrad)


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.name)
def test_transposed_stores_reach_lds_before_the_barrier(hip_abi, c):
    lib, r = hip_abi.lib, row_of(c)
    assert P.flop(r) <= P.MAX_FLOP / 32
    plans = premise(lib, c, r)
    run = P.Runner(hip_abi, r)
    got = {}
    for on in (1, 0):
        with variants(lib, on):
            for contraction in c.expect:
                got[on, contraction] = twice(c.name, '%s (variants %d)' % (contraction, on), lambda: RUN[contraction](run))
            if c.pair is not None:
                run.pair(0)      # bit-equal to the separate entries, and against float64
                got[on, 'pair'] = twice(c.name, 'pair (variants %d)' % on, lambda: run_pair(run))
    # the variants change addressing, never a value: the same bits with the switches on and off
    for (on, what), res in got.items():
        if on == 1:
            for k, v in res.items():
                if v is not None:
                    P.Runner.bitwise(v, got[0, what][k], '%s %s: %s with the variants on vs off' % (c.name, what, k))
    for contraction, p in plans.items():
        if p.splits > 1:      # the slabs are in the workspace the two runs were compared on
            ws = got[1, contraction]['ws']
            assert ws is not None and bool((ws != 0).any()), '%s %s: no slabs in the workspace' % (c.name, contraction)


def test_premises_from_the_plan(hip_abi):
    """What the cases are there for beyond the tile: K-steps per split, partial tiles, masked columns, dead stages."""
    lib = hip_abi.lib
    by = {c.name: premise(lib, c, row_of(c)) for c in CASES}
    per = lambda p: -(-p.nk // p.splits)
    assert per(by['wgrad_14_steps']['wgrad']) == 14 and by['wgrad_14_steps']['wgrad'].splits > 1, P.HOW      # 6 unrolled copies twice + 2: both table halves
    assert per(by['wgrad_13_steps_narrow']['wgrad']) == 13, P.HOW
    p = by['partial_tiles']
    assert p['wgrad'].tiles == 5 and p['wgrad'].nk == 4 and p['fwd'].tiles == 2 and p['fwd'].splits == 2, P.HOW      # 288 = 4.5 x 64 rows; 126 = 2 x 64 - 2 rows
    assert by['ragged_25']['wgrad'].ragged == 1 and by['ragged_25']['fwd'].ragged == 1, P.HOW
    assert by['channels_36_pair']['fwd'].lin == 1 and by['channels_36_pair']['wgrad'].tiles == 6, P.HOW      # 324 rows: a partial sixth tile
    assert by['compact_not_lin_pair']['fwd'].lin == 0 and by['compact_not_lin_pair']['fwd'].splits > 1, P.HOW
    assert by['compact_not_lin_pair']['wgrad'].nk == 1, P.HOW      # fewer K-steps than register stages
