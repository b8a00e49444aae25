"""GPU parity of the uniform_w loaders of the fp32 MFMA weight gradient (conv_f32_kernel.h: UW) against the generic loaders they replace.

acg_conv2d_uniform_w(0 / 1) switches the variant for the whole process and nothing else, so every case runs twice in one process -
variant on, variant off - and holds
  * the path query: uniform_w is taken (or declined) as the case states when on, never when off, and every plan field - tile, tiles,
    classes, K-steps, splits, reduction, and uniform_k, which stays 0 for a weight gradient - is the same in both runs;
  * dw of the two runs BIT FOR BIT, in accumulate mode 0.5 onto a seeded dw0, and the workspace - the split-K slabs where the plan splits;
  * each run against the float64 reference of tests/conv_path_cases.py at the project's bar TOL_CONV, as it is.
No case skips: a shape the planner has moved off its path fails its premise (conv_path_cases.HOW says what to do then).

The rule has no condition on the gathered channel count beyond "a multiple of 4" (not ragged): 36 channels take the variant.

The refill premise could not be had from the shape named for it: (4, 16, 16, 32, 64, 3, 1) has 32 K-steps, and the planner gives it 8
splits of 4 - fewer than the row-table chunk of 6, so no refill happens inside its loop.  It stays in the table as a split case (the slabs
bit for bit, and the test asserts that they are there).  The premise is asserted on three other shapes:
  * `refill_7_steps`, 200 pixels = 7 K-steps unsplit: the first refill (chunk 1, table half 1) lands in the loop and step 6 is loaded
    out of it;
  * `long_split_narrow` and `long_split_wide`: few channels on 64 x 64 maps, so that one tile meets the planner's cap of 128 splits and
    a split runs 13 (128x32 tile) and 14 (64x64 tile) K-steps - more than TWO chunks.  Their loops go through the second round of the
    unrolled loop: the table half derived from the round number, slots 3-5 of chunk 1 read out of half 1, the second refill back into
    half 0, and slots 0-1 of chunk 2 read out of it.

Not covered here: as B of conv_pair_f32 beside a 128x32 contraction A, a 64x64 weight gradient keeps the generic loaders whatever
acg_conv_path.uniform_w answers (conv_f32_pair.hip: launch_b; no query reports what a pair launches for B).  Both pair cases below have a
64x64 A - the premise test asserts it - so their B does run the variant; for the left-out combination an on / off comparison would compare
the generic loaders with themselves."""
import collections
import ctypes

import pytest
import torch

import conv_path_cases as P
from action_conditioned_gans_amd import _lib as L

pytestmark = pytest.mark.gpu

CHUNK = 6      # K-steps per row-table chunk of the UW loaders (conv_body: UNR)
NST = 3        # register stages of the K-loop (ACG_NST)

Case = collections.namedtuple('Case', 'name why desc transposed uw pair')


def case(name, why, desc, uw, transposed=False, pair=False):
    return Case(name, why, desc, transposed, uw, pair)


CASES = [
    case('partial_everything', '126 pixels: the last K-step is partial and rests on the record count alone; two taps per 64-row block, a partial row tile '
         '(288 rows) and a partial column tile (N = 40), borders on every side', P._sq(2, 9, 7, 32, 40, 3, 1), 1),
    case('narrow_stride2_pair', 'the 128x32 tile with stride 2; alone, and as B of conv_pair_f32 beside a uniform_k DGRAD as A',
         P._sq(2, 13, 11, 64, 32, 5, 2), 1, pair=True),
    case('transposed_twin_pair', 'the transposed twin on the adjoint descriptor (x and dy exchange roles); as B of conv_pair_f32 beside a uniform_k FWD as A',
         P._sq(2, 13, 11, 32, 128, 5, 2), 1, transposed=True, pair=True),
    case('split_32_steps', '1024 pixels = 32 K-steps, split: the slabs bit for bit', P._sq(4, 16, 16, 32, 64, 3, 1), 1),
    case('refill_7_steps', '200 pixels = 7 K-steps in one split: more than one row-table chunk, the refill happens inside the loop',
         P._sq(2, 10, 10, 32, 40, 3, 1), 1),
    case('long_split_narrow', '13 x 64 x 64 pixels, 4 -> 24 channels, 3 x 3: one 128x32 tile, 1664 K-steps over 128 splits = 13 per split: two refills, both table halves twice',
         P._sq(13, 64, 64, 4, 24, 3, 1), 1),
    case('long_split_wide', '14 x 64 x 64 pixels, 4 -> 36 channels, 2 x 2: one 64x64 tile (16 of its rows exist), 1792 K-steps over 128 splits = 14 per split',
         P._sq(14, 64, 64, 4, 36, 2, 1), 1),
    case('dead_stages', '32 pixels = one K-step: the prologue issues two dead stages (zero records)', P._sq(2, 4, 4, 64, 64, 3, 1), 1),
    case('tap_in_mask_hi', '49 taps: the tap bit of the lanes of taps 32..48 lies in mask_hi', P._sq(1, 8, 8, 32, 32, 7, 1), 1),
    case('at_pitch40', '32 channels stored at in_pitch 40 (pad channels hold a value): the row offsets come from the pitch', P._sq(2, 9, 7, 32, 40, 3, 1, in_pitch=40), 1),
    case('channels_36', '36 gathered channels: not ragged, not a multiple of the K-step - a 64-row block straddles taps at odd places; pad rows',
         P._sq(2, 9, 7, 36, 40, 3, 1), 1),
    # neighbours that must decline
    case('ragged_3', 'a ragged gather: 3 channels', P._sq(2, 9, 7, 3, 40, 3, 1), 0),
    case('ragged_138', 'a ragged gather: 138 channels', P._sq(2, 8, 8, 138, 64, 3, 1), 0),
    case('novec_25', 'N = 25: dY rows are not float4-able (nvec off)', P._sq(2, 9, 7, 32, 25, 3, 1), 0),
]

PLAN_FIELDS = P.PLAN_FIELDS + ('uniform_k',)


def variant(lib, on, uk=1):
    """acg_conv2d_uniform_w(on) and acg_conv2d_uniform_k(uk) for a block (conv_path_cases.switches, shared with the other variant tests)."""
    return P.switches(lib, uk=uk, uw=on)


def row_of(c):
    return P.row(c.name, c.why, c.desc, {}, transposed=c.transposed)


def paths(lib, r):
    """The weight gradient's path with the variant on and off: identical plans, the variant reported off when it is switched off."""
    with variant(lib, 1):
        on = P.query(lib, r, 'wgrad')
    with variant(lib, 0):
        off = P.query(lib, r, 'wgrad')
    P.same_plan(on, off, r.name, PLAN_FIELDS)
    assert off.uniform_w == 0, '%s: the variant is reported with the switch off' % r.name
    assert on.uniform_k == 0, '%s: a weight gradient reports uniform_k' % r.name
    assert on.family == L.ConvPath.FAMILIES.index('mfma_f32'), '%s: not on the fp32 MFMA kernels.  %s' % (r.name, P.HOW)
    return on


def run_wgrad(run):
    abi, d, t = run.abi, run.d, run.r.transposed
    x, dy = run.wgrad_io()
    dw0 = run.dw0(23)
    dw = dw0.clone()
    ws = abi.wgrad_d(d, t, x, dy, dw, 0.5)
    run.keep(ws)
    run.done()
    run.close(dw, 0.5 * dw0.double() + run.lay.dW.to(dw.device), P.TOL_CONV, 'wgrad accumulate 0.5')
    return dict(dw=dw, ws=ws)


def run_pair(run):
    abi, d, t = run.abi, run.d, run.r.transposed
    dy, ref, side, c, n = run.dgrad_io()
    x, dyw = run.wgrad_io()
    dw0 = run.dw0(13)
    dx, dw = run.output(side), dw0.clone()
    wsd, wsw = abi.bwd_pair_d(d, t, dy, run.lay.w, x, dx, dw, 0.5, 0)
    run.keep(wsd, wsw)
    run.done()
    run.check_out(dx, ref, c, n, 'pair dx')
    run.close(dw, 0.5 * dw0.double() + run.lay.dW.to(dw.device), P.TOL_CONV, 'pair dw')
    return dict(dx=dx, dw=dw, ws_dx=wsd, ws_dw=wsw)


def both_ways(lib, name, what, fn, uk=1):
    return P.both_ways(lib, '%s %s' % (name, what), fn, dict(uk=uk, uw=1), dict(uk=uk, uw=0))


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.name)
def test_uniform_w_matches_the_generic_loaders(hip_abi, c):
    lib, r = hip_abi.lib, row_of(c)
    assert P.flop(r) <= P.MAX_FLOP / 32
    p = paths(lib, r)
    assert p.uniform_w == c.uw, '%s: uniform_w = %d, the case is there for %d (%s).  %s' % (c.name, p.uniform_w, c.uw, P.path_str(p), P.HOW)
    run = P.Runner(hip_abi, r)
    got = both_ways(lib, c.name, 'wgrad', lambda: run_wgrad(run))
    if p.splits > 1:      # "the slabs bit for bit": they are there - `splits` slabs of dw's size, and the kernels wrote them
        slabs = got['ws'][:p.splits * got['dw'].numel() * 4]
        assert got['ws'].numel() >= p.splits * got['dw'].numel() * 4 and bool((slabs != 0).any()), '%s: no slabs in the workspace' % c.name
    if c.pair:
        d = P.desc_of(r)
        kind = L.PAIR_KINDS[lib.conv2d_pair_path(ctypes.byref(d), 1 if c.transposed else 0, L.ACG_F32, 0)]
        assert kind == 'conv_pair_f32', '%s: the pair entry answers %s.  %s' % (c.name, kind, P.HOW)
        with variant(lib, 1):
            pa = P.query(lib, r, 'dgrad', True)
        assert pa.uniform_k == 1, '%s: contraction A of the pair is not a uniform_k one (%s).  %s' % (c.name, P.path_str(pa), P.HOW)
        both_ways(lib, c.name, 'pair (UK A, UW B)', lambda: run_pair(run))
        both_ways(lib, c.name, 'pair (generic A, UW B)', lambda: run_pair(run), uk=0)
        both_ways(lib, c.name, 'wgrad with uniform_k off', lambda: run_wgrad(run), uk=0)


def test_premises_from_the_plan(hip_abi):
    """What the cases are there for, out of the path query: the tiles, the splits, the refills inside the loop, the dead stages."""
    lib = hip_abi.lib
    by = {c.name: paths(lib, row_of(c)) for c in CASES}
    per = {n: -(-p.nk // p.splits) for n, p in by.items()}
    tile = {n: (p.tile_rows, p.tile_cols) for n, p in by.items()}
    assert tile['partial_everything'] == (64, 64) and by['partial_everything'].nk == 4 and by['partial_everything'].tiles == 5, P.HOW
    assert tile['narrow_stride2_pair'] == (128, 32) and tile['transposed_twin_pair'] == (64, 64), P.HOW
    for c in CASES:      # contraction A of both pairs runs on the 64x64 tile: B takes the variant in the paired launch as well (module docstring)
        if c.pair:
            with variant(lib, 1):
                pa = P.query(lib, row_of(c), 'dgrad', True)
            assert (pa.tile_rows, pa.tile_cols) == (64, 64), (c.name, P.path_str(pa), P.HOW)
    assert by['split_32_steps'].nk == 32 and by['split_32_steps'].splits > 1, P.HOW
    assert by['refill_7_steps'].uniform_w == 1 and per['refill_7_steps'] > CHUNK, (per['refill_7_steps'], P.HOW)
    for name, t in (('long_split_narrow', (128, 32)), ('long_split_wide', (64, 64))):
        p = by[name]
        assert p.uniform_w == 1 and tile[name] == t and p.splits > 1 and per[name] > 2 * CHUNK, (name, P.path_str(p), p.nk, p.splits, P.HOW)
    assert tile['tap_in_mask_hi'] == (128, 32) and by['tap_in_mask_hi'].nk == 2, P.HOW      # 49 taps x 32 channels: rows of taps 32..48 exist
    assert tile['channels_36'] == (64, 64) and by['channels_36'].tiles == 6 and by['channels_36'].ragged == 0, P.HOW      # 324 rows: a partial sixth tile
    assert by['dead_stages'].uniform_w == 1 and per['dead_stages'] < NST, (per['dead_stages'], P.HOW)
    assert by['novec_25'].nvec == 0 and by['ragged_3'].ragged == 1 and by['ragged_138'].ragged == 1, P.HOW


def test_uniform_k_leaves_the_weight_gradient_alone(hip_abi):
    """acg_conv2d_uniform_k switches what it switched before: with it off, a weight gradient still reports (and runs) uniform_w."""
    lib, r = hip_abi.lib, row_of(CASES[0])
    with variant(lib, 1, uk=0):
        p = P.query(lib, r, 'wgrad')
    assert p.uniform_w == 1 and p.uniform_k == 0
    with variant(lib, 0, uk=1):
        p = P.query(lib, r, 'wgrad')
        f = P.query(lib, r, 'fwd')
    assert p.uniform_w == 0 and p.uniform_k == 0 and f.uniform_k == 1 and f.uniform_w == 0


def test_the_switch_takes_zero_and_one_only(hip_abi):
    with pytest.raises(L.AcgError):
        hip_abi.lib.conv2d_uniform_w(2)
    hip_abi.lib.conv2d_uniform_w(1)
