"""GPU parity of the uniform_k loaders of the fp32 MFMA convolution (conv_f32_kernel.h: UK) against the generic loaders they replace.

acg_conv2d_uniform_k(0 / 1) switches the variant for the whole process and nothing else, so every case runs twice in one process -
variant on, variant off - and holds
  * the path query: uniform_k is taken (or declined) as the case states when on, never when off, and tile, tiles, classes, K-steps,
    splits and reduction are the same in both runs;
  * the results of the two runs BIT FOR BIT: outputs, pad channels, and the workspace - the split-K slabs where the plan splits;
  * each run against the float64 reference of tests/conv_path_cases.py at the project's bar TOL_CONV, as it is.
No case skips: a shape the planner has moved off its path fails its premise (conv_path_cases.HOW says what to do then).

Shapes are (b, h, w, cin, cout, k, stride) layers with SAME padding, a few MFLOP each; a transposed case gives the adjoint descriptor
(in side = the layer's output), so its forward is the descriptor's DGRAD - stride classes, tap subsets - and its input gradient the
descriptor's FWD."""
import collections
import ctypes

import pytest
import torch

import conv_path_cases as P
from action_conditioned_gans_amd import _lib as L

pytestmark = pytest.mark.gpu

Case = collections.namedtuple('Case', 'name why desc transposed uk pair')


def case(name, why, desc, uk, transposed=False, pair=False):
    return Case(name, why, desc, transposed, uk, pair)


# uk: the LAYER's contractions to run -> is the variant taken.  Weight gradients never take it (their gathered rows change every
# K-step); they run here because the paired launch instantiates them beside a uniform_k contraction A.
CASES = [
    case('cp32_tap_per_step', 'Cp = 32: the tap changes every K-step; odd extents, partial row and column tiles (N = 40); FWD LIN, split in two',
         P._sq(2, 9, 7, 32, 40, 3, 1), dict(fwd=1, dgrad=0)),
    case('cp64_stride2_pair', 'two K-steps per tap, stride 2: FWD 128x32 over 12 splits; DGRAD with four stride classes of unequal size; conv_pair_f32 with DGRAD as A',
         P._sq(2, 13, 11, 64, 32, 5, 2), dict(fwd=1, dgrad=1, wgrad=0), pair=True),
    case('cp256_split_mid_tap', 'Cp = 256, 72 K-steps over 18 splits: four K-steps each, so every other split starts in the middle of a tap; FWD and DGRAD',
         P._sq(1, 4, 4, 256, 256, 3, 1), dict(fwd=1, dgrad=1)),
    case('transposed_128_to_32', 'a transposed layer 128 -> 32 channels, 5x5 / 2, on the adjoint descriptor: forward = DGRAD mode with tap subsets (128 gathered), '
         'input gradient = FWD LIN (32 gathered), weight gradient, acg_deconv2d_bwd_pair with FWD as A',
         P._sq(2, 13, 11, 32, 128, 5, 2), dict(fwd=1, dgrad=1, wgrad=0), transposed=True, pair=True),
    case('transposed_32_to_25', 'a transposed layer 32 -> 25 channels (the DNA logits): DGRAD mode with N = 25 columns - NVEC off, which DGRAD never reads - '
         'partial column tile, stride classes of unequal size',
         P._sq(2, 13, 11, 25, 32, 5, 2), dict(fwd=1), transposed=True),
    case('cp32_at_pitch40', '32 channels stored at in_pitch 40 (pad channels hold a value): the lane offsets come from the pitch, not the count',
         P._sq(2, 9, 7, 32, 40, 3, 1, in_pitch=40), dict(fwd=1)),
    case('compact_small_map', 'compact tiles (batch 8, 2 x 2 outputs): FWD declines - its taps are compacted, so it is not LIN; DGRAD takes the variant on the compacted tap table',
         P._sq(8, 4, 4, 64, 64, 5, 2), dict(fwd=0, dgrad=1)),
    case('merged_input_gradient', 'the merged input gradient of a stride-2 layer with 6 input channels runs as a stride-1 FWD LIN over dy (64 gathered): pixel-shuffle epilogue',
         P._sq(4, 16, 16, 6, 64, 5, 2), dict(dgrad=1)),
    # neighbours that must not take the variant
    case('not_48_channels', '48 gathered channels: a multiple of 4 (LIN), not of the K-step', P._sq(2, 9, 7, 48, 40, 3, 1), dict(fwd=0, dgrad=0)),
    case('not_36_channels', '36 gathered channels', P._sq(2, 9, 7, 36, 40, 3, 1), dict(fwd=0, dgrad=0)),
    case('not_138_channels_limit128', 'a 138-channel map with dgrad_c = 128: the FORWARD gathers 138 channels, whatever the limit says, and must decline; '
         'the input gradient gathers the 64 channels of dy and computes 128 of the 138 columns (column-wise reduction)',
         P._sq(2, 8, 8, 138, 64, 3, 1, dgrad_c=128), dict(fwd=0, dgrad=1)),
]

def variant(lib, on):
    """acg_conv2d_uniform_k(on) for a block (conv_path_cases.switches: the helper the variant tests and the random sweep share)."""
    return P.switches(lib, uk=on)


def row_of(c):
    return P.row(c.name, c.why, c.desc, {}, transposed=c.transposed)


def paths(lib, r, contraction, as_pair_a=False):
    """The path with the variant on and off: identical plans, and the variant reported off when it is switched off."""
    with variant(lib, 1):
        on = P.query(lib, r, contraction, as_pair_a)
    with variant(lib, 0):
        off = P.query(lib, r, contraction, as_pair_a)
    P.same_plan(on, off, '%s %s' % (r.name, contraction))
    assert off.uniform_k == 0, '%s %s: the variant is reported with the switch off' % (r.name, contraction)
    assert on.family == L.ConvPath.FAMILIES.index('mfma_f32'), '%s %s: not on the fp32 MFMA kernels.  %s' % (r.name, contraction, P.HOW)
    return on


run_once = P.run_once      # one contraction through its plain entry -> {tag: tensor}: the result and the workspace; a weight gradient at accumulate 0.5


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


def both_ways(lib, name, what, fn):
    P.both_ways(lib, '%s %s' % (name, what), fn, dict(uk=1), dict(uk=0))


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.name)
def test_uniform_k_matches_the_generic_loaders(hip_abi, c):
    lib, r = hip_abi.lib, row_of(c)
    assert P.flop(r) <= P.MAX_FLOP / 32
    run = P.Runner(hip_abi, r)
    for contraction, taken in c.uk.items():
        p = paths(lib, r, contraction)
        assert p.uniform_k == taken, '%s %s: uniform_k = %d, the case is there for %d (%s).  %s' % (c.name, contraction, p.uniform_k, taken, P.path_str(p), P.HOW)
        both_ways(lib, c.name, contraction, lambda: run_once(run, contraction))
    if c.pair:
        d = P.desc_of(r)
        kind = L.PAIR_KINDS[lib.conv2d_pair_path(ctypes.byref(d), 1 if c.transposed else 0, L.ACG_F32, 0)]
        assert kind == 'conv_pair_f32', '%s: the pair entry answers %s.  %s' % (c.name, kind, P.HOW)
        pa = paths(lib, r, 'dgrad', as_pair_a=True)
        assert pa.uniform_k == c.uk['dgrad'], (c.name, P.path_str(pa), pa.uniform_k)
        both_ways(lib, c.name, 'pair', lambda: run_pair(run))


def test_a_split_starts_in_the_middle_of_a_tap(hip_abi):
    """The premise of cp256_split_mid_tap, from the plan: K-steps per split times 32 is not a multiple of the padded channel count."""
    c = next(c for c in CASES if c.name == 'cp256_split_mid_tap')
    r = row_of(c)
    for contraction, cp in (('fwd', 256), ('dgrad', 256)):
        p = paths(hip_abi.lib, r, contraction)
        per = -(-p.nk // p.splits)
        starts = [z * per * 32 for z in range(1, p.splits) if z * per < p.nk]
        assert p.uniform_k == 1 and p.splits > 1 and any(k % cp for k in starts), (contraction, p.nk, p.splits, starts, P.HOW)


def test_stats_partials_are_bit_identical(hip_abi):
    """acg_conv2d_fwd_stats on a uniform_k forward (2 x 2 filter, 32 channels: four K-steps, unsplit): result and BatchNorm partials
    bit for bit, and the whole BatchNorm of conv_path_cases.case_stats against float64 in both runs."""
    lib = hip_abi.lib
    desc = P._sq(2, 9, 7, 32, 40, 2, 1)
    r = P.row('uk_stats', 'statistics epilogue of a uniform_k forward', desc, {})
    p = paths(lib, r, 'fwd')
    assert p.uniform_k == 1 and p.splits == 1, (P.path_str(p), P.HOW)
    run = P.Runner(hip_abi, r)

    def once():
        x, ref, side = run.fwd_io()
        y = run.output(side)
        got = run.abi.fwd_stats_d(run.d, False, x, run.lay.w, y, 1)
        assert got is not None, 'acg_conv2d_stats_layout provides no partials.  ' + P.HOW
        run.keep(got[4])
        run.done()
        run.check_out(y, ref, ref.shape[-1], ref.shape[-1], 'fwd_stats')
        return dict(y=y, partials=got[0])

    both_ways(lib, r.name, 'fwd_stats', once)
    for on in (1, 0):
        with variant(lib, on):
            P.case_stats(hip_abi, 'uk_stats_%d' % on, desc, False, 1, True)


def test_bias_act_epilogue_is_bit_identical(hip_abi):
    """acg_deconv2d_fwd_bias_act (the EPI instantiation) on an adjoint descriptor whose forward gathers 32 channels: 3 x 3 / 2, unsplit,
    the 128 x 32 tile."""
    lib = hip_abi.lib
    desc = P._sq(4, 16, 16, 3, 32, 3, 2)
    r = P.row('uk_epi', 'fused bias + activation on a uniform_k transposed forward', desc, {}, transposed=True)
    d = P.desc_of(r)
    assert lib.deconv2d_fwd_bias_act_ok(ctypes.byref(d), L.ACG_F32) == 1, 'the fused epilogue refuses this shape.  ' + P.HOW
    p = paths(lib, r, 'fwd', as_pair_a=True)      # the plan the entry launches: the class-wise DGRAD, never the merged form
    assert p.uniform_k == 1 and p.splits == 1 and (p.tile_rows, p.tile_cols) == (128, 32), (P.path_str(p), P.HOW)
    run = P.Runner(hip_abi, r)
    x = run.tensor('out', run.lay.B)
    bias = (torch.randn((d.in_c,), generator=torch.Generator().manual_seed(5)) * 0.5).to(hip_abi.device)
    want = torch.tanh(run.lay.CtB + bias.double().to(run.lay.CtB.device))

    def once():
        y = torch.full((d.batch, d.in_h, d.in_w, d.in_c), P.SENTINEL, device=hip_abi.device)
        run.abi.fwd_bias_act_d(d, x, run.lay.w, bias, y, 'tanh', 0.2)
        run.done()
        run.close(y, want, P.TOL_CONV, 'bias + tanh')
        return dict(y=y)

    both_ways(lib, r.name, 'bias_act', once)


def test_the_switch_takes_zero_and_one_only(hip_abi):
    with pytest.raises(L.AcgError):
        hip_abi.lib.conv2d_uniform_k(2)
    hip_abi.lib.conv2d_uniform_k(1)
