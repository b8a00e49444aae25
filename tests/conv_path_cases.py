"""One small convolution case per kernel variant and reduction the planner of conv_f32.hip can pick (the conv sibling of
bn_cases.py): the table ROWS, the float64 reference of a full descriptor, and the case functions shared by the GPU suite
(test_gpu_conv_paths.py: libacgan_hip.so) and the CPU suite (test_conv_paths_cpu.py: the C oracle on the fp32 rows, and the
table's expectations against tools/conv_path_sweep.hip).

A row is a descriptor, a storage type and, for each contraction it runs, the PATH it is there to reach, written as
``path_str`` prints an acg_conv_path (include/acgan_conv_plan.h):

    direct nb8                                   the direct kernels, template argument NB
    mfma_f32 128x32 s4 ragged novec red=plain    fp32 MFMA kernel: tile, split count, then the switches that are on -
                                                 ragged, novec (NVEC off), lin, compact, merged - and the reduction that follows
    mfma_bf16 64x64 s2 red=bf16 / glds_bf16 256x128 s1

``fwd`` / ``dgrad`` / ``wgrad`` are the LAYER's contractions: a transposed row gives the adjoint descriptor (in side = the layer's
output), its forward is the descriptor's DGRAD and its input gradient the descriptor's FWD.  ``pair`` maps a flag word of
acg_(de)conv2d_bwd_pair to what the entry does (_lib.PAIR_KINDS).

WHEN A PREMISE FAILS the planner (or a constant it reads) has moved the row's shape to another kernel and the variant named in the
row's ``why`` has lost its case.  Do not edit the expectation to whatever the library now answers: find a shape that reaches the
variant again (PYTHONPATH=. python tests/conv_path_cases.py | conv_path_sweep prints the path of every row on a host without a GPU; the
command is in tools/conv_path_sweep.hip) and keep the row's purpose.  test_every_launch_statement_has_a_row names the variants
that are left without a row.

Run as a script, this file prints the table as the queries tools/conv_path_sweep.hip reads."""
import collections
import contextlib
import ctypes

import torch
import torch.nn.functional as F

from action_conditioned_gans_amd import _lib as L

TOL_CONV = 1e-4     # tests/test_gpu_ops.py: the project's bars, used as they are
TOL_BF16 = 4e-3
X_PAD = 3.0         # fp32 x pad channels: finite and non-zero - they must not reach a result
SENTINEL = -777.0   # outputs start here (exact in bfloat16): what a call must not write comes back bit-identical
MAX_FLOP = 2.0 * 16 * 16 * 16 * 25 * 128 * 128      # the cost of (16, 32, 32, 128, 128, 5, 2): no row of the table may exceed it

FIELDS = [n for n, _ in L.ConvDesc._fields_]


def conv(b, h, w, cin, cout, kh, kw, sh, sw, pad, in_pitch=0, out_pitch=0, dgrad_c=0, adj_dgrad_c=0):
    """The 17 descriptor fields.  ``pad``: 'SAME', 'VALID' (TensorFlow's geometry) or explicit (top, bottom, left, right)."""
    if pad == 'SAME':
        oh, ow = -(-h // sh), -(-w // sw)
        pt, pl = max((oh - 1) * sh + kh - h, 0) // 2, max((ow - 1) * sw + kw - w, 0) // 2
    elif pad == 'VALID':
        oh, ow, pt, pl = (h - kh) // sh + 1, (w - kw) // sw + 1, 0, 0
    else:
        pt, pb, pl, pr = pad
        oh, ow = (h + pt + pb - kh) // sh + 1, (w + pl + pr - kw) // sw + 1
    return (b, h, w, cin, oh, ow, cout, kh, kw, sh, sw, pt, pl, in_pitch, out_pitch, dgrad_c, adj_dgrad_c)


Row = collections.namedtuple('Row', 'name why desc transposed storage expect acc')


def row(name, why, desc, expect, transposed=False, storage='f32', acc=(0.0, 0.5)):
    return Row(name, why, desc, transposed, storage, expect, acc)


def _sq(b, h, w, cin, cout, k, s, pad='SAME', **kw):
    return conv(b, h, w, cin, cout, k, k, s, s, pad, **kw)


# ---- the table -------------------------------------------------------------------------------------------------------------------
# B1: fp32 MFMA.  FWD variants per tile: lin | plain (3 channels at pitch 4) | ragged | novec; partial row / column tiles.
ROWS = [
    row('f32_narrow_lin', 'FWD 128x32 LIN; DGRAD 128x32 stride 2, classes of unequal size (odd extents); WGRAD 128x32 nvec, unsplit neighbours',
        _sq(2, 13, 11, 8, 32, 3, 2), dict(fwd='mfma_f32 128x32 s1 lin', dgrad='mfma_f32 128x32 s1', wgrad='mfma_f32 128x32 s1', pair={0: 'conv_pair_f32'})),
    row('f32_wide_lin', 'FWD 64x64 LIN with a partial last row tile and a partial last column tile (N = 72); DGRAD 128x32 stride 1; WGRAD 64x64',
        _sq(3, 7, 9, 16, 72, 3, 1), dict(fwd='mfma_f32 64x64 s1 lin', dgrad='mfma_f32 128x32 s5 red=plain', wgrad='mfma_f32 64x64 s1', pair={0: 'conv_pair_f32'})),
    row('f32_narrow_pad3', 'FWD 128x32 non-LIN at a padded pitch (3 channels at pitch 4); x pad channel holds a value',
        _sq(2, 16, 16, 3, 32, 5, 2, in_pitch=4), dict(fwd='mfma_f32 128x32 s1', dgrad='mfma_f32 128x32 s2 lin merged red=cols', wgrad='mfma_f32 128x32 s1', pair={0: 'merged'})),
    row('f32_wide_pad3', 'FWD 64x64 non-LIN at a padded pitch (3 channels at pitch 4)',
        _sq(2, 16, 16, 3, 64, 5, 2, in_pitch=4), dict(fwd='mfma_f32 64x64 s1', dgrad='mfma_f32 128x32 s4 lin merged red=cols', wgrad='mfma_f32 64x64 s1', pair={0: 'merged'})),
    row('f32_narrow_ragged', 'FWD 128x32 ragged (pitch 5); WGRAD ragged x; DGRAD novec (N = 5)',
        _sq(2, 12, 12, 5, 24, 3, 1), dict(fwd='mfma_f32 128x32 s1 ragged', dgrad='mfma_f32 128x32 s1 novec', wgrad='mfma_f32 128x32 s2 ragged red=plain', pair={0: 'two_launches'})),
    row('f32_wide_ragged', 'FWD 64x64 ragged (6 channels at pitch 7), partial column tile (N = 68)',
        _sq(2, 12, 12, 6, 68, 3, 1, in_pitch=7), dict(fwd='mfma_f32 64x64 s1 ragged', dgrad='mfma_f32 128x32 s5 novec red=cols', wgrad='mfma_f32 64x64 s2 ragged red=plain', pair={0: 'two_launches'})),
    row('f32_narrow_novec', 'FWD 128x32 nvec off (N = 25); DGRAD with a ragged dy pitch; WGRAD nvec off',
        _sq(2, 12, 12, 16, 25, 3, 1), dict(fwd='mfma_f32 128x32 s1 novec', dgrad='mfma_f32 128x32 s2 ragged red=plain', wgrad='mfma_f32 128x32 s2 novec red=plain', pair={0: 'two_launches'})),
    row('f32_wide_novec', 'FWD / WGRAD 64x64 nvec off (out_c = 41, not a multiple of 4); DGRAD 64x64 ragged dy',
        _sq(2, 12, 12, 36, 41, 3, 1), dict(fwd='mfma_f32 64x64 s2 novec red=plain', dgrad='mfma_f32 64x64 s3 ragged red=plain', wgrad='mfma_f32 64x64 s2 novec red=plain', pair={0: 'two_launches'})),
    row('f32_ragged_novec', 'FWD ragged and nvec off at once on both tiles is two rows: 128x32 here (5 -> 9 channels)',
        _sq(4, 20, 20, 5, 9, 3, 1), dict(fwd='mfma_f32 128x32 s1 ragged novec', dgrad='mfma_f32 128x32 s1 ragged novec', wgrad='mfma_f32 128x32 s12 ragged novec red=plain')),
    row('f32_wide_ragged_novec', 'FWD 64x64 ragged + nvec off (7 -> 37 channels); DGRAD 128x32 ragged + nvec off',
        _sq(2, 12, 12, 7, 37, 3, 1), dict(fwd='mfma_f32 64x64 s1 ragged novec', dgrad='mfma_f32 128x32 s3 ragged novec red=plain', wgrad='mfma_f32 64x64 s2 ragged novec red=plain')),
    row('f32_n_tiny', 'nvec off at N = 3 and N = 1 columns would be direct-sized: 40 -> 3 channels above the direct limit of 8 MFLOP',
        _sq(8, 24, 24, 40, 3, 3, 1), dict(fwd='mfma_f32 128x32 s3 novec red=plain', dgrad='mfma_f32 64x64 s1 ragged', wgrad='mfma_f32 128x32 s36 novec red=plain')),
    row('f32_n_one', 'nvec off at N = 1 on the tiled path (128 -> 1 channels, above the direct limit of 8 MFLOP)',
        _sq(8, 24, 24, 128, 1, 3, 1), dict(fwd='mfma_f32 128x32 s7 novec red=plain', wgrad='mfma_f32 128x32 s36 novec red=plain')),
    row('f32_dgrad_wide', 'DGRAD 64x64 (N = 40 input channels) stride 2 with even extents; nvec on',
        _sq(2, 16, 16, 40, 32, 5, 2), dict(fwd='mfma_f32 128x32 s8 lin red=plain', dgrad='mfma_f32 64x64 s2 red=plain', wgrad='mfma_f32 128x32 s1', pair={0: 'conv_pair_f32'})),
    row('f32_dgrad_wide_novec', 'DGRAD 64x64 nvec off (N = 37) with a ragged dy pitch (out_c = 35)',
        _sq(2, 12, 12, 37, 35, 3, 1), dict(fwd='mfma_f32 64x64 s3 ragged novec red=plain', dgrad='mfma_f32 64x64 s2 ragged novec red=plain', wgrad='mfma_f32 64x64 s2 ragged novec red=plain')),
    row('f32_dgrad_narrow_ragged', 'DGRAD 128x32 with a ragged dy pitch (out_c = 18) and nvec on (N = 16)',
        _sq(2, 12, 12, 16, 18, 3, 1), dict(fwd='mfma_f32 128x32 s1 novec', dgrad='mfma_f32 128x32 s1 ragged', wgrad='mfma_f32 128x32 s2 novec red=plain')),
    # compact and its neighbours
    row('f32_compact', 'compact FWD and DGRAD: batch 8, 4 output pixels / 4 pixels per stride class',
        _sq(8, 4, 4, 64, 64, 5, 2), dict(fwd='mfma_f32 64x64 s12 compact red=plain', dgrad='mfma_f32 64x64 s4 compact red=plain', wgrad='mfma_f32 64x64 s1', pair={0: 'conv_pair_f32'})),
    row('f32_compact_batch7', 'the neighbour that must not be compact: batch 7',
        _sq(7, 4, 4, 64, 64, 5, 2), dict(fwd='mfma_f32 64x64 s12 lin red=plain', dgrad='mfma_f32 64x64 s4 red=plain')),
    row('f32_compact_5px', 'the neighbour that must not be compact: 5 output pixels (5 x 1), 5 per stride class',
        _sq(8, 10, 2, 64, 64, 5, 2), dict(fwd='mfma_f32 64x64 s12 lin red=plain', dgrad='mfma_f32 64x64 s4 red=plain')),
    row('f32_compact_1x1', 'the neighbour that must not be compact: a 1 x 1 filter',
        _sq(8, 2, 2, 64, 64, 1, 1), dict(fwd='mfma_f32 64x64 s1 lin', dgrad='mfma_f32 64x64 s1')),
    # splits
    row('f32_splits_cap', 'FWD / DGRAD splits held by the nk / min_steps cap',
        _sq(2, 8, 8, 32, 64, 3, 1), dict(fwd='mfma_f32 64x64 s2 lin red=plain', dgrad='mfma_f32 128x32 s4 red=plain', wgrad='mfma_f32 64x64 s1')),
    row('f32_splits_fill', 'FWD / DGRAD splits at the target-filling value (256 / tiles)',
        _sq(8, 16, 16, 64, 64, 5, 1), dict(fwd='mfma_f32 64x64 s8 lin red=plain', dgrad='mfma_f32 64x64 s8 red=plain')),
    row('f32_splits_one', 'FWD / DGRAD unsplit (256 tiles or more); WGRAD split',
        _sq(16, 32, 32, 8, 64, 3, 1), dict(fwd='mfma_f32 64x64 s1 lin', dgrad='mfma_f32 128x32 s2 red=plain', wgrad='mfma_f32 64x64 s128 red=plain')),
    # (the boosts need tiles x nk >= 12800 K-steps of a tile: 4 output columns of the 32 keep that under the cost limit)
    row('f32_longk_x2_fwd', 'FWD x2 long-K boost: 128 tiles, 2 splits, nk / s = 50', _sq(16, 32, 32, 128, 4, 5, 1), dict(fwd='mfma_f32 128x32 s4 lin red=plain')),
    row('f32_longk_x4_fwd', 'FWD x4 long-K boost: 128 tiles, 2 splits, nk / s = 100', _sq(16, 32, 32, 256, 4, 5, 1), dict(fwd='mfma_f32 128x32 s8 lin red=plain')),
    row('f32_longk_x2_dgrad', 'DGRAD x2 long-K boost', _sq(16, 32, 32, 4, 128, 5, 1), dict(dgrad='mfma_f32 128x32 s4 red=plain')),
    row('f32_longk_x4_dgrad', 'DGRAD x4 long-K boost', _sq(16, 32, 32, 4, 256, 5, 1), dict(dgrad='mfma_f32 128x32 s8 red=plain')),
    # reductions
    row('f32_reduce_tail', 'splitk_reduce with numel % 4 != 0 (the scalar tail): 3 x 5 x 5 x 9 outputs',
        _sq(3, 5, 5, 64, 9, 5, 1), dict(fwd='mfma_f32 128x32 s12 novec red=plain')),
    row('f32_reduce_cols_pitch', 'splitk_reduce_cols<float> through a pitched output (dx at pitch 44 for 42 channels)',
        _sq(2, 8, 8, 42, 64, 5, 1, in_pitch=44), dict(dgrad='mfma_f32 64x64 s12 novec red=cols', wgrad='mfma_f32 64x64 s1', pair={0: 'two_launches'})),
    row('f32_reduce_cols_limit', 'splitk_reduce_cols<float> through a channel limit (dgrad_c 32 of 42)',
        _sq(2, 8, 8, 42, 64, 5, 1, in_pitch=44, dgrad_c=32), dict(dgrad='mfma_f32 128x32 s12 red=cols', wgrad='mfma_f32 64x64 s1', pair={0: 'conv_pair_f32'})),
    # merged input gradient
    row('f32_merged_split', 'merged input gradient, split',
        _sq(4, 16, 16, 6, 64, 5, 2), dict(fwd='mfma_f32 64x64 s1 ragged', dgrad='mfma_f32 128x32 s4 lin merged red=plain', wgrad='mfma_f32 64x64 s2 ragged red=plain', pair={0: 'merged', 1: 'merged'})),
    row('f32_merged_unsplit', 'merged input gradient, unsplit (256 tiles or more)',
        _sq(32, 64, 64, 1, 16, 5, 2), dict(dgrad='mfma_f32 128x32 s1 lin merged')),
    row('f32_merged_pair_refusals', 'found by the random sweep (tests/conv_random_cases.py): neither contraction splits, so the pair entry refuses the slabs-only '
        'flag words 1 and 2 - and acg_conv2d_pair_path answered "merged" for them, without looking at the flag word',
        _sq(8, 8, 6, 4, 16, 5, 2), dict(fwd='mfma_f32 128x32 s1 lin', dgrad='mfma_f32 128x32 s1 lin merged', wgrad='mfma_f32 128x32 s1', pair={0: 'merged', 1: 'refused', 2: 'refused'})),
    # B2: pairs - the A tile x B tile combinations beyond the rows above, MODE_FWD A (transposed layers), the flag words
    row('pair_t_narrow_narrow_lin', 'conv_pair_f32 MODE_FWD A 128x32 LIN, B 128x32',
        _sq(2, 16, 16, 24, 16, 5, 2), dict(fwd='mfma_f32 128x32 s1', dgrad='mfma_f32 128x32 s4 lin red=plain', wgrad='mfma_f32 128x32 s1', pair={0: 'conv_pair_f32', 2: 'conv_pair_f32', 6: 'conv_pair_f32'}), transposed=True),
    row('pair_t_wide_wide_lin', 'conv_pair_f32 MODE_FWD A 64x64 LIN, B 64x64',
        _sq(2, 16, 16, 48, 40, 5, 2), dict(fwd='mfma_f32 64x64 s3 red=plain', dgrad='mfma_f32 64x64 s9 lin red=plain', wgrad='mfma_f32 64x64 s1', pair={0: 'conv_pair_f32'}), transposed=True),
    row('pair_t_wide_wide_plain', 'conv_pair_f32 MODE_FWD A 64x64 non-LIN (6 channels at pitch 8), B 64x64',
        _sq(2, 16, 16, 6, 40, 5, 2, in_pitch=8), dict(dgrad='mfma_f32 64x64 s1', wgrad='mfma_f32 64x64 s1', pair={0: 'conv_pair_f32'}), transposed=True),
    row('pair_t_narrow_narrow_plain', 'conv_pair_f32 MODE_FWD A 128x32 non-LIN, B 128x32',
        _sq(2, 16, 16, 6, 16, 5, 2, in_pitch=8), dict(dgrad='mfma_f32 128x32 s1', wgrad='mfma_f32 128x32 s1', pair={0: 'conv_pair_f32'}), transposed=True),
    row('pair_t_wide_wide_ragged', 'conv_pair_f32 MODE_FWD A 64x64 ragged, B 64x64 ragged',
        _sq(2, 16, 16, 6, 40, 5, 2), dict(dgrad='mfma_f32 64x64 s1 ragged', wgrad='mfma_f32 64x64 s1 ragged', pair={0: 'conv_pair_f32'}), transposed=True),
    row('pair_t_narrow_narrow_ragged', 'conv_pair_f32 MODE_FWD A 128x32 ragged, B 128x32 ragged',
        _sq(2, 16, 16, 6, 16, 5, 2), dict(dgrad='mfma_f32 128x32 s1 ragged', wgrad='mfma_f32 128x32 s1 ragged', pair={0: 'conv_pair_f32'}), transposed=True),
    # (in MODE_FWD both sides have N = out_c columns: A is narrower than B only under a channel limit, and never wider)
    row('pair_t_narrow_wide_lin', 'conv_pair_f32 MODE_FWD A 128x32 LIN under adj_dgrad_c = 32 of 40, B 64x64',
        _sq(2, 16, 16, 24, 40, 5, 2, adj_dgrad_c=32), dict(dgrad='mfma_f32 128x32 s4 lin red=cols', wgrad='mfma_f32 64x64 s1', pair={0: 'conv_pair_f32'}), transposed=True),
    row('pair_t_narrow_wide_plain', 'conv_pair_f32 MODE_FWD A 128x32 non-LIN under a channel limit, B 64x64',
        _sq(2, 16, 16, 6, 40, 5, 2, in_pitch=8, adj_dgrad_c=32), dict(dgrad='mfma_f32 128x32 s1', wgrad='mfma_f32 64x64 s1', pair={0: 'conv_pair_f32'}), transposed=True),
    row('pair_t_narrow_wide_ragged', 'conv_pair_f32 MODE_FWD A 128x32 ragged under a channel limit, B 64x64 ragged',
        _sq(2, 16, 16, 6, 40, 5, 2, adj_dgrad_c=32), dict(dgrad='mfma_f32 128x32 s1 ragged', wgrad='mfma_f32 64x64 s1 ragged', pair={0: 'conv_pair_f32'}), transposed=True),
    row('pair_flags', 'the flag words 0, 1, 2, 3 and 6 on a plan that splits both contractions',
        _sq(4, 16, 16, 32, 64, 3, 1), dict(dgrad='mfma_f32 128x32 s4 red=plain', wgrad='mfma_f32 64x64 s8 red=plain', pair={0: 'conv_pair_f32', 1: 'conv_pair_f32', 2: 'conv_pair_f32', 3: 'conv_pair_f32', 6: 'conv_pair_f32'})),
    row('pair_refused_raggedness', 'pair_supported refuses: unequal raggedness (x at pitch 9, dy at pitch 24), nvec on both sides',
        _sq(2, 12, 12, 8, 24, 3, 1, in_pitch=9), dict(dgrad='mfma_f32 128x32 s1', wgrad='mfma_f32 128x32 s2 ragged red=plain', pair={0: 'two_launches'})),
    row('pair_refused_novec', 'pair_supported refuses: nvec off on the weight-gradient side (out_c = 25)',
        _sq(2, 12, 12, 16, 25, 3, 1), dict(dgrad='mfma_f32 128x32 s2 ragged red=plain', wgrad='mfma_f32 128x32 s2 novec red=plain', pair={0: 'two_launches'})),
    # B3: direct kernels
    row('direct_fwd8_k2', 'direct_fwd<8>, Ktot = 5 x 5 x 96 = 2400: two full passes of 1024 and a partial one; out_c = 2', _sq(2, 8, 8, 96, 2, 5, 2), dict(fwd='direct nb8', dgrad='direct nb8', wgrad='direct nb8', pair={0: 'direct_pair'})),
    row('direct_fwd8_k5', 'direct_fwd<8>, Ktot = 2 full passes + a partial one (5 x 5 x 96 = 2400); out_c = 5', _sq(2, 8, 8, 96, 5, 5, 2), dict(fwd='direct nb8', dgrad='direct nb8', wgrad='direct nb8', pair={0: 'direct_pair'})),
    row('direct_fwd8_k8', 'direct_fwd<8>, out_c = 8', _sq(2, 8, 8, 96, 8, 5, 2), dict(fwd='direct nb8', dgrad='direct nb8', wgrad='direct nb8', pair={0: 'direct_pair'})),
    row('direct_fwd1_k2250', 'direct_fwd<1>, Ktot = 3 x 3 x 250 = 2250 > 2048, not a multiple of 256', _sq(2, 6, 6, 250, 1, 3, 1), dict(fwd='direct nb1', dgrad='direct nb1', wgrad='direct nb1', pair={0: 'direct_pair'})),
    row('direct_wgrad8_m646', 'direct_wgrad<8>, M = 2 x 17 x 19 = 646: two passes of 256 + a remainder; accumulate 0 and 0.5', _sq(2, 17, 19, 3, 5, 3, 1), dict(fwd='direct nb8', dgrad='direct nb8', wgrad='direct nb8', pair={0: 'direct_pair'})),
    row('direct_wgrad1_m1292', 'direct_wgrad<1>, M = 4 x 17 x 19 = 1292: two passes of 512 + a remainder', _sq(4, 17, 19, 3, 1, 3, 1), dict(fwd='direct nb1', dgrad='direct nb1', wgrad='direct nb1', pair={0: 'direct_pair'})),
    row('direct_dgrad_stride', 'direct_dgrad past 2048 blocks: 4 x 384 x 384 x 2 elements, a 1 x 1 filter', _sq(4, 384, 384, 2, 1, 1, 1), dict(dgrad='direct nb1')),
    row('direct_dgrad_valid', 'direct_dgrad with VALID padding and stride 2', _sq(2, 11, 9, 6, 4, 3, 2, 'VALID'), dict(fwd='direct nb8', dgrad='direct nb8', wgrad='direct nb8', pair={0: 'direct_pair'})),
    row('direct_dgrad_pitched', 'direct_dgrad with in_pitch and out_pitch set: the dx pad channels stay', _sq(2, 9, 9, 5, 3, 3, 1, in_pitch=8, out_pitch=4), dict(fwd='direct nb8', dgrad='direct nb8', wgrad='direct nb8', pair={0: 'direct_pair'})),
    row('direct_transposed', 'a transposed layer on the direct kernels: forward (direct_dgrad), input gradient (direct_fwd), weight gradient; its pair is two launches',
        _sq(2, 12, 12, 4, 6, 5, 2), dict(fwd='direct nb8', dgrad='direct nb8', wgrad='direct nb8', pair={0: 'two_launches'}), transposed=True),
    row('direct_limit_conv', 'dgrad_c < in_c on a direct-sized conv: the input gradient leaves the direct kernels (they store every channel), the weight gradient stays: a mixed pair',
        _sq(2, 9, 9, 6, 4, 3, 1, dgrad_c=4), dict(dgrad='mfma_f32 128x32 s1', wgrad='direct nb8', pair={0: 'two_launches'})),
    row('direct_limit_transposed', 'adj_dgrad_c < out_c on a direct-sized transposed layer',
        _sq(2, 12, 12, 4, 6, 5, 2, adj_dgrad_c=4), dict(dgrad='mfma_f32 128x32 s1 novec', wgrad='direct nb8', pair={0: 'two_launches'}), transposed=True),
    # B4: bf16
    row('bf16_wide', 'conv_mfma_bf16 64x64 all three contractions, splits 1 .. ; splitk_reduce_bf16; conv_pair_bf16',
        _sq(4, 8, 8, 64, 128, 5, 2), dict(fwd='mfma_bf16 64x64 s6 red=bf16', dgrad='mfma_bf16 64x64 s4 red=bf16', wgrad='mfma_bf16 64x64 s1', pair={0: 'conv_pair_bf16'}), storage='bf16'),
    row('bf16_narrow', 'conv_mfma_bf16 128x32 FWD (N = 25 logits) and DGRAD (N = 16)',
        _sq(2, 16, 16, 16, 25, 3, 1), dict(fwd='mfma_bf16 128x32 s1', dgrad='mfma_bf16 128x32 s1', wgrad='mfma_bf16 64x64 s2 red=plain', pair={0: 'conv_pair_bf16'}), storage='bf16'),
    row('bf16_unsplit', 'bf16 splits == 1 (128 tiles or more, short K)',
        _sq(8, 32, 32, 16, 64, 3, 1), dict(fwd='mfma_bf16 64x64 s1', dgrad='mfma_bf16 128x32 s2 red=bf16', wgrad='mfma_bf16 64x64 s32 red=plain', pair={0: 'conv_pair_bf16'}), storage='bf16'),
    row('bf16_half_chip_longk', 'bf16 splits == 2: half a chip of tiles (128 of 128x32) with nk = 64',
        _sq(16, 32, 32, 256, 12, 4, 1), dict(fwd='mfma_bf16 128x32 s2 red=cols'), storage='bf16'),
    row('bf16_reduce_cols', 'splitk_reduce_cols<bf16>: a channel limit on a split input gradient',
        _sq(2, 8, 8, 40, 128, 5, 1, dgrad_c=32), dict(dgrad='mfma_bf16 128x32 s12 red=cols'), storage='bf16'),
    row('bf16_head_cols', 'ACG_DTYPE2(BF16, F32) head output, split, 12 channels at pitch 16: splitk_reduce_cols<float>', _sq(2, 8, 8, 64, 12, 5, 1), dict(fwd='mfma_bf16 128x32 s6 red=cols'), storage='bf16_f32'),
    row('bf16_head_split', 'ACG_DTYPE2(BF16, F32) head output, split', _sq(2, 8, 8, 64, 16, 5, 1), dict(fwd='mfma_bf16 128x32 s6 red=plain'), storage='bf16_f32'),
    row('bf16_head_unsplit', 'ACG_DTYPE2(BF16, F32) head output, unsplit', _sq(8, 32, 32, 16, 16, 3, 1), dict(fwd='mfma_bf16 128x32 s1'), storage='bf16_f32'),
    row('bf16_merged', 'bf16 merged input gradient', _sq(4, 16, 16, 6, 64, 5, 2), dict(dgrad='mfma_bf16 128x32 s2 merged red=cols', wgrad='mfma_bf16 64x64 s1', pair={0: 'merged'}), storage='bf16'),
    row('bf16_wgrad_xcd', 'bf16 WGRAD split count rounded up to a multiple of the 8 XCDs (384 / 7 tiles = 54 -> 56)',
        _sq(16, 32, 32, 48, 64, 3, 1), dict(wgrad='mfma_bf16 64x64 s56 red=plain'), storage='bf16'),
    row('bf16_big_fwd', 'conv_mfma_bf16 128x128 FWD at 256 tiles with a short K (1 x 1 filter)',
        _sq(8, 64, 64, 8, 128, 1, 1), dict(fwd='mfma_bf16 128x128 s1'), storage='bf16'),
    # conv_pair_bf16: A {128x32, 64x64, 128x128} x B {64x64, 128x128}, both modes
    row('bf16_pair_narrow_big', 'conv_pair_bf16 MODE_DGRAD A 128x32, B 128x128 (nk = 256)', _sq(16, 32, 32, 16, 72, 3, 1), dict(dgrad='mfma_bf16 128x32 s1', wgrad='mfma_bf16 128x128 s64 red=plain', pair={0: 'conv_pair_bf16'}), storage='bf16'),
    row('bf16_pair_wide_big', 'conv_pair_bf16 MODE_DGRAD A 64x64, B 128x128', _sq(16, 32, 32, 48, 72, 3, 1), dict(dgrad='mfma_bf16 64x64 s1', wgrad='mfma_bf16 128x128 s64 red=plain', pair={0: 'conv_pair_bf16'}), storage='bf16'),
    row('bf16_pair_big_wide', 'conv_pair_bf16 MODE_DGRAD A 128x128 (256 tiles, 1 x 1 filter), B 64x64', _sq(8, 64, 64, 128, 8, 1, 1), dict(dgrad='mfma_bf16 128x128 s1', wgrad='mfma_bf16 64x64 s128 red=plain', pair={0: 'conv_pair_bf16'}), storage='bf16'),
    row('bf16_pair_big_big', 'conv_pair_bf16 MODE_DGRAD A 128x128, B 128x128', _sq(8, 64, 64, 128, 72, 1, 1), dict(dgrad='mfma_bf16 128x128 s1', wgrad='mfma_bf16 128x128 s128 red=plain', pair={0: 'conv_pair_bf16'}), storage='bf16'),
    row('bf16_pair_t_narrow_big', 'conv_pair_bf16 MODE_FWD A 128x32 under adj_dgrad_c = 32 of 72, B 128x128', _sq(16, 32, 32, 16, 72, 3, 1, adj_dgrad_c=32),
        dict(dgrad='mfma_bf16 128x32 s1', wgrad='mfma_bf16 128x128 s64 red=plain', pair={0: 'conv_pair_bf16'}), True, 'bf16'),
    row('bf16_pair_t_wide_big', 'conv_pair_bf16 MODE_FWD A 64x64, B 128x128', _sq(16, 32, 32, 16, 72, 3, 1), dict(fwd='mfma_bf16 128x32 s1', dgrad='mfma_bf16 64x64 s1', wgrad='mfma_bf16 128x128 s64 red=plain', pair={0: 'conv_pair_bf16'}), True, 'bf16'),
    row('bf16_pair_t_big_big', 'conv_pair_bf16 MODE_FWD A 128x128, B 128x128', _sq(8, 64, 64, 16, 72, 3, 1), dict(dgrad='mfma_bf16 128x128 s1', wgrad='mfma_bf16 128x128 s128 red=plain', pair={0: 'conv_pair_bf16'}), True, 'bf16'),
    row('bf16_pair_t_big_wide', 'conv_pair_bf16 MODE_FWD A 128x128, B 64x64 (8 filter rows)', _sq(8, 64, 64, 8, 72, 1, 1), dict(dgrad='mfma_bf16 128x128 s1', wgrad='mfma_bf16 64x64 s128 red=plain', pair={0: 'conv_pair_bf16'}), True, 'bf16'),
    # B6: rectangular descriptors, conv and transposed, all three contractions, both storages
    row('rect_1x5', 'kh != kw: a 1 x 5 filter', conv(2, 9, 11, 12, 20, 1, 5, 1, 1, 'SAME'), dict(fwd='mfma_f32 128x32 s1 lin', dgrad='mfma_f32 128x32 s1', wgrad='mfma_f32 128x32 s1', pair={0: 'conv_pair_f32'})),
    row('rect_5x1_s2x1', 'a 5 x 1 filter with stride 2 x 1', conv(2, 12, 10, 12, 20, 5, 1, 2, 1, 'SAME'), dict(fwd='mfma_f32 128x32 s1 lin', dgrad='mfma_f32 128x32 s1', wgrad='mfma_f32 128x32 s1', pair={0: 'conv_pair_f32'})),
    row('rect_3x5_s1x2', 'a 3 x 5 filter with stride 1 x 2', conv(2, 10, 13, 12, 20, 3, 5, 1, 2, 'SAME'), dict(fwd='mfma_f32 128x32 s1 lin', dgrad='mfma_f32 128x32 s1', wgrad='mfma_f32 128x32 s1', pair={0: 'conv_pair_f32'})),
    row('rect_stride3', 'stride 3 (5 x 5 filter, nine stride classes of unequal size)', conv(2, 14, 13, 12, 20, 5, 5, 3, 3, 'SAME'), dict(fwd='mfma_f32 128x32 s2 lin red=plain', dgrad='mfma_f32 128x32 s1', wgrad='mfma_f32 128x32 s1', pair={0: 'conv_pair_f32'})),
    row('rect_explicit_pad', 'explicit padding that is neither SAME nor VALID: (2, 0, 1, 3) around a 4 x 3 filter, stride 2',
        conv(2, 11, 12, 12, 20, 4, 3, 2, 2, (2, 0, 1, 3)), dict(fwd='mfma_f32 128x32 s1 lin', dgrad='mfma_f32 128x32 s1', wgrad='mfma_f32 128x32 s1', pair={0: 'conv_pair_f32'})),
    row('rect_direct', 'a rectangular descriptor on the direct kernels: 2 x 3 filter, stride 2 x 1, padding (1, 0, 0, 2)',
        conv(2, 9, 8, 6, 4, 2, 3, 2, 1, (1, 0, 0, 2)), dict(fwd='direct nb8', dgrad='direct nb8', wgrad='direct nb8', pair={0: 'direct_pair'})),
]
# the same descriptors as transposed layers, and both in bf16 storage (the paths differ: each variant states its own)
RECT_EXPECT = {
    'rect_1x5_t': dict(fwd='mfma_f32 128x32 s1', dgrad='mfma_f32 128x32 s1 lin', wgrad='mfma_f32 128x32 s1', pair={0: 'conv_pair_f32'}),
    'rect_5x1_s2x1_t': dict(fwd='mfma_f32 128x32 s1', dgrad='mfma_f32 128x32 s1 lin', wgrad='mfma_f32 128x32 s1', pair={0: 'conv_pair_f32'}),
    'rect_3x5_s1x2_t': dict(fwd='mfma_f32 128x32 s1', dgrad='mfma_f32 128x32 s1 lin', wgrad='mfma_f32 128x32 s1', pair={0: 'conv_pair_f32'}),
    'rect_stride3_t': dict(fwd='mfma_f32 128x32 s1', dgrad='mfma_f32 128x32 s2 lin red=plain', wgrad='mfma_f32 128x32 s1', pair={0: 'conv_pair_f32'}),
    'rect_explicit_pad_t': dict(fwd='mfma_f32 128x32 s1', dgrad='mfma_f32 128x32 s1 lin', wgrad='mfma_f32 128x32 s1', pair={0: 'conv_pair_f32'}),
    'rect_direct_t': dict(fwd='direct nb8', dgrad='direct nb8', wgrad='direct nb8', pair={0: 'two_launches'}),
    'rect_1x5_bf16': dict(fwd='mfma_bf16 128x32 s1', dgrad='mfma_bf16 128x32 s1', wgrad='mfma_bf16 64x64 s1', pair={0: 'conv_pair_bf16'}),
    'rect_5x1_s2x1_bf16': dict(fwd='mfma_bf16 64x64 s1', dgrad='mfma_bf16 64x64 s1', wgrad='mfma_bf16 64x64 s1', pair={0: 'conv_pair_bf16'}),
    'rect_3x5_s1x2_bf16': dict(fwd='mfma_bf16 128x32 s1', dgrad='mfma_bf16 128x32 s1', wgrad='mfma_bf16 64x64 s1', pair={0: 'conv_pair_bf16'}),
    'rect_stride3_bf16': dict(fwd='mfma_bf16 64x64 s1', dgrad='mfma_bf16 64x64 s1', wgrad='mfma_bf16 64x64 s1', pair={0: 'conv_pair_bf16'}),
    'rect_explicit_pad_bf16': dict(fwd='mfma_bf16 64x64 s1', dgrad='mfma_bf16 64x64 s1', wgrad='mfma_bf16 64x64 s1', pair={0: 'conv_pair_bf16'}),
    'rect_1x5_t_bf16': dict(fwd='mfma_bf16 128x32 s1', dgrad='mfma_bf16 128x32 s1', wgrad='mfma_bf16 64x64 s1', pair={0: 'conv_pair_bf16'}),
    'rect_5x1_s2x1_t_bf16': dict(fwd='mfma_bf16 64x64 s1', dgrad='mfma_bf16 64x64 s1', wgrad='mfma_bf16 64x64 s1', pair={0: 'conv_pair_bf16'}),
    'rect_3x5_s1x2_t_bf16': dict(fwd='mfma_bf16 128x32 s1', dgrad='mfma_bf16 128x32 s1', wgrad='mfma_bf16 64x64 s1', pair={0: 'conv_pair_bf16'}),
    'rect_stride3_t_bf16': dict(fwd='mfma_bf16 64x64 s1', dgrad='mfma_bf16 64x64 s1', wgrad='mfma_bf16 64x64 s1', pair={0: 'conv_pair_bf16'}),
    'rect_explicit_pad_t_bf16': dict(fwd='mfma_bf16 64x64 s1', dgrad='mfma_bf16 64x64 s1', wgrad='mfma_bf16 64x64 s1', pair={0: 'conv_pair_bf16'}),
}
ROWS += [r._replace(name=r.name + '_t', transposed=True, expect=RECT_EXPECT.get(r.name + '_t', r.expect)) for r in ROWS if r.name.startswith('rect_')]
ROWS += [r._replace(name=r.name + '_bf16', storage='bf16', expect=RECT_EXPECT.get(r.name + '_bf16', r.expect)) for r in ROWS
         if r.name.startswith('rect_') and not r.name.startswith('rect_direct')]

# The shapes of test_conv_bf16_big_tiles / _wide_tiles / test_deconv_bf16_*_tiles (tests/test_gpu_ops.py): the 128 x 128 and 256 x 128
# kernels need 192 to 256 tiles, which no row under MAX_FLOP has with a long K.  Those tests run them; the table states their paths
# and the tests take their premises from here (``premise``).
BIG_ROWS = [
    row('big_conv', 'test_conv_bf16_big_tiles', _sq(32, 64, 64, 64, 128, 5, 2), dict(fwd='mfma_bf16 128x128 s1', dgrad='mfma_bf16 64x64 s1', wgrad='mfma_bf16 128x128 s32 red=plain'), storage='bf16'),
    row('big_deconv', 'test_deconv_bf16_big_tiles', _sq(16, 64, 64, 128, 128, 5, 2), dict(fwd='mfma_bf16 128x128 s1', dgrad='mfma_bf16 64x64 s1', wgrad='mfma_bf16 128x128 s16 red=plain'), True, 'bf16'),
    row('wide_conv_a', 'test_conv_bf16_wide_tiles', _sq(48, 64, 64, 64, 128, 5, 2), dict(fwd='glds_bf16 256x128 s1'), storage='bf16'),
    row('wide_conv_b', 'test_conv_bf16_wide_tiles', _sq(52, 62, 62, 56, 96, 5, 2), dict(fwd='glds_bf16 256x128 s1'), storage='bf16'),
    row('wide_conv_c', 'test_conv_bf16_wide_tiles', _sq(12, 64, 64, 128, 160, 5, 2), dict(dgrad='glds_bf16 256x128 s1'), storage='bf16'),
    row('wide_conv_d', 'test_conv_bf16_wide_tiles', _sq(13, 63, 61, 96, 160, 5, 2), dict(dgrad='glds_bf16 256x128 s1'), storage='bf16'),
    row('wide_conv_e', 'test_conv_bf16_wide_tiles', _sq(48, 32, 32, 160, 128, 3, 1), dict(fwd='glds_bf16 256x128 s1'), storage='bf16'),
    row('wide_deconv_a', 'test_deconv_bf16_wide_tiles', _sq(12, 64, 64, 128, 160, 5, 2), dict(fwd='glds_bf16 256x128 s1'), True, 'bf16'),
    row('wide_deconv_b', 'test_deconv_bf16_wide_tiles', _sq(12, 64, 64, 121, 160, 5, 2), dict(fwd='glds_bf16 256x128 s1'), True, 'bf16'),
]

# B5: epilogues.  (name, adjoint descriptor, storage, fused?)  acg_deconv2d_fwd_bias_act: every activation on the fused rows; a row
# for which acg_deconv2d_fwd_bias_act_ok says no must be refused, not launched.
EPI_ROWS = [
    ('epi_f32', _sq(4, 16, 16, 3, 12, 5, 2), 'f32', True),
    ('epi_bf16', _sq(4, 16, 16, 3, 12, 5, 2), 'bf16', True),
    ('epi_no_wide_n', _sq(2, 16, 16, 40, 32, 5, 2), 'f32', False),        # 40 output channels: the 64 x 64 tile
    ('epi_no_split', _sq(8, 32, 32, 3, 64, 5, 2), 'f32', False),          # 18 K-steps on 64 tiles: the plan splits
]
ACTS = (None, 'relu', 'lrelu', 'tanh')
# acg_*_fwd_stats: (name, descriptor, transposed, groups, blocks > 0?)
STATS_ROWS = [
    ('stats_conv_g1', _sq(8, 16, 16, 8, 32, 5, 1), False, 1, True),
    ('stats_conv_g2', _sq(8, 16, 16, 8, 32, 5, 1), False, 2, True),
    ('stats_deconv_equal', _sq(8, 32, 32, 24, 12, 5, 2), True, 1, True),       # four stride classes of one size
    ('stats_deconv_unequal', _sq(8, 31, 33, 24, 12, 5, 2), True, 1, False),    # odd extents: stats_blocks must return 0 and the entry refuse
]
BN_TOL = dict(stat=1e-4, y=TOL_CONV)      # op_cases.case_conv_bn_stats / test_gpu_conv_inventory.BN_TOL, fp32


def by_name(name):
    return next(r for r in ROWS + BIG_ROWS if r.name == name)


def desc_of(r):
    d = L.ConvDesc(*r.desc)
    if r.storage != 'f32':
        assert d.in_pitch == 0 and d.out_pitch == 0, r.name
    return d


def dtype_of(r):
    return {'f32': L.ACG_F32, 'bf16': L.ACG_BF16, 'bf16_f32': L.dtype2(L.ACG_BF16, L.ACG_F32)}[r.storage]


def which_of(r, contraction):
    """ACG_CONV_* of a layer's contraction on the row's descriptor (a transposed row: the adjoint)."""
    w = {'fwd': L.CONV_FWD, 'dgrad': L.CONV_DGRAD, 'wgrad': L.CONV_WGRAD}[contraction]
    return {L.CONV_FWD: L.CONV_DGRAD, L.CONV_DGRAD: L.CONV_FWD}.get(w, w) if r.transposed else w


def flop(r):
    b, h, w, cin, oh, ow, cout, kh, kw = r.desc[:9]
    return 2.0 * b * oh * ow * kh * kw * cin * cout


# ---- paths -----------------------------------------------------------------------------------------------------------------------
def path_str(p):
    """An acg_conv_path - a _lib.ConvPath, or the dict test_conv_paths_cpu parses out of a conv_path_sweep line - as the table
    writes it."""
    g = (lambda k: p[k]) if isinstance(p, dict) else (lambda k: getattr(p, k))
    fam = L.ConvPath.FAMILIES[g('family')]
    if fam == 'direct':
        return 'direct nb%d' % g('direct_nb')
    s = '%s %dx%d s%d' % (fam, g('tile_rows'), g('tile_cols'), g('splits'))
    if g('ragged'):
        s += ' ragged'
    if fam == 'mfma_f32' and not g('nvec'):
        s += ' novec'
    for k in ('lin', 'compact', 'merged'):
        if g(k):
            s += ' ' + k
    if g('reduce'):
        s += ' red=' + L.ConvPath.REDUCES[g('reduce')]
    return s


def query(lib, r, contraction, as_pair_a=False):
    p = L.ConvPath()
    d = desc_of(r)
    lib.conv2d_path(ctypes.byref(d), which_of(r, contraction), dtype_of(r), 1 if as_pair_a else 0, ctypes.byref(p))
    return p


HOW = ('the planner has moved this shape to another kernel, so the variant the row is there for has lost its case: find a shape that '
       'reaches it again (tools/conv_path_sweep.hip prints every row\'s path without a GPU) - do not copy the new answer into the table')


def check_premise(lib, r):
    """The row's expectations against acg_conv2d_path / acg_conv2d_pair_path: a failure, never a skip."""
    off = []
    for c in ('fwd', 'dgrad', 'wgrad'):
        if c in r.expect:
            got = path_str(query(lib, r, c))
            if got != r.expect[c]:
                off.append('%s: expected "%s", the library answers "%s"' % (c, r.expect[c], got))
    d = desc_of(r)
    for flags, kind in r.expect.get('pair', {}).items():
        got = L.PAIR_KINDS[lib.conv2d_pair_path(ctypes.byref(d), 1 if r.transposed else 0, dtype_of(r), flags)]
        if got != kind:
            off.append('pair flags %d: expected %s, the library answers %s' % (flags, kind, got))
    assert not off, 'row %s (%s):\n  %s\n%s' % (r.name, r.why, '\n  '.join(off), HOW)


_TILE = {'128x32': 'narrow', '64x64': 'wide', '128x128': 'big', '256x128': 'glds'}
_MODE = {L.CONV_FWD: 'FWD', L.CONV_DGRAD: 'DGRAD', L.CONV_WGRAD: 'WGRAD'}


def _variant(r, contraction, s):
    """The launch statement (kernel instantiation) a path string of a row's contraction names, plus its reduction."""
    mode = _MODE[which_of(r, contraction)]
    t = s.split()
    out = []
    if 'merged' in t:          # the merged input gradient runs as a stride-1 forward contraction
        mode = 'FWD'
    if t[0] == 'direct':
        out.append('direct_%s<%s>' % (mode.lower(), t[1][2:]))
    elif t[0] == 'mfma_f32':
        sw = [k for k in ('ragged', 'novec', 'lin') if k in t]
        out.append('conv_mfma_f32<%s,%s%s>' % (mode, t[1], ''.join(',' + k for k in sw)))
    elif t[0] == 'mfma_bf16':
        out.append('conv_mfma_bf16<%s,%s>' % (mode, t[1]))
    else:
        out.append('conv_glds_bf16<%s>' % mode)
    red = [k[4:] for k in t if k.startswith('red=')]
    if red:
        out.append({'plain': 'splitk_reduce', 'bf16': 'splitk_reduce_bf16',
                    'cols': 'splitk_reduce_cols<%s>' % ('bf16' if r.storage == 'bf16' else 'float')}[red[0]])
    return out


def variants_of(r):
    """Every launch statement the row's expectations say it reaches."""
    out = []
    for c in ('fwd', 'dgrad', 'wgrad'):
        if c in r.expect:
            out += _variant(r, c, r.expect[c])
    for flags, kind in r.expect.get('pair', {}).items():
        a, b = r.expect['dgrad'].split() if 'dgrad' in r.expect else None, r.expect['wgrad'].split() if 'wgrad' in r.expect else None
        mode = 'FWD' if r.transposed else 'DGRAD'
        if kind == 'direct_pair':
            out.append('direct_pair<%s>' % a[1][2:])
        elif kind == 'conv_pair_f32':
            sw = 'ragged' if 'ragged' in a else ('lin' if 'lin' in a else 'plain')
            out.append('conv_pair_f32<%s,%s,%s,%s>' % (mode, a[1], b[1], sw))
        elif kind == 'conv_pair_bf16':
            out.append('conv_pair_bf16<%s,%s,%s>' % (mode, a[1], b[1]))
    return out


# ---- operands and the float64 reference --------------------------------------------------------------------------------------------
def conv_ref(a, w, d):
    """float64 conv of the descriptor: F.conv2d with explicit F.pad and tuple strides, cropped to the descriptor's output extent."""
    pb = max((d.out_h - 1) * d.stride_h + d.kh - d.pad_top - d.in_h, 0)
    pr = max((d.out_w - 1) * d.stride_w + d.kw - d.pad_left - d.in_w, 0)
    xn = F.pad(a.permute(0, 3, 1, 2), (d.pad_left, pr, d.pad_top, pb))
    y = F.conv2d(xn.contiguous(), w.permute(3, 2, 0, 1).contiguous(), stride=(d.stride_h, d.stride_w))[:, :, :d.out_h, :d.out_w]
    assert y.shape[2:] == (d.out_h, d.out_w), (y.shape, d.key())
    return y.permute(0, 2, 3, 1).contiguous()


class Layer:
    """Seeded operands of a descriptor's geometry (rounded to bf16 for bf16 storage) and their float64 images under its conv C:
    C(A), C^T(B) and dW(A, B).  A conv's fwd / dgrad / wgrad are C(A), C^T(B), dW; a transposed layer's are C^T(B), C(A), dW with
    x = B and dy = A."""

    def __init__(self, d, half, seed, device):
        r = (lambda t: t.bfloat16().float()) if half else (lambda t: t)
        g = torch.Generator().manual_seed(seed)
        self.A = r(torch.rand((d.batch, d.in_h, d.in_w, d.in_c), generator=g, dtype=torch.float64).float() * 2 - 1).to(device)
        self.B = r(torch.randn((d.batch, d.out_h, d.out_w, d.out_c), generator=g, dtype=torch.float64).float()).to(device)
        self.w = r(torch.randn((d.kh, d.kw, d.in_c, d.out_c), generator=g, dtype=torch.float64).float() * 0.1).to(device)
        a, w = self.A.double().requires_grad_(True), self.w.double().requires_grad_(True)
        y = conv_ref(a, w, d)
        self.CA = y.detach()
        self.CtB, self.dW = torch.autograd.grad(y, [a, w], self.B.double())


_LAYERS = {}


def layer(r, device):
    """One Layer per (geometry, storage, device) for the whole run: computed once, shared, left unchanged."""
    geo = L.ConvDesc(*r.desc)
    geo.in_pitch = geo.out_pitch = geo.dgrad_c = geo.adj_dgrad_c = 0
    key = (geo.key(), r.storage != 'f32', str(device))
    if key not in _LAYERS:
        _LAYERS[key] = Layer(geo, r.storage != 'f32', 101 + len(_LAYERS), device)
    return _LAYERS[key]


def _r8(c):
    return (c + 7) // 8 * 8


class Runner:
    """A row's contractions through the full-descriptor entries of abi_call.Abi, each against float64, with the pad channels and the
    channels beyond a limit held to the sentinel and every workspace's canary checked."""

    def __init__(self, abi, r, figures=None, dy_pad=X_PAD):
        """``dy_pad``: what the fp32 pad channels of the out-side tensors hold (acgan_hip.h wants zeros in those of dy)."""
        from abi_call import Abi
        self.r, self.d, self.half, self.dy_pad = r, desc_of(r), r.storage != 'f32', dy_pad
        self.abi = Abi(abi.lib, abi.device, conv_dtype=L.ACG_BF16 if self.half else L.ACG_F32)
        self.store = torch.bfloat16 if self.half else torch.float32
        self.lay = layer(r, abi.device)
        self.ws, self.figures = [], figures if figures is not None else {}

    def pitch(self, side):
        d = self.d
        c, p = (d.in_c, d.in_pitch) if side == 'in' else (d.out_c, d.out_pitch)
        return _r8(c) if self.half else (p or c)

    def tensor(self, side, t):
        out = torch.full(t.shape[:-1] + (self.pitch(side),), 0.0 if self.half else (X_PAD if side == 'in' else self.dy_pad), dtype=self.store, device=t.device)
        out[..., :t.shape[-1]] = t.to(self.store)
        return out

    def output(self, side, dtype=None):
        d = self.d
        shape = (d.batch, d.in_h, d.in_w) if side == 'in' else (d.batch, d.out_h, d.out_w)
        return torch.full(shape + (self.pitch(side),), SENTINEL, dtype=dtype or self.store, device=self.abi.device)

    def keep(self, *ws):
        self.ws += [w for w in ws if w is not None]

    def done(self):
        from abi_call import Abi
        self.abi.sync()
        for w in self.ws:
            Abi.canary_intact(w)
        self.ws = []

    def close(self, got, want, tol, tag):
        from op_cases import close
        tag = '%s %s' % (self.r.name, tag)
        want = want.to(got.device)
        err = float((got.double() - want).abs().max() / max(float(want.abs().max()), 1e-30))
        self.figures[tag] = max(self.figures.get(tag, 0.0), err)
        print('%-60s rel err %.3e (bar %.1e)' % (tag, err, tol))
        close(got, want, tol, tag)

    def check_out(self, got, ref, c, n, tag, tol=None):
        """``got`` [.., pitch] started at SENTINEL: channels [0, n) against ``ref``; [n, c) and the pad channels [c, pitch) untouched."""
        tol = tol if tol is not None else (TOL_BF16 if got.dtype == torch.bfloat16 else TOL_CONV)
        self.close(got[..., :n].float(), ref[..., :n], tol, tag)
        sent = torch.tensor(SENTINEL, dtype=got.dtype)
        if n < c:
            assert bool((got[..., n:c].cpu() == sent).all()), '%s %s: channels [%d, %d) at or beyond the limit were written' % (self.r.name, tag, n, c)
        if got.shape[-1] > c:
            assert bool((got[..., c:].cpu() == sent).all()), '%s %s: pad channels [%d, %d) were written' % (self.r.name, tag, c, got.shape[-1])

    @staticmethod
    def bitwise(a, b, tag):
        a, b = a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)
        assert a.shape == b.shape and bool(torch.equal(a, b)), '%s: not bit-identical (%d bytes differ)' % (tag, int((a != b).sum()))

    # operands of the layer's contractions
    def fwd_io(self):
        lay = self.lay
        return (self.tensor('out', lay.B), lay.CtB, 'in') if self.r.transposed else (self.tensor('in', lay.A), lay.CA, 'out')

    def dgrad_io(self):
        lay, d = self.lay, self.d
        if self.r.transposed:
            return self.tensor('in', lay.A), lay.CA, 'out', d.out_c, d.adj_dgrad_c or d.out_c
        return self.tensor('out', lay.B), lay.CtB, 'in', d.in_c, d.dgrad_c or d.in_c

    def wgrad_io(self):
        lay = self.lay
        return (self.tensor('out', lay.B), self.tensor('in', lay.A)) if self.r.transposed else (self.tensor('in', lay.A), self.tensor('out', lay.B))

    def dw0(self, seed):
        return torch.randn(self.lay.w.shape, generator=torch.Generator().manual_seed(seed)).to(self.abi.device)

    def fwd(self):
        x, ref, side = self.fwd_io()
        c = ref.shape[-1]
        if self.r.storage == 'bf16_f32':
            y = self.output(side, torch.float32)
            self.keep(self.abi.fwd_d(self.d, self.r.transposed, x, self.lay.w, y, dtype_of(self.r)))
            self.done()
            self.close(y[..., :c], ref, TOL_CONV, 'fwd (bf16 operands, fp32 result)')
            return
        y = self.output(side)
        self.keep(self.abi.fwd_d(self.d, self.r.transposed, x, self.lay.w, y))
        self.done()
        self.check_out(y, ref, c, c, 'fwd')

    def dgrad(self):
        dy, ref, side, c, n = self.dgrad_io()
        dx = self.output(side)
        self.keep(self.abi.dgrad_d(self.d, self.r.transposed, dy, self.lay.w, dx))
        self.done()
        self.check_out(dx, ref, c, n, 'dgrad')
        return dx

    def wgrad(self):
        x, dy = self.wgrad_io()
        for acc in self.r.acc:
            dw0 = self.dw0(23)
            dw = dw0.clone()
            self.keep(self.abi.wgrad_d(self.d, self.r.transposed, x, dy, dw, acc))
            self.done()
            self.close(dw, acc * dw0.double() + self.lay.dW.to(dw.device), TOL_CONV, 'wgrad accumulate %g' % acc)

    def pair(self, flags, slab_entries=True):
        """acg_(de)conv2d_bwd_pair with a flag word: bit-equal to the separate entries, and against float64."""
        abi, d, t = self.abi, self.d, self.r.transposed
        dy, ref, side, c, n = self.dgrad_io()
        x, dyw = self.wgrad_io()
        acc = self.r.acc[-1]
        dw0 = self.dw0(13)
        dx, dw = self.output(side), dw0.clone()
        wsd, wsw = abi.bwd_pair_d(d, t, dy, self.lay.w, x, None if flags & 2 else dx, None if flags & 1 else dw, acc, flags)
        self.keep(wsd, wsw)
        tag = 'pair flags %d' % flags
        if flags & 2:
            sep, _ = abi.dgrad_slabs_d(d, t, dy, self.lay.w, L.SLABS_QUADS if flags & 4 else L.SLABS_ROWS)
            self.keep(sep)
            self.done()
            self.bitwise(wsd, sep, '%s %s: input-gradient slabs vs acg_*_dgrad_slabs' % (self.r.name, tag))
        else:
            dx_sep = self.output(side)
            self.keep(abi.dgrad_d(d, t, dy, self.lay.w, dx_sep))
            self.done()
            self.bitwise(dx, dx_sep, '%s %s: dx vs the separate input gradient' % (self.r.name, tag))
            self.check_out(dx, ref, c, n, tag + ' dx')
        if flags & 1:
            sep, _ = abi.wgrad_slabs_d(d, t, x, dyw)
            self.keep(sep)
            self.done()
            self.bitwise(wsw, sep, '%s %s: weight-gradient slabs vs acg_*_wgrad_slabs' % (self.r.name, tag))
        else:
            dw_sep = dw0.clone()
            self.keep(abi.wgrad_d(d, t, x, dyw, dw_sep, acc))
            self.done()
            self.bitwise(dw, dw_sep, '%s %s: dw vs the separate weight gradient' % (self.r.name, tag))
            self.close(dw, acc * dw0.double() + self.lay.dW.to(dw.device), TOL_CONV, tag + ' dw')

    def pair_refused(self, flags):
        """A flag word for which acg_conv2d_pair_path answers 'refused': the entry must say so too (an error, not a launch of something else)."""
        dy, _, side, _, _ = self.dgrad_io()
        x, _ = self.wgrad_io()
        try:
            self.keep(*self.abi.bwd_pair_d(self.d, self.r.transposed, dy, self.lay.w, x, None if flags & 2 else self.output(side), None if flags & 1 else self.dw0(13), 0.0, flags))
        except L.AcgError:
            self.abi.sync()
            return
        raise AssertionError('%s pair flags %d: acg_conv2d_pair_path answers "refused", the entry ran' % (self.r.name, flags))


def case_row(abi, r, figures=None, pair_flags=None):
    """Every contraction the row lists.  ``pair_flags``: the flag words to run (None: all the row lists; the C oracle knows 0 and 1)."""
    assert flop(r) <= MAX_FLOP, '%s: %.2f GFLOP is above the table\'s cost limit' % (r.name, flop(r) / 1e9)
    run = Runner(abi, r, figures)
    if 'fwd' in r.expect:
        run.fwd()
    if 'dgrad' in r.expect:
        run.dgrad()
    if 'wgrad' in r.expect:
        run.wgrad()
    for flags, kind in r.expect.get('pair', {}).items():
        if pair_flags is None or flags in pair_flags:
            run.pair_refused(flags) if kind == 'refused' else run.pair(flags)


def planned(lib, r, pair_flags=(0,)):
    """What the planner answers for a row (acg_conv2d_path / acg_conv2d_pair_path; nothing is launched): the ConvPath of the layer's
    three contractions under 'fwd', 'dgrad', 'wgrad', and {flag word: kind} under 'pair'.  A valid descriptor the planner refuses
    raises (AcgError)."""
    d = desc_of(r)
    out = {c: query(lib, r, c) for c in ('fwd', 'dgrad', 'wgrad')}
    out['pair'] = {f: L.PAIR_KINDS[lib.conv2d_pair_path(ctypes.byref(d), 1 if r.transposed else 0, dtype_of(r), f)] for f in pair_flags}
    return out


def case_planned(abi, lib, r, figures=None, pair_flags=(0,), max_flop=MAX_FLOP, dy_pad=0.0):
    """A row WITHOUT expectations (tests/conv_random_cases.py): all three contractions, and the paired entry at every flag word of
    ``pair_flags`` - as case_row runs it where acg_conv2d_pair_path of ``lib`` names a kind, and held to its refusal where the query
    answers 'refused'.  ``lib`` answers the queries (libacgan_hip.so; they need no GPU), ``abi`` runs the row (the library on a GPU,
    or the C oracle, which knows the flag words 0 and 1).  The out-side pad channels hold ``dy_pad``: zeros, as acgan_hip.h asks of
    dy.  -> ``planned``."""
    assert not r.expect and flop(r) <= max_flop, '%s: %.1f MFLOP' % (r.name, flop(r) / 1e6)
    plan = planned(lib, r, pair_flags)
    run = Runner(abi, r, figures, dy_pad=dy_pad)
    run.fwd()
    run.dgrad()
    run.wgrad()
    for flags, kind in plan['pair'].items():
        run.pair_refused(flags) if kind == 'refused' else run.pair(flags)
    return plan


# ---- the uniform_k / uniform_w switches (acgan_conv_plan.h): shared by the variant tests and the random sweep -----------------------
PLAN_FIELDS = ('family', 'tile_rows', 'tile_cols', 'tiles', 'classes', 'nk', 'splits', 'ragged', 'nvec', 'lin', 'compact', 'merged', 'reduce', 'direct_nb')


@contextlib.contextmanager
def switches(lib, uk=1, uw=1):
    """acg_conv2d_uniform_k(uk) and acg_conv2d_uniform_w(uw) for the block; both back on afterwards, whatever happens inside."""
    lib.conv2d_uniform_k(uk)
    lib.conv2d_uniform_w(uw)
    try:
        yield
    finally:
        lib.conv2d_uniform_k(1)
        lib.conv2d_uniform_w(1)


def same_plan(on, off, tag, fields=PLAN_FIELDS):
    """Two answers of the path query for one contraction, under different switches: no plan field may move."""
    for f in fields:
        assert getattr(on, f) == getattr(off, f), '%s: the switch moved %s from %d to %d' % (tag, f, getattr(off, f), getattr(on, f))


def same_bits(a, b, tag, how):
    """Two {name: tensor or None} results of one launch: the same names, and every tensor bit for bit."""
    assert sorted(a) == sorted(b), (tag, sorted(a), sorted(b))
    for k in a:
        if a[k] is not None or b[k] is not None:
            Runner.bitwise(a[k], b[k], '%s: %s %s' % (tag, k, how))


def both_ways(lib, tag, fn, on, off):
    """``fn()`` -> {name: tensor} under switches(**on), then under switches(**off): bit-identical.  -> the result with ``on``."""
    with switches(lib, **on):
        a = fn()
    with switches(lib, **off):
        b = fn()
    same_bits(a, b, tag, 'with the variant on vs off')
    return a


def run_once(run, contraction, acc=0.5):
    """One contraction of a Runner's row through its plain entry, checked against float64 -> {name: tensor}: the result and the
    workspace (the slabs of a split plan).  Outputs start at SENTINEL, so pad channels are part of what is compared; a weight gradient
    accumulates ``acc`` times a seeded dw0, or with ``acc`` 0 writes into a sentinel-filled dw (the launch owns every bit)."""
    abi, d, t, w = run.abi, run.d, run.r.transposed, run.lay.w
    if contraction == 'fwd':
        x, ref, side = run.fwd_io()
        y = run.output(side)
        ws = abi.fwd_d(d, t, x, w, y)
        run.keep(ws)
        run.done()
        run.check_out(y, ref, ref.shape[-1], ref.shape[-1], 'fwd')
        return dict(y=y, ws=ws)
    if contraction == 'dgrad':
        dy, ref, side, c, n = run.dgrad_io()
        dx = run.output(side)
        ws = abi.dgrad_d(d, t, dy, w, dx)
        run.keep(ws)
        run.done()
        run.check_out(dx, ref, c, n, 'dgrad')
        return dict(dx=dx, ws=ws)
    x, dy = run.wgrad_io()
    dw0 = run.dw0(23) if acc else torch.full(w.shape, SENTINEL, device=abi.device)
    dw = dw0.clone()
    ws = abi.wgrad_d(d, t, x, dy, dw, acc)
    run.keep(ws)
    run.done()
    run.close(dw, acc * dw0.double() + run.lay.dW.to(dw.device), TOL_CONV, 'wgrad accumulate %g' % acc)
    return dict(dw=dw, ws=ws)


def _act(t, act, leak=0.2):
    return {None: lambda v: v, 'relu': torch.relu, 'lrelu': lambda v: torch.where(v > 0, v, leak * v), 'tanh': torch.tanh}[act](t)


def case_epi(abi, name, desc, storage, fused, figures=None, dy_pad=X_PAD):
    """acg_deconv2d_fwd_bias_act on an adjoint descriptor: every activation against float64 where acg_deconv2d_fwd_bias_act_ok says
    yes; where it says no the entry must refuse (ACG_ERR_UNSUPPORTED) and leave y alone."""
    r = row(name, 'fused bias + activation', desc, {}, transposed=True, storage=storage)
    run = Runner(abi, r, figures, dy_pad=dy_pad)
    d, lay = run.d, run.lay
    ok = run.abi.lib.deconv2d_fwd_bias_act_ok(ctypes.byref(d), dtype_of(r))
    assert bool(ok) == fused, 'row %s: acg_deconv2d_fwd_bias_act_ok answers %d.  %s' % (name, ok, HOW)
    x = run.tensor('out', lay.B)
    bias = (torch.randn((d.in_c,), generator=torch.Generator().manual_seed(5)) * 0.5).to(abi.device)
    for act in ACTS:
        y = torch.full((d.batch, d.in_h, d.in_w, d.in_pitch or d.in_c), SENTINEL, device=abi.device)      # fp32 rows at the adjoint's in_pitch
        if not fused:
            try:
                run.abi.fwd_bias_act_d(d, x, lay.w, bias, y, act, 0.2)
            except L.AcgError as e:
                assert '(code 4)' in str(e), e
                run.abi.sync()
                assert bool((y == SENTINEL).all()), name + ': a refused call wrote its output'
                continue
            raise AssertionError(name + ': the entry launched a shape acg_deconv2d_fwd_bias_act_ok refuses')
        run.abi.fwd_bias_act_d(d, x, lay.w, bias, y, act, 0.2)
        run.done()
        run.check_out(y, _act(lay.CtB + bias.double().to(lay.CtB.device), act), d.in_c, d.in_c, 'bias + %s' % act, TOL_CONV)


def case_stats(abi, name, desc, transposed, groups, provided, figures=None, dy_pad=X_PAD):
    """acg_(de)conv2d_fwd_stats + acg_bn_act_fwd_partials against float64 BatchNorm of the conv output as stored (the bars of
    op_cases.case_conv_bn_stats); where acg_conv2d_stats_blocks returns 0 the entry must refuse."""
    from abi_call import _p
    r = row(name, 'statistics epilogue', desc, {}, transposed=transposed)
    run = Runner(abi, r, figures, dy_pad=dy_pad)
    d, lay, lib = run.d, run.lay, run.abi.lib
    which = L.CONV_DGRAD if transposed else L.CONV_FWD
    nblk = lib.conv2d_stats_blocks(ctypes.byref(d), which, L.ACG_F32, groups)
    assert (nblk > 0) == provided, 'row %s: acg_conv2d_stats_blocks answers %d.  %s' % (name, nblk, HOW)
    x, ref, side = run.fwd_io()
    c = ref.shape[-1]
    conv_out = run.output(side)
    if not provided:
        part = torch.full((groups * 64 * 2 * c,), SENTINEL, device=abi.device)
        ws, n = run.abi.conv_ws(d, which)
        fn = lib.deconv2d_fwd_stats if transposed else lib.conv2d_fwd_stats
        try:
            fn(_p(x), _p(lay.w), _p(conv_out), ctypes.byref(d), L.ACG_F32, _p(ws), n, _p(part), groups, run.abi.stream())
        except L.AcgError as e:
            assert '(code 4)' in str(e), e
            run.abi.sync()
            assert bool((conv_out == SENTINEL).all()) and bool((part == SENTINEL).all()), name + ': a refused call wrote'
            return
        raise AssertionError(name + ': the entry launched a shape that provides no partials')
    part, nblk, brows, rrows, ws = run.abi.fwd_stats_d(d, transposed, x, lay.w, conv_out, groups)
    run.keep(ws)
    beta = (torch.randn((c,), generator=torch.Generator().manual_seed(11)) * 0.5).to(abi.device)
    rows_n = conv_out.numel() // conv_out.shape[-1]
    yb = torch.zeros_like(conv_out)
    mean, rstd = run.abi.empty(groups * c), run.abi.empty(groups * c)
    lib.bn_act_fwd_partials(_p(conv_out), _p(beta), _p(part), nblk, brows, rrows, _p(yb), _p(mean), _p(rstd), rows_n, c, conv_out.shape[-1],
                            yb.shape[-1], groups, 1e-3, L.ACT_RELU, 0.2, L.dtype2(L.ACG_F32, L.ACG_F32), run.abi.stream())
    run.done()
    run.check_out(conv_out, ref, c, c, 'stats conv')
    rows = conv_out[..., :c].double().reshape(groups, -1, c)
    m, v = rows.mean(1), rows.var(1, unbiased=False)
    run.close(mean, m.reshape(-1), BN_TOL['stat'], 'bn mean')
    run.close(rstd, (1.0 / torch.sqrt(v + 1e-3)).reshape(-1), BN_TOL['stat'], 'bn rstd')
    want = torch.relu((rows - m[:, None]) / torch.sqrt(v[:, None] + 1e-3) + beta.double()).reshape(conv_out[..., :c].shape)
    run.close(yb[..., :c], want, BN_TOL['y'], 'bn y')


def sweep_queries():
    """The table as the lines tools/conv_path_sweep.hip reads."""
    out = []
    for r in ROWS + BIG_ROWS:
        ints = ' '.join(str(v) for v in r.desc)
        for c in ('fwd', 'dgrad', 'wgrad'):
            if c in r.expect:
                out.append('path %s:%s %d %d 0 %s' % (r.name, c, which_of(r, c), dtype_of(r), ints))
        for flags in r.expect.get('pair', {}):
            out.append('pair %s %d %d %d %s' % (r.name, 1 if r.transposed else 0, dtype_of(r), flags, ints))
    for name, desc, storage, _ in EPI_ROWS:
        out.append('epi %s %d %s' % (name, L.ACG_BF16 if storage == 'bf16' else L.ACG_F32, ' '.join(str(v) for v in desc)))
    for name, desc, transposed, groups, _ in STATS_ROWS:
        out.append('stats %s %d %d %d %s' % (name, L.CONV_DGRAD if transposed else L.CONV_FWD, L.ACG_F32, groups, ' '.join(str(v) for v in desc)))
    return out


if __name__ == '__main__':
    print('\n'.join(sweep_queries()))
