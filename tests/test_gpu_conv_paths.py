"""GPU parity: convolution at every kernel variant and reduction the planner can pick (tests/conv_path_cases.py).  For each row:
the premise first - acg_conv2d_path / acg_conv2d_pair_path must answer the path the row is there for, a failure and never a
skip - then every contraction the row lists against the float64 reference of the operands as stored, the output's pad channels
and the channels at or beyond a limit against a sentinel, every workspace's canary, and the paired entry bit for bit against the
separate ones.  Bars: TOL_CONV for fp32 results and weight gradients, TOL_BF16 for bf16-stored results, as they are.

The direct_limit_* rows fail on the library as it was before make_plan kept limited input gradients off the direct kernels
(direct_dgrad / direct_fwd store every channel)."""
import pytest

import conv_path_cases as P

pytestmark = pytest.mark.gpu

FIGURES = {}      # tag -> largest relative error seen (printed per check; profiles/conv_paths/README.md records a run)


@pytest.mark.parametrize('r', P.ROWS, ids=lambda r: r.name)
def test_conv_path(hip_abi, r):
    P.check_premise(hip_abi.lib, r)
    P.case_row(hip_abi, r, FIGURES)


@pytest.mark.parametrize('r', P.BIG_ROWS, ids=lambda r: r.name)
def test_big_tile_rows_state_their_paths(hip_abi, r):
    """The 128 x 128 / 256 x 128 shapes that tests/test_gpu_ops.py runs: their rows in the table name the kernels they reach."""
    P.check_premise(hip_abi.lib, r)


@pytest.mark.parametrize('name,desc,storage,fused', P.EPI_ROWS, ids=[e[0] for e in P.EPI_ROWS])
def test_deconv_bias_act(hip_abi, name, desc, storage, fused):
    P.case_epi(hip_abi, name, desc, storage, fused, FIGURES)


@pytest.mark.parametrize('name,desc,transposed,groups,provided', P.STATS_ROWS, ids=[e[0] for e in P.STATS_ROWS])
def test_fwd_stats(hip_abi, name, desc, transposed, groups, provided):
    P.case_stats(hip_abi, name, desc, transposed, groups, provided, FIGURES)


def test_worst_figures_per_family():
    """Not a check of its own: the largest error of this run per kernel family beside its bar, for the record."""
    import collections
    worst = collections.defaultdict(float)
    for tag, err in FIGURES.items():
        name = tag.split()[0]
        fam = next((f for f in ('direct', 'bf16', 'rect', 'pair', 'epi', 'stats') if name.startswith(f)), 'f32')
        kind = 'wgrad/dw' if ('wgrad' in tag or tag.endswith(' dw')) else 'activations'
        worst[(fam, kind)] = max(worst[(fam, kind)], err)
    for (fam, kind), err in sorted(worst.items()):
        print('worst %-8s %-12s %.3e' % (fam, kind, err))
