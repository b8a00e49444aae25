"""GPU sweep of the random conv sample (tests/conv_random_cases.py): 400 seeded descriptors nobody picked by hand, CHUNK rows per test.

A random row has no premise.  The test asks the planner what the row reaches and runs that; for every row
  * forward, input gradient and weight gradient (accumulate 0 and 0.5) against the float64 reference of the operands as stored, at
    TOL_CONV / TOL_BF16 as they are, with the sentinel checks on pad channels and channels beyond a limit and the canary behind every
    workspace (conv_path_cases.Runner);
  * the paired entry at each flag word of 0, 1, 2 that acg_conv2d_pair_path does not answer 'refused': bit-equal to the separate
    entries, and against float64;
  * fp32 rows whose plan reports uniform_k or uniform_w on a contraction: that contraction with the switches on, then off, into
    sentinel-filled outputs - results, pad channels and workspace bit for bit - and no other plan field moves with the switch;
  * fp32 rows on a 64-wide tile: two runs of each such contraction into fresh sentinel-filled buffers, bit for bit, workspace
    included (the transposed LDS stores issued from inline assembly);
  * transposed rows for which acg_deconv2d_fwd_bias_act_ok says yes: the fused bias + activation entry at all four activations;
    fp32 rows for which acg_conv2d_stats_blocks answers more than 0 at one group: the statistics epilogue and the BatchNorm behind it.
No row is skipped or expected to fail, and an AcgError on a valid descriptor fails its chunk.  A chunk runs all its rows and then
reports every row that failed.  A row that fails here and passes on the oracle (test_conv_random_cpu.py) is a bug of a kernel or of the
planner: reduce it, add it to conv_path_cases.ROWS under a name, fix the cause.

The pad channels of the out-side tensors hold zeros here (acgan_hip.h: "pad channels of dy must be zero"); those of x hold X_PAD."""
import collections
import ctypes
import time

import pytest

import conv_path_cases as P
import conv_random_cases as R
from action_conditioned_gans_amd import _lib as L

pytestmark = pytest.mark.gpu

CHUNKS = R.chunks()
FIGURES = {}      # '<row> <check>' -> largest relative error
PLANS = {}        # row -> conv_path_cases.planned
TIMES = {}        # chunk -> seconds
STATE = dict(broken=None)      # set by an error that is neither a failed check nor a refusal: nothing more is launched after it


def sweep_row(abi, r):
    lib, d = abi.lib, P.desc_of(r)
    plan = PLANS[r.name] = P.case_planned(abi, lib, r, FIGURES, R.PAIR_FLAGS, R.MAX_FLOP)
    if r.storage == 'f32':
        run = P.Runner(abi, r, dy_pad=0.0)
        for c in ('fwd', 'dgrad', 'wgrad'):
            p, tag = plan[c], '%s %s' % (r.name, c)
            if p.uniform_k or p.uniform_w:
                with P.switches(lib, 0, 0):
                    off = P.query(lib, r, c)
                assert (off.uniform_k, off.uniform_w) == (0, 0), '%s: a variant is reported with the switches off' % tag
                P.same_plan(p, off, tag)
                P.both_ways(lib, tag, lambda: P.run_once(run, c, 0.0), dict(uk=1, uw=1), dict(uk=0, uw=0))
            if p.family == L.ConvPath.FAMILIES.index('mfma_f32') and p.tile_cols == 64:
                P.same_bits(P.run_once(run, c, 0.0), P.run_once(run, c, 0.0), tag, 'of two runs of the same launch')
    if r.transposed and lib.deconv2d_fwd_bias_act_ok(ctypes.byref(d), P.dtype_of(r)):
        P.case_epi(abi, r.name, r.desc, r.storage, True, FIGURES, dy_pad=0.0)
    if r.storage == 'f32' and lib.conv2d_stats_blocks(ctypes.byref(d), P.which_of(r, 'fwd'), L.ACG_F32, 1) > 0:
        P.case_stats(abi, r.name, r.desc, r.transposed, 1, True, FIGURES, dy_pad=0.0)


@pytest.mark.parametrize('k', range(len(CHUNKS)))
def test_random_rows(hip_abi, k):
    assert STATE['broken'] is None, 'not run: an earlier chunk ended in an error of the runtime (%s)' % STATE['broken']
    t0, failed = time.perf_counter(), []
    for r in CHUNKS[k]:
        try:
            sweep_row(hip_abi, r)
        except (AssertionError, L.AcgError) as e:
            failed.append('%s %s %s %s: %s' % (r.name, 'transposed' if r.transposed else 'conv', r.storage, r.desc, str(e).splitlines()[0][:300]))
        except Exception as e:
            STATE['broken'] = '%s: %r' % (r.name, e)
            raise
    P._LAYERS.clear()      # the references of this chunk's rows: nothing later reads them
    TIMES[k] = time.perf_counter() - t0
    print('chunk %d: %d rows in %.2f s' % (k, len(CHUNKS[k]), TIMES[k]))
    assert not failed, '%d of %d rows failed:\n  %s' % (len(failed), len(CHUNKS[k]), '\n  '.join(failed))


def test_worst_figures_per_path():
    """Not a check of its own: the largest relative error of this run per (family, tile, mode, storage) beside its bar, and the chunk
    times, for the record (profiles/conv_random/figures.txt)."""
    rows = {r.name: r for c in CHUNKS for r in c}
    worst = collections.defaultdict(float)
    for tag, err in FIGURES.items():
        name, what = tag.split(' ', 1)
        c = next((c for c in ('fwd', 'dgrad', 'wgrad') if what.startswith(c)), None)
        if c is None or name not in PLANS:
            continue      # (the pair, epilogue and statistics checks: the same kernels' figures again)
        p, r = PLANS[name][c], rows[name]
        key = (L.ConvPath.FAMILIES[p.family], '%dx%d' % (p.tile_rows, p.tile_cols) if p.family else '-', P._MODE[P.which_of(r, c)], r.storage)
        worst[key] = max(worst[key], err)
    for key, err in sorted(worst.items()):
        print('worst %-10s %-7s %-5s %-4s %.3e (bar %.0e)' % (key + (err, P.TOL_CONV if key[2] == 'WGRAD' or key[3] == 'f32' else P.TOL_BF16)))
    for k, t in sorted(TIMES.items()):
        print('time chunk %2d %.2f s' % (k, t))
