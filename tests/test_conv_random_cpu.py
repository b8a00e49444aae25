"""The random conv sample (tests/conv_random_cases.py) without a GPU: its premises, before anything goes to one.
  * the sample is the one DIGEST names, every row is a valid descriptor, and the classes it holds by construction are there;
  * tools/conv_path_sweep.hip - the planner's own source compiled for the host under AddressSanitizer and
    UndefinedBehaviorSanitizer, a stand-alone program - answers every query of the sample: a valid descriptor the planner refuses
    is a finding;
  * coverage: what the sample reaches, counted from those answers, against the conditions written out in COVERAGE below.  A sample
    that misses one is mended in the distribution, a quota or the seed - never by trimming the list or the condition;
  * the histogram of launch statements is the committed profiles/conv_random/paths.txt;
  * libacgan_hip.so answers every query as the host build does (the queries launch nothing);
  * every fp32 row runs on the C oracle through conv_path_cases.Runner - forward, input gradient, weight gradient at accumulate 0
    and 0.5, the pair at flag word 0 - against float64 at the GPU test's bars: the references, the operand layouts and the sentinel
    checks hold for the whole sample."""
import collections
import ctypes
import os
import subprocess

import pytest

import conv_path_cases as P
import conv_random_cases as R
from action_conditioned_gans_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS_TXT = os.path.join(ROOT, 'profiles', 'conv_random', 'paths.txt')
ROWS = R.rows()
MIN_CLASS = 5

TILES = ('128x32', '64x64')
# the 26 instantiations of launch_cfg (conv_f32_kernel.h) as conv_path_cases._variant names them
LAUNCH_CFG = (['conv_mfma_f32<FWD,%s%s>' % (t, s) for t in TILES for s in ('', ',lin', ',ragged', ',novec', ',ragged,novec')]
              + ['conv_mfma_f32<%s,%s%s>' % (m, t, s) for m in ('DGRAD', 'WGRAD') for t in TILES for s in ('', ',ragged', ',novec', ',ragged,novec')])
# COVERAGE: launch statement (a prefix of a histogram key) -> the least number of plans of the sample that reach it
COVERAGE = dict(
    [(v, 3) for v in LAUNCH_CFG]
    + [('direct_fwd', 1), ('direct_dgrad', 1), ('direct_wgrad', 1)]
    + [('conv_mfma_bf16<%s,%s>' % (m, t), 1) for m in ('FWD', 'DGRAD') for t in TILES] + [('conv_mfma_bf16<WGRAD,64x64>', 1)]
    + [('splitk_reduce', 1), ('splitk_reduce_bf16', 1), ('splitk_reduce_cols<float>', 1), ('splitk_reduce_cols<bf16>', 1)]
    + [('pair ' + k, 1) for k in ('direct_pair', 'conv_pair_f32', 'conv_pair_bf16', 'two_launches')])
MIN_COMPACT = MIN_MERGED = 3
MIN_UNIFORM = 10      # plans that take a variant, per mode - and plans of the same mode and tile that do not, where the rule declines


@pytest.fixture(scope='module')
def answers(tmp_path_factory):
    """tools/conv_path_sweep.hip built for the host with the sanitizers, and its parsed answers to the sample's queries."""
    out = str(tmp_path_factory.mktemp('conv_random_sweep') / 'conv_path_sweep')
    subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-std=c++17', '-O1', '-g', '--offload-arch=gfx950', '-Xarch_host',
                           '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
                           os.path.join(ROOT, 'tools', 'conv_path_sweep.hip'), '-o', out])
    queries = R.sweep_queries(ROWS)
    res = subprocess.run([out], input='\n'.join(queries) + '\n', capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(queries), 'conv_path_sweep answered %d of %d queries' % (len(lines), len(queries))
    return R.parse_answers(lines)


def test_the_sample_is_the_one_the_digest_names():
    assert len(ROWS) == R.N and len({r.name for r in ROWS}) == R.N
    assert R.rows() == ROWS and R.rows(R.SEED, 50) == ROWS[:50], 'rows() is not deterministic'
    assert R.rows(R.SEED + 1)[-1].desc != ROWS[-1].desc
    assert R.digest(ROWS) == R.DIGEST, ('the sample has changed (digest %s).  If the distribution, a quota or the seed was changed on purpose, check the '
                                        'coverage conditions and set DIGEST; otherwise find what moved the draws' % R.digest(ROWS))


def test_rows_are_valid_descriptors_without_premises():
    for r in ROWS:
        d = P.desc_of(r)      # asserts: no explicit pitch on a bf16 row
        assert R.valid(r.desc) and not r.expect and P.flop(r) <= R.MAX_FLOP <= P.MAX_FLOP, r
        assert not (d.dgrad_c and r.transposed) and not (d.adj_dgrad_c and not r.transposed), r
        assert (d.dgrad_c == 0 or d.dgrad_c < d.in_c) and (d.adj_dgrad_c == 0 or d.adj_dgrad_c < d.out_c), r


def test_every_query_is_answered(answers):
    bad = ['%s %s: error %s' % (k[1], k[2], v['error']) for k, v in answers.items() if k[0] == 'path' and 'error' in v]
    assert not bad, 'the planner refuses valid descriptors:\n  ' + '\n  '.join(bad)
    for r in ROWS:
        assert all(('path', r.name, c) in answers for c in ('fwd', 'dgrad', 'wgrad')), r.name
        assert answers['pair', r.name, 0] != 'refused', '%s: flag word 0 of the pair entry is refused' % r.name
        assert all(answers['pair', r.name, f] in L.PAIR_KINDS for f in R.PAIR_FLAGS), r.name


def test_classes_by_construction(answers):
    n = collections.Counter(c for r in ROWS for c in R.classes_of(r))
    n['limit on a split input gradient'] = sum(1 for r in ROWS if 'limit' in R.classes_of(r) and answers['path', r.name, 'dgrad']['splits'] > 1)
    for c in ('img1x1', 'bigfilter', 'out1', 'stridegtk', 'evens3', 'cin1', 'cout1', 'batch1', 'limit on a split input gradient'):
        assert n[c] >= MIN_CLASS, 'class %s: %d rows, at least %d wanted' % (c, n[c], MIN_CLASS)
    # the quota rows are in the class they were forced into
    for r in ROWS:
        tag = r.name.split('_', 1)[1]
        if tag in ('img1x1', 'bigfilter', 'out1', 'stridegtk', 'evens3', 'cin1', 'cout1', 'batch1'):
            assert tag in R.classes_of(r), r
        if tag == 'limitsplit':
            assert 'limit' in R.classes_of(r) and answers['path', r.name, 'dgrad']['splits'] > 1, (r, answers['path', r.name, 'dgrad'])


def test_coverage_conditions(answers):
    hist = collections.Counter(v for r in ROWS for v in R.variants_of(r, answers))
    count = lambda prefix: sum(n for v, n in hist.items() if v == prefix or v.startswith(prefix + ' ') or (prefix.startswith('direct_') and v.startswith(prefix + '<')))
    short = ['%s: %d of %d' % (v, count(v), n) for v, n in COVERAGE.items() if count(v) < n]
    # each fp32 MFMA instantiation both split and unsplit
    for v in LAUNCH_CFG:
        split = sum(n for k, n in hist.items() if (k == v or k.startswith(v + ' ')) and k.endswith(' split'))
        if split < 1 or count(v) - split < 1:
            short.append('%s: %d split, %d unsplit' % (v, split, count(v) - split))
    plans = [(r, c, answers['path', r.name, c]) for r in ROWS for c in ('fwd', 'dgrad', 'wgrad')]
    f32 = [(P._MODE[P.which_of(r, c)], kv) for r, c, kv in plans if kv['family'] == 'mfma_f32']
    if sum(kv['compact'] for _, kv in f32) < MIN_COMPACT:
        short.append('compact: %d of %d' % (sum(kv['compact'] for _, kv in f32), MIN_COMPACT))
    if sum(kv['merged'] for _, kv in f32) < MIN_MERGED:
        short.append('merged: %d of %d' % (sum(kv['merged'] for _, kv in f32), MIN_MERGED))
    for mode, key in (('FWD', 'uk'), ('DGRAD', 'uk'), ('WGRAD', 'uw')):
        on = collections.Counter(kv['tile'] for m, kv in f32 if m == mode and kv[key] and not kv['merged'])
        off = collections.Counter(kv['tile'] for m, kv in f32 if m == mode and not kv[key] and not kv['merged'])
        if sum(on.values()) < MIN_UNIFORM:
            short.append('%s %s = 1: %d of %d' % (mode, key, sum(on.values()), MIN_UNIFORM))
        short += ['%s %s %s = 0 beside the variant: %d of %d' % (mode, t, key, off[t], MIN_UNIFORM) for t in on if off[t] < MIN_UNIFORM]
    assert not short, 'the sample is short of:\n  %s\n(change the distribution, a quota or the seed - not this list)' % '\n  '.join(short)


def test_histogram_is_the_committed_one(answers):
    want = R.histogram(ROWS, answers)
    have = open(PATHS_TXT).read() if os.path.exists(PATHS_TXT) else ''
    assert have == want, ('profiles/conv_random/paths.txt is not the histogram of the sample under this planner.  Look at what moved, then:\n'
                          '  python tests/conv_random_cases.py | conv_path_sweep | python tests/conv_random_cases.py --histogram > profiles/conv_random/paths.txt\n'
                          + ''.join(sorted(set(want.splitlines(True)) ^ set(have.splitlines(True)))))


PATH_FIELDS = dict(tiles='tiles', classes='classes', nk='nk', splits='splits', ragged='ragged', nvec='nvec', lin='lin', compact='compact', merged='merged',
                   direct_nb='nb', uniform_k='uk', uniform_w='uw', tile_rows='tile_rows', tile_cols='tile_cols')


def test_library_answers_as_the_host_build(answers):
    """libacgan_hip.so itself: acg_conv2d_path, acg_conv2d_pair_path, acg_deconv2d_fwd_bias_act_ok and acg_conv2d_stats_blocks for
    every row, field by field.  Nothing is launched."""
    lib, off = L.get(), []
    for r in ROWS:
        plan, d = P.planned(lib, r, R.PAIR_FLAGS), P.desc_of(r)
        for c in ('fwd', 'dgrad', 'wgrad'):
            p, kv = plan[c], answers['path', r.name, c]
            got = dict({k: getattr(p, k) for k in PATH_FIELDS}, family=L.ConvPath.FAMILIES[p.family], reduce=L.ConvPath.REDUCES[p.reduce])
            want = dict({k: kv[v] for k, v in PATH_FIELDS.items()}, family=kv['family'], reduce=kv['reduce'])
            if got != want:
                off.append('%s %s: library %s, host build %s' % (r.name, c, sorted(set(got.items()) - set(want.items())), sorted(set(want.items()) - set(got.items()))))
        off += ['%s pair flags %d: library %s, host build %s' % (r.name, f, k, answers['pair', r.name, f]) for f, k in plan['pair'].items() if k != answers['pair', r.name, f]]
        if r.transposed and lib.deconv2d_fwd_bias_act_ok(ctypes.byref(d), P.dtype_of(r)) != answers['epi', r.name]:
            off.append('%s: acg_deconv2d_fwd_bias_act_ok' % r.name)
        if r.storage == 'f32' and lib.conv2d_stats_blocks(ctypes.byref(d), P.which_of(r, 'fwd'), L.ACG_F32, 1) != answers['stats', r.name]:
            off.append('%s: acg_conv2d_stats_blocks' % r.name)
    assert not off, '\n  '.join(off[:40])


ORACLE_CHUNKS = R.chunks([r for r in ROWS if r.storage == 'f32'], 40)


@pytest.mark.parametrize('k', range(len(ORACLE_CHUNKS)))
def test_fp32_rows_on_the_oracle(oracle_abi, k):
    """The fp32 rows through the C oracle (the same C ABI, the same descriptors) against the float64 reference at the bars of the
    GPU test; the planner's answers - which flag words the pair entry takes - come from libacgan_hip.so.  Of the pair entry the
    oracle knows the flag words 0 and 1; 0 is run."""
    lib = L.get()
    for r in ORACLE_CHUNKS[k]:
        P.case_planned(oracle_abi, lib, r, pair_flags=(0,), max_flop=R.MAX_FLOP)
