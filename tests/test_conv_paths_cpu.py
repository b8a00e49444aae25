"""The conv path table (tests/conv_path_cases.py) without a GPU:
  * tools/conv_path_sweep.hip - the planner's own source compiled for the host, under AddressSanitizer and
    UndefinedBehaviorSanitizer - answers every query of the table, and every answer is the table's expectation: the premises of
    test_gpu_conv_paths.py hold before anything goes to a GPU;
  * closure: every launch statement of the conv sources has a row, or is listed with the condition that keeps the shipped build
    from reaching it;
  * the fp32 rows of moderate size run on the C oracle against the float64 reference at the GPU test's bars, which proves the
    references, the operand layouts, the sentinel checks and the bars."""
import os
import subprocess

import pytest

import conv_path_cases as P
from action_conditioned_gans_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TILES = ('128x32', '64x64')
# Every launch statement (kernel instantiation) of launch_cfg, launch_mode16 (with launch_glds16), launch_pair, launch_pair16,
# launch_direct, launch_direct_pair, launch_deconv_fwd_epi, launch_deconv_fwd_epi16 and reduce().
REQUIRED = (
    # launch_cfg: FWD has the LIN variant beside the four RAGGED x NVEC ones; DGRAD and WGRAD the four
    ['conv_mfma_f32<FWD,%s%s>' % (t, s) for t in TILES for s in ('', ',lin', ',ragged', ',novec', ',ragged,novec')]
    + ['conv_mfma_f32<%s,%s%s>' % (m, t, s) for m in ('DGRAD', 'WGRAD') for t in TILES for s in ('', ',ragged', ',novec', ',ragged,novec')]
    # launch_mode16 / launch_glds16
    + ['conv_mfma_bf16<%s,%s>' % (m, t) for m in ('FWD', 'DGRAD') for t in ('128x32', '64x64', '128x128')]
    + ['conv_mfma_bf16<WGRAD,64x64>', 'conv_mfma_bf16<WGRAD,128x128>', 'conv_glds_bf16<FWD>', 'conv_glds_bf16<DGRAD>']
    # launch_pair: launch_a x launch_b
    + ['conv_pair_f32<FWD,%s,%s,%s>' % (a, b, s) for a in TILES for b in TILES for s in ('ragged', 'lin', 'plain')]
    + ['conv_pair_f32<DGRAD,%s,%s,%s>' % (a, b, s) for a in TILES for b in TILES for s in ('ragged', 'plain')]
    # launch_pair16
    + ['conv_pair_bf16<%s,%s,%s>' % (m, a, b) for m in ('FWD', 'DGRAD') for a in ('128x32', '64x64', '128x128') for b in ('64x64', '128x128')]
    # launch_direct, launch_direct_pair
    + ['direct_%s<%d>' % (m, nb) for m in ('fwd', 'dgrad', 'wgrad', 'pair') for nb in (1, 8)]
    # the epilogue launches and the reductions
    + ['conv_mfma_f32<DGRAD,128x32,epi>', 'conv_mfma_bf16<DGRAD,128x32,epi>',
       'splitk_reduce', 'splitk_reduce_bf16', 'splitk_reduce_cols<float>', 'splitk_reduce_cols<bf16>'])
# Launch statements no descriptor reaches in the shipped build, with the condition that excludes them.
UNREACHABLE = {
    # pair_supported wants both gathers ragged or neither AND float4-able dense operands.  With A = DGRAD the gathered tensor of A is
    # dy, which is B's dense operand: A ragged means the dy pitch is no multiple of 4, so B's nvec is off and the pair is refused.
    **{'conv_pair_f32<DGRAD,%s,%s,ragged>' % (a, b): 'A ragged <=> dy pitch % 4 != 0 <=> B nvec off: pair_supported refuses' for a in TILES for b in TILES},
    # with A = FWD both contractions have out_c columns (A fewer under adj_dgrad_c): A is never on the wider tile
    **{'conv_pair_f32<FWD,64x64,128x32,%s>' % s: 'A wide needs N > 32 columns, B narrow out_c <= 32, and N <= out_c' for s in ('ragged', 'lin', 'plain')},
}
# Only in -DACG_TUNING builds (never loaded by the package): conv_glds_bf16<MODE, 0 | 1> under ACG_GLDS_VAR, every tile under
# acg_debug_conv_plan, the tap_classes walk under ACG_CONV_TAP_CLASSES.  They are no launch statements of the shipped library.


@pytest.fixture(scope='module')
def sweep(tmp_path_factory):
    """tools/conv_path_sweep.hip built for the host with the sanitizers, and its answers to the table's queries."""
    out = str(tmp_path_factory.mktemp('conv_path_sweep') / 'conv_path_sweep')
    subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-std=c++17', '-O1', '-g', '--offload-arch=gfx950', '-Xarch_host',
                           '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
                           os.path.join(ROOT, 'tools', 'conv_path_sweep.hip'), '-o', out])
    queries = P.sweep_queries()
    res = subprocess.run([out], input='\n'.join(queries) + '\n', capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(queries), 'conv_path_sweep answered %d of %d queries' % (len(lines), len(queries))
    return lines


def _parse(line):
    t = line.split()
    kv = dict(x.split('=') for x in t[3:] if '=' in x)
    if 'error' in kv:
        return 'error %s' % kv['error']
    rows, cols = kv['tile'].split('x')
    return P.path_str(dict(family=L.ConvPath.FAMILIES.index(kv['family']), tile_rows=int(rows), tile_cols=int(cols), splits=int(kv['splits']),
                           ragged=int(kv['ragged']), nvec=int(kv['nvec']), lin=int(kv['lin']), compact=int(kv['compact']),
                           merged=int(kv['merged']), reduce=L.ConvPath.REDUCES.index(kv['reduce']), direct_nb=int(kv['nb'])))


def test_sweep_tool_answers_the_table(sweep):
    """Every query of the table has an answer, and the answer is what the row expects."""
    got, off = {}, []
    for line in sweep:
        t = line.split()
        if t[0] == 'path':
            got[('path', t[1])] = _parse(line)
        elif t[0] == 'pair':
            got[('pair', t[1], int(t[2].split('=')[1]))] = t[3].split('=')[1]
        else:
            got[(t[0], t[1])] = int(t[-1].split('=')[1])
    for r in P.ROWS + P.BIG_ROWS:
        for c in ('fwd', 'dgrad', 'wgrad'):
            if c in r.expect and got.get(('path', '%s:%s' % (r.name, c))) != r.expect[c]:
                off.append('%s %s: expected "%s", the planner answers "%s"' % (r.name, c, r.expect[c], got.get(('path', '%s:%s' % (r.name, c)))))
        for flags, kind in r.expect.get('pair', {}).items():
            if got.get(('pair', r.name, flags)) != kind:
                off.append('%s pair flags %d: expected %s, the planner answers %s' % (r.name, flags, kind, got.get(('pair', r.name, flags))))
    for name, _, _, fused in P.EPI_ROWS:
        if bool(got.get(('epi', name))) != fused:
            off.append('%s: acg_deconv2d_fwd_bias_act_ok = %s' % (name, got.get(('epi', name))))
    for name, _, _, _, provided in P.STATS_ROWS:
        if (got.get(('stats', name), 0) > 0) != provided:
            off.append('%s: acg_conv2d_stats_blocks = %s' % (name, got.get(('stats', name))))
    assert not off, '%d expectations of the table are off:\n  %s\n%s' % (len(off), '\n  '.join(off), P.HOW)


def test_library_answers_the_table():
    """The same premises on libacgan_hip.so itself: the queries launch nothing, so they run without a GPU.  An invalid descriptor
    is the entry's own error, and a flag word the pair entry would refuse is 'refused'."""
    import ctypes
    lib = L.get()
    for r in P.ROWS + P.BIG_ROWS:
        P.check_premise(lib, r)
    bad = L.ConvDesc(*P.by_name('f32_narrow_lin').desc)
    bad.pad_top = bad.kh
    with pytest.raises(L.AcgError, match='code 1'):
        lib.conv2d_path(ctypes.byref(bad), L.CONV_FWD, L.ACG_F32, 0, ctypes.byref(L.ConvPath()))
    assert lib.conv2d_pair_path(ctypes.byref(bad), 0, L.ACG_F32, 0) == 0
    unsplit = P.desc_of(P.by_name('f32_narrow_lin'))
    assert L.PAIR_KINDS[lib.conv2d_pair_path(ctypes.byref(unsplit), 0, L.ACG_F32, 1)] == 'refused'      # flag 1 on an unsplit weight gradient
    assert L.PAIR_KINDS[lib.conv2d_pair_path(ctypes.byref(unsplit), 0, L.ACG_F32, 4)] == 'refused'      # flag 4 without flag 2


def reached():
    out = {}
    for r in P.ROWS + P.BIG_ROWS:
        for v in P.variants_of(r):
            out.setdefault(v, []).append(r.name)
    for name, _, storage, fused in P.EPI_ROWS:
        if fused:
            out.setdefault('conv_mfma_%s<DGRAD,128x32,epi>' % ('bf16' if storage == 'bf16' else 'f32'), []).append(name)
    return out


def test_every_launch_statement_has_a_row():
    """Closure: the variants the table's expectations reach against the list written out above."""
    have = reached()
    assert not set(UNREACHABLE) - set(REQUIRED) and len(set(REQUIRED)) == len(REQUIRED)
    missing = [v for v in REQUIRED if v not in have and v not in UNREACHABLE]
    assert not missing, 'launch statements without a row in tests/conv_path_cases.py: %s' % ', '.join(missing)
    stale = [v for v in UNREACHABLE if v in have]
    assert not stale, 'listed as unreachable, but a row reaches them: %s' % ', '.join(stale)
    unknown = sorted(set(have) - set(REQUIRED))
    assert not unknown, 'the table reaches launch statements the list does not name: %s' % ', '.join(unknown)
    small = [r.name for r in P.ROWS if P.flop(r) > P.MAX_FLOP]
    assert not small, 'rows above the cost limit: %s' % small
    names = [r.name for r in P.ROWS + P.BIG_ROWS]
    assert len(names) == len(set(names))


ORACLE_FLOP = 40e6      # the C oracle is three nested loops in double precision: the rows up to 40 MFLOP
ORACLE_ROWS = [r for r in P.ROWS if r.storage == 'f32' and P.flop(r) <= ORACLE_FLOP]


@pytest.mark.parametrize('r', ORACLE_ROWS, ids=lambda r: r.name)
def test_row_on_the_oracle(oracle_abi, r):
    """The row's contractions through the C oracle (the same C ABI, the same descriptor) against the float64 reference at the bars
    of the GPU test.  Of the pair entry the oracle knows the flag words 0 and 1; 0 is run."""
    P.case_row(oracle_abi, r, pair_flags=(0,))


def test_oracle_rows_cover_the_descriptor_classes():
    names = {r.name for r in ORACLE_ROWS}
    want = {'rect_1x5', 'rect_5x1_s2x1', 'rect_3x5_s1x2', 'rect_stride3', 'rect_explicit_pad', 'rect_direct', 'direct_limit_conv',
            'direct_limit_transposed', 'f32_reduce_cols_limit', 'direct_dgrad_pitched'}
    assert want <= names and {n + '_t' for n in want if n.startswith('rect_')} <= names, sorted(want - names)
