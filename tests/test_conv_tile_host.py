"""The addressing of the convolution kernels without a GPU: csrc/conv_tile.h itself - the geometry, tap tables, row infos, tap
compaction and output map that the three MFMA block programs share - compiled for the host (tools/micro/conv_tile_host.cpp) under
AddressSanitizer and UndefinedBehaviorSanitizer, run for every block of the grid, and held against a brute-force enumeration of
the convolution's definition (oracle/tf_ops.conv_geometry for the padding).  Per output pixel and as SETS, because the K order is
a free permutation:
  * the unmasked (gather, filter) pairs of a row are exactly the in-bounds (input element, filter element) pairs of its pixel -
    the pixel being the one the row's results are WRITTEN to; pad channels beyond C never appear;
  * masked K positions are exactly the out-of-bounds taps and the pad channels; every offset lies inside its tensor;
  * rows at or beyond M carry zero masks;
  * the blocks' rows cover every output pixel - of every stride class - and the output map hits every output element once and no
    pad channel, in the row layout and in the quad slab layout.
Cases are (batch, h, w, cin, cout, k, stride): the smallest shapes that still reach a branch."""
import os
import subprocess

import numpy as np
import pytest

from oracle.tf_ops import conv_geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, DGRAD, WGRAD = 0, 1, 2
TILES = [(64, 64), (128, 32), (256, 128)]      # the three row-tile heights of the kernels, each with a column tile it ships with


def case(which, shape, padding='SAME', unit=4, in_pitch=0, out_pitch=0, dgrad_c=0, compact=0, tap_classes=0, quads=0):
    return dict(which=which, shape=shape, padding=padding, unit=unit, in_pitch=in_pitch, out_pitch=out_pitch, dgrad_c=dgrad_c,
                compact=compact, tap_classes=tap_classes, quads=quads)


GROUPS = [
    [case(FWD, (2, 5, 7, 3, 5, 3, 2)), case(FWD, (2, 5, 7, 3, 5, 3, 2), in_pitch=4), case(FWD, (2, 6, 6, 4, 8, 5, 1), 'VALID'),
     case(FWD, (2, 5, 7, 3, 5, 3, 2), quads=1, out_pitch=8)],
    [case(FWD, (9, 3, 4, 16, 8, 3, 2), compact=1), case(FWD, (8, 2, 2, 64, 16, 3, 1), compact=1), case(FWD, (9, 3, 4, 16, 8, 3, 2), compact=1, quads=1)],
    [case(FWD, (2, 8, 8, 4, 8, 5, 2), tap_classes=1), case(FWD, (2, 7, 9, 4, 8, 3, 2), tap_classes=1)],
    # odd extents: the stride classes have unequal sizes
    [case(DGRAD, (2, 7, 5, 3, 6, 5, 2)), case(DGRAD, (2, 7, 5, 3, 6, 5, 2), dgrad_c=2), case(DGRAD, (2, 6, 6, 4, 4, 3, 1)),
     case(DGRAD, (12, 4, 4, 24, 40, 5, 2), compact=1), case(DGRAD, (2, 7, 5, 3, 6, 5, 2), quads=1, in_pitch=4)],
    [case(WGRAD, (2, 5, 7, 3, 5, 3, 2))],
]
# the first case of each group again with the 16-byte unit of bf16 tensors (8 channels, round8 pitches; no small-map path there)
CASES = [c for g in GROUPS for c in g] + [dict(g[0], unit=8, compact=0) for g in GROUPS]


def _id(c):
    return '%s-%s-%s-u%d%s' % ('FDW'[c['which']], 'x'.join(map(str, c['shape'])), c['padding'], c['unit'],
                              ''.join('-%s%s' % (k, c[k]) for k in ('in_pitch', 'out_pitch', 'dgrad_c', 'compact', 'tap_classes', 'quads') if c[k]))


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('conv_tile_host') / 'conv_tile_host')
    subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-x', 'c++', '-std=c++17', '-O1', '-Xarch_host', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'tools', 'micro', 'hip_host'), '-pthread',
                           os.path.join(ROOT, 'tools', 'micro', 'conv_tile_host.cpp'), '-o', out])
    return out


class Problem:
    """The convolution of a case, from its definition."""

    def __init__(self, c):
        self.B, self.H, self.W, self.C, self.K, k, s = c['shape']
        self.KH = self.KW = k
        self.s = s
        self.OH, self.OW, self.pt, _, self.pl, _ = conv_geometry(self.H, self.W, k, k, s, s, c['padding'])
        r8 = lambda v: (v + 7) & ~7      # noqa: E731
        self.unit = c['unit']
        self.xp = r8(self.C) if self.unit == 8 else (c['in_pitch'] or self.C)
        self.yp = r8(self.K) if self.unit == 8 else (c['out_pitch'] or self.K)
        self.nx, self.ny = self.B * self.H * self.W * self.xp, self.B * self.OH * self.OW * self.yp

    def args(self, c, bm, bn):
        return [c['which'], c['unit'], bm, bn, 4, c['tap_classes'], c['quads'], self.B, self.H, self.W, self.C, self.OH, self.OW, self.K, self.KH, self.KW,
                self.s, self.s, self.pt, self.pl, 0 if self.unit == 8 else c['in_pitch'], 0 if self.unit == 8 else c['out_pitch'], c['dgrad_c'], 0]

    def fwd_pairs(self, b, p, q):
        """{(offset in x, tap, channel)} that output pixel (b, p, q) contracts with the filter elements (tap, channel, :)"""
        out = set()
        for i in range(self.KH):
            for j in range(self.KW):
                y, x = p * self.s - self.pt + i, q * self.s - self.pl + j
                if 0 <= y < self.H and 0 <= x < self.W:
                    out.update((((b * self.H + y) * self.W + x) * self.xp + ch, i * self.KW + j, ch) for ch in range(self.C))
        return out

    def dgrad_pairs(self, b, y, x):
        """{(offset in dy, tap, output channel)} that input pixel (b, y, x) contracts with the filter elements (tap, :, channel)"""
        out = set()
        for i in range(self.KH):
            for j in range(self.KW):
                pn, qn = y + self.pt - i, x + self.pl - j
                if pn % self.s == 0 and qn % self.s == 0 and 0 <= pn // self.s < self.OH and 0 <= qn // self.s < self.OW:
                    out.update((((b * self.OH + pn // self.s) * self.OW + qn // self.s) * self.yp + o, i * self.KW + j, o) for o in range(self.K))
        return out


def _run(program, tmp_path, pr, c, bm, bn):
    dst = str(tmp_path / 'out.txt')
    r = subprocess.run([program, dst] + [str(v) for v in pr.args(c, bm, bn)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    flags, blocks, wrows = None, [], []
    for line in open(dst):
        f = line.split()
        v = [int(t) for t in f[1:]]
        if f[0] == 'A':
            flags = dict(compact=v[0], tap_classes=v[1], slab_rows=v[2], Nv=v[3])
        elif f[0] == 'G':
            grid = dict(gx=v[0], gy=v[1], N=v[2])
        elif f[0] == 'B':
            blocks.append(dict(zip(('by', 'bx', 'empty', 'm0', 'n0', 'M', 'ntaps', 'Kdim', 'Cp', 'Cs'), v), rows={}, outs={}))
        elif f[0] == 'R':
            blocks[-1]['rows'][v[0]] = (v[1], np.array(v[2:], dtype=np.int64).reshape(-1, 3))
        elif f[0] == 'O':
            blocks[-1]['outs'][v[0]] = (v[1], v[3:])
            assert len(v[3:]) == v[2]
        elif f[0] == 'W':
            wrows.append(v)
    return flags, grid, blocks, wrows


def _check_row(pr, blk, kpos, expected, tap_of, gathered_numel, what):
    """kpos [Kdim, 3]: (gather or -1, tapB, channel) - against the expected {(gather, tap, channel)} of the row's pixel"""
    assert len(kpos) == blk['Kdim'] == blk['ntaps'] * blk['Cp'], what
    got, positions, needed = set(), set(), {(e[1], e[2]) for e in expected}
    for k, (gather, tapb, ch) in enumerate(kpos.tolist()):
        tap = tap_of(k, tapb)
        assert (tap, ch) not in positions, '%s: K position %d repeats (tap %d, channel %d)' % (what, k, tap, ch)
        positions.add((tap, ch))
        if gather >= 0:
            assert gather < gathered_numel, '%s: gather offset %d outside the tensor' % (what, gather)
            got.add((gather, tap, ch))
        else:   # masked: an out-of-bounds tap or a pad channel, never a pair the pixel needs
            assert (tap, ch) not in needed, '%s: K position %d (tap %d, channel %d) is masked but in bounds' % (what, k, tap, ch)
    assert got == expected, '%s: %d pairs missing, %d pairs too many' % (what, len(expected - got), len(got - expected))


def _out_offset(pr, flags, pix, n, pitch):
    return ((n >> 2) * flags['slab_rows'] + pix) * 4 + (n & 3) if flags['slab_rows'] else pix * pitch + n


@pytest.mark.parametrize('tile', TILES, ids=lambda t: '%dx%d' % t)
@pytest.mark.parametrize('c', CASES, ids=_id)
def test_addresses_against_the_definition(program, tmp_path, c, tile):
    pr = Problem(c)
    bm, bn = tile
    flags, grid, blocks, wrows = _run(program, tmp_path, pr, c, bm, bn)
    assert flags['compact'] == c['compact'] and flags['tap_classes'] == c['tap_classes'] and (flags['slab_rows'] > 0) == bool(c['quads']), 'the case does not reach its branch'
    which, N = c['which'], grid['N']
    written = []
    if which == WGRAD:
        (blk,) = blocks
        assert blk['M'] == pr.B * pr.OH * pr.OW and blk['ntaps'] == pr.KH * pr.KW and N == pr.K
        for r in range(blk['M']):
            q, t2 = r % pr.OW, r // pr.OW
            _check_row(pr, blk, blk['rows'][r][1], pr.fwd_pairs(t2 // pr.OH, t2 % pr.OH, q), lambda k, tapb: k // blk['Cp'], pr.nx, 'pixel %d' % r)
        assert len(wrows) == blk['ntaps'] * blk['Cp']
        for m, valid, base in wrows:
            tap, ch = divmod(m, blk['Cp'])
            assert valid == (ch < pr.C) and (not valid or base == (tap * pr.C + ch) * pr.K)
            if valid:
                assert blk['outs'][m][1] == [base + n for n in range(pr.K)]
                written += blk['outs'][m][1]
        assert sorted(written) == list(range(pr.KH * pr.KW * pr.C * pr.K)), 'the output map does not hit every element of dw once'
        return
    assert N == (c['dgrad_c'] or (pr.C if which == DGRAD else pr.K))
    assert len(blocks) == grid['gx'] * grid['gy'] and grid['gy'] == (pr.s * pr.s if which == DGRAD else 1)
    # the filter copy each contraction reads: float32 HWIO for both; bf16 [tap][o][c8] (FWD) and [tap][c][o8] (DGRAD)
    r8 = lambda v: (v + 7) & ~7      # noqa: E731
    tap_stride = pr.C * pr.K if pr.unit == 4 else (pr.K * r8(pr.C) if which == FWD else pr.C * r8(pr.K))
    pitch = pr.yp if which == FWD else pr.xp                      # of the tensor written
    opix = pr.B * (pr.OH * pr.OW if which == FWD else pr.H * pr.W)
    seen = {}      # output pixel -> the column tiles that covered it
    for blk in blocks:
        if blk['empty']:
            assert blk['m0'] >= blk['M']
            continue
        what = 'block (%d, %d)' % (blk['by'], blk['bx'])
        assert len(blk['rows']) == bm and blk['ntaps'] <= pr.KH * pr.KW
        assert flags['compact'] or which == DGRAD or blk['ntaps'] == pr.KH * pr.KW
        for row in range(bm):
            out_off, kpos = blk['rows'][row]
            if blk['m0'] + row >= blk['M']:
                assert (kpos[:, 0] == -1).all() and row not in blk['outs'], '%s: row %d beyond M carries a mask' % (what, row)
                continue
            n0, offs = blk['outs'][row]
            assert n0 == blk['n0'] and len(offs) == min(bn, N - n0)
            # the pixel this row's results are written to
            pix = (offs[0] // 4 - (n0 >> 2) * flags['slab_rows']) if flags['slab_rows'] else (offs[0] - n0) // pitch
            assert 0 <= pix < opix
            assert offs == [_out_offset(pr, flags, pix, n, pitch) for n in range(n0, n0 + len(offs))], '%s row %d: output offsets' % (what, row)
            if which == DGRAD:
                assert out_off == pix * (4 if flags['slab_rows'] else pitch)
            x, t2 = pix % (pr.OW if which == FWD else pr.W), pix // (pr.OW if which == FWD else pr.W)
            y, b = t2 % (pr.OH if which == FWD else pr.H), t2 // (pr.OH if which == FWD else pr.H)
            if which == DGRAD:
                assert (y % pr.s) * pr.s + (x % pr.s) == blk['by'], '%s row %d: a pixel of another stride class' % (what, row)
            expected = pr.fwd_pairs(b, y, x) if which == FWD else pr.dgrad_pairs(b, y, x)
            _check_row(pr, blk, kpos, expected, lambda k, tapb: tapb // tap_stride, pr.nx if which == FWD else pr.ny, '%s row %d' % (what, row))
            assert all(tapb % tap_stride == 0 for tapb in kpos[:, 1].tolist())
            seen.setdefault(pix, []).append(n0)
            written += offs
    tiles_n = -(-N // bn)
    assert sorted(seen) == list(range(opix)) and all(sorted(v) == [t * bn for t in range(tiles_n)] for v in seen.values()), \
        'the rows of the grid do not cover every output pixel once per column tile'
    assert sorted(written) == sorted(_out_offset(pr, flags, pix, n, pitch) for pix in range(opix) for n in range(N)), \
        'the output map does not hit every output element once (or hits a pad channel)'
    assert max(written) < (flags['slab_rows'] * 4 * -(-N // 4) if flags['slab_rows'] else opix * pitch)
