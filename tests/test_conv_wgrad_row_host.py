"""The row table of the weight gradient's UW loaders without a GPU: conv_tile.h's straight-line forms (bit_range, tap_mask_closed,
wgrad_row) compiled for the host (tools/micro/wgrad_row_host.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer and held
  * against the definition, bit by bit, for every filter KH x KW of at most 64 taps and every pair of row and column ranges - the
    empty ranges and the 64-bit-wide one (a 1 x 64 filter) included - and against the looped tap_mask wherever that is defined;
  * against row_info for every pixel row of a few shapes and for rows beyond the last one: complemented masks, the byte offset
    from the padding corner (never negative), and "all taps dead, offset 0" beyond the limit.
Independent of the GPU parity test (tests/test_gpu_conv_wgrad_uniform.py)."""
import os
import subprocess

import pytest

from oracle.tf_ops import conv_geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (batch, h, w, kh, kw, stride, padding, channel pitch)
SHAPES = [
    (2, 9, 7, 3, 3, 1, 'SAME', 40),        # borders on every side, pitch != a power of two
    (2, 13, 11, 5, 5, 2, 'SAME', 32),      # stride 2, odd extents
    (1, 8, 8, 7, 7, 1, 'SAME', 32),        # 49 taps: both mask words
    (3, 5, 6, 4, 4, 2, 'SAME', 4),         # even filter: unequal padding
    (2, 7, 9, 3, 3, 2, 'VALID', 8),        # no padding: the corner is the tensor's first element
    (2, 3, 40, 1, 64, 1, 'SAME', 4),       # a 1 x 64 filter (40 wide: the looped reference shifts by the range's width)
    (2, 40, 3, 64, 1, 1, 'SAME', 4),       # and the 64 x 1 one
]


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('wgrad_row_host') / 'wgrad_row_host')
    subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-x', 'c++', '-std=c++17', '-O1', '-Xarch_host', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'tools', 'micro', 'hip_host'), '-pthread',
                           os.path.join(ROOT, 'tools', 'micro', 'wgrad_row_host.cpp'), '-o', out])
    return out


def _run(program, args):
    r = subprocess.run([program] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:]
    return int(out.split()[-1])


def test_closed_form_masks_against_the_definition(program):
    assert _run(program, ['masks']) > 100000


@pytest.mark.parametrize('s', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_rows_against_row_info(program, s):
    b, h, w, kh, kw, st, padding, cx = s
    oh, ow, pt, _, pl, _ = conv_geometry(h, w, kh, kw, st, st, padding)
    assert _run(program, ['rows', b, h, w, kh, kw, st, st, pt, pl, oh, ow, cx, 300]) == b * oh * ow + 300
