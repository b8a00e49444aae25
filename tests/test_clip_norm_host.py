"""The global-norm clip kernels without a GPU: csrc/grad_norm.hip itself compiled for the host (tools/micro/grad_norm_host.cpp:
blocks in turn, a block's threads as real threads at a barrier) under AddressSanitizer and UndefinedBehaviorSanitizer.  Checks
what tests/test_gpu_clip_norm.py checks at its small sizes - norms within 1e-6 of float64, the buffer bitwise unchanged where
the scale is 1, elements within 2.4e-7 where it clips, gaps untouched - plus that no access leaves the gradient buffer, stats
or the workspace (exact-size heap blocks).  Host arithmetic: the same IEEE operations in the same order, not the device's
instruction stream."""
import os
import subprocess

import numpy as np
import pytest

import clip_norm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float('inf')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('grad_norm_host') / 'grad_norm_host')
    subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-x', 'c++', '-std=c++17', '-O1', '-Xarch_host', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'tools', 'micro', 'hip_host'), '-pthread',
                           os.path.join(ROOT, 'tools', 'micro', 'grad_norm_host.cpp'), '-o', out])
    return out


def _run(program, tmp_path, host, windows, pre_scale, max_norm, expect=0):
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    np.asarray(host, np.float32).tofile(src)
    args = [program, src, dst, repr(float(pre_scale)), repr(float(max_norm))] + [str(v) for w in windows for v in w]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), timeout=300)
    assert r.returncode == expect, r.stdout.decode()[-4000:]
    if expect:
        return r.stdout.decode()
    out = np.fromfile(dst, np.float32)
    return out[:host.size], out[host.size:]


def _check(program, tmp_path, host, windows, pre_scale, max_norm):
    max_norm = float(np.float32(max_norm))
    norm, scale, norms = R.stats64(host, windows, pre_scale, max_norm)
    got, stats = _run(program, tmp_path, host, windows, pre_scale, max_norm)
    assert stats.size == 2 + len(windows)
    covered = np.zeros(host.size, bool)
    for o, n in windows:
        covered[o:o + n] = True
    assert np.array_equal(got.view(np.uint32)[~covered], host.view(np.uint32)[~covered])
    if not np.isfinite(norm):
        assert not np.isfinite(stats[0]) and stats[1] == 1.0
    else:
        want = np.array([norm] + norms)
        assert np.all(np.abs(np.concatenate([stats[:1], stats[2:]]).astype(np.float64) - want) <= 1e-6 * want)
    if scale == np.float32(1.0):
        assert stats[1] == 1.0 and np.array_equal(got.view(np.uint32), host.view(np.uint32))
    else:
        want = (host * scale).astype(np.float64)
        assert np.all(np.abs(got.astype(np.float64) - want)[covered] <= 2.4e-7 * np.abs(want[covered]))
        assert R.stats64(got, windows, pre_scale, INF)[0] <= max_norm * (1 + 1e-6)
    return scale


def _bounds(host, windows):
    norm = R.stats64(host, windows, 1.0, INF)[0]
    return [2 * norm, 0.5 * norm, INF]


@pytest.mark.parametrize('n', [1, 3, 4, 5, 255, 256, 257, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1])
def test_one_segment_on_the_host(program, tmp_path, n):
    host = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    scales = [_check(program, tmp_path, host, [(0, n)], 1.0, b) for b in _bounds(host, [(0, n)])]
    assert scales[0] == 1.0 and scales[1] != 1.0 and scales[2] == 1.0


@pytest.mark.parametrize('kind', ['tiny', 'huge', 'nan', 'inf'])
def test_value_classes_on_the_host(program, tmp_path, kind):
    n = 261
    host = np.random.default_rng(1).standard_normal(n).astype(np.float32)
    if kind in ('nan', 'inf'):
        host[77] = np.nan if kind == 'nan' else np.inf
        bounds = [1.0, INF]
    else:
        host[:] = 1e-30 if kind == 'tiny' else 1e25
        bounds = _bounds(host, [(0, n)])
    for b in bounds:
        _check(program, tmp_path, host, [(0, n)], 1.0, b)


def test_gaps_and_many_segments_on_the_host(program, tmp_path):
    windows = [(0, 3), (4, 1), (8, 1029)]
    host = np.full(8 + 1029 + 3, np.nan, np.float32)
    rng = np.random.default_rng(3)
    for o, n in windows:
        host[o:o + n] = rng.standard_normal(n)
    for b in _bounds(host, windows)[1:]:
        _check(program, tmp_path, host, windows, -0.5, b)
    # more segments than the finalizing block has waves (two trips), listed back to front
    sizes = [1, 2, 3, 4, 5, 31, 32, 33, 255, 257, 1, 7, 64, 100, 1000, 5, 9, R.CHUNK + 1, 3, 12]
    windows, off = [], 0
    for n in sizes:
        windows.append((off, n))
        off += -(-n // 4) * 4
    host = rng.standard_normal(off).astype(np.float32)
    assert _check(program, tmp_path, host, windows[::-1], 1.0, _bounds(host, windows)[1]) != 1.0


def test_errors_on_the_host(program, tmp_path):
    host = np.ones(64, np.float32)
    for windows, max_norm, word in [([(0, 64)], 0.0, 'max_norm'), ([(0, 64)], -1.0, 'max_norm'), ([(0, 64)], float('nan'), 'max_norm'),
                                    ([(0, 4), (6, 4)], 1.0, 'multiple of 4'), ([(0, 9), (8, 4)], 1.0, 'overlap'), ([(60, 5)], 1.0, 'outside'),
                                    ([(0, 1)] * 65, 1.0, 'segments')]:
        assert word in _run(program, tmp_path, host, windows, 1.0, max_norm, expect=11)
