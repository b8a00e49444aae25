"""The augmentation kernels without a GPU: csrc/d_augment.hip itself compiled for the host (tools/micro/d_augment_host.cpp: blocks
in turn, a block's threads as real threads at a barrier) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
program.  Checks what tests/test_gpu_d_augment.py checks at its small shapes - forward and adjoint within 64 * 2^-24 * max(1,
max|x|) of float64, pad channels, both access paths, the draw bit for bit - plus that no access leaves the input, the output, the
parameters or the workspace (exact-size heap blocks), also under hostile parameters: NaN, +-inf, +-1e30 and non-integers in the
shift and cut fields.  Host arithmetic: the same IEEE operations in the same order, not the device's instruction stream.  The
row limit (1024 rows) and 128 x 128 are left to the GPU test: a million host threads prove nothing more about bounds."""
import os
import subprocess

import numpy as np
import pytest

import d_augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (rows, h, w, pitch, frames, cf, off): off = 1 puts both bases 4 bytes behind a 16-byte boundary (the element path)
SHAPES = [(1, 1, 1, 1, 1, 1, 0), (2, 5, 7, 8, 2, 3, 0), (2, 5, 7, 8, 2, 3, 1), (3, 16, 16, 8, 2, 3, 0), (2, 9, 6, 4, 1, 3, 1), (2, 9, 6, 4, 1, 3, 0),
          (2, 8, 8, 4, 1, 4, 0), (1, 40, 40, 8, 2, 3, 0), (2, 3, 5, 12, 2, 4, 0), (2, 3, 5, 7, 2, 3, 0)]


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('d_augment_host') / 'd_augment_host')
    subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-x', 'c++', '-std=c++17', '-O1', '-Xarch_host', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'tools', 'micro', 'hip_host'), '-pthread',
                           os.path.join(ROOT, 'tools', 'micro', 'd_augment_host.cpp'), '-o', out])
    return out


def _run(program, tmp_path, mode, x, params, shape):
    rows, h, w, pitch, frames, cf, off = shape
    src, par, dst = (str(tmp_path / n) for n in ('in.bin', 'params.bin', 'out.bin'))
    np.asarray(x, np.float32).tofile(src)
    np.asarray(params, np.float32).tofile(par)
    r = subprocess.run([program, mode, src, par, dst] + [str(v) for v in (rows, h, w, pitch, frames, cf, off)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    return np.fromfile(dst, np.float32).reshape(rows, h, w, pitch)


def _params(rng, rows, h, w):
    """Drawn rows (every policy bit) and, in row 1, a negative shift with a cut across the border."""
    p = R.draw(int(rng.integers(1, 2 ** 62)), 3, 1, rows, h, w, 7)
    if rows > 1:
        p[1, 3:] = (-(h // 2), w // 3, -1, w - 1, 2)
    return p


def _check(mode, got, x, params, shape, scale):
    rows, h, w, pitch, frames, cf, off = shape
    nv = frames * cf
    want = (R.apply if mode == 'fwd' else R.adjoint)(x[..., :nv].astype(np.float64), params, frames, cf).numpy()
    bar = 64 * 2.0 ** -24 * max(1.0, scale)
    assert np.abs(got[..., :nv].astype(np.float64) - want).max() <= bar
    if mode == 'fwd':
        assert np.array_equal(got[..., nv:].view(np.uint32), x[..., nv:].view(np.uint32))          # pad channels: the input's bits
    else:
        assert np.array_equal(got[..., nv:].view(np.uint32), np.zeros_like(got[..., nv:]).view(np.uint32))


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_forward_and_adjoint_on_the_host(program, tmp_path, shape):
    rows, h, w, pitch, frames, cf, off = shape
    rng = np.random.default_rng(rows * 1000 + h * 10 + pitch + off)
    params = _params(rng, rows, h, w)
    for scale in (1.0, 1e3):
        x = (rng.uniform(-1, 1, (rows, h, w, pitch)) * scale).astype(np.float32)
        x[..., frames * cf:] = rng.standard_normal((rows, h, w, pitch - frames * cf)).astype(np.float32) * 1e6       # pad: anything
        for mode in ('fwd', 'bwd'):
            _check(mode, _run(program, tmp_path, mode, x, params, shape), x, params, shape, float(np.abs(x[..., :frames * cf]).max()))
    # the identity row returns its frame (x holds no -0.0 and no non-finite value: bit for bit)
    x = rng.uniform(-1, 1, (rows, h, w, pitch)).astype(np.float32)
    got = _run(program, tmp_path, 'fwd', x, np.array([R.IDENTITY] * rows), shape)
    assert np.array_equal(got.view(np.uint32), x.view(np.uint32))


HOSTILE = [float('nan'), float('inf'), float('-inf'), 1e30, -1e30, 4097.0, -4097.0, 3.0e9, -2147483648.0]


@pytest.mark.parametrize('shape', [(2, 5, 7, 8, 2, 3, 0), (2, 9, 6, 4, 1, 3, 1)], ids=str)
def test_hostile_parameters_leave_no_tensor(program, tmp_path, shape):
    rows, h, w, pitch, frames, cf, off = shape
    nv = frames * cf
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (rows, h, w, pitch)).astype(np.float32)
    for field in (range(3, 8) if off == 0 else (4, 7)):                     # (the element path: one shift and one cut field)
        for bad in (HOSTILE if off == 0 else HOSTILE[:5]):
            params = np.array([(0.1, 1.3, 0.8, 1, -1, 1, 1, 2)] * rows, np.float64)
            params[0, field] = bad                                          # row 0 is dead, row 1 an ordinary one
            fwd = _run(program, tmp_path, 'fwd', x, params, shape)
            assert not fwd[0, ..., :nv].any() and np.array_equal(fwd[0, ..., nv:].view(np.uint32), x[0, ..., nv:].view(np.uint32))
            bwd = _run(program, tmp_path, 'bwd', x, params, shape)
            assert not bwd[0].any()                                         # g' = 0: every term of the adjoint is 0
            for mode, got in (('fwd', fwd), ('bwd', bwd)):
                _check(mode, got[1:], x[1:], params[1:], (rows - 1,) + shape[1:], 1.0)
    # non-integers are truncated towards zero behind the range check
    params = np.array([(0.1, 1.3, 0.8, 1.75, -1.5, 1.25, -0.75, 2.9), (0.0, 1.0, 1.0, -0.99, 0.99, 0.5, 0.5, 0.5)][:rows], np.float64)
    trunc = params.copy()
    trunc[:, 3:] = np.trunc(trunc[:, 3:])
    for mode in ('fwd', 'bwd'):
        _check(mode, _run(program, tmp_path, mode, x, params, shape), x, trunc, shape, 1.0)
    # hostile colour fields touch no index: the call ends clean
    params = np.array([(float('nan'), float('inf'), -1e30, 1, 0, 0, 0, 2)] * rows, np.float64)
    for mode in ('fwd', 'bwd'):
        _run(program, tmp_path, mode, x, params, shape)


@pytest.mark.parametrize('seed,counter,sid,rows,h,w,policy', [(1, 0, 0, 5, 64, 64, 7), (2 ** 64 - 2, 2 ** 32 + 7, 130, 300, 5, 7, 7),
                                                              (77, 2 ** 64 - 1, 2, 1024, 128, 96, 5), (9, 4, 1, 3, 1, 1, 2), (9, 4, 1, 3, 64, 64, 0)])
def test_the_draw_on_the_host_bit_for_bit(program, tmp_path, seed, counter, sid, rows, h, w, policy):
    dst = str(tmp_path / 'draw.bin')
    r = subprocess.run([program, 'draw', dst] + [str(v) for v in (seed, counter, sid, rows, h, w, policy)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    raw = np.fromfile(dst, np.uint8)
    params, state = raw[:rows * 32].view(np.float32).reshape(rows, 8), raw[rows * 32:].view(np.uint64)
    assert np.array_equal(params.astype(np.float64), R.draw(seed, counter, sid, rows, h, w, policy))
    assert state.tolist() == [seed, (counter + 1) % 2 ** 64]
