"""The SSIM loss kernels without a GPU: csrc/ssim_loss.hip itself compiled for the host (tools/micro/ssim_loss_host.cpp: blocks
in turn, a block's threads as real threads at a barrier) under AddressSanitizer and UndefinedBehaviorSanitizer.  Checks what
the GPU cases of tests/test_gpu_ssim_loss.py check - the gradient within 8 x the float32 floor of float64, the value within
n x 1e-5, the three kinds of call agreeing to the bit - plus that no access of these shapes leaves its buffer (pred, truth,
dpred and the workspace are exact-size heap blocks, the LDS arrays are globals).  Host arithmetic: the same IEEE operations in
the same order, not the device's instruction stream."""
import os
import subprocess

import numpy as np
import pytest
import torch

import ssim_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 11, 11, 1), (2, 12, 13, 3), (1, 21, 27, 4), (2, 33, 75, 3)]


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('ssim_loss_host') / 'ssim_loss_host')
    subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-x', 'c++', '-std=c++17', '-O1', '-Xarch_host', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'tools', 'micro', 'hip_host'), '-pthread',
                           os.path.join(ROOT, 'tools', 'micro', 'ssim_loss_host.cpp'), '-o', out])
    return out


def _run(program, tmp_path, x, y, mode=0):
    src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    np.concatenate([x.ravel(), y.ravel()]).astype(np.float32).tofile(src)
    r = subprocess.run([program] + [str(v) for v in x.shape] + [str(mode), src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0'), timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    out = np.fromfile(dst, np.float32)
    return out[0], out[1:].reshape(x.shape)


@pytest.mark.parametrize('shape', SHAPES, ids=str)
@pytest.mark.parametrize('kind', R.CLASSES)
def test_kernel_source_on_the_host(program, tmp_path, kind, shape):
    x, y = R.case(kind, shape, seed=sum(shape))
    g64 = R.grad_autograd(x, y)
    e_a = np.abs(R.grad_autograd(x, y, torch.float32) - g64).max()
    e_b = np.abs(R.grad_closed32(x, y) - g64).max()
    value, grad = _run(program, tmp_path, x, y)
    assert np.isfinite(grad).all(), 'an element of dpred was not written'
    err = np.abs(grad.astype(np.float64) - g64).max()
    print('%s %s: err / bar %.3f' % (kind, shape, err / (8 * max(e_a, e_b))))
    assert err <= 8 * max(e_a, e_b)
    assert abs(float(value) - R.value64(x, y)) <= shape[0] * 1e-5
    if kind == 'uniform':
        nan, g_only = _run(program, tmp_path, x, y, mode=1)
        v_only, untouched = _run(program, tmp_path, x, y, mode=2)
        assert np.isnan(nan) and np.isnan(untouched).all()
        assert np.array_equal(g_only, grad) and v_only == value


def test_product_shape_on_the_host(program, tmp_path):
    x, y = R.case('smooth', (2, 64, 64, 3), seed=5)
    g64 = R.grad_autograd(x, y)
    bar = 8 * max(np.abs(R.grad_autograd(x, y, torch.float32) - g64).max(), np.abs(R.grad_closed32(x, y) - g64).max())
    value, grad = _run(program, tmp_path, x, y)
    assert np.abs(grad.astype(np.float64) - g64).max() <= bar and abs(float(value) - R.value64(x, y)) <= 2e-5
