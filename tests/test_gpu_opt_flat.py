"""GPU: the flat optimizer entries (acg_adam_step, acg_rmsprop_step) where no other test runs them - past the launch grid and
through a strided scalar tail - and pinned to the bits the commit before their kernels shared one body left behind.

The launch grid is min(4096, ceil((n / 4 + 1) / 256)) blocks of 256 threads: the grid-stride loop of the float4 path runs only
for n > 4 * 4096 * 256; the scalar loop (buffers off the 16-byte grid) runs on the same grid, a quarter of n threads, and
strides at any size - at the size below as 1025 blocks over a million elements.  The update is elementwise and these entries
do not advance the step counter, so one launch over a buffer must leave what launches over consecutive windows of it leave;
no window is long enough for the float4 path to stride."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))

import make_opt_flat_parent as MP                             # noqa: E402
from action_conditioned_gans_amd import _lib                  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GRID = 4096 * 256                           # threads of the largest launch
N_STRIDE = 4 * GRID + 2051                  # one float4 past the grid for the first blocks, n % 4 == 3
N_TAIL = GRID + 5                           # with views one float off the 16-byte grid: everything scalar, every thread strides
WINDOW = GRID                               # elements: a multiple of 4 (a window keeps its buffer's alignment), a quarter of the grid in float4


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(*values):
    return tuple(float(np.float32(v)) for v in values)


def _buffers(kind, n, offset):
    """param, grad, slots as views ``offset`` floats into their allocations; the floats in front hold a sentinel."""
    gen = torch.Generator().manual_seed(n + offset)
    host = [torch.randn(n, generator=gen) * 0.02, torch.randn(n, generator=gen) * 0.3]
    host += [torch.zeros(n), torch.zeros(n)] if kind == 'adam' else [torch.ones(n)]
    whole = [torch.full((n + offset,), 7.0, device=DEV) for _ in host]
    for w, h in zip(whole, host):
        w[offset:].copy_(h)
    return whole, [w[offset:] for w in whole]


def _launch(lib, kind, views, lo, hi, step):
    tail = _f32(0.5) + (1,) + _f32(-0.01, 0.01)          # grad_scale 0.5, clip on
    ptrs = [_p(v[lo:hi]) for v in views]
    if kind == 'adam':
        lib.adam_step(*ptrs, _p(step), hi - lo, *_f32(1e-3, 0.9, 0.999, 1e-8), *tail, _stream())
    else:
        lib.rmsprop_step(*ptrs, hi - lo, *_f32(5e-5, 0.9, 1e-10), *tail, _stream())


@pytest.mark.parametrize('n,offset', [(N_STRIDE, 0), (N_TAIL, 1)], ids=['grid_stride', 'strided_scalar_tail'])
@pytest.mark.parametrize('kind', ['adam', 'rmsprop'])
def test_one_launch_equals_launches_over_windows(kind, n, offset):
    lib = _lib.get()
    step = torch.full((1,), 3, dtype=torch.int32, device=DEV)
    whole, one = _buffers(kind, n, offset)
    param0, grad = one[0].clone(), one[1].clone()
    _launch(lib, kind, one, 0, n, step)
    _, many = _buffers(kind, n, offset)
    for lo in range(0, n, WINDOW):
        _launch(lib, kind, many, lo, min(lo + WINDOW, n), step)
    torch.cuda.synchronize()
    for name, a, b in zip(('param', 'grad', 'slot 1', 'slot 2'), one, many):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name + ' differs between one launch and the windows'
    assert torch.equal(one[1], grad), 'the gradient was written'
    assert not torch.equal(one[0], param0) and float(one[0].abs().max()) <= float(np.float32(0.01))
    assert all(bool((w[:offset] == 7.0).all()) for w in whole) and int(step.item()) == 3


@pytest.mark.parametrize('kind,clip', MP.CASES)
def test_flat_steps_leave_the_bits_of_the_parent_commit(kind, clip):
    gold = np.load(MP.PATH)
    assert str(gold['parent']) == MP.PARENT
    got = MP.run(_lib.get(), kind, clip, DEV)
    assert set(got) == ({'param', 'slot1', 'slot2'} if kind == 'adam' else {'param', 'slot1'})
    for name, a in got.items():
        want = gold[MP.key(kind, clip, name)]
        diff = int((a.view(np.uint32) != want.view(np.uint32)).sum())
        assert a.shape == want.shape == (MP.N,) and diff == 0, '%s: %d of %d elements differ from %s' % (name, diff, MP.N, MP.PARENT[:7])
    assert not np.array_equal(got['param'], MP.inputs(kind, clip, 'cpu')[0].numpy())
