"""GPU: acg_grad_clip_norm (include/acgan_rollout.h) through the C ABI against tests/clip_norm_ref.py (numpy float64).

Bars, all derived:  the reported norms within 1e-6 relative of float64 (one float32 rounding, 6e-8, plus double sums in another
order);  where the reference scale is 1 - the gradient fits, is not finite, or max_norm = +inf - the buffer is BITWISE unchanged
and stats[1] == 1;  where it clips every element within 2.4e-7 relative of float32(g) * float32(scale_ref) (the scale may be one
float32 ulp off, the product rounds once: 2 x 1.2e-7) and the norm afterwards <= max_norm (1 + 1e-6);  a second launch gives the
same bits;  sentinels around the buffer, stats and the workspace, and the gaps between segments, keep their bit patterns."""
import ctypes

import numpy as np
import pytest
import torch

import clip_norm_ref as R
from action_conditioned_gans_amd import _lib
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
PAD = 64                       # sentinel floats in front of and behind the gradient buffer (a multiple of 4: the buffer stays aligned)
SENTINEL = np.float32(-7.25)
INF = float('inf')


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _segs(windows):
    s = _lib.NormSegments()
    s.count = len(windows)
    for i, (o, n) in enumerate(windows[:64]):
        s.offset[i], s.length[i] = o, n
    return s


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _launch(host, windows, pre_scale, max_norm, fill=0xA5):
    """One call on a fresh copy of ``host``, the workspace holding ``fill`` bytes on entry -> (buffer after, stats, workspace bytes
    after); asserts every sentinel."""
    lib = _lib.get()
    n, count = host.size, len(windows)
    segs = _segs(windows)
    nbytes = lib.grad_clip_norm_workspace_bytes(n, ctypes.byref(segs))
    assert nbytes == 8 * sum(-(-length // R.CHUNK) for _, length in windows)
    buf = torch.full((PAD + n + PAD,), float(SENTINEL), device=DEV)
    grad = buf[PAD:PAD + n]
    grad.copy_(torch.from_numpy(host))
    sbuf = torch.full((8 + 2 + count + 8,), float(SENTINEL), device=DEV)
    stats = sbuf[8:8 + 2 + count]
    wbuf = torch.full((64 + nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = wbuf[64:64 + nbytes]
    ws.fill_(fill)
    lib.grad_clip_norm(_p(grad), n, ctypes.byref(segs), pre_scale, max_norm, _p(stats), _p(ws), nbytes, _stream())
    torch.cuda.synchronize()
    b, s, w = buf.cpu().numpy(), sbuf.cpu().numpy(), wbuf.cpu().numpy()
    assert (b[:PAD] == SENTINEL).all() and (b[PAD + n:] == SENTINEL).all(), 'a sentinel around the gradient buffer changed'
    assert (s[:8] == SENTINEL).all() and (s[8 + 2 + count:] == SENTINEL).all(), 'a sentinel around stats changed'
    assert (w[:64] == 0xA5).all() and (w[64 + nbytes:] == 0xA5).all(), 'a sentinel around the workspace changed'
    return b[PAD:PAD + n].copy(), s[8:8 + 2 + count].copy(), w[64:64 + nbytes].copy()


def _check(host, windows, pre_scale, max_norm):
    """The whole contract for one call; -> (stats, reference scale)."""
    max_norm = float(np.float32(max_norm))                 # (what the float argument holds)
    norm, scale, norms = R.stats64(host, windows, pre_scale, max_norm)
    got, stats, ws = _launch(host, windows, pre_scale, max_norm)
    got2, stats2, _ = _launch(host, windows, pre_scale, max_norm, fill=0x7F)          # (0x7f7f...: other, NaN-free garbage in the workspace)
    assert np.array_equal(_bits(got), _bits(got2)) and np.array_equal(_bits(stats), _bits(stats2)), \
        'a second launch, on a workspace with other content, gives other bits'
    covered = np.zeros(host.size, bool)
    for o, n in windows:
        covered[o:o + n] = True
    assert np.array_equal(_bits(got)[~covered], _bits(host)[~covered]), 'an element between the segments was written'
    if not np.isfinite(norm):
        assert not np.isfinite(stats[0]) and stats[1] == 1.0
    else:
        want = np.array([norm] + norms)
        have = np.concatenate([stats[:1], stats[2:]]).astype(np.float64)
        print('norm %.9g (ref %.9g), scale %.9g (ref %.9g)' % (stats[0], norm, stats[1], scale))
        assert np.all(np.abs(have - want) <= 1e-6 * want), (have, want)
    if scale == np.float32(1.0):
        assert stats[1] == 1.0
        assert np.array_equal(_bits(got), _bits(host)), 'the buffer was written although the scale is 1'
    else:
        want = (host * scale).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want)[covered]
        assert np.all(err <= 2.4e-7 * np.abs(want[covered])), 'worst %.3g relative' % float((err / np.maximum(np.abs(want[covered]), 1e-300)).max())
        assert abs(float(stats[1]) - float(scale)) <= 1.2e-7 * float(scale)
        after, _, _ = R.stats64(got, windows, pre_scale, INF)
        assert after <= float(max_norm) * (1 + 1e-6), (after, max_norm)
    return stats, scale


def _values(kind, n, seed=0):
    rng = np.random.default_rng(seed + n)
    if kind == 'normal':
        return rng.standard_normal(n).astype(np.float32)
    if kind == 'tiny':
        return np.full(n, 1e-30, np.float32)
    if kind == 'huge':
        return np.full(n, 1e25, np.float32)
    x = rng.standard_normal(n).astype(np.float32)
    x[(n * 2) // 3] = np.float32(np.nan if kind == 'nan' else np.inf)
    return x


def _bounds(host, windows, pre_scale=1.0):
    norm = R.stats64(host, windows, pre_scale, INF)[0]
    return [float(np.float32(2 * norm)), float(np.float32(0.5 * norm)), INF]


SIZES = [1, 3, 4, 5, 255, 256, 257, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 65537, 1048579]


@pytest.mark.parametrize('n', SIZES)
def test_one_segment(n):
    host = _values('normal', n)
    for bound in _bounds(host, [(0, n)]):
        stats, scale = _check(host, [(0, n)], 1.0, bound)
        assert (scale != 1.0) == (bound < R.stats64(host, [(0, n)], 1.0, INF)[0])


@pytest.mark.parametrize('kind', ['tiny', 'huge', 'nan', 'inf'])
@pytest.mark.parametrize('n', [5, 257, R.CHUNK + 1, 65537])
def test_value_classes(kind, n):
    host = _values(kind, n)
    if kind in ('nan', 'inf'):
        for bound in (1.0, INF):
            _check(host, [(0, n)], 1.0, bound)
        return
    norm = R.stats64(host, [(0, n)], 1.0, INF)[0]
    assert np.isfinite(np.float32(norm)) and np.float32(norm) > 0          # (1e25 sqrt(n) stays inside float32; 1e-30 squares do not)
    if kind == 'tiny':
        assert np.square(host).max() == 0.0                               # float32 squares underflow: only a double sum sees them
    for bound in _bounds(host, [(0, n)]):
        _check(host, [(0, n)], 1.0, bound)


@pytest.mark.parametrize('n', [257, 65537])
def test_pre_scale(n):
    host = _values('normal', n)
    norm = R.stats64(host, [(0, n)], 1.0, INF)[0]
    stats, scale = _check(host, [(0, n)], 0.5, 0.75 * norm)               # between 0.5 |g| and |g|: the averaged gradient fits
    assert scale == 1.0
    for pre_scale in (0.5, -0.5):                                         # (only |pre_scale| counts)
        stats, scale = _check(host, [(0, n)], pre_scale, 0.25 * norm)     # below 0.5 |g|: clipped, to the bound of the AVERAGED gradient
        assert abs(float(scale) - 0.5) <= 1e-6


def test_gaps_are_neither_read_nor_written():
    windows = [(0, 3), (4, 1), (8, 1029)]
    host = np.full(8 + 1029 + 3, np.nan, np.float32)
    rng = np.random.default_rng(3)
    for o, n in windows:
        host[o:o + n] = rng.standard_normal(n)
    for bound in _bounds(host, windows):
        stats, _ = _check(host, windows, 1.0, bound)
        assert np.isfinite(stats).all()


def test_64_segments_of_mixed_sizes():
    rng = np.random.default_rng(11)
    sizes = [1, 2, 3, 4, 5, 31, 32, 33, 255, 256, 257, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 40000, 2 * R.CHUNK + 7]
    sizes += [int(v) for v in rng.integers(1, 40001, size=64 - len(sizes))]
    windows, off = [], 0
    for n in sizes:
        windows.append((off, n))
        off += -(-n // 4) * 4
    host = rng.standard_normal(off).astype(np.float32) * rng.choice([1e-3, 1.0, 30.0], size=off).astype(np.float32)
    shuffled = [windows[i] for i in rng.permutation(64)]                  # the list's order is the caller's
    for w in (windows, shuffled):
        for bound in _bounds(host, w):
            _check(host, w, 1.0, bound)


def test_the_dna_generators_layout():
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device=DEV)
    T.Trainer(sess, True, 'bce', 'adam', True, batch_size=2, lookahead=False)
    _, windows = optim.GradNorm(1.0, 'g').segments()
    total = G.get_default_graph().layout('g')[1]
    sess.close()
    assert 1 < len(windows) <= 64
    host = np.random.default_rng(5).standard_normal(total).astype(np.float32)
    for bound in _bounds(host, windows, 0.5):
        _check(host, windows, 0.5, bound)


def test_errors():
    lib = _lib.get()
    grad, stats, ws = torch.ones(64, device=DEV), torch.zeros(8, device=DEV), torch.zeros(64, dtype=torch.uint8, device=DEV)

    def call(windows, max_norm=1.0, nbytes=64, count=None, g=grad):
        segs = _segs(windows)
        if count is not None:
            segs.count = count
        lib.grad_clip_norm(_p(g), 64, ctypes.byref(segs), 1.0, max_norm, _p(stats), _p(ws), nbytes, _stream())
    call([(0, 64)], max_norm=INF)
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(_lib.AcgError, match='max_norm'):
            call([(0, 64)], max_norm=bad)
    for count in (0, 65):
        with pytest.raises(_lib.AcgError, match='segments'):
            call([(0, 4)], count=count)
    with pytest.raises(_lib.AcgError, match='multiple of 4'):
        call([(0, 4), (6, 4)])
    with pytest.raises(_lib.AcgError, match='overlap'):
        call([(0, 9), (8, 4)])
    with pytest.raises(_lib.AcgError, match='outside'):
        call([(60, 5)])
    with pytest.raises(_lib.AcgError, match='workspace'):
        call([(0, 32), (32, 32)], nbytes=8)
    with pytest.raises(_lib.AcgError, match='aligned'):
        call([(0, 8)], g=grad[1:])
    torch.cuda.synchronize()
    assert bool((grad == 1).all())


def test_library_exports_the_new_entries():
    lib = _lib.get()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('acg_grad_clip_norm', 'acg_grad_clip_norm_workspace_bytes'):
        assert hasattr(cdll, name) and callable(getattr(lib, name[4:])) and name in _lib.EXTENSIONS['rollout'].signatures
    assert lib.version() == _lib.ABI_VERSION == 8
