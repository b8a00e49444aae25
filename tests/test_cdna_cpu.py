"""The CDNA generator without a GPU: the float64 restatement (tests/cdna_ref.py) against brute force, its gradients, the
one-hot limits, the graph's variables, the CLI's argument errors and the clear error on the C oracle."""
import numpy as np
import pytest
import torch

import cdna_ref as R
from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import models as M
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T


def _inputs(b, h, w, c, m, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    params = torch.randn(b, k * k * m, generator=g, dtype=torch.float64) * 0.7 + 0.3
    logits = torch.randn(b, h, w, m + 1, generator=g, dtype=torch.float64) * 2
    img = torch.rand(b, h, w, c, generator=g, dtype=torch.float64) * 2 - 1
    return params, logits, img


def _brute(params, logits, img, m, k):
    """Loops over pixels, taps and channels: normalised kernels, the depthwise SAME correlation, piece j channel i =
    colour (jC+i)/M under mask (jC+i)%M, softmax, composite."""
    b, h, w, c = img.shape
    pad = (k - 1) // 2
    kern = np.maximum(params.numpy().reshape(b, k, k, m) - R.RELU_SHIFT, 0) + R.RELU_SHIFT
    kern = kern / kern.sum(axis=(1, 2), keepdims=True)
    x, z = img.numpy(), logits.numpy()
    out = np.zeros((b, h, w, c))
    for n in range(b):
        for y in range(h):
            for xx in range(w):
                e = np.exp(z[n, y, xx] - z[n, y, xx].max())
                s = e / e.sum()
                for i in range(c):
                    v = s[0] * x[n, y, xx, i]
                    for j in range(m):
                        q = j * c + i
                        col, mask = q // m, q % m
                        t = 0.0
                        for u in range(k):
                            for vv in range(k):
                                yy, xs = y + u - pad, xx + vv - pad
                                if 0 <= yy < h and 0 <= xs < w:
                                    t += x[n, yy, xs, col] * kern[n, u, vv, mask]
                        v += s[j + 1] * t
                    out[n, y, xx, i] = v
    return out


@pytest.mark.parametrize('shape', [(1, 4, 5, 3, 2, 3), (2, 3, 4, 1, 3, 3), (1, 5, 3, 4, 5, 5)], ids=str)
def test_composite_matches_brute_force(shape):
    b, h, w, c, m, k = shape
    params, logits, img = _inputs(*shape)
    params[0, :m] = -1.0                                       # some clamped taps
    got = R.composite(logits, img, params, m, k).numpy()
    assert np.abs(got - _brute(params, logits, img, m, k)).max() <= 1e-12


def test_composite_gradcheck():
    params, logits, img = _inputs(1, 4, 4, 3, 3, 3, seed=2)
    params, logits = params.requires_grad_(True), logits.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda p, z: R.composite(z, img, p, 3, 3), (params, logits))


def test_one_hot_masks_give_a_piece_or_the_image():
    from oracle import tf_ops as OT
    b, h, w, c, m, k = 2, 6, 7, 3, 4, 5
    params, _, img = _inputs(b, h, w, c, m, k, seed=3)
    pieces = OT.cdna_transform(params, img, m, k, R.RELU_SHIFT)
    for j in range(m + 1):
        z = torch.full((b, h, w, m + 1), -1e4, dtype=torch.float64)
        z[..., j] = 0.0
        got = R.composite(z, img, params, m, k)
        want = img if j == 0 else pieces[j - 1]
        assert torch.equal(got, want), j


def test_graph_variables_match_the_restatement():
    G.reset_default_graph()
    optim.set_data_parallel(1)
    img, act = G.placeholder((2, 64, 64, 3), name='img'), G.placeholder((2, 10), name='act')
    frame, state = M.build_generator_cdna(img, act, num_masks=6, ksize=3)
    assert frame.shape == (2, 64, 64, 3) and state.shape == (2, 5)
    got = {n: v.shape for n, v in G.get_default_graph().variables.items()}
    want = {n: tuple(v.shape) for n, v in R.init_params_cdna(ksize=3, num_masks=6).items() if n.startswith('g/')}
    assert got == want
    assert got['g/cdna_params/weights'] == (4, 4, 266, 54) and got['g/tconv4/weights'] == (5, 5, 7, 128)


@pytest.mark.parametrize('kw', [dict(ksize=4), dict(num_masks=0), dict(num_masks=33), dict(size=40)], ids=str)
def test_builder_rejects_unsupported_geometry(kw):
    G.reset_default_graph()
    s = kw.pop('size', 64)
    img, act = G.placeholder((2, s, s, 3), name='img'), G.placeholder((2, 10), name='act')
    with pytest.raises(ValueError):
        M.build_generator_cdna(img, act, **kw)


def test_trainer_names_the_generators():
    assert [T.model_kind(v) for v in (False, True, 'dna', 'cdna')] == ['plain', 'dna', 'dna', 'cdna']
    with pytest.raises(ValueError):
        T.model_kind('stp')


@pytest.mark.parametrize('extra', [['--dna', '--cdna'], ['--cdna', '--dtype', 'bf16'], ['--num_masks', '0'], ['--num_masks', '33'],
                                   ['--cdna', '--ksize', '4']], ids=str)
def test_cli_argument_errors(tmp_path, monkeypatch, extra):
    monkeypatch.setattr(T, 'train', lambda *a, **kw: pytest.fail('train() reached'))
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: pytest.fail('evaluate() reached'))
    with pytest.raises(SystemExit):
        T.main(['synthetic', str(tmp_path / 'out')] + extra)
    assert not (tmp_path / 'out').exists()
    with pytest.raises(SystemExit):
        E.main(['models', 'synthetic', str(tmp_path / 'eval'), '--num_sequences', '4'] + extra)
    assert not (tmp_path / 'eval').exists()


def test_cli_passes_the_cdna_generator_on(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(T, 'train', lambda *a, **kw: seen.update(kw, positional=a))
    T.main(['synthetic', str(tmp_path / 'out'), '--cdna', '--num_masks', '7', '--ksize', '3'])
    assert seen['positional'][8] == 'cdna' and seen['num_masks'] == 7 and seen['ksize'] == 3
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: seen.update(kw))
    E.main(['models', 'synthetic', str(tmp_path / 'eval'), '--cdna', '--num_masks', '5', '--num_sequences', '4'])
    assert seen['cdna'] is True and seen['dna'] is False and seen['num_masks'] == 5


def test_the_c_oracle_raises_a_clear_error():
    from oracle import cbind
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cpu', lib=cbind.load())
    tr = T.Trainer(sess, True, 'bce', 'adam', 'cdna', batch_size=2)
    sess.run(G.global_variables_initializer())
    x, a = np.zeros((2, 64, 64, 3), np.float32), np.zeros((2, 10), np.float32)
    with pytest.raises(RuntimeError, match='acg_cdna_composite_fwd'):
        tr.test(x, x, a)
