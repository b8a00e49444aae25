"""The affine (STP) generator without a GPU: the float64 restatement (tests/affine_ref.py) against grid_sample / affine_grid,
its gradients, the identity and the one-hot limits, the graph's variables and the argument errors of the builder and the CLIs."""
import pytest
import torch
import torch.nn.functional as F

import affine_ref as R
from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import models as M
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import plan as P
from action_conditioned_gans_amd import train as T


def _grid_sample(image, params):
    """[B, M, H, W, C] by torch's spatial transformer."""
    b, h, w, c = image.shape
    theta = params.reshape(b, -1, 6) + torch.tensor(R.IDENTITY, dtype=params.dtype)
    m = theta.shape[1]
    grid = F.affine_grid(theta.reshape(b * m, 2, 3), (b * m, c, h, w), align_corners=True)
    src = image.permute(0, 3, 1, 2).repeat_interleave(m, dim=0)
    out = F.grid_sample(src, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    return out.view(b, m, c, h, w).permute(0, 1, 3, 4, 2)


@pytest.mark.parametrize('shape,spread', [((2, 9, 13, 3, 4), 1), ((1, 16, 16, 4, 3), 8), ((2, 7, 5, 1, 2), 2)], ids=str)
def test_restatement_equals_grid_sample(shape, spread):
    params, _, image, dout = R.case(shape, seed=4, spread=spread)
    params, image = params.double(), image.double()
    weight = torch.randn(shape[0], shape[4], *shape[1:4], dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    # (the kink rule: grid_sample may take the other side of an integer coordinate, which is no error)
    px, py = R.coords(params, shape[1], shape[2])
    away = (((px - px.round()).abs() > R.KINK) & ((py - py.round()).abs() > R.KINK)).unsqueeze(-1).double()
    weight = weight * away
    p1, p2 = params.clone().requires_grad_(True), params.clone().requires_grad_(True)
    got, want = R.warp(image, p1), _grid_sample(image, p2)
    assert (got - want).abs().max().item() <= 1e-12
    (got * weight).sum().backward()
    (want * weight).sum().backward()
    assert (p1.grad - p2.grad).abs().max().item() <= 1e-12 * max(1.0, p2.grad.abs().max().item())
    assert p2.grad.abs().max().item() > 0


def test_composite_gradcheck():
    b, h, w, c, m = 1, 4, 5, 2, 2
    g = torch.Generator().manual_seed(2)
    # parameters chosen away from the kinks: every coordinate at least 0.02 from an integer
    for _ in range(200):
        params = (torch.randn(b, m * 6, generator=g, dtype=torch.float64) * 0.2)
        px, py = R.coords(params, h, w)
        if min((px - px.round()).abs().min().item(), (py - py.round()).abs().min().item()) > 0.02:
            break
    else:
        pytest.fail('no parameters away from the kinks')
    logits = torch.randn(b, h, w, m + 1, generator=g, dtype=torch.float64).requires_grad_(True)
    image = torch.rand(b, h, w, c, generator=g, dtype=torch.float64)
    params.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda p, z: R.composite(z, image, p, m), (params, logits), eps=1e-6)


def test_zero_parameters_reproduce_the_image():
    _, z, image, _ = R.case((2, 6, 9, 3, 4), seed=3)
    image = image.double()
    t = R.warp(image, torch.zeros(2, 24, dtype=torch.float64))
    assert all(torch.equal(t[:, m], image) for m in range(4))
    assert (R.composite(z.double(), image, torch.zeros(2, 24, dtype=torch.float64), 4) - image).abs().max().item() <= 1e-15


def test_one_hot_masks_give_a_piece_or_the_image():
    shape = (2, 6, 7, 3, 4)
    params, _, image, _ = R.case(shape, seed=3, spread=2)
    params, image = params.double(), image.double()
    pieces = R.warp(image, params)
    for j in range(5):
        z = torch.full((2, 6, 7, 5), -1e4, dtype=torch.float64)
        z[..., j] = 0.0
        got = R.composite(z, image, params, 4)
        assert torch.equal(got, image if j == 0 else pieces[:, j - 1]), j


def test_graph_variables_match_the_restatement():
    G.reset_default_graph()
    optim.set_data_parallel(1)
    img, act = G.placeholder((2, 64, 64, 3), name='img'), G.placeholder((2, 10), name='act')
    frame, state = M.build_generator_affine(img, act, num_masks=6)
    assert frame.shape == (2, 64, 64, 3) and state.shape == (2, 5)
    got = {n: v.shape for n, v in G.get_default_graph().variables.items()}
    want = {n: tuple(v.shape) for n, v in R.init_params_affine(num_masks=6).items() if n.startswith('g/')}
    assert got == want
    assert got['g/affine_params/weights'] == (4, 4, 266, 36) and got['g/tconv4/weights'] == (5, 5, 7, 128)
    assert 'g/cdna_params/weights' not in got


@pytest.mark.parametrize('kw', [dict(num_masks=0), dict(num_masks=33), dict(size=40), dict(color_channels=1), dict(batch_size=3)], ids=str)
def test_builder_rejects_unsupported_geometry(kw):
    G.reset_default_graph()
    s = kw.pop('size', 64)
    img, act = G.placeholder((2, s, s, 3), name='img'), G.placeholder((2, 10), name='act')
    with pytest.raises(ValueError):
        M.build_generator_affine(img, act, **kw)
    assert not G.get_default_graph().variables


def test_builder_rejects_bf16():
    G.reset_default_graph()
    G.get_default_graph().act_dtype = torch.bfloat16
    try:
        img, act = G.placeholder((2, 64, 64, 3), name='img'), G.placeholder((2, 10), name='act')
        with pytest.raises(NotImplementedError):
            M.build_generator_affine(img, act)
        assert not G.get_default_graph().variables
    finally:
        G.reset_default_graph()


def test_trainer_names_the_generator_and_declines_rollouts_and_maps():
    assert T.model_kind('affine') == 'affine'
    with pytest.raises(ValueError, match='image gradient'):
        T.check_rollout(2, 'affine')
    assert T.check_rollout(1, 'affine') == 1
    with pytest.raises(ValueError, match='map advection'):
        T.check_pixel_maps(1, 'affine')
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cpu', lib=object())
    with pytest.raises(ValueError, match='image gradient'):
        T.Trainer(sess, True, 'bce', 'adam', 'affine', batch_size=2, rollout_steps=2)
    with pytest.raises(ValueError, match='map advection'):
        T.Trainer(sess, True, 'bce', 'adam', 'affine', batch_size=2, pixel_maps=1)
    assert not G.get_default_graph().variables
    with pytest.raises(ValueError, match='map advection'):
        P.check_pixel_args([[1, 2]], [[3.0, 4.0]], None, 'affine', 64)


@pytest.mark.parametrize('extra', [['--affine', '--dna'], ['--affine', '--cdna'], ['--affine', '--dtype', 'bf16'],
                                   ['--affine', '--num_masks', '0'], ['--affine', '--num_masks', '33']], ids=str)
def test_cli_argument_errors(tmp_path, monkeypatch, extra):
    monkeypatch.setattr(T, 'train', lambda *a, **kw: pytest.fail('train() reached'))
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: pytest.fail('evaluate() reached'))
    monkeypatch.setattr(P, 'plan_sequences', lambda *a, **kw: pytest.fail('plan_sequences() reached'))
    with pytest.raises(SystemExit):
        T.main(['synthetic', str(tmp_path / 'out')] + extra)
    assert not (tmp_path / 'out').exists()
    with pytest.raises(SystemExit):
        E.main(['models', 'synthetic', str(tmp_path / 'eval'), '--num_sequences', '4'] + extra)
    assert not (tmp_path / 'eval').exists()
    with pytest.raises(SystemExit):
        P.main(['models', 'synthetic', str(tmp_path / 'plan'), '--num_sequences', '4'] + extra)
    assert not (tmp_path / 'plan').exists()


def test_cli_declines_rollout_steps(tmp_path, monkeypatch):
    monkeypatch.setattr(T, 'train', lambda *a, **kw: pytest.fail('train() reached'))
    with pytest.raises(SystemExit):
        T.main(['synthetic', str(tmp_path / 'out'), '--affine', '--rollout_steps', '2'])
    assert not (tmp_path / 'out').exists()


def test_clis_pass_the_affine_generator_on(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(T, 'train', lambda *a, **kw: seen.update(kw, positional=a))
    T.main(['synthetic', str(tmp_path / 'out'), '--affine', '--num_masks', '7', '--ksize', '4'])      # (--ksize is not read)
    assert seen['positional'][8] == 'affine' and seen['num_masks'] == 7
    assert 'affine' not in seen.get('options', {})
    seen.clear()
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: seen.update(kw))
    E.main(['models', 'synthetic', str(tmp_path / 'eval'), '--affine', '--num_masks', '5', '--num_sequences', '4'])
    assert seen['affine'] is True and seen['dna'] is False and seen['cdna'] is False and seen['num_masks'] == 5
    seen.clear()
    monkeypatch.setattr(P, 'plan_sequences', lambda *a, **kw: seen.update(kw))
    P.main(['models', 'synthetic', str(tmp_path / 'plan'), '--affine', '--num_masks', '5', '--num_sequences', '4'])
    assert seen['affine'] is True and seen['dna'] is False and seen['cdna'] is False and seen['num_masks'] == 5


def test_library_functions_decline_two_generators():
    with pytest.raises(ValueError, match='two different generators'):
        E.evaluate('models', 'synthetic', 'out', affine=True, cdna=True)
    with pytest.raises(ValueError, match='two different generators'):
        P.plan_sequences('models', 'synthetic', 'out', affine=True, dna=True)


def test_the_c_oracle_raises_a_clear_error():
    import numpy as np
    from oracle import cbind
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cpu', lib=cbind.load())
    tr = T.Trainer(sess, True, 'bce', 'adam', 'affine', batch_size=2, num_masks=3)
    sess.run(G.global_variables_initializer())
    x, a = np.zeros((2, 64, 64, 3), np.float32), np.zeros((2, 10), np.float32)
    with pytest.raises(RuntimeError, match='acg_affine_composite_fwd'):
        tr.test(x, x, a)
