"""The latent posterior without a GPU: known answers of the restatement (tests/latent_ref.py) and its gradients against torch
float64 autograd, the graph with ``posterior`` off and on, the single backward launch that carries the KL weight, every
refusal of the Trainer, train(), evaluate() and the two CLIs, the binding, and the clear error on the C oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import latent_ref as R
import noise_ref as NR
from action_conditioned_gans_amd import _lib
from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import models as M
from action_conditioned_gans_amd import ops as O
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement
def test_kl_known_answers():
    assert R.kl_sum(np.zeros((3, 10))) == 0.0                                         # mu = 0, logvar = 0
    stats = np.concatenate([np.ones((3, 5)), np.zeros((3, 5))], axis=1)               # mu = 1, logvar = 0 over n = 15 values
    assert R.kl_sum(stats) == 15 / 2
    out, kl, eps = R.latent_fwd(np.zeros((3, 2)), stats, 7, 0)
    assert kl == 7.5 and np.array_equal(out[:, 2:], 1.0 + eps)                        # sigma = 1


def test_forward_modes_of_the_restatement():
    rng = np.random.default_rng(0)
    a, stats = rng.standard_normal((3, 10)), rng.uniform(-2, 2, (3, 10))
    eps = NR.normals(7, 2, 1, 15).reshape(3, 5)
    mu, lv = stats[:, :5], stats[:, 5:]
    out, kl, e = R.latent_fwd(a, stats, 7, 2, stream_id=1, scale=0.5, posterior=True)
    assert np.array_equal(e, eps) and np.array_equal(out[:, :10], a)
    np.testing.assert_allclose(out[:, 10:], mu + 0.5 * np.exp(lv / 2) * eps, rtol=1e-15)
    assert np.array_equal(R.latent_fwd(a, stats, 7, 2, 1, 0.0, True)[0][:, 10:], mu)                       # the posterior mean
    for scale in (1.0, 0.5, 0.0):                                                                          # the prior: noise_concat
        assert np.array_equal(R.latent_fwd(a, stats, 7, 2, 1, scale, False)[0], NR.noise_concat(a, 5, 7, 2, 1, scale))
    assert R.latent_fwd(a, stats, 7, 2, 1, 1.0, False)[1] == kl                                            # kl in both modes


@pytest.mark.parametrize('posterior', [True, False])
@pytest.mark.parametrize('kl_weight', [0.0, 0.37])
def test_backward_of_the_restatement_against_autograd(posterior, kl_weight):
    rng = np.random.default_rng(1)
    b, a, z = 4, 3, 5
    actions, stats = rng.standard_normal((b, a)), np.concatenate([rng.uniform(-2, 2, (b, z)), rng.uniform(-6, 3, (b, z))], axis=1)
    dout = rng.standard_normal((b, a + z))
    out, _, eps = R.latent_fwd(actions, stats, 11, 3, posterior=posterior)
    dstats, dactions, mags = R.latent_bwd(dout, out, stats, posterior, kl_weight)
    ta, ts = torch.tensor(actions, requires_grad=True), torch.tensor(stats, requires_grad=True)
    mu, lv = ts[:, :z], ts[:, z:]
    lat = mu + torch.exp(0.5 * lv) * torch.tensor(eps) if posterior else torch.tensor(eps) + 0.0 * mu
    vec = torch.cat([ta, lat], dim=1)
    loss = (vec * torch.tensor(dout)).sum() + kl_weight * 0.5 * (mu * mu + torch.exp(lv) - lv - 1.0).sum()
    ga, gs = torch.autograd.grad(loss, [ta, ts])
    np.testing.assert_allclose(dstats, gs.numpy(), rtol=1e-12, atol=1e-12)
    assert np.array_equal(dactions, ga.numpy()) and (mags >= np.abs(dstats) - 1e-15).all()
    kl_only = R.latent_bwd(None, out, stats, posterior, 0.37)[0]                                           # a NULL dout
    np.testing.assert_allclose(kl_only, np.concatenate([0.37 * stats[:, :z], 0.37 * 0.5 * np.expm1(stats[:, z:])], axis=1), rtol=1e-15)


def test_oracle_trainer_draws_what_the_restatement_draws():
    z, b = 3, 2
    params = {k: v.double() for k, v in R.init_params(False, z, batch=b, img=32, seed=2).items()}
    assert {k for k in params if k.startswith('g/posterior/')} == \
        {'g/posterior/conv%d/%s' % (i, s) for i in range(1, 5) for s in ('weights', 'BatchNorm/beta')} | {'g/posterior/head/weights', 'g/posterior/head/biases'}
    assert tuple(params['g/posterior/head/weights'].shape) == (2, 2, 256, 2 * z) and tuple(params['g/posterior/conv1/weights'].shape) == (5, 5, 6, 32)
    ot = R.LatentOracleTrainer(params, False, 'bce', 'adam', False, latent_dim=z, kl_weight=0.5)
    rng = np.random.default_rng(3)
    x, y = (torch.from_numpy(rng.uniform(-1, 1, (b, 32, 32, 3))) for _ in range(2))
    a = torch.from_numpy(rng.standard_normal((b, 10)))
    ot.draw = (5, 9)
    p = ot._with_grad(ot.g_names)
    out = ot._g_losses(p, x, y, a, None)
    stats = ot.last_stats.numpy()
    want, kl, _ = R.latent_fwd(a.numpy(), stats, 5, 9)
    np.testing.assert_allclose(ot.last_z.numpy(), want[:, 10:], rtol=1e-12)
    np.testing.assert_allclose(float(out['g_kl'].detach()), kl / b, rtol=1e-12)
    plain = float((torch.abs(out['frame'] - y).sum() / b).detach())
    np.testing.assert_allclose(float(out['g_loss'].detach()), plain + 0.5 * kl / b, rtol=1e-12)
    grads = torch.autograd.grad(out['g_loss'], [p[n] for n in ot.g_names], allow_unused=True)
    assert all(g is not None and float(g.abs().max()) > 0 for n, g in zip(ot.g_names, grads) if n.startswith('g/posterior/'))


# ---- the binding
def test_binding_and_header():
    sigs = _lib.EXTENSIONS['rollout'].signatures
    header = open(os.path.join(ROOT, 'include', 'acgan_rollout.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (('acg_latent_fwd', 11), ('acg_latent_bwd', 11)):
        assert sigs[name][0] is _lib.STATUS and len(sigs[name][1]) == nargs and re.search(r'int32_t %s\(' % name, code) and hasattr(cdll, name)
        assert name not in _lib.SIGNATURES and not any(name in e.signatures for k, e in _lib.EXTENSIONS.items() if k != 'rollout')
    assert sigs['acg_latent_bwd'][1][4] is ctypes.c_float                              # kl_weight, by value
    assert 'NO clamp on logvar' in header
    assert _lib.ABI_VERSION == 8
    assert 'the latent posterior' in _lib.EXTENSIONS['rollout'].what and _lib.EXTENSIONS['rollout'].what.endswith('run on the HIP library only')


# ---- Trainer
def _trainer(transform=True, **kw):
    from oracle import cbind
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cpu', lib=cbind.load())
    tr = T.Trainer(sess, True, 'bce', 'adam', transform, batch_size=2, **kw)
    return sess, tr, G.get_default_graph()


def _describe(tr, g):
    return ([(type(o).__name__, o.name, o.index, [t.shape for t in o.outputs]) for o in g.ops],
            [(n, v.shape) for n, v in g.variables.items()], [(s.name, s.shape, s.dtype) for s in g.state], sorted(tr.summaries))


@pytest.mark.parametrize('transform', [False, True, 'cdna'], ids=str)
@pytest.mark.parametrize('base', [dict(), dict(noise_dim=4, noise_seed=3)], ids=['plain', 'noise'])
def test_posterior_off_builds_the_graph_it_always_built(transform, base):
    a = _describe(*_trainer(transform, **base)[1:])
    b = _describe(*_trainer(transform, posterior=False, kl_weight=0.25, **base)[1:])
    assert a == b
    g = G.get_default_graph()
    assert not any(isinstance(o, (O.LatentOp, O.LatentBwdOp)) for o in g.ops) and 'latent' not in g.collections
    assert not any(n.startswith('g/posterior') for n in g.variables)


@pytest.mark.parametrize('transform', [False, True], ids=['plain', 'dna'])
def test_posterior_on_adds_the_encoder_under_g_posterior(transform):
    _, base_tr, base_g = _trainer(transform, noise_dim=4, noise_seed=11)
    base_vars, base_state, base_summ = {n: v.shape for n, v in base_g.variables.items()}, {s.name for s in base_g.state}, set(base_tr.summaries)
    _, tr, g = _trainer(transform, noise_dim=4, noise_seed=11, posterior=True, kl_weight=0.5)
    new = [n for n in g.variables if n not in base_vars]
    assert new and all(n.startswith('g/posterior/') for n in new)
    assert {n: v.shape for n, v in g.variables.items() if n in base_vars} == base_vars
    assert g.variables['g/posterior/conv1/weights'].shape == (5, 5, 6, 32) and g.variables['g/posterior/head/weights'].shape == (4, 4, 256, 8)
    assert g.variables['g/posterior/head/biases'].shape == (8,) and 'g/posterior/head/BatchNorm/beta' not in g.variables
    assert not g.variables['g/posterior/head/biases'].value.any() and g.variables['g/posterior/head/weights'].value.any()
    assert all(g.variables[n] in tr.g_vars for n in new) and not any(v.name.startswith('g/posterior') for v in tr.d_vars)
    assert set(tr.summaries) == base_summ | {'g_kl'}
    # one LatentOp in place of the NoiseOp, on the SAME named state; the mode is unnamed; no new named state
    assert sum(isinstance(o, O.LatentOp) for o in g.ops) == 1 and not any(isinstance(o, O.NoiseOp) for o in g.ops) and not tr.lookahead
    state, mode = O.latent_state()
    assert state is O.noise_state()[0] and (state.name, state.init) == ('g/noise/state', (11, 0))
    assert (mode.name, mode.shape, mode.dtype, mode.init) == (None, (2,), torch.float32, (1.0, 1.0))
    assert {s.name for s in g.state if s.name} == base_state - {None}           # (the optimizers' flat slots grow; no new name)
    from action_conditioned_gans_amd.saver import Saver
    keys = set(Saver()._tensors())
    assert 'state:g/noise/state' in keys and sum('noise' in k for k in keys) == 1 and 'var:g/posterior/head/weights' in keys
    assert tr._noise.shape == (2, 14) and tr._noise.op.inputs[1].shape == (2, 8)


def test_one_backward_launch_carries_the_kl_weight():
    """Each G update holds ONE LatentBwdOp, fed the generator's gradient of the vector, with kl_weight / B: no seed launch, no AddOp
    on the gradient of the stats.  The D update holds none (nothing of D's loss reaches the encoder)."""
    _, tr, g = _trainer(True, noise_dim=4, posterior=True, kl_weight=0.5)
    bwd = [o for o in g.ops if isinstance(o, O.LatentBwdOp)]
    assert len(bwd) == 2                                             # g_opt and g_pretrain_opt
    for op in bwd:
        assert op.kl_weight == 0.5 / 2 and op.has_dvec and op.dactions is None and len(op.inputs) == 3
        assert op.inputs[1] is tr._noise and op.inputs[2] is tr._noise.op.inputs[1]
        users = [o for o in g.ops if any(i is op.dstats for i in o.inputs)]
        assert users and not any(type(o).__name__ == 'AddOp' for o in users)
    # the loss value: kl is one more term of both Scalars, weighed the same
    kl_op = tr._noise.op
    for loss in (tr.g_loss, tr.g_l2_loss):
        assert [(h, i, w) for h, i, w in loss.terms if h is kl_op] == [(kl_op, 1, 0.25)]
    assert tr.summaries['g_kl'].terms == [(kl_op, 1, 0.5)]


def test_latent_op_gradient_protocol():
    G.reset_default_graph()
    a, stats = G.placeholder((3, 10), name='a'), G.placeholder((3, 10), name='stats')
    vec, kl = O.append_latent(a, stats)
    op = vec.op
    assert vec.shape == (3, 15) and kl.terms == [(op, 1, 1.0)] and op.outputs[1].shape == (1,)
    assert op.seed({1: 0.5}, [False, False]) == []
    (t, mark), = op.seed({1: 0.5}, [False, True])
    assert t is op.outputs[1] and mark.weight == 0.5
    with pytest.raises(ValueError):
        op.seed({0: 1.0}, [False, True])
    n = len(G.get_default_graph().ops)
    assert len(G.get_default_graph().ops) == n                      # (seed launched nothing)
    gout = G.placeholder((3, 15), name='gout')
    da, ds = op.grad([gout, mark], [True, True], None)
    assert isinstance(ds.op, O.LatentBwdOp) and ds.op is da.op and ds.shape == (3, 10) and da.shape == (3, 10) and ds.op.kl_weight == 0.5
    da, ds = op.grad([None, mark], [False, True], None)             # the KL term alone
    assert da is None and not ds.op.has_dvec and len(ds.op.inputs) == 2
    da, ds = op.grad([gout, None], [False, True], None)             # no KL term in this loss
    assert ds.op.kl_weight == 0.0
    da, ds = op.grad([gout, None], [True, False], None)             # the actions alone: NoiseOp's slice
    assert ds is None and isinstance(da.op, O.SliceOp) and (da.op.c_off, da.op.c_dst, da.shape) == (0, 10, (3, 10))


def test_append_latent_rejections():
    G.reset_default_graph()
    a = G.placeholder((2, 10), name='a')
    for shape in ((2, 7), (3, 8), (2, 130), (2, 2, 4)):
        with pytest.raises(ValueError):
            O.append_latent(a, G.placeholder(shape, name='s'))
    with pytest.raises(ValueError):
        O.append_latent(G.placeholder((256, 10), name='b'), G.placeholder((256, 128), name='s'))
    with pytest.raises(ValueError):
        M.build_posterior(G.placeholder((2, 64, 64, 3), name='x'), 4)
    assert not G.get_default_graph().ops and not G.get_default_graph().variables


@pytest.mark.parametrize('kw,match', [
    (dict(posterior=True), 'posterior needs noise_dim'),
    (dict(posterior=True, noise_dim=0), 'posterior needs noise_dim'),
    (dict(posterior=True, noise_dim=4, kl_weight=-1.0), 'kl_weight'),
    (dict(posterior=True, noise_dim=4, kl_weight=float('nan')), 'kl_weight'),
    (dict(posterior=True, noise_dim=4, kl_weight=float('inf')), 'kl_weight'),
    (dict(posterior=True, noise_dim=4, kl_weight='x'), 'kl_weight'),
    (dict(posterior=False, noise_dim=4, kl_weight=-1.0), 'kl_weight'),
    (dict(posterior=True, noise_dim=4, rollout_steps=2), r'noise_dim > 0 does not go with rollout_steps'),
    (dict(posterior=True, noise_dim=4, bn_inference=True), r'noise_dim > 0 does not go with bn_inference')], ids=str)
def test_trainer_rejections_leave_the_graph_alone(kw, match):
    G.reset_default_graph()
    optim.set_data_parallel(1)
    g = G.get_default_graph()
    with pytest.raises(ValueError, match=match):
        T.Trainer(None, True, 'bce', 'adam', True, batch_size=2, **kw)
    assert len(g.ops) == 0 and not g.variables and not g.state and not g.collections.get('noise') and not g.collections.get('latent')


def test_a_bf16_graph_is_declined_before_anything_is_created():
    G.reset_default_graph()
    optim.set_data_parallel(1)
    g = G.get_default_graph()
    g.act_dtype = torch.bfloat16
    with pytest.raises(ValueError, match='bf16'):
        T.Trainer(None, True, 'bce', 'adam', True, batch_size=2, noise_dim=4, posterior=True)
    assert len(g.ops) == 0 and not g.variables and not g.state
    with pytest.raises(ValueError, match='bf16'):
        T.check_posterior(True, 1.0, 4, bf16=True)
    assert T.check_posterior(True, 0, 4) == (True, 0.0) and T.check_posterior(False, 2, 0) == (False, 2.0)


def test_posterior_modes_need_a_posterior():
    sess, tr, _ = _trainer(noise_dim=4)
    x, a = np.zeros((2, 64, 64, 3), np.float32), np.zeros((2, 10), np.float32)
    for mode in ('posterior', 'posterior_mean'):
        with pytest.raises(RuntimeError, match='without posterior'):
            tr.test(x, x, a, noise=mode)
        with pytest.raises(RuntimeError, match='without posterior'):
            tr.test_sequence(np.stack([x, x], 1), np.stack([x, x], 1), np.stack([a, a], 1), noise=mode)
    with pytest.raises(ValueError, match='noise must be'):
        tr.test(x, x, a, noise='gauss')
    assert T.NOISE_MODES == {'zero': (0.0, 0.0), 'sample': (1.0, 0.0), 'posterior': (1.0, 1.0), 'posterior_mean': (0.0, 1.0)}


def test_the_mode_is_written_only_when_it_changes():
    sess, tr, _ = _trainer(noise_dim=4, posterior=True)
    sess.run(G.global_variables_initializer())
    buf = sess._materialize(O.latent_state()[1])
    assert buf.tolist() == [1.0, 1.0] and tr._noise_on is None
    for mode, want in T.NOISE_MODES.items():
        tr._noise_switch(mode)
        assert buf.tolist() == list(want) and tr._noise_on == mode
    tr._noise_switch(True)
    assert buf.tolist() == [1.0, 1.0] and tr._noise_on == 'posterior'
    buf.fill_(5.0)                                        # behind the Trainer's back: an unchanged mode is not written again ...
    tr._noise_switch(True)
    assert buf.tolist() == [5.0, 5.0]
    tr._noise_switch('posterior', always=True)            # ... unless the caller says so (the predicting calls)
    assert buf.tolist() == [1.0, 1.0]


def test_the_c_oracle_raises_the_extensions_message():
    sess, tr, _ = _trainer(noise_dim=4, posterior=True)
    sess.run(G.global_variables_initializer())
    x = np.zeros((2, 64, 64, 3), np.float32)
    with pytest.raises(RuntimeError, match=r'acg_latent_fwd \(include/acgan_rollout.h\)') as err:
        tr.test(x, x, np.zeros((2, 10), np.float32), noise='posterior')
    assert 'the latent posterior' in str(err.value) and 'run on the HIP library only' in str(err.value)


def test_a_predicting_restore_skips_the_flat_g_slots_of_a_posterior_checkpoint(tmp_path):
    """Extra variable keys are ignored by the Saver; the G optimizers' flat slots are laid out with the encoder and fit no buffer
    of a plain noise_dim graph: a bare restore stops there, evaluate.predicting_trainer's skip_state leaves them out."""
    from action_conditioned_gans_amd.saver import Saver
    sess, tr, g = _trainer(noise_dim=4, posterior=True)
    sess.run(G.global_variables_initializer())
    post = Saver().save(sess, str(tmp_path / 'post'))
    want = {n: sess.get_value(v).clone() for n, v in g.variables.items()}
    assert E._slots_to_skip(post, True, 'raw') is None
    sess, tr, g = _trainer(noise_dim=4, seed=1)
    sess.run(G.global_variables_initializer())
    plain = Saver().save(sess, str(tmp_path / 'plain'))
    assert E._slots_to_skip(plain, False, 'raw') is None and E._slots_to_skip(plain, True, 'raw') is None
    with pytest.raises(ValueError, match='state:g_opt/m has shape'):
        Saver().restore(sess, post)
    skip = E._slots_to_skip(post, False, 'raw')
    assert skip('g_opt/m') and skip('g_pretrain_opt/v') and skip('g/ema/shadow') and not skip('d_opt/m') and not skip('g/noise/state')
    Saver().restore(sess, post, skip_state=skip)
    assert all(torch.equal(sess.get_value(v), want[n]) for n, v in g.variables.items())
    with pytest.raises(ValueError, match='add --posterior'):
        E._slots_to_skip(post, False, 'ema')
    sess, tr, g = _trainer(noise_dim=4, posterior=True)
    sess.run(G.global_variables_initializer())
    with pytest.raises(ValueError, match='lacks variables: g/posterior/|lacks variables: var:g/posterior/'):
        Saver().restore(sess, plain)


# ---- train() / evaluate() and the CLIs
def test_train_cli_passes_the_posterior_flags_on(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(T, 'train', lambda *a, **kw: seen.update(kw))
    T.main(['synthetic', str(tmp_path / 'a'), '--dna', '--noise_dim', '4', '--posterior', '--kl_weight', '0.5'])
    assert seen['posterior'] is True and seen['kl_weight'] == 0.5 and seen['noise_dim'] == 4
    T.main(['synthetic', str(tmp_path / 'b'), '--noise_dim', '4'])
    assert seen['posterior'] is False and seen['kl_weight'] == 1.0


@pytest.mark.parametrize('extra', [['--posterior'], ['--posterior', '--noise_dim', '0'], ['--noise_dim', '4', '--posterior', '--kl_weight', '-1'],
                                   ['--noise_dim', '4', '--posterior', '--kl_weight', 'nan'], ['--noise_dim', '4', '--posterior', '--kl_weight', 'inf'],
                                   ['--noise_dim', '4', '--posterior', '--dtype', 'bf16'],
                                   ['--dna', '--noise_dim', '4', '--posterior', '--rollout_steps', '2']], ids=str)
def test_train_cli_rejections_create_nothing(tmp_path, monkeypatch, extra):
    monkeypatch.setattr(T, 'train', lambda *a, **kw: pytest.fail('train() reached'))
    with pytest.raises(SystemExit):
        T.main(['synthetic', str(tmp_path / 'out')] + extra)
    assert not (tmp_path / 'out').exists()


def test_train_rejects_before_anything_is_created():
    G.reset_default_graph()
    g = G.get_default_graph()
    for kw in (dict(posterior=True), dict(posterior=True, noise_dim=4, kl_weight=-0.5), dict(posterior=True, noise_dim=4, dtype='bf16'),
               dict(posterior=True, noise_dim=4, rollout_steps=2)):
        with pytest.raises(ValueError):
            T.train('synthetic', None, None, None, None, True, 'bce', 'adam', True, batch_size=2, train_iter=1, **kw)
    assert G.get_default_graph() is g and not g.ops


def test_evaluate_cli_passes_the_posterior_flags_on(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: seen.update(kw))
    base = [str(tmp_path / 'm'), 'synthetic', str(tmp_path / 'o'), '--num_sequences', '4']
    E.main(base + ['--noise_dim', '4'])
    assert 'posterior' not in seen                                    # without the flag: the call it always made
    E.main(base + ['--noise_dim', '4', '--posterior', '--noise', 'posterior', '--noise_samples', '3'])
    assert (seen['posterior'], seen['noise'], seen['noise_samples']) == (True, 'posterior', 3)
    E.main(base + ['--noise_dim', '4', '--posterior', '--noise', 'posterior_mean'])
    assert (seen['posterior'], seen['noise'], seen['noise_samples']) == (True, 'posterior_mean', 1)
    E.main(base + ['--noise_dim', '4', '--posterior', '--noise', 'sample', '--noise_samples', '2'])
    assert (seen['posterior'], seen['noise'], seen['noise_samples']) == (True, 'sample', 2)


@pytest.mark.parametrize('extra', [['--posterior'], ['--noise_dim', '4', '--noise', 'posterior'], ['--noise_dim', '4', '--noise', 'posterior_mean'],
                                   ['--noise_dim', '4', '--posterior', '--noise', 'posterior_mean', '--noise_samples', '3'],
                                   ['--noise_dim', '4', '--posterior', '--noise', 'posterior', '--noise_samples', '0'],
                                   ['--noise_dim', '4', '--posterior', '--dtype', 'bf16'], ['--noise_dim', '4', '--posterior', '--kl_weight', '1']], ids=str)
def test_evaluate_cli_rejections_create_nothing(tmp_path, monkeypatch, extra):
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: pytest.fail('evaluate() reached'))
    with pytest.raises(SystemExit):
        E.main([str(tmp_path / 'm'), 'synthetic', str(tmp_path / 'o'), '--num_sequences', '4'] + extra)
    assert not (tmp_path / 'o').exists()


@pytest.mark.parametrize('kw', [dict(posterior=True), dict(noise_dim=4, noise='posterior'), dict(noise_dim=4, posterior=True, noise='posterior_mean', noise_samples=2),
                                dict(noise_dim=4, posterior=True, dtype='bf16'), dict(noise_dim=4, posterior=True, noise='gauss')], ids=str)
def test_evaluate_rejects_before_anything_is_created(tmp_path, kw):
    with pytest.raises(ValueError):
        E.evaluate(str(tmp_path / 'm'), 'synthetic', str(tmp_path / 'o'), num_sequences=4, **kw)
    assert not (tmp_path / 'o').exists()
