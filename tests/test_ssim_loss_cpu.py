"""The SSIM training loss without a GPU: the restatements' own identities (tests/ssim_loss_ref.py), the graph a Trainer builds
with and without ``ssim_weight``, the clear error on the C oracle, the CLI flag, and loss values of more than four heads."""
import numpy as np
import pytest
import torch

import ssim_loss_ref as R
import ssim_ref as SR
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import ops as O
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T
from action_conditioned_gans_amd.saver import Saver

SHAPES = [(1, 11, 11, 1), (2, 12, 13, 3), (1, 21, 27, 4), (2, 33, 75, 3)]


def _session():
    from oracle import cbind
    G.reset_default_graph()
    optim.set_data_parallel(1)
    return G.Session(device='cpu', lib=cbind.load())


def _ops(transform=True, **kw):
    """(session, trainer, op list) in the form tests/test_ema_cpu.py compares graphs in."""
    sess = _session()
    tr = T.Trainer(sess, True, 'bce', 'adam', transform, batch_size=2, **kw)
    return sess, tr, [(type(o).__name__, o.name, o.index, [t.shape for t in o.outputs]) for o in G.get_default_graph().ops]


def _inputs(b=2, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (b, 64, 64, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (b, 64, 64, 3)).astype(np.float32)
    a = rng.standard_normal((b, 10)).astype(np.float32)
    return x, y, a, a[:, 5:].copy()


# ---- the restatements ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@pytest.mark.parametrize('kind', R.CLASSES)
def test_closed_form_equals_autograd_in_float64(kind, shape):
    x, y = R.case(kind, shape, seed=1)
    want, got = R.grad_autograd(x, y), R.grad_closed64(x, y)
    scale = np.abs(want).max()
    # both are float64 evaluations of one function: they differ by rounding only (measured <= 2e-12 of max|g|, the largest on
    # constant frames where sigma^2 is a difference of equal numbers); a wrong term is off by 1e-2 and more
    assert scale > 0 and np.abs(got - want).max() <= 1e-10 * scale


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_value_is_the_metric(shape):
    x, y = R.case('smooth', shape, seed=2)
    want = float((1.0 - SR.ssim(x, y)).sum())
    assert R.value64(x, y) == want
    got = float(R.loss_t(torch.from_numpy(x).double(), torch.from_numpy(y).double()))
    assert abs(got - want) <= 1e-12 * shape[0]
    assert abs(R.value64(x, x)) <= 1e-12 * shape[0]             # SSIM(x, x) = 1


@pytest.mark.parametrize('kind', R.CLASSES)
def test_float32_floors_are_float32_sized(kind):
    """The two float32 evaluations the GPU test takes its bar from: they differ from float64, and by a float32-sized amount."""
    x, y = R.case(kind, (2, 33, 75, 3), seed=3)
    g64 = R.grad_autograd(x, y)
    scale = np.abs(g64).max()
    e_a = np.abs(R.grad_autograd(x, y, torch.float32) - g64).max() / scale
    e_b = np.abs(R.grad_closed32(x, y) - g64).max() / scale
    print('%s: e_a %.2e e_b %.2e of max|g| %.3e' % (kind, e_a, e_b, scale))
    assert 0 < max(e_a, e_b) <= 5e-3


def test_gradient_is_shift_invariant_in_exact_arithmetic():
    """The closed form with and without the per-(frame, channel) shift, both in float64: one function."""
    x, y = R.case('smooth', (2, 12, 13, 3), seed=4)
    a = R._closed(x, y, np.float64, shift=False, rewrite=False)
    b = R._closed(x, y, np.float64, shift=True, rewrite=True)
    assert np.abs(a - b).max() <= 1e-10 * np.abs(a).max()


# ---- the graph, on the C oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('transform,kw', [(False, {}), (True, {}), ('cdna', {}), (True, dict(rollout_steps=2, lookahead=False)),
                                          (False, dict(rollout_steps=2, lookahead=False))], ids=str)
def test_weight_zero_builds_the_graph_it_always_built(transform, kw):
    _, tr0, a = _ops(transform, **kw)
    keys_a, names_a, state_a = sorted(Saver()._tensors()), list(tr0._summary_names), len(G.get_default_graph().state)
    _, tr, b = _ops(transform, ssim_weight=0, **kw)
    assert a == b and sorted(Saver()._tensors()) == keys_a and tr._summary_names == names_a
    assert len(G.get_default_graph().state) == state_a
    assert tr.g_ssim_loss is None and 'ssim_loss_heads' not in G.get_default_graph().collections
    assert not any(isinstance(o, O.SsimLossOp) for o in G.get_default_graph().ops)


@pytest.mark.parametrize('transform', [False, True, 'cdna'], ids=str)
def test_weight_adds_the_head_the_summary_and_nothing_to_checkpoints(transform):
    _, tr0, _ = _ops(transform)
    keys0, names0, vars0 = sorted(Saver()._tensors()), list(tr0._summary_names), list(G.get_default_graph().variables)
    _, tr, _ = _ops(transform, ssim_weight=50.0)
    g = G.get_default_graph()
    assert sorted(Saver()._tensors()) == keys0 and list(g.variables) == vars0
    assert tr._summary_names == sorted(names0 + ['g_ssim_loss'])
    heads = [o for o in g.ops if isinstance(o, O.SsimLossOp) and o.dgen is None]
    grads = [o for o in g.ops if isinstance(o, O.SsimLossOp) and o.dgen is not None]
    assert len(heads) == 1 and heads[0].inputs == [tr.g_out, tr.next_frame_ph]
    # one gradient op per optimizer that sees the term (G step, pretraining step), each with the head's weight W / B
    assert len(grads) == 2 and all(o.grad_weight == 50.0 / 2 and o.inputs[0] is tr.g_out for o in grads)
    assert tr.g_ssim_loss.terms == [(heads[0], 0, 0.5)]
    n_heads = 5 if transform else 4                        # L1, (state), SSIM, adversarial, GDL
    assert len(tr.g_loss.terms) == n_heads and (heads[0], 0, 25.0) in tr.g_loss.terms and (heads[0], 0, 25.0) in tr.g_l2_loss.terms
    t = tr.g_loss.tensor()
    assert t.shape == (1,) and isinstance(t.op, O.CombineOp)
    if n_heads == 5:                                       # the first four, then the partial result plus the fifth
        assert len(t.op.terms) == 2 and isinstance(t.op.terms[0][0], O.CombineOp) and len(t.op.terms[0][0].terms) == 4


def test_every_rollout_step_carries_the_term():
    _, tr, _ = _ops(True, ssim_weight=8.0, rollout_steps=3, lookahead=False)
    g = G.get_default_graph()
    heads = [o for o in g.ops if isinstance(o, O.SsimLossOp) and o.dgen is None]
    assert [tuple(o.inputs) for o in heads[1:]] == [(tr.rollout_frames[j], tr.roll_next_ph[j]) for j in range(3)]
    for j, loss in enumerate(tr.rollout_losses):
        assert (heads[1 + j], 0, 4.0) in loss.terms and len(loss.terms) == 5
    # one gradient op per step in each of the two rollout updates, at W / (B K)
    grads = [o for o in g.ops if isinstance(o, O.SsimLossOp) and o.dgen is not None and o.name.startswith('ssim_loss') and
             any(o.inputs[0] is f for f in tr.rollout_frames)]
    assert len(grads) == 6 and all(abs(o.grad_weight - 8.0 / 2 / 3) < 1e-12 for o in grads)


@pytest.mark.parametrize('weight', [-1, -1e-9, float('nan'), float('inf'), 1e39, 'x', True, None], ids=repr)
def test_invalid_weights_raise_before_anything_is_created(weight):
    sess = _session()
    with pytest.raises(ValueError, match='ssim_weight'):
        T.Trainer(sess, True, 'bce', 'adam', True, batch_size=2, ssim_weight=weight)
    g = G.get_default_graph()
    assert not g.ops and not g.variables and not g.state
    with pytest.raises(ValueError, match='ssim_weight'):
        T.train('synthetic', None, None, None, None, True, 'bce', 'adam', True, ssim_weight=weight, device='cpu')


def test_the_c_oracle_raises_a_clear_error():
    x, y, a, s = _inputs()
    sess, tr, _ = _ops(True, ssim_weight=50.0, lookahead=False)
    sess.run(G.global_variables_initializer())
    tr.train_d(x, y, a)                                     # the D step carries no SSIM term: it runs
    with pytest.raises(RuntimeError, match='acg_ssim_loss'):
        tr.train_g(x, y, a, s)
    with pytest.raises(RuntimeError, match='acg_ssim_loss'):
        tr.pretrain_g(x, y, a, s)
    with pytest.raises(RuntimeError, match='acg_ssim_loss'):
        tr.test(x, y, a)                                    # the summaries read the head


def test_head_rejects_what_the_kernel_does_not_take():
    _session()
    ok = G.placeholder((2, 16, 16, 3))
    for shape in [(2, 10, 16, 3), (2, 16, 10, 3), (2, 16, 16, 5), (2, 16, 16)]:
        with pytest.raises(ValueError, match='ssim loss'):
            O.ssim_loss(G.placeholder(shape), G.placeholder(shape))
    with pytest.raises(ValueError, match='shapes differ'):
        O.ssim_loss(ok, G.placeholder((2, 16, 17, 3)))
    with pytest.raises(ValueError, match='dense float32'):
        O.ssim_loss(G.placeholder((2, 16, 16, 3), channel_pitch=4), G.placeholder((2, 16, 16, 3), channel_pitch=4))
    a = O.ssim_loss(ok, G.placeholder((2, 16, 16, 3), name='t'))
    assert len(a.terms) == 1


def test_one_head_per_pair_of_tensors():
    _session()
    x, y = G.placeholder((2, 16, 16, 3)), G.placeholder((2, 16, 16, 3))
    assert O.ssim_loss(x, y).terms[0][0] is O.ssim_loss(x, y).terms[0][0] is O.ssim_loss(y, x).terms[0][0]


# ---- loss values of more than four heads ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_terms', [1, 4, 5, 6, 7, 8])
def test_scalar_tensor_chains_combine_ops(n_terms):
    sess = _session()
    rng = np.random.default_rng(n_terms)
    phs = [G.placeholder((3, 5), name='x%d' % k) for k in range(n_terms)]
    vals = [rng.standard_normal((3, 5)).astype(np.float32) for _ in range(n_terms)]
    weights = [float(w) for w in rng.uniform(-2, 2, n_terms)]
    loss = sum((O.reduce_mean(ph, name='m%d' % k) * w for k, (ph, w) in enumerate(zip(phs, weights))), 0)
    assert len(loss.terms) == n_terms
    n_ops = len(G.get_default_graph().ops)
    t = loss.tensor()
    combines = [o for o in G.get_default_graph().ops[n_ops:]]
    assert all(isinstance(o, O.CombineOp) and len(o.terms) <= 4 for o in combines)
    assert len(combines) == (1 if n_terms <= 4 else 1 + -(-(n_terms - 4) // 3))
    sess.run(G.global_variables_initializer())
    got = float(np.asarray(sess.run([loss], dict(zip(phs, vals)))[0]).reshape(-1)[0])
    want = sum(w * float(v.astype(np.float64).mean()) for w, v in zip(weights, vals))
    assert abs(got - want) <= 1e-5 * sum(abs(w) for w in weights)
    assert loss.tensor() is t


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_passes_ssim_weight_on(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(T, 'train', lambda *a, **kw: seen.update(kw))
    T.main(['synthetic', str(tmp_path / 'out'), '--dna', '--adv', 'True', '--ssim_weight', '50'])
    assert seen['ssim_weight'] == 50.0
    T.main(['synthetic', str(tmp_path / 'out2')])
    assert seen['ssim_weight'] == 0.0


@pytest.mark.parametrize('value', ['-1', '-0.5', 'nan', 'inf'])
def test_cli_rejects_a_negative_or_non_finite_weight(tmp_path, monkeypatch, value):
    monkeypatch.setattr(T, 'train', lambda *a, **kw: pytest.fail('train() reached'))
    with pytest.raises(SystemExit):
        T.main(['synthetic', str(tmp_path / 'out'), '--ssim_weight', value])
    assert not (tmp_path / 'out').exists()


def test_help_text_states_the_scale(capsys):
    with pytest.raises(SystemExit):
        T.main(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert '--ssim_weight' in text and 'tens to hundreds' in text


# ---- the whole step on the C oracle, with the missing entry stood in by the float64 closed form ---------------------------------
def _numpy_entry(monkeypatch, lib):
    """acg_ssim_loss / acg_ssim_loss_workspace_bytes on host pointers by tests/ssim_loss_ref.py (undone after the test)."""
    import ctypes

    def arr(p, shape):
        n = int(np.prod(shape))
        return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_float)), (n,)).reshape(shape)

    def ssim_loss(pred, truth, value, dpred, gw, n, h, w, c, data_range, k1, k2, ws, nbytes, stream):
        assert (data_range, k1, k2) == (2.0, 0.01, 0.03) and nbytes >= 16
        x, y = arr(pred, (n, h, w, c)), arr(truth, (n, h, w, c))
        if value is not None:
            arr(value, (1,))[0] = R.value64(x, y)
        if dpred is not None:
            arr(dpred, (n, h, w, c))[...] = gw * R.grad_closed64(x, y)
    monkeypatch.setattr(lib, 'ssim_loss', ssim_loss, raising=False)
    monkeypatch.setattr(lib, 'ssim_loss_workspace_bytes', lambda n, h, w, c: 16, raising=False)


@pytest.mark.parametrize('dna,step,weight', [(True, 'train_g', 5000.0), (False, 'pretrain_g', 2000.0)], ids=['dna_train_g', 'plain_pretrain_g'])
def test_step_on_the_c_oracle_matches_the_oracle_trainer(monkeypatch, dna, step, weight):
    """The host side end to end - head, weight W / B, gradient fan-in, the 5-term loss value, the summary - with the one missing
    kernel stood in by the float64 closed form: frames, losses and per-variable gradient norms against SsimOracleTrainer."""
    import train_cases as TC
    from oracle import cbind, models as OM
    _numpy_entry(monkeypatch, cbind.load())
    x, y, a, s = TC.MG.inputs(2)
    sess = _session()
    tr = T.Trainer(sess, True, 'bce', 'adam', dna, batch_size=2, ssim_weight=weight, lookahead=False)
    sess.run(G.global_variables_initializer())
    params = OM.init_params(dna, batch=2, ksize=5, seed=TC.MG.PARAM_SEED, dtype=torch.float32)
    for n, v in G.get_default_graph().variables.items():
        sess.set_value(v, params[n])
    opt_op, key = (tr.g_opt_op, 'g_loss') if step == 'train_g' else (tr.g_pretrain_opt_op, 'g_l2_loss')
    res = sess.run([opt_op, tr.g_loss, tr.g_l2_loss, tr.g_ssim_loss, tr.g_next_frame], tr._feed(x, y, a, s))
    ref = R.SsimOracleTrainer({k: v.double() for k, v in params.items()}, True, 'bce', 'adam', dna, 5, ssim_weight=weight)
    td = lambda t: torch.from_numpy(t).double()     # noqa: E731
    p = ref._with_grad(ref.g_names)
    out = ref._g_losses(p, td(x), td(y), td(a), td(s))
    total, = torch.autograd.grad(out[key], out['frame'], retain_graph=True)
    part, = torch.autograd.grad(weight * out['g_ssim_loss'], out['frame'], retain_graph=True)
    assert float(part.norm() / total.norm()) >= 0.10          # the term is a visible part of what is compared
    grads = torch.autograd.grad(out[key], [p[n] for n in ref.g_names], allow_unused=True)
    want = {'g/' + n: g.norm() for n, g in zip(ref.g_names, grads) if g is not None}
    assert TC.rel(res[4], out['frame'].detach().numpy()) <= 1e-4
    for got, k in ((res[1], 'g_loss'), (res[2], 'g_l2_loss'), (res[3], 'g_ssim_loss')):
        assert abs(float(got[0]) - float(out[k])) <= 1e-4 * abs(float(out[k])), (k, float(got[0]), float(out[k]))
    TC.check_norms(TC.flat_grad_norms(sess, opt_op), want, 'g/', 1e-3, step + ' grad')
