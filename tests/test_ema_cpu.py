"""The generator's weight average without a GPU: the restatement's own identities (tests/ema_ref.py), the graph a Trainer
builds with and without ``ema_decay``, the checkpoint keys, the clear error on the C oracle, the two CLIs' flags, and the
share of elements of a real float32 trajectory whose update meets a subnormal intermediate."""
import numpy as np
import pytest
import torch

import ema_ref as R
from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T
from action_conditioned_gans_amd.saver import Saver


def _ops(**kw):
    """(session, trainer, op list) in the form tests/test_rollout_train_cpu.py compares graphs in."""
    from oracle import cbind
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cpu', lib=cbind.load())
    tr = T.Trainer(sess, True, 'bce', 'adam', True, batch_size=2, **kw)
    return sess, tr, [(type(o).__name__, o.name, o.index, [t.shape for t in o.outputs]) for o in G.get_default_graph().ops]


def _inputs(b=2, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (b, 64, 64, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (b, 64, 64, 3)).astype(np.float32)
    a = rng.standard_normal((b, 10)).astype(np.float32)
    return x, y, a, a[:, 5:].copy()


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_float32_restatement_tracks_the_float64_one():
    rng = np.random.default_rng(0)
    n_steps, decay = 50, 0.999
    p = R.kernel_values(rng, 4096)
    s32, s64 = np.zeros_like(p), np.zeros(p.shape, np.float64)
    bound = 0.0
    for k in range(n_steps):
        s32, s64 = R.update(s32, p, k, decay), R.update64(s64, p, k, decay)
        bound = max(bound, float(np.abs(p).max()))
        p = (p + R.kernel_values(rng, p.size) * np.float32(0.01)).astype(np.float32)
    # three roundings per step (the difference, the product, the result), carried on with a contraction < 1
    err = float(np.abs(s32.astype(np.float64) - s64).max())
    print('float32 vs float64 after %d steps: %.3e (bound %.3e)' % (n_steps, err, 4 * n_steps * 2.0 ** -24 * bound))
    assert err <= 4 * n_steps * 2.0 ** -24 * bound


def test_constant_parameter_is_the_fixed_point():
    p = R.kernel_values(np.random.default_rng(1), 1000)
    s = R.kernel_values(np.random.default_rng(2), 1000)
    s64 = s.astype(np.float64)
    for k in range(1, 400):
        s, s64 = R.update(s, p, k, 0.9), R.update64(s64, p, k, 0.9)
    assert np.abs(s64 - p).max() <= 1e-12 * np.abs(p).max()
    assert np.abs(s.astype(np.float64) - p).max() <= 8 * 2.0 ** -24 * np.abs(p).max()
    assert np.array_equal(R.update(p, p, 7, 0.9), p)           # and the shadow that equals p stays there exactly


def test_warm_up_coefficient_and_its_crossover():
    decay = np.float32(0.999)
    for k in (1, 2, 8, 100, 8989):
        d, omd = R.coefficient(k, decay)
        assert d == (1.0 + k) / (10.0 + k) and d < np.float64(decay) and omd == np.float32(1.0 - d)
    for k in (8991, 10 ** 4, 10 ** 7):
        d, omd = R.coefficient(k, decay)
        assert d == np.float64(decay) and omd == np.float32(1.0 - np.float64(decay))
    # the real-valued crossover of 0.999 is k = 8990: (1 + k) / (10 + k) = 8991 / 9000 = 0.999
    assert abs((1.0 + 8990) / (10.0 + 8990) - 0.999) < 1e-15
    assert R.coefficient(1, 0.5)[0] == 2.0 / 11.0 and R.coefficient(10, 0.5)[0] == 0.5


def test_a_counter_of_zero_copies():
    p = R.kernel_values(np.random.default_rng(3), 64)
    junk = np.full(64, np.nan, np.float32)
    assert np.array_equal(R.update(junk, p, 0, 0.999), p) and np.array_equal(R.update64(junk, p, 0, 0.999), p.astype(np.float64))
    shadow, sub, k = R.fold([p, p], 0.999)
    assert np.array_equal(shadow, p) and not sub.any() and k == 2


def test_kernel_case_values_never_meet_a_subnormal():
    """The inputs of the kernel cases of tests/test_gpu_ema.py (same generator, same sizes, same counters): `update` asserts."""
    for n in (1, 3, 4, 5, 255, 257, 4097, 1048579):
        for start in (0, 1, 2, 8, 8989, 8991, 10 ** 7):
            rng = np.random.default_rng(n + start)
            s = R.kernel_values(rng, n)
            params = [R.kernel_values(rng, n) for _ in range(4)]
            assert np.abs(s).min() >= 2.0 ** -10 and np.abs(s).max() <= 2.0 ** 7
            for j in range(4):
                s = R.update(s, params[j], start + j, 0.999)


def test_subnormal_intermediates_are_reported():
    s, p = np.array([1e-39, 1.0], np.float32), np.array([0.0, 0.5], np.float32)
    _, sub = R.update(s, p, 5, 0.999, return_subnormal=True)
    assert sub.tolist() == [True, False]
    with pytest.raises(AssertionError):
        R.update(s, p, 5, 0.999)


# ---- the graph, on the C oracle -------------------------------------------------------------------------------------------
def test_ema_off_builds_the_graph_and_the_checkpoint_it_always_built():
    _, _, a = _ops()
    keys_a = sorted(Saver()._tensors())
    state_a = len(G.get_default_graph().state)
    _, tr, b = _ops(ema_decay=0)
    assert a == b and sorted(Saver()._tensors()) == keys_a and len(G.get_default_graph().state) == state_a
    assert tr.ema is None and tr.g_opt_op.ema is None
    _, _, c = _ops(ema_decay=0.0, rollout_steps=2, lookahead=False)
    _, _, d = _ops(rollout_steps=2, lookahead=False)
    assert c == d


def test_ema_on_adds_state_and_nothing_else():
    _, tr0, ops0 = _ops()
    g0 = G.get_default_graph()
    keys0, vars0 = sorted(Saver()._tensors()), list(g0.variables)
    inputs0 = [[t.name for t in op.inputs] for op in (tr0.g_opt_op, tr0.g_pretrain_opt_op, tr0.d_opt_op)]
    _, tr, ops1 = _ops(ema_decay=0.999)
    g1 = G.get_default_graph()
    assert ops1 == ops0                                    # every op - the D step's among them - where it was, as it was
    assert list(g1.variables) == vars0
    assert [[t.name for t in op.inputs] for op in (tr.g_opt_op, tr.g_pretrain_opt_op, tr.d_opt_op)] == inputs0
    keys1 = sorted(Saver()._tensors())
    assert sorted(set(keys1) - set(keys0)) == ['state:g/ema/num_updates', 'state:g/ema/shadow'] and set(keys0) < set(keys1)
    shadow, count = Saver()._tensors()['state:g/ema/shadow'], Saver()._tensors()['state:g/ema/num_updates']
    total = g1.layout('g')[1]
    assert shadow.shape == (total,) and shadow.dtype == torch.float32
    assert count.shape == (1,) and count.dtype == torch.int64 and count.init == 0
    assert len(g1.state) == len(g0.state) + 3              # + the unnamed retired-block word, which no checkpoint holds
    assert tr.d_opt_op.ema is None and tr.ema.decay == float(np.float32(0.999))
    # neither a variable nor part of a flat buffer nor an optimizer slot
    assert shadow.view_of is None and not any(shadow is t for op in (tr.g_opt_op, tr.g_pretrain_opt_op) for t in op.inputs)


def test_all_g_steps_share_one_average():
    _, tr, _ = _ops(ema_decay=0.99, rollout_steps=2, lookahead=False)
    steps = [tr.g_opt_op, tr.g_pretrain_opt_op, tr.g_rollout_opt_op, tr.g_rollout_pretrain_opt_op]
    assert all(op.ema is tr.ema for op in steps)
    assert all(op.extras[-3] is tr.ema.shadow and op.extras[-2] is tr.ema.num_updates for op in steps)
    names = [s.name for s in G.get_default_graph().state]
    assert names.count('g/ema/shadow') == 1 and names.count('g/ema/num_updates') == 1


@pytest.mark.parametrize('decay', [1, 1.0, -0.1, 1.5, float('nan'), 'x', True, 1 - 1e-12], ids=repr)
def test_invalid_decays_raise_before_anything_is_created(decay):
    from oracle import cbind
    G.reset_default_graph()
    sess = G.Session(device='cpu', lib=cbind.load())
    with pytest.raises(ValueError, match='ema_decay'):
        T.Trainer(sess, True, 'bce', 'adam', True, batch_size=2, ema_decay=decay)
    g = G.get_default_graph()
    assert not g.ops and not g.variables and not g.state
    with pytest.raises(ValueError, match='ema_decay'):
        T.train('synthetic', None, None, None, None, True, 'bce', 'adam', True, ema_decay=decay, device='cpu')


def test_minimize_rejects_an_average_of_another_scope():
    _, tr, _ = _ops()
    with pytest.raises(ValueError, match='scope'):
        optim.AdamOptimizer(1e-3, name='x').minimize(tr.d_loss, var_list=tr.d_vars, ema=optim.WeightAverage(0.9, 'g'))
    with pytest.raises(ValueError, match='decay'):
        optim.WeightAverage(1.0, 'g')


def test_methods_without_an_average_and_at_count_zero():
    x, y, a, s = _inputs()
    sess, tr, _ = _ops()
    sess.run(G.global_variables_initializer())
    for call in (tr.ema_updates, tr.ema_statistics, tr.reset_ema, lambda: tr.ema_weights().__enter__(), lambda: tr.test(x, y, a, weights='ema')):
        with pytest.raises(RuntimeError, match='ema_decay'):
            call()
    with pytest.raises(ValueError, match="'raw' or 'ema'"):
        tr.test(x, y, a, weights='average')
    sess, tr, _ = _ops(ema_decay=0.999)
    sess.run(G.global_variables_initializer())
    assert tr.ema_updates() == 0
    stats = tr.ema_statistics()
    assert sorted(stats) == sorted(v.name for v in tr.g_vars) and all(stats[v.name].shape == v.shape for v in tr.g_vars)
    with pytest.raises(RuntimeError, match='0 updates'):
        with tr.ema_weights():
            pass
    with pytest.raises(RuntimeError, match='0 updates'):
        tr.test(x, y, a, weights='ema')
    sess._materialize(tr.ema.num_updates).fill_(3)
    assert tr.ema_updates() == 3
    tr.reset_ema()
    assert tr.ema_updates() == 0


def test_the_c_oracle_raises_a_clear_error():
    x, y, a, s = _inputs()
    sess, tr, _ = _ops(ema_decay=0.999)
    sess.run(G.global_variables_initializer())
    tr.train_d(x, y, a)                                     # the D step carries no average: it runs
    with pytest.raises(RuntimeError, match='acg_(ema_update|adam_step_ema|rmsprop_step_ema)'):
        tr.train_g(x, y, a, s)
    with pytest.raises(RuntimeError, match='acg_(ema_update|adam_step_ema|rmsprop_step_ema)'):
        tr.pretrain_g(x, y, a, s)
    sess._materialize(tr.ema.num_updates).fill_(1)
    with pytest.raises(RuntimeError, match='acg_swap_f32'):
        with tr.ema_weights():
            pass


def test_checkpoints_cross_between_graphs_with_and_without_the_average(tmp_path):
    sess, tr, _ = _ops(ema_decay=0.999)
    sess.run(G.global_variables_initializer())
    g = torch.Generator().manual_seed(0)
    sess._materialize(tr.ema.shadow).copy_(torch.randn(tr.ema.shadow.shape, generator=g))
    sess._materialize(tr.ema.num_updates).fill_(12345678901)
    want = tr.ema_statistics()
    path = Saver().save(sess, str(tmp_path / 'with_ema'))
    saved = np.load(path)
    assert saved['state:g/ema/num_updates'].dtype == np.int64 and saved['state:g/ema/shadow'].dtype == np.float32
    assert not any(k == 'state:None' or k.endswith('/done') for k in saved.files)
    sess, tr, _ = _ops(ema_decay=0.5)
    sess.run(G.global_variables_initializer())
    Saver().restore(sess, str(tmp_path / 'with_ema'))
    got = tr.ema_statistics()
    assert tr.ema_updates() == 12345678901 and all(np.array_equal(got[k], want[k]) for k in want)
    # a plain graph restores it and writes the checkpoint it always wrote
    sess, tr, _ = _ops()
    sess.run(G.global_variables_initializer())
    Saver().restore(sess, str(tmp_path / 'with_ema'))
    old = Saver().save(sess, str(tmp_path / 'old'))
    assert not any('/ema/' in k for k in np.load(old).files)
    # a graph with the average restores that: the count stays 0, the first update will seed the shadow
    sess, tr, _ = _ops(ema_decay=0.999)
    sess.run(G.global_variables_initializer())
    Saver().restore(sess, str(tmp_path / 'old'))
    assert tr.ema_updates() == 0


def test_float32_trajectory_stays_inside_the_subnormal_cap():
    """The steps of test_gpu_ema's trajectory test (batch 2, 64 x 64, DNA, bce / Adam, five G updates) on the C oracle in float32:
    at most 0.01 % of the elements may meet a subnormal intermediate in the restatement (they are compared to 2^-126 there)."""
    x, y, a, s = _inputs()
    sess, tr, _ = _ops(lookahead=False)
    sess.run(G.global_variables_initializer())
    flat = G.get_default_graph().layout('g')[2]
    trajectory = []
    for _ in range(5):
        tr.train_g(x, y, a, s)
        trajectory.append(sess._materialize(flat).detach().cpu().numpy().copy())
    _, sub, k = R.fold(trajectory, 0.999)
    share = float(sub.mean())
    print('elements with a subnormal intermediate: %d of %d (%.5f %%)' % (int(sub.sum()), sub.size, 100 * share))
    assert k == 5 and share <= 1e-4


# ---- the CLIs ----------------------------------------------------------------------------------------------------------------
def test_cli_passes_g_ema_on(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(T, 'train', lambda *a, **kw: seen.update(kw))
    T.main(['synthetic', str(tmp_path / 'out'), '--dna', '--g_ema', '0.99'])
    assert seen['ema_decay'] == 0.99
    T.main(['synthetic', str(tmp_path / 'out2')])
    assert seen['ema_decay'] == 0.0


@pytest.mark.parametrize('value', ['1', '-0.1', '1.5', 'nan'])
def test_cli_rejects_a_decay_outside_the_unit_interval(tmp_path, monkeypatch, value):
    monkeypatch.setattr(T, 'train', lambda *a, **kw: pytest.fail('train() reached'))
    with pytest.raises(SystemExit):
        T.main(['synthetic', str(tmp_path / 'out'), '--g_ema', value])
    assert not (tmp_path / 'out').exists()


def test_evaluate_cli_passes_weights_on(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: seen.update(kw))
    E.main([str(tmp_path / 'm'), 'synthetic', str(tmp_path / 'o'), '--num_sequences', '4', '--weights', 'ema'])
    assert seen['weights'] == 'ema'
    seen.clear()
    E.main([str(tmp_path / 'm'), 'synthetic', str(tmp_path / 'o'), '--num_sequences', '4'])
    assert seen.get('weights', 'raw') == 'raw'


def test_evaluate_cli_rejects_unknown_weights(tmp_path, monkeypatch):
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: pytest.fail('evaluate() reached'))
    with pytest.raises(SystemExit):
        E.main([str(tmp_path / 'm'), 'synthetic', str(tmp_path / 'o'), '--num_sequences', '4', '--weights', 'bogus'])
    assert not (tmp_path / 'o').exists()


def test_evaluate_rejects_unknown_weights_before_anything_is_created(tmp_path):
    with pytest.raises(ValueError, match='weights'):
        E.evaluate(str(tmp_path / 'm'), 'synthetic', str(tmp_path / 'o'), num_sequences=2, weights='bogus')
    assert not (tmp_path / 'o').exists()
