"""The generator's noise input without a GPU: known answers of Philox4x32-10, the restatement's normals and their statistics,
the CLI flags and their rejections, the Trainer's own rejections, the graph at noise_dim = 0, the variable shapes at
noise_dim = 4, best-of-N scoring and the clear error on the C oracle."""
import math

import numpy as np
import pytest
import torch

import noise_ref as R
from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import ops as O
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T


def _words(text):
    return np.array([int(w, 16) for w in text.split()], np.uint32)


@pytest.mark.parametrize('ctr,key,out', [
    ('0 0 0 0', '0 0', '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ('ffffffff ffffffff ffffffff ffffffff', 'ffffffff ffffffff', '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ('243f6a88 85a308d3 13198a2e 03707344', 'a4093822 299f31d0', 'd16cfe09 94fdcceb 5001e420 24126ea1')])
def test_philox_known_answers(ctr, key, out):
    assert np.array_equal(R.philox4x32_10(_words(ctr), _words(key)), _words(out))


@pytest.mark.parametrize('seed,counter,stream,want', [
    (7, 0, 0, (2.914691440e-04, -3.048468178e-01, 1.788756994, 1.067872705)),
    (7, 1, 0, (0.376403945, -1.287011548, 1.811504039, -0.491240689)),
    (7, 0, 1, (-0.558482932, 0.201105477, 0.845537748, 1.492511178))])
def test_normals_of_the_restatement(seed, counter, stream, want):
    """(the values are given to 10 significant digits: rel 1e-8 leaves 5e-10 for their own rounding)"""
    np.testing.assert_allclose(R.normals(seed, counter, stream, 4), want, rtol=1e-8, atol=0)


def test_a_prefix_of_a_draw_is_the_draw_and_the_tail_is_dropped():
    z = R.normals(7, 3, 1, 23)
    assert z.shape == (23,) and np.array_equal(z, R.normals(7, 3, 1, 64)[:23])


N_STAT = 65536


@pytest.fixture(scope='module')
def draws():
    """{(seed, counter, stream): 65 536 normals}, computed once."""
    return {(s, c, st): R.normals(s, c, st, N_STAT) for s in (0, 7, 0x123456789abcdef) for c in (0, 1, 2 ** 32 + 5) for st in (0, 3)}


def _ks(z):
    zs = np.sort(z)
    cdf = 0.5 * (1.0 + np.array([math.erf(v) for v in zs / math.sqrt(2.0)]))
    n = zs.size
    return max(np.max(np.arange(1, n + 1) / n - cdf), np.max(cdf - np.arange(n) / n))


def test_statistics_of_65536_draws(draws):
    """5 standard errors of the mean (5 / 256 = 0.0195 -> 0.02) and of the variance (5 * sqrt(2 / n) = 0.0276 -> 0.03); the
    Kolmogorov-Smirnov alpha = 0.001 critical value 1.95 / sqrt(n) = 0.0076."""
    assert len(draws) == 18
    for key, z in draws.items():
        assert np.abs(z).max() <= 5.77, key
        assert abs(z.mean()) <= 0.02, (key, z.mean())
        assert abs(z.var() - 1.0) <= 0.03, (key, z.var())
        assert _ks(z) <= 0.0076, (key, _ks(z))


def test_counters_and_streams_are_independent(draws):
    a = draws[(7, 0, 0)]
    assert abs(np.corrcoef(a, draws[(7, 1, 0)])[0, 1]) < 0.02
    assert abs(np.corrcoef(a, R.normals(7, 0, 1, N_STAT))[0, 1]) < 0.02


def test_noise_concat_restatement_layout():
    a = np.arange(30, dtype=np.float32).reshape(3, 10)
    out = R.noise_concat(a, 5, 7, 2, stream_id=1, scale=0.5)
    assert out.shape == (3, 15) and np.array_equal(out[:, :10], a)
    assert np.array_equal(out[:, 10:].reshape(-1), 0.5 * R.normals(7, 2, 1, 15))
    assert np.array_equal(R.noise_concat(a, 5, 7, 2, scale=0.0)[:, 10:], np.zeros((3, 5)))


# ---- CLI
def test_train_cli_passes_the_noise_flags_on(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(T, 'train', lambda *a, **kw: seen.update(kw))
    T.main(['synthetic', str(tmp_path / 'out'), '--dna', '--noise_dim', '8', '--noise_seed', '12345678901234567890'])
    assert seen['noise_dim'] == 8 and seen['noise_seed'] == 12345678901234567890
    T.main(['synthetic', str(tmp_path / 'out2')])
    assert seen['noise_dim'] == 0 and seen['noise_seed'] == 0


@pytest.mark.parametrize('extra', [['--noise_dim', '-1'], ['--noise_dim', '65'], ['--noise_dim', '4', '--noise_seed', '-1'],
                                   ['--noise_dim', '4', '--noise_seed', str(2 ** 64)], ['--dna', '--noise_dim', '4', '--rollout_steps', '2'],
                                   ['--noise_dim', '64', '--batch_size', '256']], ids=str)
def test_train_cli_rejections_create_nothing(tmp_path, monkeypatch, extra):
    monkeypatch.setattr(T, 'train', lambda *a, **kw: pytest.fail('train() reached'))
    with pytest.raises(SystemExit):
        T.main(['synthetic', str(tmp_path / 'out')] + extra)
    assert not (tmp_path / 'out').exists()


def test_train_rejects_before_anything_is_created():
    G.reset_default_graph()
    g = G.get_default_graph()
    for kw in (dict(noise_dim=65), dict(noise_dim=4, rollout_steps=2), dict(noise_dim=4, noise_seed=-1)):
        with pytest.raises(ValueError):
            T.train('synthetic', None, None, None, None, True, 'bce', 'adam', True, batch_size=2, train_iter=1, **kw)
    assert G.get_default_graph() is g and not g.ops


def test_evaluate_cli_passes_the_noise_flags_on(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: seen.update(kw))
    base = [str(tmp_path / 'm'), 'synthetic', str(tmp_path / 'o'), '--num_sequences', '4']
    E.main(base)
    assert not any(k.startswith('noise') for k in seen)            # without the flag: the call it always made
    E.main(base + ['--noise_dim', '4'])
    assert (seen['noise_dim'], seen['noise'], seen['noise_samples'], seen['noise_seed']) == (4, 'zero', 1, 0)
    E.main(base + ['--noise_dim', '4', '--noise', 'sample', '--noise_samples', '3', '--noise_seed', '9'])
    assert (seen['noise_dim'], seen['noise'], seen['noise_samples'], seen['noise_seed']) == (4, 'sample', 3, 9)


@pytest.mark.parametrize('extra', [['--noise_dim', '65'], ['--noise', 'sample'], ['--noise_dim', '4', '--noise_samples', '3'],
                                   ['--noise_dim', '4', '--noise', 'sample', '--noise_samples', '0'],
                                   ['--noise_dim', '4', '--bn_stats', 'stored'], ['--noise_dim', '4', '--bn_stats', 'calibrate'],
                                   ['--noise_dim', '4', '--noise', 'gauss']], ids=str)
def test_evaluate_cli_rejections_create_nothing(tmp_path, monkeypatch, extra):
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: pytest.fail('evaluate() reached'))
    with pytest.raises(SystemExit):
        E.main([str(tmp_path / 'm'), 'synthetic', str(tmp_path / 'o'), '--num_sequences', '4'] + extra)
    assert not (tmp_path / 'o').exists()


@pytest.mark.parametrize('kw', [dict(noise_dim=4, bn_stats='stored'), dict(noise_dim=0, noise='sample'), dict(noise_dim=4, noise='gauss'),
                                dict(noise_dim=4, noise='zero', noise_samples=2), dict(noise_dim=65)], ids=str)
def test_evaluate_rejects_before_anything_is_created(tmp_path, kw):
    with pytest.raises(ValueError):
        E.evaluate(str(tmp_path / 'm'), 'synthetic', str(tmp_path / 'o'), num_sequences=4, **kw)
    assert not (tmp_path / 'o').exists()


def test_train_record_holds_noise_dim_only_when_it_is_on():
    assert 'noise_dim' not in T.train_record({'g_loss': 1.0}, 0, 0.0, 1)
    assert T.train_record({'g_loss': 1.0}, 0, 0.0, 1, noise_dim=8)['noise_dim'] == 8


def test_best_of_n_picks_per_sequence_and_per_metric():
    """Two draws, two sequences, two steps; count_per_frame = 1, so a frame's PSNR is -10 log10(sqerr)."""
    ssim = np.array([[[0.9, 0.1], [0.2, 0.2]],          # draw 0: sequence 0 mean 0.5, sequence 1 mean 0.2
                     [[0.4, 0.4], [0.3, 0.5]]])         # draw 1:            0.4              0.4
    sqerr = np.array([[[1.0, 1.0], [0.1, 0.1]],
                      [[0.1, 0.1], [1.0, 1.0]]])
    out = E.best_of_n(ssim, sqerr, 1)
    np.testing.assert_allclose(out['best_ssim'], [(0.9 + 0.3) / 2, (0.1 + 0.5) / 2])
    np.testing.assert_allclose(out['best_psnr'], [10.0, 10.0])                      # sequence 0 from draw 1, sequence 1 from draw 0
    np.testing.assert_allclose(out['ssim'], ssim.mean(axis=(0, 1)))
    np.testing.assert_allclose(out['psnr'], [-10 * math.log10(0.55)] * 2)           # each draw: MSE (1 + 0.1) / 2


# ---- Trainer
def _trainer(transform=True, **kw):
    from oracle import cbind
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cpu', lib=cbind.load())
    tr = T.Trainer(sess, True, 'bce', 'adam', transform, batch_size=2, **kw)
    g = G.get_default_graph()
    return sess, tr, g


def _describe(g):
    return ([(type(o).__name__, o.name, o.index, [t.shape for t in o.outputs]) for o in g.ops],
            [(n, v.shape) for n, v in g.variables.items()], [(s.name, s.shape, s.dtype) for s in g.state])


@pytest.mark.parametrize('kw', [dict(noise_dim=-1), dict(noise_dim=65), dict(noise_dim=2.5), dict(noise_dim=True),
                                dict(noise_dim=4, rollout_steps=2), dict(noise_dim=4, bn_inference=True), dict(noise_dim=4, noise_seed=-1),
                                dict(noise_dim=4, noise_seed=2 ** 64), dict(noise_dim=64, batch_size=256)], ids=str)
def test_trainer_rejections_leave_the_graph_alone(kw):
    G.reset_default_graph()
    optim.set_data_parallel(1)
    g = G.get_default_graph()
    kw = dict(dict(batch_size=2), **kw)
    with pytest.raises(ValueError):
        T.Trainer(None, True, 'bce', 'adam', True, **kw)
    assert len(g.ops) == 0 and not g.variables and not g.state and not g.collections.get('noise')


@pytest.mark.parametrize('transform', [False, True, 'cdna'], ids=str)
def test_noise_dim_0_builds_the_graph_it_always_built(transform):
    a = _describe(_trainer(transform)[2])
    b = _describe(_trainer(transform, noise_dim=0, noise_seed=5)[2])
    assert a == b
    assert not any(isinstance(o, O.NoiseOp) for o in G.get_default_graph().ops) and 'noise' not in G.get_default_graph().collections


@pytest.mark.parametrize('transform,wider', [(False, {'g/tconv1/weights': 2}), (True, {'g/tconv1/weights': 2}),
                                             ('cdna', {'g/tconv1/weights': 2, 'g/cdna_params/weights': 2})], ids=str)
def test_noise_dim_4_widens_the_bottleneck_layers_only(transform, wider):
    """The layers that read the concatenated bottleneck get 4 more input channels (slim stores them on axis 2 of a conv filter
    and on axis 3 of a transposed one: exactly one axis grows, by 4); every other variable, all of d/ included, keeps its shape."""
    base = {n: v.shape for n, v in _trainer(transform)[2].variables.items()}
    _, tr, g = _trainer(transform, noise_dim=4, noise_seed=11)
    got = {n: v.shape for n, v in g.variables.items()}
    assert list(got) == list(base)
    changed = {n for n in got if got[n] != base[n]}
    assert changed == set(wider)
    for n in changed:
        diff = [x - y for x, y in zip(got[n], base[n])]
        assert sorted(diff) == [0, 0, 0, 4], (n, got[n], base[n])
    assert all(got[n] == base[n] for n in got if n.startswith('d/'))
    # one NoiseOp, one named state (a checkpoint key), one unnamed scale; no look-ahead pair pass
    assert sum(isinstance(o, O.NoiseOp) for o in g.ops) == 1 and not tr.lookahead
    state, scale = O.noise_state()
    assert (state.name, state.shape, state.dtype, state.init) == ('g/noise/state', (2,), torch.int64, (11, 0))
    assert scale.name is None and scale.init == 1.0
    from action_conditioned_gans_amd.saver import Saver
    keys = set(Saver()._tensors())
    assert 'state:g/noise/state' in keys and sum('noise' in k for k in keys) == 1


def test_seeds_above_2_63_keep_their_bits():
    _, _, g = _trainer(noise_dim=4, noise_seed=2 ** 64 - 2)
    assert O.noise_state()[0].init == (-2, 0)


def test_noise_sample_needs_noise_dim():
    sess, tr, _ = _trainer()
    x = np.zeros((2, 64, 64, 3), np.float32)
    with pytest.raises(RuntimeError, match='noise_dim'):
        tr.test(x, x, np.zeros((2, 10), np.float32), noise='sample')
    with pytest.raises(ValueError, match='noise'):
        tr.test(x, x, np.zeros((2, 10), np.float32), noise='gauss')
    with pytest.raises(RuntimeError, match='noise_dim'):
        tr.last_noise()


def test_append_noise_rejections():
    G.reset_default_graph()
    a = G.placeholder((2, 10), name='a')
    for z in (0, 65):
        with pytest.raises(ValueError):
            O.append_noise(a, z)
    with pytest.raises(ValueError):
        O.append_noise(G.placeholder((256, 10), name='b'), 64)
    with pytest.raises(ValueError):
        O.append_noise(G.placeholder((2, 4, 4, 10), name='c'), 4)
    assert not G.get_default_graph().ops


def test_the_c_oracle_raises_a_clear_error():
    sess, tr, _ = _trainer(noise_dim=4)
    sess.run(G.global_variables_initializer())
    x = np.zeros((2, 64, 64, 3), np.float32)
    with pytest.raises(RuntimeError, match='acg_noise_concat'):
        tr.test(x, x, np.zeros((2, 10), np.float32))


def test_the_gradient_is_the_action_columns_of_the_output_gradient():
    """No gradient to z (it is no input); the action columns' is their slice of d(out) - one SliceOp over columns [0, A)."""
    G.reset_default_graph()
    a = G.placeholder((3, 10), name='a')
    out = O.append_noise(a, 5)
    op = out.op
    assert op.inputs == [a] and out.shape == (3, 15)
    gout = G.placeholder((3, 15), name='gout')
    assert op.grad([gout], [False], None) == [None]
    (ga,) = op.grad([gout], [True], None)
    assert isinstance(ga.op, O.SliceOp) and ga.op.inputs == [gout] and (ga.op.c_off, ga.op.c_dst, ga.shape) == (0, 10, (3, 10))
