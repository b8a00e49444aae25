"""Training through K-step rollouts without a GPU: the CLI flag and its rejections, the window draws against select_pairs,
the frames announced to the dataset, the graph at K = 1, the Trainer's own rejections and the clear error on the C oracle."""
import numpy as np
import pytest
import torch

import rollout_train_ref as R
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T
from action_conditioned_gans_amd.util import build_all_mask


def test_cli_passes_rollout_steps_on(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(T, 'train', lambda *a, **kw: seen.update(kw))
    T.main(['synthetic', str(tmp_path / 'out'), '--dna', '--rollout_steps', '3'])
    assert seen['rollout_steps'] == 3
    T.main(['synthetic', str(tmp_path / 'out2')])
    assert seen['rollout_steps'] == 1


@pytest.mark.parametrize('extra,env', [(['--rollout_steps', '0'], {}), (['--rollout_steps', '8'], {}),
                                       (['--rollout_steps', '3', '--seq_len', '3'], {}), (['--cdna', '--rollout_steps', '2'], {}),
                                       (['--dna', '--dtype', 'bf16', '--rollout_steps', '2'], {}),
                                       (['--dna', '--rollout_steps', '2'], {'WORLD_SIZE': '2'}),
                                       (['--dna', '--sync_bn', '--rollout_steps', '2'], {}),
                                       (['--dna', '--exact_global_batch', '--rollout_steps', '2'], {})], ids=str)
def test_cli_rejections_create_nothing(tmp_path, monkeypatch, extra, env):
    monkeypatch.setattr(T, 'train', lambda *a, **kw: pytest.fail('train() reached'))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(SystemExit):
        T.main(['synthetic', str(tmp_path / 'out')] + extra)
    assert not (tmp_path / 'out').exists()


def test_k1_windows_are_select_pairs_bit_for_bit():
    mask = build_all_mask(8)
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    for _ in range(20):
        want = T.select_pairs(a.randint, mask, 16)
        got = T.select_windows(b.randint, mask, 16, 1)
        assert len(got) == 2 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert a.randint(1 << 30) == b.randint(1 << 30)          # the same number of draws from the stream


@pytest.mark.parametrize('K', [2, 3, 7])
def test_windows_stay_in_range(K):
    T_ = 8
    mask = build_all_mask(T_)
    rng = np.random.RandomState(1)
    for _ in range(50):
        m = T.select_windows(rng.randint, mask, 32, K)
        assert len(m) == K + 1
        start = m[0].argmax(axis=1)
        assert (start >= 0).all() and (start + K <= T_ - 1).all()
        for i in range(K + 1):
            assert (m[i].sum(axis=1) == 1).all() and np.array_equal(m[i].argmax(axis=1), start + i)


def test_window_batch_shapes_and_order():
    B, T_, K = 4, 8, 3
    rng = np.random.RandomState(2)
    img = rng.rand(B, T_, 2, 2, 3).astype(np.float32)
    acts = rng.rand(B, T_, 10).astype(np.float32)
    m = T.select_windows(rng.randint, build_all_mask(T_), B, K)
    frames, actions, states = T.window_batch(m, img, img, acts, acts[:, :, 5:].copy())
    t = m[0].argmax(axis=1)
    assert frames.shape == (B, K + 1, 2, 2, 3) and actions.shape == (B, K, 10) and states.shape == (B, K, 5)
    for n in range(B):
        assert np.array_equal(frames[n], img[n, t[n]:t[n] + K + 1])
        assert np.array_equal(actions[n], acts[n, t[n]:t[n] + K])
        assert np.array_equal(states[n], acts[n, t[n] + 1:t[n] + K + 1, 5:])


@pytest.mark.parametrize('K', [1, 3])
def test_selections_announce_the_window_frames(K):
    seen = []

    class Src:
        def announce(self, need):
            seen.append(np.array(need))
    mask = build_all_mask(8)
    np.random.seed(3)
    sel = T._PairSelections(mask, 6, 2, 1, 4, Src(), rollout_steps=K)
    plan = [sel.next() for _ in range(4)]
    assert len(seen) == 1 + 3 * 2
    pre = plan[0][0]
    assert np.array_equal(seen[0], np.logical_or.reduce(pre))
    for it in range(1, 4):
        d1, d2, g = plan[it]
        assert len(g) == K + 1
        assert np.array_equal(seen[1 + 2 * (it - 1)], d1[0] | d1[1])
        assert np.array_equal(seen[2 + 2 * (it - 1)], d2[0] | d2[1] | np.logical_or.reduce(g))


def test_k1_selections_equal_the_one_step_loop():
    mask = build_all_mask(8)
    np.random.seed(4)
    a = T._PairSelections(mask, 6, 3, 2, 6, None)
    b = T._PairSelections(mask, 6, 3, 2, 6, None, rollout_steps=1)
    for _ in range(6):
        for x, y in zip(a.next(), b.next()):
            assert all(np.array_equal(u, v) for u, v in zip(x, y))


def _ops(**kw):
    from oracle import cbind
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cpu', lib=cbind.load())
    tr = T.Trainer(sess, True, 'bce', 'adam', True, batch_size=2, **kw)
    return sess, tr, [(type(o).__name__, o.name, o.index, [t.shape for t in o.outputs]) for o in G.get_default_graph().ops]


def test_trainer_k1_builds_the_one_step_graph():
    _, _, a = _ops()
    _, _, b = _ops(rollout_steps=1)
    assert a == b
    _, tr, c = _ops(rollout_steps=2)
    assert c[:len(a)] == a and len(c) > len(a)


def test_rollout_shares_variables_and_optimizer_state():
    sess, tr, _ = _ops(rollout_steps=3)
    g = G.get_default_graph()
    G.reset_default_graph()
    optim.set_data_parallel(1)
    T.Trainer(G.Session(device='cpu', lib=__import__('oracle.cbind', fromlist=['load']).load()), True, 'bce', 'adam', True, batch_size=2)
    g1 = G.get_default_graph()
    assert list(g.variables) == list(g1.variables)
    names = lambda gr: sorted(s.name for s in gr.state if not s.name.endswith('/flat_grad'))      # noqa: E731
    assert names(g) == names(g1)                         # no optimizer slots of its own: checkpoints are unchanged
    assert tr.g_rollout_opt_op.inputs[2:] == tr.g_opt_op.inputs[2:]
    assert tr.g_rollout_pretrain_opt_op.inputs[2:] == tr.g_pretrain_opt_op.inputs[2:]


@pytest.mark.parametrize('kw,dtype,dp', [(dict(rollout_steps=0), 'f32', False), (dict(rollout_steps=2, arg_transform='cdna'), 'f32', False),
                                        (dict(rollout_steps=2), 'bf16', False), (dict(rollout_steps=2), 'f32', True)], ids=str)
def test_trainer_rejections(kw, dtype, dp):
    G.reset_default_graph()
    optim.set_data_parallel(1, force=dp)
    if dtype == 'bf16':
        G.get_default_graph().act_dtype = torch.bfloat16
    n_ops = len(G.get_default_graph().ops)
    transform = kw.pop('arg_transform', True)
    with pytest.raises(ValueError):
        T.Trainer(None, True, 'bce', 'adam', transform, batch_size=2, **kw)
    assert len(G.get_default_graph().ops) == n_ops


def test_the_c_oracle_raises_a_clear_error():
    sess, tr, _ = _ops(rollout_steps=2)
    sess.run(G.global_variables_initializer())
    x = np.zeros((2, 3, 64, 64, 3), np.float32)
    with pytest.raises(RuntimeError, match='acg_(action_grad|dna_bwd_image)'):
        tr.train_g_rollout(x, np.zeros((2, 2, 10), np.float32), np.zeros((2, 2, 5), np.float32))


def test_restatement_k1_is_the_one_step_oracle():
    from oracle import models as OM
    from oracle.trainer import OracleTrainer
    params = {k: v.double() for k, v in OM.init_params(True, batch=2, seed=1, dtype=torch.float32).items()}
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 2, 64, 64, 3, generator=g, dtype=torch.float64) * 2 - 1
    a = torch.randn(2, 1, 10, generator=g, dtype=torch.float64)
    s = torch.randn(2, 1, 5, generator=g, dtype=torch.float64)
    want = OracleTrainer(params, True, 'bce', 'adam', True).train_g(x[:, 0], x[:, 1], a[:, 0], s[:, 0], return_all=True)
    got = R.rollout(params, True, True, 'bce', 5, x, a, s)
    assert torch.allclose(got['g_loss'], want['g_loss'], rtol=1e-12) and torch.equal(got['frames'][0], want['frame'])
