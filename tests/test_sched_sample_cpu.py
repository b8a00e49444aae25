"""Scheduled sampling of the K-step rollout without a GPU: the CLI flags and their rejections, the Trainer's rejections, the graph
with sampling off and on, the clear error on the C oracle, and the restatement's own checks (tests/sched_sample_ref.py)."""
import numpy as np
import pytest
import torch

import rollout_train_ref as RR
import sched_sample_ref as R
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import ops as O
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T


# ---- CLI
def test_cli_passes_the_flags_on(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(T, 'train', lambda *a, **kw: seen.update(kw))
    T.main(['synthetic', str(tmp_path / 'out'), '--dna', '--rollout_steps', '3', '--sched_sampling', 'inverse_sigmoid', '--ss_start', '0.9',
            '--ss_final', '0.1', '--ss_decay_iters', '500', '--ss_seed', '12345678901234567890'])
    assert (seen['sched_sampling'], seen['ss_start'], seen['ss_final'], seen['ss_decay_steps'], seen['ss_seed']) == \
        ('inverse_sigmoid', 0.9, 0.1, 500, 12345678901234567890)
    T.main(['synthetic', str(tmp_path / 'out2')])
    assert (seen['sched_sampling'], seen['ss_start'], seen['ss_final'], seen['ss_decay_steps'], seen['ss_seed']) == ('off', 1.0, 0.0, 0, 0)


@pytest.mark.parametrize('extra', [['--sched_sampling', 'linear', '--ss_decay_iters', '4'],                       # no --rollout_steps
                                   ['--rollout_steps', '1', '--sched_sampling', 'constant'],
                                   ['--rollout_steps', '3', '--sched_sampling', 'cosine'],
                                   ['--rollout_steps', '3', '--sched_sampling', 'linear'],                       # no decay
                                   ['--rollout_steps', '3', '--sched_sampling', 'inverse_sigmoid', '--ss_decay_iters', '-2'],
                                   ['--rollout_steps', '3', '--sched_sampling', 'constant', '--ss_start', '1.5'],
                                   ['--rollout_steps', '3', '--sched_sampling', 'linear', '--ss_decay_iters', '4', '--ss_final', '-0.1'],
                                   ['--rollout_steps', '3', '--sched_sampling', 'constant', '--ss_seed', '-1'],
                                   ['--rollout_steps', '3', '--sched_sampling', 'constant', '--ss_seed', str(2 ** 64)],
                                   ['--rollout_steps', '3', '--ss_start', 'nan']], ids=str)
def test_cli_rejections_create_nothing(tmp_path, monkeypatch, extra):
    monkeypatch.setattr(T, 'train', lambda *a, **kw: pytest.fail('train() reached'))
    with pytest.raises(SystemExit):
        T.main(['synthetic', str(tmp_path / 'out'), '--dna'] + extra)
    assert not (tmp_path / 'out').exists()


def test_train_rejects_before_anything_is_created_and_offsets_by_pretraining(monkeypatch):
    G.reset_default_graph()
    g = G.get_default_graph()
    for kw in (dict(sched_sampling='linear', ss_decay_steps=4), dict(sched_sampling='linear', rollout_steps=3),
               dict(sched_sampling='constant', rollout_steps=3, ss_start=2.0)):
        with pytest.raises(ValueError):
            T.train('synthetic', None, None, None, None, True, 'bce', 'adam', True, batch_size=2, train_iter=1, **kw)
    assert G.get_default_graph() is g and not g.ops
    seen = {}

    class NoSession:                             # train() up to its loop: what the loop is handed is the point
        def __init__(self, **kw):
            self.rt = self

        def check_exchange_flags(self):
            pass

    monkeypatch.setattr(G, 'Session', NoSession)
    monkeypatch.setattr(T, '_train_loop', lambda *a, **kw: seen.update(kw))
    T.train('synthetic', None, None, None, None, True, 'bce', 'adam', True, batch_size=2, train_iter=9, pretrain_iter=7, rollout_steps=3,
            sched_sampling='linear', ss_decay_steps=4, ss_seed=5)
    sampling = lambda: {k: v for k, v in seen['options'].items() if k == 'sched_sampling' or k.startswith('ss_')}     # noqa: E731
    assert sampling() == {'sched_sampling': 'linear', 'ss_start': 1.0, 'ss_final': 0.0, 'ss_decay_steps': 4, 'ss_offset': 7, 'ss_seed': 5}
    T.train('synthetic', None, None, None, None, True, 'bce', 'adam', True, batch_size=2, train_iter=9, rollout_steps=3)
    assert sampling() == {}                      # nothing at all for sampling off


def test_train_record_holds_ss_prob_only_when_sampling_is_on():
    assert 'ss_prob' not in T.train_record({'g_loss': 1.0}, 0, 0.0, 3)
    assert T.train_record({'g_loss': 1.0}, 0, 0.0, 3, ss_prob=0.25)['ss_prob'] == 0.25
    # the positional order is kept
    assert T.train_record({}, 4, 1.5, 3, 0.9, 2.0, None, None, 8)['noise_dim'] == 8


# ---- Trainer
def _trainer(transform=True, **kw):
    from oracle import cbind
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cpu', lib=cbind.load())
    tr = T.Trainer(sess, True, 'bce', 'adam', transform, batch_size=2, **kw)
    return sess, tr, G.get_default_graph()


def _describe(g):
    return ([(type(o).__name__, o.name, o.index, [t.shape for t in o.outputs]) for o in g.ops],
            [(n, v.shape) for n, v in g.variables.items()], [(s.name, s.shape, s.dtype, s.init) for s in g.state])


@pytest.mark.parametrize('kw', [dict(rollout_steps=1, sched_sampling='linear', ss_decay_steps=4), dict(sched_sampling='constant'),
                                dict(rollout_steps=3, sched_sampling='cosine'), dict(rollout_steps=3, sched_sampling=None),
                                dict(rollout_steps=3, sched_sampling='linear'), dict(rollout_steps=3, sched_sampling='linear', ss_decay_steps=2.5),
                                dict(rollout_steps=3, sched_sampling='inverse_sigmoid', ss_decay_steps=-1),
                                dict(rollout_steps=3, sched_sampling='constant', ss_start=1.01),
                                dict(rollout_steps=3, sched_sampling='constant', ss_start=float('nan')),
                                dict(rollout_steps=3, sched_sampling='constant', ss_final=-0.5),
                                dict(rollout_steps=3, sched_sampling='constant', ss_start=True),
                                dict(rollout_steps=3, sched_sampling='constant', ss_offset=-1),
                                dict(rollout_steps=3, sched_sampling='constant', ss_seed=-1),
                                dict(rollout_steps=3, sched_sampling='constant', ss_seed=2 ** 64),
                                dict(rollout_steps=3, sched_sampling='off', ss_start=7.0),
                                dict(rollout_steps=3, sched_sampling='constant', batch_size=4097)], ids=str)
def test_trainer_rejections_leave_the_graph_alone(kw):
    G.reset_default_graph()
    optim.set_data_parallel(1)
    g = G.get_default_graph()
    n_ops = len(g.ops)
    kw = dict(dict(batch_size=2), **kw)
    with pytest.raises(ValueError):
        T.Trainer(None, True, 'bce', 'adam', True, **kw)
    assert len(g.ops) == n_ops == 0 and not g.variables and not g.state and 'sched_sampling' not in g.collections


@pytest.mark.parametrize('transform', [False, True], ids=str)
def test_off_builds_the_graph_it_always_built(transform):
    a = _describe(_trainer(transform, rollout_steps=3)[2])
    b = _describe(_trainer(transform, rollout_steps=3, sched_sampling='off', ss_start=0.5, ss_final=0.25, ss_decay_steps=9, ss_offset=2, ss_seed=5)[2])
    assert a == b
    g = G.get_default_graph()
    assert not any(isinstance(o, (O.SchedSampleDrawOp, O.SchedSampleOp)) for o in g.ops) and 'sched_sampling' not in g.collections


@pytest.mark.parametrize('transform', [False, True], ids=str)
def test_on_adds_one_state_and_no_variable_or_slot(transform):
    base = _describe(_trainer(transform, rollout_steps=3)[2])
    _, tr, g = _trainer(transform, rollout_steps=3, sched_sampling='linear', ss_decay_steps=10, ss_offset=3, ss_seed=2 ** 64 - 2)
    got = _describe(g)
    assert got[1] == base[1]                                                  # the variables
    named = lambda states: [s for s in states if s[0] and not s[0].endswith('/flat_grad')]      # noqa: E731
    new = [s for s in named(got[2]) if s not in named(base[2])]
    assert [s for s in named(got[2]) if s not in new] == named(base[2])       # every slot and counter, in order
    assert new == [('g/sched_sampling/state', (2,), torch.int64, (-2, 0))]    # the seed keeps its bits
    assert tr.g_rollout_opt_op.inputs[2:] == tr.g_opt_op.inputs[2:]
    draws = [o for o in g.ops if isinstance(o, O.SchedSampleDrawOp)]
    mixes = [o for o in g.ops if isinstance(o, O.SchedSampleOp)]
    adjoints = [o for o in g.ops if isinstance(o, O.SchedSampleBwdOp)]
    assert len(draws) == 1 and [t.shape for t in draws[0].outputs] == [(2, 2), (1,)]
    assert draws[0].sched == (1, 3, 10, 1.0, 0.0)
    assert len(mixes) == 2 and all(len(o.outputs) == (2 if transform else 1) for o in mixes)
    assert len(adjoints) == 2 * 2                                             # per fed-back position, in each of the two K-step programs
    from action_conditioned_gans_amd.saver import Saver
    keys = set(Saver()._tensors())
    assert 'state:g/sched_sampling/state' in keys and sum('sched_sampling' in k for k in keys) == 1
    # both K-step programs hold the one draw, the one-step programs none
    for step, want in ((tr.g_rollout_opt_op, 1), (tr.g_rollout_pretrain_opt_op, 1), (tr.g_opt_op, 0), (tr.d_opt_op, 0)):
        seen, stack = set(), [step]
        while stack:
            op = stack.pop()
            if id(op) in seen:
                continue
            seen.add(id(op))
            stack.extend(t.op for t in op.inputs if t.op is not None)
            stack.extend(op.control_inputs)
        assert sum(id(d) in seen for d in draws) == want


def test_accessors_need_sampling():
    _, tr, _ = _trainer(rollout_steps=3)
    for call in (tr.sched_sampling_last, tr.sched_sampling_state, lambda: tr.set_sched_sampling_state(1)):
        with pytest.raises(RuntimeError, match='sched_sampling'):
            call()


def test_state_accessors_on_the_host():
    sess, tr, _ = _trainer(rollout_steps=3, sched_sampling='constant', ss_start=0.5, ss_seed=2 ** 63 + 5)
    sess.run(G.global_variables_initializer())
    assert tr.sched_sampling_state() == (2 ** 63 + 5, 0)
    tr.set_sched_sampling_state(2 ** 64 - 1, 17)
    assert tr.sched_sampling_state() == (2 ** 64 - 1, 17)
    with pytest.raises(ValueError):
        tr.set_sched_sampling_state(-1)
    last = tr.sched_sampling_last()
    assert last['prob'] == 0.0 and last['mask'].shape == (2, 2) and last['mask'].dtype == bool and not last['mask'].any()


def test_the_c_oracle_raises_a_clear_error():
    sess, tr, _ = _trainer(rollout_steps=2, sched_sampling='constant', ss_start=0.5)
    sess.run(G.global_variables_initializer())
    x = np.zeros((2, 3, 64, 64, 3), np.float32)
    with pytest.raises(RuntimeError, match='acg_sched_sample_(draw|fwd|bwd)'):
        tr.train_g_rollout(x, np.zeros((2, 2, 10), np.float32), np.zeros((2, 2, 5), np.float32))


def test_the_adjoint_goes_to_the_predicted_inputs_only():
    G.reset_default_graph()
    mask, _ = O.sched_sample_draw(2, 3, 'constant', 0.5)
    row = mask.view(3, (3,))
    pred, truth = G.placeholder((3, 4, 4, 3), name='pred'), G.placeholder((3, 4, 4, 3), name='truth')
    ps, ts = G.placeholder((3, 5), name='ps'), G.placeholder((3, 5), name='ts')
    frame, state = O.sched_sample(row, pred, truth, ps, ts)
    op = frame.op
    assert op.inputs == [row, pred, truth, ps, ts] and frame.shape == (3, 4, 4, 3) and state.shape == (3, 5)
    gf, gs = G.placeholder((3, 4, 4, 3), name='gf'), G.placeholder((3, 5), name='gs')
    assert op.grad([gf, gs], [False] * 5, None) == [None] * 5
    got = op.grad([gf, gs], [False, True, False, True, False], None)
    assert got[0] is None and got[2] is None and got[4] is None
    assert isinstance(got[1].op, O.SchedSampleBwdOp) and got[1].op is got[3].op and got[1].op.inputs == [row, gf, gs]
    assert got[1].shape == gf.shape and got[3].shape == gs.shape
    only = op.grad([gf, None], [False, True, False, True, False], None)          # no gradient reached the state
    assert only[3] is None and only[1].op.inputs == [row, gf]
    with pytest.raises(ValueError):
        O.sched_sample(mask.view(0, (2,)), pred, truth)
    with pytest.raises(ValueError):
        O.sched_sample(row, pred, G.placeholder((3, 4, 4, 4), name='t4'))
    with pytest.raises(ValueError):
        O.sched_sample_draw(2, 4097, 'constant')
    with pytest.raises(ValueError):
        O.sched_sample_draw(2, 3, 'cosine')


# ---- the restatement
def test_schedules_of_the_restatement():
    assert R.probability('constant', 10 ** 9, 0.25, 0.0, 0, 0) == 0.25
    lin = [R.probability('linear', k, 1.0, 0.0, 4, 2) for k in range(9)]
    assert lin == [1.0, 1.0, 1.0, 0.75, 0.5, 0.25, 0.0, 0.0, 0.0]
    assert R.probability('linear', 3, 0.2, 0.8, 2, 0) == np.float64(np.float32(0.8))          # rising schedules clamp too
    d = 100
    sig = [R.probability('inverse_sigmoid', k, 1.0, 0.0, d, 5) for k in (0, 5, 105, 10 ** 6)]
    assert sig[0] == sig[1] == d / (d + 1.0)                                        # Bengio's eps_0 = k / (k + 1)
    assert abs(sig[2] - d / (d + np.e)) < 1e-15 and sig[3] == 0.0                   # exp overflows to +inf: p = final
    assert all(a >= b for a, b in zip(sig, sig[1:]))
    assert R.probability('inverse_sigmoid', 10 ** 6, 0.9, 0.125, 3, 0) == 0.125


def test_p0_and_p1_give_constant_masks():
    for seed, counter, stream in ((0, 0, 0), (7, 3, 3), (2 ** 64 - 1, 2 ** 32 + 5, 1)):
        assert not R.coins(seed, counter, stream, 7, 64, 0.0).any()
        assert R.coins(seed, counter, stream, 7, 64, 1.0).all()
        u = R.uniforms(seed, counter, stream, 7, 64)
        assert u.min() > 0.0 and u.max() < 1.0 and np.array_equal(u, u.astype(np.float32).astype(np.float64))


def test_coins_are_lanes_of_philox_blocks_apart_from_the_noise_stream():
    import noise_ref as NR
    u = R.uniforms(7, 2, 1, 3, 5)
    ctr = np.array([[2, 0, blk, 1 ^ R.STREAM_TAG] for blk in range(4)], np.uint32)
    x = NR.philox4x32_10(ctr, np.array([7, 0], np.uint32)).reshape(-1)[:15]
    assert np.array_equal(u.reshape(-1), ((x >> 9).astype(np.float64) + 0.5) * 2.0 ** -23)
    assert np.array_equal(R.uniforms(7, 2, 1, 3, 5).reshape(-1)[:8], R.uniforms(7, 2, 1, 2, 4).reshape(-1))      # a prefix of the draw
    noise_words = NR.philox4x32_10(np.array([[2, 0, 0, 1]], np.uint32), np.array([7, 0], np.uint32)).reshape(-1)
    assert not np.array_equal(noise_words, x[:4])
    assert not np.array_equal(u, R.uniforms(7, 3, 1, 3, 5)) and not np.array_equal(u, R.uniforms(7, 2, 0, 3, 5))


def test_the_share_of_truth_coins_at_p03():
    """8192 draws at p = 0.3: sigma = sqrt(0.3 * 0.7 / 8192) = 0.00506, so 0.3 +- 0.03 is 6 sigma."""
    for seed, counter in ((0, 0), (7, 1), (0x123456789abcdef, 2 ** 32 + 5)):
        share = R.coins(seed, counter, 0, 128, 64, np.float32(0.3)).mean()
        assert abs(share - 0.3) <= 0.03, (seed, counter, share)


def test_select_and_adjoint_of_the_restatement():
    pred, truth = np.arange(12, dtype=np.float32).reshape(3, 4), -np.arange(12, dtype=np.float32).reshape(3, 4)
    got = R.select([0.0, 1.0, 0.0], pred, truth)
    assert np.array_equal(got[0], pred[0]) and np.array_equal(got[1], truth[1]) and np.array_equal(got[2], pred[2])
    back = R.select_adjoint([0.0, 1.0, 0.0], pred)
    assert np.array_equal(back[0], pred[0]) and not back[1].any() and np.array_equal(back[2], pred[2])


def _tiny(dna, K=3, B=2):
    from oracle import models as OM
    params = {k: v.double() for k, v in OM.init_params(dna, batch=B, seed=1, dtype=torch.float32).items()}
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, K + 1, 64, 64, 3, generator=g, dtype=torch.float64) * 2 - 1
    a = torch.randn(B, K, 10, generator=g, dtype=torch.float64)
    s = torch.randn(B, K, 5, generator=g, dtype=torch.float64)
    return params, x, a, s


@pytest.mark.parametrize('dna', [True, False], ids=['dna', 'plain'])
def test_masked_restatement_with_no_truth_is_the_rollout_restatement(dna):
    params, x, a, s = _tiny(dna)
    want = RR.rollout(params, dna, True, 'bce', 5, x, a, s)
    got = R.rollout(params, dna, True, 'bce', 5, x, a, s, np.zeros((2, 2), bool))
    assert torch.equal(got['g_loss'], want['g_loss']) and torch.equal(got['l2_loss'], want['l2_loss'])
    for j in range(3):
        assert torch.equal(got['frames'][j], want['frames'][j])
        assert got['states'][j] is None if not dna else torch.equal(got['states'][j], want['states'][j])


def test_masked_restatement_with_all_truth_is_k_teacher_forced_steps():
    params, x, a, s = _tiny(True)
    got = R.rollout(params, True, True, 'bce', 5, x, a, s, np.ones((2, 2), bool))
    for j in range(3):
        act = a[:, j] if j == 0 else torch.cat([a[:, j, :5], s[:, j - 1]], dim=1)
        one = RR.rollout(params, True, True, 'bce', 5, x[:, j:j + 2], act[:, None], s[:, j:j + 1])
        assert torch.equal(got['frames'][j], one['frames'][0]) and torch.equal(got['step_loss'][j], one['step_loss'][0])
    mixed = R.rollout(params, True, True, 'bce', 5, x, a, s, np.array([[True, False], [False, False]]))
    assert torch.equal(mixed['frames'][0], got['frames'][0]) and not torch.equal(mixed['frames'][1], got['frames'][1])
