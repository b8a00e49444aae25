"""Planning with the generator without a GPU: known answers of the float64 restatement (tests/plan_ref.py), the restated CEM loop
on a quadratic cost, the binding of the three entries, the Planner's refusals and the plan CLI's argument handling."""
import ctypes
import os

import numpy as np
import pytest

import plan_ref as R

from action_conditioned_gans_amd import _lib
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import plan as P
from action_conditioned_gans_amd import train as T

ENTRIES = ('acg_plan_sample', 'acg_plan_cost', 'acg_plan_refit')


# ---- known answers of the restatement ------------------------------------------------------------------------------------------------
def test_cost_by_hand():
    """A 2 x 2 frame of one channel against a goal: (1-0)^2 + (2-0)^2 + (3-1)^2 + (4-1)^2 = 18; two state values: 0.25 + 4."""
    frames = np.array([[[[1.0], [2.0]], [[3.0], [4.0]]], [[[0.0], [0.0]], [[1.0], [1.0]]]])
    goal = np.array([[[0.0], [0.0]], [[1.0], [1.0]]])
    assert np.array_equal(R.cost(frames, goal), [18.0, 0.0])
    states, gs = np.array([[0.5, 2.0], [0.0, 0.0]]), np.array([0.0, 0.0])
    assert np.array_equal(R.cost(frames, goal, states, gs, frame_weight=2.0, state_weight=0.5), [36.0 + 2.125, 0.0])
    assert np.array_equal(R.cost(frames, goal, old=np.array([1.0, -1.0])), [19.0, -1.0])
    padded = np.concatenate([frames, np.full_like(frames, 1e30)], axis=-1)          # a pad channel is not scored
    assert np.array_equal(R.cost(padded, goal, channels=1), [18.0, 0.0])


def test_ranking_with_a_tie_a_nan_and_an_inf():
    costs = np.array([2.0, np.nan, 1.0, np.inf, 1.0])
    assert R.ranks(costs).tolist() == [2, 3, 0, 4, 1]            # the tie by index; NaN ranks as +inf, so before the later inf
    actions = np.arange(5, dtype=np.float64).reshape(5, 1, 1)
    res = R.refit(costs, actions, [[0.0]], [[1.0]], 3, 0.0, 0.0)
    assert res['elite_idx'].tolist() == [2, 4, 0]
    assert res['mean'][0, 0] == 2.0 and abs(res['std'][0, 0] - np.sqrt(8.0 / 3.0)) < 1e-15
    assert res['best_cost'] == 1.0 and res['best_actions'][0, 0] == 2.0 and res['history'] == 1.0


def test_best_updates_on_strict_improvement_only():
    actions = np.array([[[7.0]], [[9.0]]])
    old = np.array([[5.0]])
    same = R.refit([3.0, 4.0], actions, [[0.0]], [[1.0]], 1, 0.5, 0.0, best_cost=3.0, best_actions=old)
    assert same['best_cost'] == 3.0 and same['best_actions'][0, 0] == 5.0
    worse = R.refit([3.5, 4.0], actions, [[0.0]], [[1.0]], 1, 0.5, 0.0, best_cost=3.0, best_actions=old)
    assert worse['best_cost'] == 3.0 and worse['best_actions'][0, 0] == 5.0
    better = R.refit([4.0, 2.0], actions, [[0.0]], [[1.0]], 1, 0.5, 0.0, best_cost=3.0, best_actions=old)
    assert better['best_cost'] == 2.0 and better['best_actions'][0, 0] == 9.0
    nans = R.refit([np.nan, np.nan], actions, [[0.0]], [[1.0]], 2, 0.0, 0.0, best_cost=np.inf, best_actions=old)
    assert nans['best_cost'] == np.inf and nans['best_actions'][0, 0] == 5.0 and nans['elite_idx'].tolist() == [0, 1]
    assert nans['mean'][0, 0] == 8.0 and nans['std'][0, 0] == 1.0


def test_alpha_one_keeps_the_distribution_and_min_std_floors_it():
    rng = np.random.default_rng(0)
    actions, costs = rng.standard_normal((9, 3, 2)), rng.uniform(0, 1, 9)
    mean, std = rng.standard_normal((3, 2)), rng.uniform(0.5, 1, (3, 2))
    res = R.refit(costs, actions, mean, std, 4, 1.0, 0.1)
    assert np.array_equal(res['mean'], mean) and np.array_equal(res['std'], std)
    same = np.broadcast_to(actions[:1], actions.shape)            # identical elites: their deviation is 0, the floor holds
    res = R.refit(costs, same, mean, std, 4, 0.0, 0.25)
    assert np.array_equal(res['std'], np.full((3, 2), 0.25)) and np.allclose(res['mean'], actions[0], rtol=0, atol=1e-15)


def test_sample_clamps_keeps_the_mean_row_and_is_a_function_of_the_state():
    shape = (6, 2, 5)
    mean, std = np.linspace(-0.3, 0.3, 10).reshape(2, 5), np.full((2, 5), 0.5)
    lo, hi = np.full(5, -0.4), np.full(5, 0.25)
    one = R.sample(mean, std, lo, hi, 7, 3, shape)
    assert one.min() >= -0.4 and one.max() <= 0.25 and (one == 0.25).any() and (one == -0.4).any()
    assert np.array_equal(one[0], np.clip(mean, lo, hi))
    assert np.array_equal(one, R.sample(mean, std, lo, hi, 7, 3, shape))
    assert not np.array_equal(one, R.sample(mean, std, lo, hi, 7, 4, shape))
    assert not np.array_equal(one, R.sample(mean, std, lo, hi, 7, 3, shape, stream_id=1))
    free = R.sample(mean, std, lo, hi, 7, 3, shape, keep_mean=False)
    assert not np.array_equal(free[0], one[0]) and np.array_equal(free[1:], one[1:])
    # the tag: not the noise input's draw, not the scheduled-sampling coins' stream word
    import noise_ref
    assert R.PLAN_STREAM_TAG != R.SS_STREAM_TAG != 0
    assert not np.array_equal(R.normals(7, 3, 0, 60), noise_ref.normals(7, 3, 0, 60))


def test_restated_cem_drives_a_quadratic_cost_down():
    target = np.linspace(-0.5, 0.5, 15).reshape(3, 5)
    res = R.cem(lambda c: ((c - target[None]) ** 2).sum(axis=(1, 2)), (64, 3, 5), 8, 12, 0.5, 0.01, 0.1, -1.0, 1.0, seed=5)
    h = res['history']
    assert (np.diff(h) <= 0).all() and h[-1] < 0.1 * h[0] and res['cost'] == h[-1]
    assert np.array_equal(h, np.minimum.accumulate(res['costs'].min(axis=1)))
    assert np.isclose(((res['actions'] - target) ** 2).sum(), res['cost'], rtol=1e-12, atol=0) and res['counter'] == 12
    assert h[0] <= res['costs'][0][0]                                # the mean row (zero) is a candidate of the first round
    assert np.isclose(res['costs'][0][0], (target ** 2).sum(), rtol=1e-12, atol=0)


# ---- binding -------------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_bound_in_the_rollout_table():
    sigs = _lib.EXTENSIONS['rollout'].signatures
    for name in ENTRIES:
        assert sigs[name][0] is _lib.STATUS, name
    assert len(sigs['acg_plan_sample'][1]) == 12 and len(sigs['acg_plan_cost'][1]) == 16 and len(sigs['acg_plan_refit'][1]) == 15
    assert sigs['acg_plan_cost'][1][4:6] == [ctypes.c_float] * 2 and sigs['acg_plan_refit'][1][12:14] == [ctypes.c_float] * 2
    assert (_lib.PLAN_CANDIDATES_MAX, _lib.PLAN_HORIZON_MAX, _lib.PLAN_ACTION_DIM_MAX, _lib.PLAN_STATE_DIM_MAX) == (1024, 16, 8, 16)
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'acgan_rollout.h')).read()
    for text in ('#define ACG_PLAN_CANDIDATES_MAX 1024', '#define ACG_PLAN_HORIZON_MAX 16', '#define ACG_PLAN_ACTION_DIM_MAX 8',
                 '#define ACG_PLAN_STATE_DIM_MAX 16', '#define ACG_PLAN_STREAM_TAG 0x%08Xu' % R.PLAN_STREAM_TAG,
                 '#define ACG_SS_STREAM_TAG 0x%08Xu' % R.SS_STREAM_TAG):
        assert text in header, text
    lib = _lib.get()
    for name in ENTRIES:
        assert callable(getattr(lib, name[4:]))


def _cpu_trainer(transform=True, batch_size=2, lib=None, **kw):
    from oracle import cbind
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cpu', lib=lib or cbind.load())
    return sess, T.Trainer(sess, False, 'bce', 'adam', transform, batch_size=batch_size, lookahead=False, **kw)


def _graph_print():
    g = G.get_default_graph()
    return len(g.ops), len(g.state), len(g.variables)


def test_planner_refuses_the_c_oracle_and_a_cpu_session():
    from oracle import cbind
    sess, tr = _cpu_trainer()
    before = _graph_print()
    with pytest.raises(_lib.AcgError) as err:
        P.Planner(tr, 2, 1, 1)
    for part in ('acg_plan_sample', 'include/acgan_rollout.h', cbind.SO_PATH):
        assert part in str(err.value), (part, str(err.value))
    import torch
    x = torch.zeros(2, 2, 5)
    for call in (lambda: P.sample_actions(x[0], x[0], x[0, 0], x[0, 0], torch.zeros(2, dtype=torch.int64), x, lib=cbind.load()),
                 lambda: P.accumulate_cost(torch.zeros(2, 4, 4, 3), torch.zeros(4, 4, 3), torch.zeros(2), lib=cbind.load()),
                 lambda: P.refit(torch.zeros(2), x, x[0], x[0], torch.zeros(1), x[0], torch.zeros(1, dtype=torch.int32), 0.1, 0.1,
                                 lib=cbind.load())):
        with pytest.raises(_lib.AcgError, match='acg_plan_'):
            call()

    class WithPlan:                       # a library that has the entries, on a session without a GPU
        path = 'stand-in'

        def __getattr__(self, name):
            if name.startswith('plan_'):
                return lambda *a: pytest.fail('launched')
            return getattr(cbind.load(), name)
    sess, tr = _cpu_trainer(lib=WithPlan())
    with pytest.raises(RuntimeError, match='the session has no GPU device'):
        P.Planner(tr, 2, 1, 1)
    assert _graph_print() == before


# ---- rejections ----------------------------------------------------------------------------------------------------------------------
BAD = [
    (dict(horizon=0), 'horizon'), (dict(horizon=17), 'horizon'), (dict(horizon=2.0), 'horizon'),
    (dict(elites=0), 'elites'), (dict(elites=3), 'elites'), (dict(iterations=0), 'iterations'),
    (dict(init_std=0.0), 'init_std'), (dict(init_std=-1.0), 'init_std'), (dict(init_std=float('nan')), 'init_std'),
    (dict(min_std=-0.1), 'min_std'), (dict(alpha=1.5), 'alpha'), (dict(lo=0.5, hi=0.25), 'lo'),
    (dict(lo=[0, 0, 0, 0, 1.0], hi=[1, 1, 1, 1, 0.5]), 'lo'), (dict(hi=[1.0, 1.0]), 'hi'), (dict(cost_steps='first'), 'cost_steps'),
    (dict(frame_weight=-1.0), 'frame_weight'), (dict(state_weight=float('inf')), 'state_weight'), (dict(seed=-1), 'seed'),
    (dict(bn='moving'), 'bn'), (dict(weights='best'), 'weights'),
]


@pytest.mark.parametrize('kw,name', BAD, ids=[repr(k) for k, _ in BAD])
def test_bad_arguments_are_value_errors_that_leave_the_graph_alone(kw, name):
    sess, tr = _cpu_trainer()
    before = _graph_print()
    args = dict(horizon=2, elites=2, iterations=1)
    args.update(kw)
    with pytest.raises(ValueError, match=name):
        P.Planner(tr, **args)
    assert _graph_print() == before


def test_state_weight_needs_a_state_head_and_a_goal_state():
    sess, tr = _cpu_trainer(transform=False)
    before = _graph_print()
    with pytest.raises(ValueError, match='state_weight'):
        P.Planner(tr, 2, 1, 1, state_weight=1.0)
    assert _graph_print() == before
    # with a state head the Planner is built (on a GPU) and plan() refuses a missing goal_state before it touches anything
    planner = P.Planner.__new__(P.Planner)
    planner.args = P.check_plan(2, 2, 1, 1, state_weight=1.0)
    with pytest.raises(ValueError, match='goal_state'):
        planner.plan(np.zeros((64, 64, 3), np.float32), np.zeros(5, np.float32), np.zeros((64, 64, 3), np.float32))


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------------
def _npy(tmp_path, n=3, t=6):
    f, a = str(tmp_path / 'frames.npy'), str(tmp_path / 'actions.npy')
    np.save(f, np.zeros((n, t, 64, 64, 3), np.uint8))
    np.save(a, np.zeros((n, t, 10), np.float32))
    return f, a


def test_cli_reaches_the_worker(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(P, 'plan_sequences', lambda *a, **kw: seen.update(kw, positional=a))
    f, a = _npy(tmp_path)
    P.main(['models', f, str(tmp_path / 'out'), '--actions', a, '--dna', '--ksize', '7', '--bn_stats', 'stored', '--weights', 'ema',
            '--candidates', '16', '--elites', '4', '--iterations', '2', '--horizon', '3', '--goal_step', '5', '--init_std', '0.25',
            '--min_std', '0.01', '--alpha', '0.5', '--state_weight', '2.0', '--cost_steps', 'last', '--seed', '9', '--num_sequences', '2',
            '--dump'])
    assert seen['positional'] == ('models', f, str(tmp_path / 'out')) and seen['actions_path'] == a
    assert seen['dna'] is True and seen['cdna'] is False and seen['ksize'] == 7 and seen['bn_stats'] == 'stored' and seen['weights'] == 'ema'
    assert (seen['candidates'], seen['elites'], seen['iterations'], seen['horizon'], seen['goal_step']) == (16, 4, 2, 3, 5)
    assert (seen['init_std'], seen['min_std'], seen['alpha'], seen['state_weight']) == (0.25, 0.01, 0.5, 2.0)
    assert seen['cost_steps'] == 'last' and seen['seed'] == 9 and seen['num_sequences'] == 2 and seen['dump'] is True
    P.main(['models', 'synthetic', str(tmp_path / 'o2'), '--num_sequences', '4', '--cdna'])
    assert seen['cdna'] is True and seen['goal_step'] == seen['horizon'] == 5 and seen['candidates'] == 64 and seen['dump'] is False
    assert seen['bn_stats'] == 'batch' and seen['weights'] == 'raw' and seen['cost_steps'] == 'all' and seen['state_weight'] == 0.0
    assert not os.path.exists(tmp_path / 'out') and not os.path.exists(tmp_path / 'o2')       # (the worker creates it)


@pytest.mark.parametrize('flags', [
    ['--elites', '9', '--candidates', '8'], ['--horizon', '17'], ['--horizon', '0'], ['--iterations', '0'], ['--candidates', '1025'],
    ['--init_std', '0'], ['--alpha', '2'], ['--state_weight', '1.0'], ['--dna', '--cdna'], ['--goal_step', '0'], ['--goal_step', '6'],
    ['--horizon', '7'], ['--num_sequences', '0'], ['--cost_steps', 'some'], ['--bn_stats', 'calibrate'], ['--no_actions'],
], ids=' '.join)
def test_cli_argument_errors_create_nothing(tmp_path, monkeypatch, flags):
    """(--state_weight without --dna: the plain generator has no state head; --goal_step 6 / --horizon 7: sequences of 6 frames)"""
    monkeypatch.setattr(P, 'plan_sequences', lambda *a, **kw: pytest.fail('the worker was reached'))
    f, a = _npy(tmp_path)
    argv = ['models', f, str(tmp_path / 'out')] + ([] if flags == ['--no_actions'] else ['--actions', a] + flags)
    with pytest.raises(SystemExit):
        P.main(argv)
    assert not os.path.exists(tmp_path / 'out')
    with pytest.raises(SystemExit):
        P.main(['models', 'synthetic', str(tmp_path / 'out')])          # synthetic needs a count
    assert not os.path.exists(tmp_path / 'out')
