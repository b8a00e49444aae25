"""The planner's designated-pixel cost without a GPU: known answers of the float64 restatement (tests/pixel_cost_ref.py), the
binding of acg_plan_pixel_cost, the Trainer's map path (graph shape, refusals, and the twin against the float64 gather on the C
oracle), the Planner's refusals and the plan CLI's pixel arguments."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pixel_cost_ref as R

from action_conditioned_gans_amd import _lib
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import ops as O
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import plan as P
from action_conditioned_gans_amd import train as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- known answers of the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tap', [(0, 0), (2, 2), (1, 4), (4, 0)], ids=str)
def test_a_one_hot_under_one_tap_lands_where_the_tap_says(tap):
    """out[y, x] = sum_ij w[y, x][i, j] * in[y + i - p, x + j - p]: with all weight on tap (i, j) the point (y0, x0) is read by
    (y0 + p - i, x0 + p - j) and by nobody else."""
    k, p, (y0, x0) = 5, 2, (6, 5)
    out = R.gather(R.tap_logits(1, 12, 11, k, tap), R.one_hot(1, 12, 11, [(y0, x0)]), k)
    want = (y0 + p - tap[0], x0 + p - tap[1])
    assert np.unravel_index(out[0, :, :, 0].argmax(), (12, 11)) == want
    assert abs(out[0][want][0] - 1.0) < 1e-15 and abs(out.sum() - 1.0) < 1e-15
    res = R.pixel_cost(out, [[float(want[0]), float(want[1])]])
    assert abs(res['cost'][0]) < 1e-15 and np.allclose(res['expected'][0, 0], want, rtol=0, atol=1e-13)


def test_three_four_five_and_the_goal_on_the_point():
    maps = R.one_hot(2, 9, 10, [(2, 3), (7, 7)])
    res = R.pixel_cost(maps, [[5.0, 7.0], [7.0, 7.0]])                     # (3, 4) away; on the point
    assert np.array_equal(res['cost'], [5.0, 5.0]) and np.array_equal(res['mass'], np.ones((2, 2)))
    assert np.array_equal(res['expected'][0], [[2.0, 3.0], [7.0, 7.0]]) and np.array_equal(res['maps'], maps)
    assert np.array_equal(R.pixel_cost(maps, [[2.0, 3.0], [7.0, 7.0]])['cost'], [0.0, 0.0])
    assert np.array_equal(R.pixel_cost(maps, [[5.0, 7.0], [7.0, 7.0]], pixel_weight=0.5, old=[1.0, -1.0])['cost'], [3.5, 1.5])
    # the cost does not depend on the scale of a map; the normalised map does
    res3 = R.pixel_cost(3.0 * maps, [[5.0, 7.0], [7.0, 7.0]])
    assert np.array_equal(res3['cost'], [5.0, 5.0]) and np.array_equal(res3['maps'], maps) and np.array_equal(res3['mass'], np.full((2, 2), 3.0))


def test_mass_pushed_over_the_border_is_lost_and_renormalised():
    """Two points of mass 1/2 under a tap that moves everything up by two rows: the one in row 1 leaves the image, the other
    stays; the map then holds half the mass, and the cost is the survivor's distance, not half of it."""
    k = 5
    maps = np.zeros((1, 8, 8, 1))
    maps[0, 1, 4, 0] = maps[0, 5, 4, 0] = 0.5
    out = R.gather(R.tap_logits(1, 8, 8, k, (4, 2)), maps, k)              # lands on (y0 + 2 - 4, x0)
    assert abs(out.sum() - 0.5) < 1e-15 and abs(out[0, 3, 4, 0] - 0.5) < 1e-15
    res = R.pixel_cost(out, [[3.0, 0.0]])
    assert abs(res['mass'][0, 0] - 0.5) < 1e-15 and abs(res['cost'][0] - 4.0) < 1e-13 and abs(res['maps'].sum() - 1.0) < 1e-15
    cost, kept, expected = R.rollout([R.tap_logits(1, 8, 8, k, (4, 2))] * 2, maps, k, [[1.0, 4.0]])
    assert kept.shape == (1, 2, 8, 8, 1) and np.allclose(kept.sum(axis=(2, 3, 4)), 1.0, rtol=0, atol=1e-14)
    assert np.allclose(expected[0, 0], [1.0, 4.0], rtol=0, atol=1e-13) and abs(cost[0] - 2.0) < 1e-13      # 2 away, then 0


def test_zero_mass_is_an_infinite_cost():
    maps = R.one_hot(2, 4, 4, [(1, 1), (2, 2)])
    maps[1, :, :, 0] = 0.0
    res = R.pixel_cost(maps, [[0.0, 0.0], [0.0, 0.0]])
    assert np.isfinite(res['cost'][0]) and res['cost'][1] == np.inf and np.isnan(res['expected'][1, 0]).all()
    assert np.array_equal(res['expected'][1, 1], [2.0, 2.0]) and np.array_equal(res['maps'][1], maps[1]) and res['mass'][1, 0] == 0.0
    assert R.pixel_cost(maps, [[0.0, 0.0], [0.0, 0.0]], pixel_weight=0.0)['cost'][1] == np.inf
    nan = maps.copy()
    nan[0, 0, 0, 1] = np.nan
    assert R.pixel_cost(nan, [[0.0, 0.0], [0.0, 0.0]])['cost'][0] == np.inf


# ---- binding -------------------------------------------------------------------------------------------------------------------------
def test_the_entry_is_bound_in_the_rollout_table():
    sigs = _lib.EXTENSIONS['rollout'].signatures
    res, args = sigs['acg_plan_pixel_cost']
    assert res is _lib.STATUS and len(args) == 12 and args[2] is ctypes.c_float and args[4] is ctypes.c_int32
    assert args[7:11] == [ctypes.c_int32] * 4
    assert _lib.ABI_VERSION == 8 and (_lib.PLAN_PIXEL_MAPS_MAX, _lib.PLAN_MAP_SIDE_MAX) == (4, 1024)
    header = open(os.path.join(ROOT, 'include', 'acgan_rollout.h')).read()
    for text in ('int32_t acg_plan_pixel_cost(float* maps, const float* goals, float pixel_weight, float* cost, int32_t accumulate,',
                 '#define ACG_PLAN_PIXEL_MAPS_MAX 4', '#define ACG_PLAN_MAP_SIDE_MAX 1024'):
        assert text in header, text
    assert '#define ACG_ABI_VERSION 8' in open(os.path.join(ROOT, 'include', 'acgan_hip.h')).read()
    lib = _lib.get()
    assert callable(lib.plan_pixel_cost) and lib.version() == 8


# ---- the Trainer's map path ----------------------------------------------------------------------------------------------------------
def _cpu_trainer(transform=True, batch_size=2, lib=None, **kw):
    from oracle import cbind
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cpu', lib=lib or cbind.load())
    kw.setdefault('lookahead', False)
    return sess, T.Trainer(sess, True, 'bce', 'adam', transform, batch_size=batch_size, **kw)


def _graph_print():
    g = G.get_default_graph()
    return ([(type(o).__name__, o.name, o.index, [t.shape for t in o.outputs]) for o in g.ops], [s.name for s in g.state],
            sorted(g.variables))


def _program(sess, fetches):
    if not sess._initialized:
        sess.run(G.global_variables_initializer())
    return [op for kind, seg in sess._compile(sess._flatten(fetches), []).segments if kind == 'dev' for op, _ in seg]


def test_pixel_maps_zero_builds_the_graph_it_always_built():
    _cpu_trainer(lookahead=True, bn_inference=True)
    plain = _graph_print()
    sess, tr = _cpu_trainer(lookahead=True, bn_inference=True, pixel_maps=0)
    assert _graph_print() == plain
    assert tr.pixel_maps == 0 and tr.pixel_map_ph is None and tr.g_map_out is None and tr.g_map_stored is None


def test_pixel_maps_adds_twins_and_nothing_a_training_program_runs():
    sess0, tr0 = _cpu_trainer(lookahead=True, bn_inference=True, rollout_steps=1)
    ops0, state0, vars0 = _graph_print()
    programs0 = [[(type(o).__name__, o.name) for o in _program(sess0, [f])] for f in (tr0.g_opt_op, tr0.d_opt_op, tr0.g_pretrain_opt_op)]
    sess, tr = _cpu_trainer(lookahead=True, bn_inference=True, pixel_maps=2)
    ops2, state2, vars2 = _graph_print()
    assert state2 == state0 and vars2 == vars0                                  # no variable, no state: the checkpoint keys
    assert tr.pixel_maps == 2 and tr.pixel_map_ph.shape == (2, 64, 64, 2) and tr.pixel_map_ph.dtype == torch.float32
    twins = [tr.g_map_out.op, tr.g_map_stored.op]
    for twin, frame in zip(twins, (tr.g_out.op, tr.g_out_stored.op)):
        assert isinstance(twin, O.DnaOp) and isinstance(frame, O.DnaOp) and twin is not frame
        assert twin.inputs[0] is frame.inputs[0] and twin.inputs[2] is frame.inputs[2] and twin.inputs[2].name == 'g/tconv4/biases'
        assert twin.inputs[1] is tr.pixel_map_ph and twin.ksize == frame.ksize and twin.outputs[0].shape == (2, 64, 64, 2)
    added = [o for o in ops2 if o not in ops0]
    assert sorted(o[0] for o in added) == ['DnaOp', 'DnaOp'] and len(ops2) == len(ops0) + 2
    # every training program is the one of the Trainer without the argument, and no other op of the graph reads a twin
    programs2 = [_program(sess, [f]) for f in (tr.g_opt_op, tr.d_opt_op, tr.g_pretrain_opt_op)]
    for prog0, prog2 in zip(programs0, programs2):
        assert [(type(o).__name__, o.name) for o in prog2] == prog0
        assert not any(o is t for o in prog2 for t in twins)
    outs = {id(t.outputs[0]) for t in twins}
    assert not any(id(t) in outs for o in G.get_default_graph().ops for t in o.inputs)
    # the predict program that fetches the map holds its twin and not the other instance's
    prog = _program(sess, [tr.g_next_frame, tr.g_state_out, tr.g_map_out])
    assert any(o is twins[0] for o in prog) and not any(o is twins[1] for o in prog)


def test_the_rollout_instances_have_no_twin():
    sess, tr = _cpu_trainer(rollout_steps=2, pixel_maps=1)
    dna = [o for o in G.get_default_graph().ops if isinstance(o, O.DnaOp)]
    assert sum(o.inputs[1] is tr.pixel_map_ph for o in dna) == 1 and len(dna) >= 3
    import train_cases as TC
    for step in (tr.g_rollout_opt_op, tr.g_rollout_pretrain_opt_op):          # (the dependency walk: the C oracle cannot bind these)
        walked = TC.program_op_names(sess, [step], {})
        assert len(walked) > 100 and not any(i == tr.g_map_out.op.index for i, _, _ in walked)


@pytest.mark.parametrize('kw,match', [
    (dict(transform=False, pixel_maps=1), 'plain generator'), (dict(transform='cdna', pixel_maps=1), 'CDNA generator is declined'),
    (dict(pixel_maps=5), '0..4'), (dict(pixel_maps=1.5), 'integer'), (dict(pixel_maps=-1), '0..4'), (dict(pixel_maps=True), 'integer'),
], ids=str)
def test_pixel_maps_refusals_create_nothing(kw, match):
    G.reset_default_graph()
    g = G.get_default_graph()
    with pytest.raises(ValueError, match=match):
        _cpu_trainer(**kw)
    g = G.get_default_graph()
    assert not g.ops and not g.variables and not g.state
    if kw.get('transform') == 'cdna':            # the refusal says why
        with pytest.raises(ValueError, match='no single flow'):
            T.check_pixel_maps(1, 'cdna')


def test_the_twin_is_the_float64_gather_of_the_fetched_logits():
    """C-oracle CPU session, DNA, batch 2: the map the twin returns for a one-hot input is the float64 gather under
    softmax(logits + bias) of the logits the same program computed - the project's acg_dna_fwd bar, 2e-5 absolute."""
    sess, tr = _cpu_trainer(pixel_maps=1)
    sess.run(G.global_variables_initializer())
    rng = np.random.default_rng(3)
    x = rng.uniform(0, 1, (2, 64, 64, 3)).astype(np.float32)
    a = rng.uniform(-1, 1, (2, 10)).astype(np.float32)
    maps = R.one_hot(2, 64, 64, [(20, 30)]).astype(np.float32)
    twin = tr.g_map_out.op
    feed = tr._feed(x, x, a)
    feed[tr.pixel_map_ph] = maps
    got, logits, frame = sess.run([tr.g_map_out, twin.inputs[0], tr.g_next_frame], feed)
    k = tr.ksize
    bias = sess.get_value(twin.inputs[2]).double().numpy()
    want = R.gather(logits[..., :k * k], maps, k, bias)
    assert got.shape == (2, 64, 64, 1) and np.abs(got - want).max() <= 2e-5
    assert np.abs(frame - R.gather(logits[..., :k * k], x, k, bias)).max() <= 2e-5           # (the frame's own op, same bar)
    assert got.sum() > 0.5 and (got[:, 18:23, 28:33] > 0).any() and np.abs(got).sum() - np.abs(got[:, 18:23, 28:33]).sum() < 1e-6


# ---- Planner ---------------------------------------------------------------------------------------------------------------------------
def test_pixel_weight_on_the_c_oracle_names_the_entry():
    from oracle import cbind
    sess, tr = _cpu_trainer(pixel_maps=1)
    before = _graph_print()
    with pytest.raises(_lib.AcgError) as err:
        P.Planner(tr, 2, 1, 1, pixel_weight=1.0)
    for part in ('acg_plan_pixel_cost', 'include/acgan_rollout.h', cbind.SO_PATH):
        assert part in str(err.value), (part, str(err.value))
    with pytest.raises(_lib.AcgError, match='acg_plan_pixel_cost'):
        P.accumulate_pixel_cost(torch.zeros(2, 4, 4, 1), torch.zeros(1, 2), torch.zeros(2), lib=cbind.load())
    assert _graph_print() == before


class _WithPlan:
    """A library that has the plan entries (and launches none of them) over the C oracle."""
    path = 'stand-in'

    def __getattr__(self, name):
        from oracle import cbind
        if name.startswith('plan_'):
            return lambda *a: pytest.fail('launched')
        return getattr(cbind.load(), name)


def test_planner_refusals_leave_the_graph_alone():
    sess, tr = _cpu_trainer()
    before = _graph_print()
    with pytest.raises(ValueError, match='pixel_maps >= 1'):
        P.Planner(tr, 2, 1, 1, pixel_weight=1.0)
    for bad in (-1.0, float('nan'), float('inf'), 'one'):
        with pytest.raises(ValueError, match='pixel_weight'):
            P.Planner(tr, 2, 1, 1, pixel_weight=bad)
    assert _graph_print() == before


def _bare_planner(pixel_weight, frame_weight=1.0, state_weight=0.0, pixel_maps=2):
    """A Planner as far as the argument checks of plan() / evaluate_actions() go: everything they refuse is refused before the
    first upload or launch, so nothing else is needed (and a session that is touched fails the test)."""
    planner = P.Planner.__new__(P.Planner)
    planner.args = P.check_plan(2, 2, 1, 1, frame_weight=frame_weight, state_weight=state_weight, pixel_weight=pixel_weight)

    class NoTrainer:
        img_size = 64

        def _predicting(self, *a, **kw):
            pytest.fail('the rollout was entered')
    NoTrainer.pixel_maps = pixel_maps
    planner.trainer, planner.bn, planner.weights = NoTrainer(), 'batch', 'raw'
    return planner


FRAME, STATE = np.zeros((64, 64, 3), np.float32), np.zeros(5, np.float32)
PX, GP = np.array([[20, 30], [5, 6]]), np.array([[24.5, 30.0], [0.0, 63.0]])


@pytest.mark.parametrize('kw,match', [
    (dict(), 'needs pixels and goal_pixels'), (dict(pixels=PX), 'needs pixels and goal_pixels'), (dict(goal_pixels=GP), 'needs pixels'),
    (dict(pixels=PX[:1], goal_pixels=GP[:1]), r'pixel_maps=2'), (dict(pixels=PX.astype(np.float32), goal_pixels=GP), 'integer'),
    (dict(pixels=[[20, 64], [5, 6]], goal_pixels=GP), 'inside'), (dict(pixels=[[-1, 3], [5, 6]], goal_pixels=GP), 'inside'),
    (dict(pixels=PX, goal_pixels=[[24.5, 63.5], [0, 0]]), r'within \[0, 63\]'), (dict(pixels=PX, goal_pixels=[[-0.5, 3], [0, 0]]), 'within'),
    (dict(pixels=PX, goal_pixels=[[np.nan, 3], [0, 0]]), 'within'), (dict(pixels=PX, goal_pixels=GP[:1]), r'goal_pixels must be a float \[2, 2\]'),
], ids=str)
def test_plan_checks_the_pixels_before_it_touches_anything(kw, match):
    planner = _bare_planner(1.0)
    with pytest.raises(ValueError, match=match):
        planner.plan(FRAME, STATE, FRAME, **kw)
    with pytest.raises(ValueError, match=match):
        planner.evaluate_actions(FRAME, STATE, np.zeros((2, 2, 5), np.float32), FRAME, **kw)


def test_goal_frame_and_pixels_follow_the_weights():
    with pytest.raises(ValueError, match='frame_weight and state_weight are 0'):
        _bare_planner(1.0).plan(FRAME, STATE, None, pixels=PX, goal_pixels=GP)
    with pytest.raises(ValueError, match='frame_weight and state_weight are 0'):
        _bare_planner(1.0, frame_weight=0.0, state_weight=1.0).plan(FRAME, STATE, None, goal_state=STATE, pixels=PX, goal_pixels=GP)
    for kw in (dict(pixels=PX, goal_pixels=GP), dict(pixels=PX), dict(goal_pixels=GP)):
        with pytest.raises(ValueError, match='pixel_weight 0'):
            _bare_planner(0.0).plan(FRAME, STATE, FRAME, **kw)
        with pytest.raises(ValueError, match='pixel_weight 0'):
            _bare_planner(0.0).evaluate_actions(FRAME, STATE, np.zeros((2, 2, 5), np.float32), FRAME, **kw)
    with pytest.raises(ValueError, match='goal_frame may be None only with a pixel cost'):
        _bare_planner(0.0, frame_weight=0.0).plan(FRAME, STATE, None)
    with pytest.raises(ValueError, match='return_maps'):
        _bare_planner(0.0).evaluate_actions(FRAME, STATE, np.zeros((2, 2, 5), np.float32), FRAME, return_maps=True)
    # and what is allowed reaches the rollout
    with pytest.raises(pytest.fail.Exception, match='the rollout was entered'):
        _bare_planner(1.0, frame_weight=0.0).plan(FRAME, STATE, None, pixels=PX, goal_pixels=GP)


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------------
def _npy(tmp_path, n=3, t=6):
    f, a = str(tmp_path / 'frames.npy'), str(tmp_path / 'actions.npy')
    np.save(f, np.zeros((n, t, 64, 64, 3), np.uint8))
    np.save(a, np.zeros((n, t, 10), np.float32))
    return f, a


def test_cli_reaches_the_worker_with_the_parsed_pixels(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(P, 'plan_sequences', lambda *a, **kw: seen.update(kw, positional=a))
    f, a = _npy(tmp_path)
    base = ['models', f, str(tmp_path / 'out'), '--actions', a, '--dna']
    P.main(base + ['--pixel', '20,30', '--goal_pixel', '24.5,30', '--pixel', '5,6', '--goal_pixel', '0,63', '--frame_weight', '0'])
    assert seen['pixels'].dtype == np.int64 and seen['pixels'].tolist() == [[20, 30], [5, 6]]
    assert seen['goal_pixels'].dtype == np.float32 and seen['goal_pixels'].tolist() == [[24.5, 30.0], [0.0, 63.0]]
    assert seen['pixel_weight'] == 1.0 and seen['frame_weight'] == 0.0 and seen['dna'] is True
    P.main(base + ['--pixel', '1,2', '--goal_pixel', '3,4', '--pixel_weight', '2.5'])
    assert seen['pixel_weight'] == 2.5 and seen['frame_weight'] == 1.0 and seen['pixels'].shape == (1, 2)
    pf, gf = str(tmp_path / 'px.npy'), str(tmp_path / 'gp.npy')
    np.save(pf, np.tile(PX, (3, 1, 1)))
    np.save(gf, np.tile(GP, (3, 1, 1)))
    P.main(base + ['--pixels', pf, '--goal_pixels', gf])
    assert seen['pixels'].shape == (3, 2, 2) and seen['goal_pixels'].shape == (3, 2, 2) and seen['pixel_weight'] == 1.0
    P.main(base)                                                    # without pixels: the worker is called as it always was
    assert seen['pixels'] is None and seen['goal_pixels'] is None and seen['pixel_weight'] is None and seen['frame_weight'] == 1.0
    assert not os.path.exists(tmp_path / 'out')


@pytest.mark.parametrize('flags', [
    ['--dna', '--pixel', '1,2'], ['--dna', '--pixel', '1,2', '--goal_pixel', '3,4', '--goal_pixel', '5,6'], ['--dna', '--goal_pixel', '3,4'],
    ['--dna', '--pixel', '64,2', '--goal_pixel', '3,4'], ['--dna', '--pixel', '1,2', '--goal_pixel', '3,63.5'],
    ['--dna', '--pixel', '1', '--goal_pixel', '3,4'], ['--dna', '--pixel', '1,x', '--goal_pixel', '3,4'],
    ['--dna'] + ['--pixel', '1,2', '--goal_pixel', '3,4'] * 5, ['--pixel', '1,2', '--goal_pixel', '3,4'],
    ['--cdna', '--pixel', '1,2', '--goal_pixel', '3,4'], ['--dna', '--pixel_weight', '1.0'],
    ['--dna', '--pixel', '1,2', '--goal_pixel', '3,4', '--pixel_weight', '0'], ['--dna', '--pixel', '1,2', '--goal_pixel', '3,4', '--pixel_weight', '-1'],
    ['--dna', '--frame_weight', '0'], ['--dna', '--frame_weight', '-1'],
    ['--dna', '--pixel', '1,2', '--goal_pixel', '3,4', '--pixels', 'PX2', '--goal_pixels', 'GP2'], ['--dna', '--pixels', 'PX2'],
    ['--dna', '--pixels', 'PX2', '--goal_pixels', 'GP2'], ['--dna', '--pixels', 'PX3', '--goal_pixels', 'GP3', '--num_sequences', '4'],
    ['--dna', '--pixels', 'missing.npy', '--goal_pixels', 'GP3'], ['--dna', '--pixels', 'FLAT', '--goal_pixels', 'FLAT'],
], ids=' '.join)
def test_cli_pixel_argument_errors_create_nothing(tmp_path, monkeypatch, flags):
    """(PX2 / GP2: pixel files with 2 rows for the 3 sequences of the input; PX3 / GP3: 3 rows, but 4 sequences asked for; FLAT: a
    [D, 2] file where [n, D, 2] is expected)"""
    monkeypatch.setattr(P, 'plan_sequences', lambda *a, **kw: pytest.fail('the worker was reached'))
    f, a = _npy(tmp_path)
    files = {'PX2': np.tile(PX, (2, 1, 1)), 'GP2': np.tile(GP, (2, 1, 1)), 'PX3': np.tile(PX, (3, 1, 1)), 'GP3': np.tile(GP, (3, 1, 1)), 'FLAT': PX}
    for name, value in files.items():
        np.save(str(tmp_path / (name + '.npy')), value)
    flags = [str(tmp_path / (v + '.npy')) if v in files or v == 'missing' else v for v in flags]
    with pytest.raises(SystemExit):
        P.main(['models', f, str(tmp_path / 'out'), '--actions', a] + flags)
    assert not os.path.exists(tmp_path / 'out')


def test_plan_sequences_refuses_before_it_creates_the_output(tmp_path):
    out = str(tmp_path / 'out')
    for kw, match in ((dict(dna=True, pixels=PX), 'go together'), (dict(cdna=True, pixels=PX, goal_pixels=GP), 'CDNA generator is declined'),
                      (dict(pixels=PX, goal_pixels=GP), 'plain generator'), (dict(dna=True, pixel_weight=1.0), 'without pixels'),
                      (dict(dna=True, frame_weight=0.0), 'nothing is scored'),
                      (dict(dna=True, pixels=np.tile(PX, (2, 1, 1)), goal_pixels=np.tile(GP, (2, 1, 1)), num_sequences=3), '3 are planned')):
        with pytest.raises(ValueError, match=match):
            P.plan_sequences(str(tmp_path / 'models'), 'synthetic', out, **kw)
        assert not os.path.exists(out)
