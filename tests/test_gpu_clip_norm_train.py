"""GPU: clipping by global norm through the runtime - Trainer(g_clip_norm=, d_clip_norm=, grad_norms=), the programs it builds and
the CLI - against ClipOracleTrainer (tests/clip_norm_ref.py), the float64 rollout restatement, and the run without the feature."""
import json
import math

import numpy as np
import pytest
import torch

import clip_norm_ref as R
import rollout_train_ref as RR
import train_cases as TC
from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T
from action_conditioned_gans_amd.saver import Saver

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _inputs(b=2, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (b, 64, 64, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (b, 64, 64, 3)).astype(np.float32)
    a = rng.standard_normal((b, 10)).astype(np.float32)
    return x, y, a, a[:, 5:].copy()


def _window(k, b=2, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (b, k + 1, 64, 64, 3)).astype(np.float32), rng.standard_normal((b, k, 10)).astype(np.float32),
            rng.standard_normal((b, k, 5)).astype(np.float32))


def _trainer(dtype='f32', loss='bce', opt='adam', dna=True, use_hip_graphs=True, **kw):
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device=DEV, dtype=dtype, use_hip_graphs=use_hip_graphs)
    tr = T.Trainer(sess, True, loss, opt, dna, batch_size=2, **kw)
    sess.run(G.global_variables_initializer())
    return sess, tr


def _snapshot(sess):
    """Every variable and every named piece of state (optimizer slots, step counters, flat gradients)."""
    return {k: sess._materialize(t).detach().clone() for k, t in Saver(sess.graph)._tensors().items()}


def _stats_bits(sess, tr):
    return {sc: sess._materialize(n.stats).detach().cpu().numpy().view(np.uint32).copy() for sc, n in tr.grad_norm.items() if n is not None}


def _flat_norm(step_op):
    return float(step_op.inputs[1].buf.detach().double().norm())


# ---- (a) a bound that never binds is invisible ---------------------------------------------------------------------------------
def test_a_bound_that_never_binds_changes_nothing():
    def run(**kw):
        sess, tr = _trainer(**kw)
        frames = []
        for i in range(3):
            x, y, a, s = _inputs(seed=i)
            tr.train_d(x, y, a, next_g=(x, a) if i % 2 else None)          # (the look-ahead call path too)
            frames.append(np.array(tr.train_g(x, y, a, s), copy=True))
        snap = _snapshot(sess)
        stats = {sc: tr.grad_norm_stats(sc) for sc in ('g', 'd')} if kw else None
        sess.close()
        return frames, snap, stats
    want_frames, want, _ = run()
    got_frames, got, stats = run(g_clip_norm=1e30, d_clip_norm=1e30)
    assert set(got) == set(want) and len(want) > 40
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert all(np.array_equal(a, b) for a, b in zip(got_frames, want_frames))
    for sc in ('g', 'd'):
        assert stats[sc]['scale'] == 1.0 and 0 < stats[sc]['norm'] < math.inf


# ---- (b) a bound that binds matches the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize('dna', [True, False], ids=['dna', 'plain'])
def test_a_bound_that_binds_matches_the_clipping_oracle(dna):
    """bce / RMSProp at B = 2, both bounds at half the norms ClipOracleTrainer measures: the reported norm and scale, the clipped
    per-variable gradient norms and the weight steps within 1e-3 - and the unclipped oracle's steps outside that bar
    (clip_norm_ref.check_case), so an op that is created but does not scale fails here."""
    case = R.oracle_case(dna)
    sess, tr = _trainer(opt='rmsprop', dna=dna, g_clip_norm=case['g_bound'], d_clip_norm=case['d_bound'], lookahead=False)
    got = R.run_case(sess, tr, case)
    for sc in ('d', 'g'):
        print(sc, 'norm %.6g (oracle %.6g) scale %.6g (oracle %.6g)' % (got[sc][0]['norm'], case[sc]['norm'], got[sc][0]['scale'], case[sc]['scale']))
    R.check_case(got, case, stats_tol=1e-3)
    sess.close()


# ---- (c) the rollout G step -----------------------------------------------------------------------------------------------------
def test_rollout_step_reports_the_norm_of_the_rollout_gradient():
    from oracle import models as OM
    params = OM.init_params(True, batch=2, img=64, ksize=5, seed=9, dtype=torch.float32)
    x, a, s = _window(2, seed=21)
    ref = RR.RolloutOracle({k: v.double() for k, v in params.items()}, True, 'bce', 'adam', True, 5)
    ref.train_g(R.t64(x), R.t64(a), R.t64(s))
    want = math.sqrt(sum(float((g ** 2).sum()) for g in ref.last_grads.values()))
    bound = float(np.float32(0.5 * want))
    sess, tr = _trainer(rollout_steps=2, lookahead=False, g_clip_norm=bound)
    for n, v in G.get_default_graph().variables.items():
        sess.set_value(v, params[n])
    tr.train_g_rollout(x, a, s)
    stats = tr.grad_norm_stats('g')
    print('rollout norm %.6g (float64 %.6g), scale %.6g' % (stats['norm'], want, stats['scale']))
    assert abs(stats['norm'] - want) <= 1e-3 * want
    assert abs(stats['scale'] - bound / stats['norm']) <= 1e-6 * stats['scale'] and abs(stats['scale'] - 0.5) <= 1e-3
    assert abs(_flat_norm(tr.g_rollout_opt_op) - bound) <= 1e-6 * bound          # the buffer the optimizer read
    sess.close()


# ---- (d) bf16 ---------------------------------------------------------------------------------------------------------------
def test_bf16_graph_measures_its_float32_flat_gradient():
    x, y, a, s = _inputs(seed=4)
    sess, tr = _trainer(dtype='bf16', grad_norms=True, lookahead=False)
    assert tr.g_opt_op.inputs[1].dtype == torch.float32
    tr.train_d(x, y, a)
    tr.train_g(x, y, a, s)
    free = {sc: tr.grad_norm_stats(sc) for sc in ('g', 'd')}
    for sc, op in (('g', tr.g_opt_op), ('d', tr.d_opt_op)):
        want = _flat_norm(op)
        assert free[sc]['scale'] == 1.0 and abs(free[sc]['norm'] - want) <= 1e-6 * want, (sc, free[sc]['norm'], want)
    sess.close()
    bounds = {sc: float(np.float32(0.5 * free[sc]['norm'])) for sc in free}
    sess, tr = _trainer(dtype='bf16', g_clip_norm=bounds['g'], d_clip_norm=bounds['d'], lookahead=False)
    tr.train_d(x, y, a)
    tr.train_g(x, y, a, s)
    for sc, op in (('g', tr.g_opt_op), ('d', tr.d_opt_op)):
        st = tr.grad_norm_stats(sc)
        want = _flat_norm(op) / st['scale']
        assert st['scale'] < 1.0 and abs(st['norm'] - want) <= 1e-6 * want, (sc, st, want)
    sess.close()


# ---- (e) graph replay ---------------------------------------------------------------------------------------------------------
def test_hip_graph_replay_equals_eager_launches():
    x, y, a, s = _inputs(seed=6)
    got = {}
    for graphs in (False, True):
        sess, tr = _trainer(opt='rmsprop', g_clip_norm=1.0, d_clip_norm=1e-3, use_hip_graphs=graphs, lookahead=False)
        seen = []
        for _ in range(5):                                   # eager, capture and three replays | five eager runs
            tr.train_d(x, y, a)
            tr.train_g(x, y, a, s)
            seen.append(_stats_bits(sess, tr))
        if graphs:
            assert all(p.graphs is not None for p in sess._programs.values())
        got[graphs] = (seen, _snapshot(sess), tr.grad_norm_stats('g')['scale'], tr.grad_norm_stats('d')['scale'])
        sess.close()
    assert got[True][2] < 1.0 and got[True][3] < 1.0         # both bounds bind
    for a_, b_ in zip(got[False][0], got[True][0]):
        assert all(np.array_equal(a_[sc], b_[sc]) for sc in ('g', 'd'))
    assert all(torch.equal(got[False][1][k], got[True][1][k]) for k in got[True][1])


# ---- (f) look-ahead -----------------------------------------------------------------------------------------------------------
def test_lookahead_path_reports_what_the_plain_path_reports():
    """Iteration 0 on distinct D-step and G-step samples.  NOT bitwise: the two call paths are the same arithmetic in another
    summation order (BatchNorm over the halves of a joined batch).  Bars from what the project records about exactly that
    difference: the D gradient moves by at most 1e-4 of its norm (test_gpu_train.py), the G gradient by 1.6e-3 where a kink of the
    L1 / GDL losses flips (profiles/r5/e_lookahead_divergence.txt) plus the same 1e-4 of rounding: 2e-3.  A norm differs by no more
    than the norm of the difference, and the scale is bound / norm."""
    x, y, a, s = TC.MG.inputs(2)
    xb, yb, ab, sb = [np.ascontiguousarray(t[::-1]) for t in (y, x, a, s)]
    got = {}
    for use in (False, True):
        sess, tr = _trainer(opt='rmsprop', g_clip_norm=1.0, d_clip_norm=1e-3)
        assert tr.lookahead
        tr.train_d(x, y, a, next_g=(xb, ab) if use else None)
        tr.train_g(xb, yb, ab, sb)
        got[use] = {sc: tr.grad_norm_stats(sc) for sc in ('g', 'd')}
        sess.close()
    for sc, bar in (('d', 1e-4), ('g', 2e-3)):
        p, l = got[False][sc], got[True][sc]
        print(sc, p['norm'], l['norm'], p['scale'], l['scale'])
        assert abs(l['norm'] - p['norm']) <= bar * p['norm'] and abs(l['scale'] - p['scale']) <= bar * p['scale'] and l['scale'] < 1.0


# ---- (g) one state per scope ----------------------------------------------------------------------------------------------------
def test_every_g_update_writes_the_same_statistics():
    x, y, a, s = _inputs(seed=8)
    w = _window(2, seed=8)
    sess, tr = _trainer(rollout_steps=2, lookahead=False, grad_norms=True)
    steps = [(tr.g_pretrain_opt_op, lambda: tr.pretrain_g(x, y, a, s)), (tr.g_opt_op, lambda: tr.train_g(x, y, a, s)),
             (tr.g_rollout_pretrain_opt_op, lambda: tr.pretrain_g_rollout(*w)), (tr.g_rollout_opt_op, lambda: tr.train_g_rollout(*w))]
    assert len({id(op.clip_norm_op.norm) for op, _ in steps}) == 1 and len({id(op.inputs[1]) for op, _ in steps}) == 4
    seen = []
    for op, run in steps:
        run()
        st = tr.grad_norm_stats('g')
        want = _flat_norm(op)                                # (every update has a flat gradient buffer of its own)
        assert st['scale'] == 1.0 and abs(st['norm'] - want) <= 1e-6 * want, (op.name, st['norm'], want)
        offs = G.get_default_graph().layout('g')[0]
        flat = op.inputs[1].buf.detach().double()
        for v in tr.g_vars:
            part = float(flat[offs[v.name]:offs[v.name] + v.numel].norm())
            assert abs(st['per_variable'][v.name] - part) <= 1e-6 * part + 1e-30, v.name
        seen.append(st['norm'])
    assert len(set(seen)) == 4
    assert tr.grad_norm_stats('d')['norm'] == 0.0            # no D update ran
    sess.close()


# ---- (h) the CLI --------------------------------------------------------------------------------------------------------------
def test_cli_train_with_a_bound_then_evaluate(tmp_path):
    out, plain, ev = tmp_path / 'run', tmp_path / 'plain', tmp_path / 'eval'
    common = ['--adv', 'True', '--dna', '--batch_size', '4', '--pretrain_iter', '0']
    T.main(['synthetic', str(out)] + common + ['--train_iter', '4', '--g_clip_norm', '5', '--log_grad_norms'])
    rec = [json.loads(line) for line in open(out / 'logs' / 'train.jsonl')]
    assert rec and rec[0]['g_clip_norm'] == 5.0 and rec[0]['d_clip_norm'] == 0.0 and all('g_clip_norm' not in r for r in rec[1:])
    for r in rec:
        vals = [r[k] for k in ('g_grad_norm', 'g_clip_scale', 'd_grad_norm', 'd_clip_scale')]
        assert np.isfinite(vals).all() and r['g_grad_norm'] > 0 and r['d_clip_scale'] == 1.0
        assert r['g_clip_scale'] <= 1.0 and r['g_grad_norm'] * r['g_clip_scale'] <= 5.0 * (1 + 1e-5)
    T.main(['synthetic', str(plain)] + common + ['--train_iter', '2'])
    first = json.loads(open(plain / 'logs' / 'train.jsonl').readline())
    assert not any('grad_norm' in k or 'clip' in k for k in first)
    got, want = np.load(str(out / 'models' / 'model0.npz')), np.load(str(plain / 'models' / 'model0.npz'))
    assert sorted(got.files) == sorted(want.files)
    res = E.main([str(out / 'models'), 'synthetic', str(ev), '--dna', '--num_sequences', '4', '--batch_size', '4'])
    assert np.isfinite(res['psnr']).all() and np.isfinite(res['ssim']).all()
