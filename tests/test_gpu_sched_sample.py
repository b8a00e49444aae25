"""GPU: scheduled sampling of the K-step rollout (include/acgan_rollout.h, acg_sched_sample_*; ops.SchedSampleDrawOp / SchedSampleOp;
Trainer sched_sampling).  The three kernels against the restatement of tests/sched_sample_ref.py bit for bit, live K-step G steps
against its float64 rollout with the mask the Trainer drew (at the 1e-3 bars of test_gpu_rollout_train.py), HIP-graph replay, the
checkpoint and the CLI end to end."""
import ctypes
import json

import numpy as np
import pytest
import torch

import sched_sample_ref as R
import train_cases as TC
from action_conditioned_gans_amd import _lib
from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T
from action_conditioned_gans_amd.saver import Saver

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = np.float32(-7.25)
GUARD = 256


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _i64(v):
    return v - 2 ** 64 if v >= 2 ** 63 else v


def _state(seed, counter):
    return torch.tensor([_i64(seed), _i64(counter)], dtype=torch.int64, device=DEV)


def _read_state(state):
    return tuple(int(v) % 2 ** 64 for v in state.cpu().numpy())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _guarded(n):
    return torch.full((n + GUARD,), float(SENTINEL), dtype=torch.float32, device=DEV)


def _split(buf, n, what):
    host = buf.cpu().numpy()
    assert np.array_equal(_bits(host[n:]), _bits(np.full(GUARD, SENTINEL))), 'written behind ' + what
    return host[:n].copy()


# ---- the draw ------------------------------------------------------------------------------------------------------------------
# (kind, start, final, decay_steps, offset, counter): two counters per kind, one of them above 2^32; both halves of the seed are set
SCHEDULES = [('constant', 0.3, 0.0, 0, 0, 5), ('constant', 0.3, 0.0, 0, 0, 2 ** 32 + 5),
             ('linear', 0.9, 0.1, 7, 2, 5), ('linear', 1.0, 0.0, 2 ** 33, 2 ** 31, 2 ** 32 + 5),
             ('inverse_sigmoid', 1.0, 0.0, 100, 2, 52), ('inverse_sigmoid', 0.95, 0.05, 2 ** 31, 0, 2 ** 32 + 5)]
SEED = 0x123456789abcdef


def _sched(kind, start, final, decay_steps, offset):
    return _lib.SsSched(R.KINDS.index(kind), offset, decay_steps, start, final)


def _draw(state, sched, mask, prob, steps, batch, stream_id):
    _lib.get().sched_sample_draw(_p(state), ctypes.byref(sched), _p(mask), _p(prob), steps, batch, stream_id, _stream())


@pytest.mark.parametrize('steps,batch', [(1, 1), (2, 3), (3, 32), (7, 64)], ids=str)
@pytest.mark.parametrize('case', SCHEDULES, ids=lambda c: '%s@%d' % (c[0], c[5]))
def test_draw_matches_the_restatement(steps, batch, case):
    kind, start, final, decay, offset, counter = case
    n = steps * batch
    for stream_id in (0, 3):
        state, mask, prob = _state(SEED, counter), _guarded(n), _guarded(1)
        _draw(state, _sched(kind, start, final, decay, offset), mask, prob, steps, batch, stream_id)
        torch.cuda.synchronize()
        got_mask, got_prob = _split(mask, n, 'the mask').reshape(steps, batch), _split(prob, 1, 'prob_out')[0]
        want_prob = R.probability32(kind, counter, start, final, decay, offset)
        print('draw %s k=%d: prob_out %.9g, restatement %.9g' % (kind, counter, got_prob, want_prob))
        if kind == 'inverse_sigmoid':        # double exp on the device is not correctly rounded: that float32 or a neighbour
            assert got_prob in (want_prob, np.nextafter(want_prob, np.float32(0)), np.nextafter(want_prob, np.float32(1))), (got_prob, want_prob)
        else:
            assert _bits(got_prob) == _bits(want_prob), (got_prob, want_prob)
        want = R.coins(SEED, counter, stream_id, steps, batch, got_prob)
        assert np.array_equal(_bits(got_mask), _bits(want.astype(np.float32))), 'mask differs (stream %d)' % stream_id
        assert _read_state(state) == (SEED, counter + 1)
        # the same state again: the same bits; then the advanced counter draws the restatement's next coins
        state2, mask2, prob2 = _state(SEED, counter), _guarded(n), _guarded(1)
        sched = _sched(kind, start, final, decay, offset)
        _draw(state2, sched, mask2, prob2, steps, batch, stream_id)
        _draw(state2, sched, mask, prob, steps, batch, stream_id)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(_split(mask2, n, 'the mask')), _bits(got_mask.reshape(-1))) and _bits(_split(prob2, 1, 'prob_out')[0]) == _bits(got_prob)
        assert _read_state(state2) == (SEED, counter + 2)
        nxt = R.coins(SEED, counter + 1, stream_id, steps, batch, _split(prob, 1, 'prob_out')[0])
        assert np.array_equal(_bits(_split(mask, n, 'the mask')), _bits(nxt.astype(np.float32).reshape(-1)))


def test_draw_at_p0_and_p1_is_constant():
    for p in (0.0, 1.0):
        state, mask, prob = _state(7, 3), _guarded(7 * 64), _guarded(1)
        _draw(state, _sched('constant', p, 0.0, 0, 0), mask, prob, 7, 64, 0)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(_split(mask, 7 * 64, 'the mask')), _bits(np.full(7 * 64, p, np.float32)))


@pytest.mark.parametrize('what,over', [
    ('null state', dict(state=None)), ('null sched', dict(sched=None)), ('null mask', dict(mask=None)), ('null prob', dict(prob=None)),
    ('kind -1', dict(kind=-1)), ('kind 3', dict(kind=3)), ('start > 1', dict(start=1.5)), ('start < 0', dict(start=-0.25)),
    ('final > 1', dict(final=1.5)), ('final < 0', dict(final=-0.25)), ('start nan', dict(start=float('nan'))),
    ('offset < 0', dict(offset=-1)), ('linear without decay', dict(kind=1, decay=0)), ('sigmoid without decay', dict(kind=2, decay=0)),
    ('no steps', dict(steps=0)), ('no batch', dict(batch=0)), ('too many coins', dict(steps=129, batch=64))], ids=lambda v: v if isinstance(v, str) else '')
def test_draw_refusals_launch_nothing(what, over):
    kw = dict(kind=1, start=0.75, final=0.25, decay=8, offset=0, steps=2, batch=4)
    kw.update({k: v for k, v in over.items() if k in kw})
    state, mask, prob = _state(7, 3), _guarded(8192 + 64), _guarded(1)
    sched = _lib.SsSched(kw['kind'], kw['offset'], kw['decay'], kw['start'], kw['final'])
    ptr = dict(state=_p(state), sched=ctypes.byref(sched), mask=_p(mask), prob=_p(prob))
    ptr.update({k: v for k, v in over.items() if k in ptr})
    with pytest.raises(_lib.AcgError, match='sched_sample_draw'):
        _lib.get().sched_sample_draw(ptr['state'], ptr['sched'], ptr['mask'], ptr['prob'], kw['steps'], kw['batch'], 0, _stream())
    torch.cuda.synchronize()
    assert _read_state(state) == (7, 3)
    assert np.array_equal(_bits(mask.cpu().numpy()), _bits(np.full(mask.numel(), SENTINEL)))
    assert _bits(prob.cpu().numpy()[0]) == _bits(SENTINEL)


# ---- select and adjoint --------------------------------------------------------------------------------------------------------
B_SEL, STATE_DIM = 3, 5
MASKS = {'none': [0.0, 0.0, 0.0], 'all': [1.0, 1.0, 1.0], 'mixed': [0.0, 2.0, 0.0], 'mixed2': [-1.0, 0.0, 1.0]}


def _values(shape, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape).astype(np.float32)
    v.reshape(-1)[::11] = [np.float32(-0.0), np.float32(1e-40), np.float32(3.0e38)][seed % 3]        # copied, not computed with
    return v


def _poison(clean, rows):
    out = clean.copy()
    out[rows] = np.nan
    return out


@pytest.mark.parametrize('per_sample,offset', [(17 * 19 * 3, 0), (64 * 64 * 3, 0), (64 * 64 * 3, 1)], ids=['scalar', 'vector', 'vector_size_unaligned'])
@pytest.mark.parametrize('mask_name', list(MASKS))
@pytest.mark.parametrize('mode', ['both', 'frame', 'state'])
def test_select_and_adjoint_match_the_restatement(per_sample, offset, mask_name, mode):
    """Bits: the values hold -0, a denormal and 3e38.  The rows of the source that is NOT selected (and, in the adjoint, the output
    gradient of the rows that read the truth) are NaN: none of it may reach an output.  ``offset`` shifts every frame pointer by one
    float, off the 16-byte alignment of the vector path."""
    lib = _lib.get()
    m = np.array(MASKS[mask_name], np.float32)
    sel = m != 0
    mask = torch.from_numpy(m).to(DEV)
    frame, state = mode in ('both', 'frame'), mode in ('both', 'state')

    def dev(a):
        buf = _guarded(a.size + offset)
        buf[offset:offset + a.size] = torch.from_numpy(a.reshape(-1)).to(DEV)
        return buf, buf[offset:]

    pred, truth = _values((B_SEL, per_sample), 1), _values((B_SEL, per_sample), 2)
    ps, ts = _values((B_SEL, STATE_DIM), 3), _values((B_SEL, STATE_DIM), 4)
    d_pred, d_truth = dev(_poison(pred, sel))[1], dev(_poison(truth, ~sel))[1]
    d_ps, d_ts = torch.from_numpy(_poison(ps, sel)).to(DEV), torch.from_numpy(_poison(ts, ~sel)).to(DEV)
    outs = []
    for _ in range(2):
        out_buf = _guarded(B_SEL * per_sample + offset)
        out = out_buf[offset:]
        out_state = _guarded(B_SEL * STATE_DIM)
        lib.sched_sample_fwd(_p(mask), _p(d_pred) if frame else None, _p(d_truth) if frame else None, _p(out) if frame else None, per_sample,
                             _p(d_ps) if state else None, _p(d_ts) if state else None, _p(out_state) if state else None, STATE_DIM, B_SEL,
                             _stream())
        torch.cuda.synchronize()
        outs.append((out_buf.cpu().numpy(), out_state.cpu().numpy()))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(outs[0], outs[1])), 'two launches differ'
    got, got_state = outs[0]
    n, ns = B_SEL * per_sample, B_SEL * STATE_DIM
    assert np.array_equal(_bits(got[:offset]), _bits(np.full(offset, SENTINEL))), 'written in front of the output'
    want = R.select(m, pred, truth).reshape(-1) if frame else np.full(n, SENTINEL)
    assert np.array_equal(_bits(got[offset:offset + n]), _bits(want))
    assert np.array_equal(_bits(got[offset + n:]), _bits(np.full(GUARD, SENTINEL))), 'written behind the output'
    want_state = R.select(m, ps, ts).reshape(-1) if state else np.full(ns, SENTINEL)
    assert np.array_equal(_bits(got_state[:ns]), _bits(want_state)) and np.array_equal(_bits(got_state[ns:]), _bits(np.full(GUARD, SENTINEL)))

    # the adjoint
    dout, dst = _values((B_SEL, per_sample), 5), _values((B_SEL, STATE_DIM), 6)
    d_dout, d_dst = dev(_poison(dout, sel))[1], torch.from_numpy(_poison(dst, sel)).to(DEV)
    dp_buf, dps = _guarded(n + offset), _guarded(ns)
    dp = dp_buf[offset:]
    lib.sched_sample_bwd(_p(mask), _p(d_dout) if frame else None, _p(dp) if frame else None, per_sample, _p(d_dst) if state else None,
                         _p(dps) if state else None, STATE_DIM, B_SEL, _stream())
    torch.cuda.synchronize()
    got, got_state = dp_buf.cpu().numpy(), dps.cpu().numpy()
    want = R.select_adjoint(m, dout).reshape(-1) if frame else np.full(n, SENTINEL)          # (+0 bits in the truth rows)
    assert np.array_equal(_bits(got[:offset]), _bits(np.full(offset, SENTINEL)))
    assert np.array_equal(_bits(got[offset:offset + n]), _bits(want)) and np.array_equal(_bits(got[offset + n:]), _bits(np.full(GUARD, SENTINEL)))
    want_state = R.select_adjoint(m, dst).reshape(-1) if state else np.full(ns, SENTINEL)
    assert np.array_equal(_bits(got_state[:ns]), _bits(want_state)) and np.array_equal(_bits(got_state[ns:]), _bits(np.full(GUARD, SENTINEL)))


def test_select_and_adjoint_refusals_launch_nothing():
    lib = _lib.get()
    mask = torch.zeros(3, device=DEV)
    a, b, out = (torch.ones(3 * 8, device=DEV) for _ in range(3))
    sa, sb, sout = (torch.ones(3 * 5, device=DEV) for _ in range(3))
    P = _p
    bad_fwd = [(None, P(a), P(b), P(out), 8, P(sa), P(sb), P(sout), 5, 3), (P(mask), None, None, None, 8, None, None, None, 5, 3),
               (P(mask), P(a), None, P(out), 8, None, None, None, 0, 3), (P(mask), P(a), P(b), None, 8, None, None, None, 0, 3),
               (P(mask), P(a), P(b), P(out), 0, None, None, None, 0, 3), (P(mask), None, None, None, 0, P(sa), P(sb), None, 5, 3),
               (P(mask), None, None, None, 0, P(sa), P(sb), P(sout), 0, 3), (P(mask), P(a), P(b), P(out), 8, None, None, None, 0, 0),
               (P(mask), P(a), P(b), P(out), 8, None, None, None, 0, 65536)]
    for args in bad_fwd:
        with pytest.raises(_lib.AcgError, match='sched_sample_fwd'):
            lib.sched_sample_fwd(*args, _stream())
    bad_bwd = [(None, P(a), P(out), 8, None, None, 0, 3), (P(mask), None, None, 8, None, None, 5, 3), (P(mask), P(a), None, 8, None, None, 0, 3),
               (P(mask), P(a), P(out), 0, None, None, 0, 3), (P(mask), None, None, 0, P(sa), None, 5, 3), (P(mask), None, None, 0, P(sa), P(sout), 0, 3),
               (P(mask), P(a), P(out), 8, None, None, 0, 0)]
    for args in bad_bwd:
        with pytest.raises(_lib.AcgError, match='sched_sample_bwd'):
            lib.sched_sample_bwd(*args, _stream())
    torch.cuda.synchronize()
    assert bool((out == 1).all()) and bool((sout == 1).all())


# ---- live K-step steps ---------------------------------------------------------------------------------------------------------
B, K = 4, 3
SS_SEED = 5          # its first draw at p = 0.5 has truth and predicted rows in step slot 0 (asserted on the restatement below)


def _inputs(B, K, S=64, seed=21):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (B, K + 1, S, S, 3)).astype(np.float32)
    for j in range(1, K + 1):                 # frames that follow from their predecessors: a shift plus noise
        x[:, j] = np.clip(np.roll(x[:, j - 1], 2, axis=2) + 0.05 * rng.standard_normal(x[:, j].shape).astype(np.float32), -1, 1)
    a = rng.standard_normal((B, K, 10)).astype(np.float32)
    s = rng.standard_normal((B, K, 5)).astype(np.float32)
    return x, a, s


def _params(dna, seed=9):
    from oracle import models as OM
    return OM.init_params(dna, batch=B, img=64, ksize=5, seed=seed, dtype=torch.float32)


def _trainer(loss='bce', opt='adam', dna=True, sess_kw=None, **kw):
    params = _params(dna)
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device=DEV, **(sess_kw or {}))
    tr = T.Trainer(sess, True, loss, opt, dna, batch_size=B, img_size=64, ksize=5, rollout_steps=K, **kw)
    sess.run(G.global_variables_initializer())
    for n, v in G.get_default_graph().variables.items():
        sess.set_value(v, params[n])
    return sess, tr, params


def _step(sess, tr, x, a, s, dna):
    fetch = [tr.g_rollout_opt_op, tr.rollout_losses, tr.rollout_frames] + ([tr.rollout_states] if dna else [])
    return sess.run(fetch, tr._rollout_feed(x, a, s))


_plain_steps = {}


def _step_without_sampling(loss, opt, dna):
    """The frames and states of one K-step G step of a Trainer built without the keywords, computed once per configuration."""
    key = (loss, opt, dna)
    if key not in _plain_steps:
        sess, tr, _ = _trainer(loss, opt, dna)
        res = _step(sess, tr, *_inputs(B, K), dna)
        _plain_steps[key] = (res[2], res[3] if dna else None)
        sess.close()
    return _plain_steps[key]


def _check_against_restatement(sess, tr, params, res, mask, loss, opt, dna, x, a, s):
    td = lambda t: torch.from_numpy(np.ascontiguousarray(t)).double()     # noqa: E731
    torch.set_num_threads(16)
    ref = R.SchedOracle({k: v.double() for k, v in params.items()}, True, loss, opt, dna, 5)
    ref.mask = mask
    out = ref.train_g(td(x), td(a), td(s))
    for j in range(K):
        err = TC.rel(res[2][j], out['frames'][j].numpy())
        print('step %d: frame rel %.3e' % (j, err))
        assert err <= 1e-3, 'frame of step %d' % j
        if dna:
            assert TC.rel(res[3][j], out['states'][j].numpy()) <= 1e-3, 'state of step %d' % j
    g_loss = float(np.mean([v[0] for v in res[1]]))
    want = float(out['g_loss'])
    print('G loss %.7g, restatement %.7g' % (g_loss, want))
    assert abs(g_loss - want) <= 1e-3 * max(abs(want), 1e-2), (g_loss, want)
    TC.check_norms(TC.flat_grad_norms(sess, tr.g_rollout_opt_op), {'g/' + k: v.norm() for k, v in ref.last_grads.items()},
                   'g/', 1e-3, 'sampled rollout G grad')
    if opt == 'rmsprop':
        for n, v in G.get_default_graph().variables.items():
            if n.startswith('g/'):
                got, w = sess.get_value(v).double().cpu(), ref.p[n]
                assert (got - w).abs().max().item() <= 1e-3 * max(w.abs().max().item(), 1e-3) + 2e-6, n


@pytest.mark.parametrize('dna', [True, False], ids=['dna', 'plain'])
def test_p0_is_the_rollout_step_bit_for_bit(dna):
    """Forward is a copy: the frames and states of every step are those of a Trainer without sampling, in bits.  (The update is
    not held to that: the gradient sums are associated differently.)  Loss and gradient norms against float64."""
    x, a, s = _inputs(B, K)
    frames, states = _step_without_sampling('bce', 'adam', dna)
    sess, tr, params = _trainer('bce', 'adam', dna, sched_sampling='constant', ss_start=0.0, ss_seed=SS_SEED)
    res = _step(sess, tr, x, a, s, dna)
    last = tr.sched_sampling_last()
    assert last['prob'] == 0.0 and not last['mask'].any() and tr.sched_sampling_state() == (SS_SEED, 1)
    for j in range(K):
        assert np.array_equal(_bits(res[2][j]), _bits(frames[j])), 'frame of step %d' % j
        if dna:
            assert np.array_equal(_bits(res[3][j]), _bits(states[j])), 'state of step %d' % j
    _check_against_restatement(sess, tr, params, res, np.zeros((K - 1, B), bool), 'bce', 'adam', dna, x, a, s)
    sess.close()


@pytest.mark.parametrize('dna', [True, False], ids=['dna', 'plain'])
def test_p1_is_k_teacher_forced_steps(dna):
    x, a, s = _inputs(B, K)
    sess, tr, params = _trainer('bce', 'adam', dna, sched_sampling='constant', ss_start=1.0, ss_seed=SS_SEED)
    res = _step(sess, tr, x, a, s, dna)
    last = tr.sched_sampling_last()
    assert last['prob'] == 1.0 and last['mask'].all()
    _check_against_restatement(sess, tr, params, res, np.ones((K - 1, B), bool), 'bce', 'adam', dna, x, a, s)
    sess.close()


@pytest.mark.parametrize('loss,dna', [('wass', True), ('bce', False)], ids=['dna', 'plain'])
def test_p05_matches_the_masked_restatement(loss, dna):
    want = R.coins(SS_SEED, 0, 0, K - 1, B, np.float32(0.5))
    assert want[0].any() and not want[0].all(), 'the seed must give step slot 0 a truth row and a predicted row'
    x, a, s = _inputs(B, K)
    sess, tr, params = _trainer(loss, 'rmsprop', dna, sched_sampling='constant', ss_start=0.5, ss_seed=SS_SEED)
    res = _step(sess, tr, x, a, s, dna)
    last = tr.sched_sampling_last()
    assert last['prob'] == 0.5 and last['mask'].dtype == bool and np.array_equal(last['mask'], want)
    _check_against_restatement(sess, tr, params, res, want, loss, 'rmsprop', dna, x, a, s)
    sess.close()


def test_side_branch_session_gives_the_same_bits():
    """The state head is a side chain (Graph.side_branch): with ``side_branches=True`` the select reads a state the second stream
    produced and its adjoint feeds that stream's backward chain - the joins and forks of Session._launch_segment, eager and
    captured.  Same frames, states and weights as the one-stream session, bit for bit (both sessions on the BatchNorm kernels a
    side-branch session takes)."""
    x, a, s = _inputs(B, K, seed=8)
    got = {}
    for side in (False, True):
        sess, tr, _ = _trainer('bce', 'adam', True, sess_kw=dict(side_branches=side, bn_grid_exchange=False), sched_sampling='constant', ss_start=0.5, ss_seed=SS_SEED)
        for _ in range(3):                      # eager -> capture -> replay
            res = _step(sess, tr, x, a, s, True)
        got[side] = (res[2], res[3], tr.sched_sampling_last()['mask'],
                     {n: sess.get_value(v).cpu().clone() for n, v in G.get_default_graph().variables.items()})
        sess.close()
    assert np.array_equal(got[False][2], got[True][2]) and got[True][2].any() and not got[True][2].all()
    for j in range(K):
        assert np.array_equal(_bits(got[False][0][j]), _bits(got[True][0][j])) and np.array_equal(_bits(got[False][1][j]), _bits(got[True][1][j]))
    assert all(torch.equal(got[False][3][n], got[True][3][n]) for n in got[True][3])


def test_hip_graph_replay_draws_fresh_coins_and_equals_eager_launches():
    """eager -> capture -> replay: every run draws the coins of its own counter, at the schedule's probability there; weights and
    frames are those of the eager launches bit for bit.  The pretraining step holds the same draw: it takes counter 0."""
    x, a, s = _inputs(B, K, seed=4)
    kw = dict(sched_sampling='linear', ss_start=0.75, ss_final=0.25, ss_decay_steps=4, ss_offset=1, ss_seed=SS_SEED)
    got = {}
    for graphs in (False, True):
        sess, tr, _ = _trainer('wass', 'rmsprop', True, sess_kw=dict(use_hip_graphs=graphs), **kw)
        tr.pretrain_g_rollout(x, a, s)
        seen = [tr.sched_sampling_last()]
        for _ in range(3):
            frames = tr.train_g_rollout(x, a, s)
            seen.append(tr.sched_sampling_last())
        assert tr.sched_sampling_state() == (SS_SEED, 4)
        got[graphs] = (frames, {n: sess.get_value(v).cpu().clone() for n, v in G.get_default_graph().variables.items()}, seen)
        sess.close()
    for graphs in (False, True):
        for k, last in enumerate(got[graphs][2]):
            prob = R.probability32('linear', k, 0.75, 0.25, 4, 1)
            assert last['prob'] == float(prob), (graphs, k, last['prob'], prob)
            assert np.array_equal(last['mask'], R.coins(SS_SEED, k, 0, K - 1, B, prob)), (graphs, k)
        masks = [m['mask'].tobytes() for m in got[graphs][2][1:]]
        assert len(set(masks)) == 3, 'three G steps drew the same coins'
    assert np.array_equal(got[False][0], got[True][0])
    assert all(torch.equal(got[False][1][n], got[True][1][n]) for n in got[True][1])


def test_checkpoint_continues_the_coins(tmp_path):
    x, a, s = _inputs(B, K, seed=6)
    kw = dict(sched_sampling='constant', ss_start=0.5, ss_seed=SS_SEED)
    sess, tr, _ = _trainer(**kw)
    for _ in range(2):
        tr.train_g_rollout(x, a, s)
    path = Saver().save(sess, str(tmp_path / 'model2'))
    assert 'state:g/sched_sampling/state' in np.load(path).files
    frames = tr.train_g_rollout(x, a, s)
    third = tr.sched_sampling_last()
    assert tr.sched_sampling_state() == (SS_SEED, 3) and np.array_equal(third['mask'], R.coins(SS_SEED, 2, 0, K - 1, B, np.float32(0.5)))
    sess.close()
    sess, tr, _ = _trainer(sched_sampling='constant', ss_start=0.5, ss_seed=SS_SEED + 1)          # (its own seed is overwritten too)
    Saver().restore(sess, str(tmp_path / 'model2'))
    assert tr.sched_sampling_state() == (SS_SEED, 2)
    again = tr.train_g_rollout(x, a, s)
    assert np.array_equal(tr.sched_sampling_last()['mask'], third['mask']) and np.array_equal(_bits(again), _bits(frames))
    sess.close()


def test_a_checkpoint_without_the_state_starts_the_counter_at_0(tmp_path):
    sess, tr, _ = _trainer()
    path = Saver().save(sess, str(tmp_path / 'plain'))
    assert not any('sched_sampling' in k for k in np.load(path).files)
    sess.close()
    sess, tr, _ = _trainer(sched_sampling='constant', ss_start=0.5, ss_seed=SS_SEED)
    Saver().restore(sess, str(tmp_path / 'plain'))
    assert tr.sched_sampling_state() == (SS_SEED, 0)
    sess.close()


def test_train_logs_a_decaying_probability(tmp_path):
    """train() with a log interval of 1: the pretraining update is teacher-forced (the offset), then the decay over 2 iterations."""
    tr = T.train('synthetic', None, None, str(tmp_path), None, True, 'bce', 'adam', True, batch_size=4, train_iter=5, pretrain_iter=1,
                 log_every=1, eval_every=0, quiet=True, rollout_steps=3, sched_sampling='linear', ss_decay_steps=2, ss_seed=3)
    tr.sess.close()
    rec = [json.loads(l) for l in open(tmp_path / 'train.jsonl')]
    assert [r['iteration'] for r in rec] == [0, 1, 2, 3, 4] and [r['ss_prob'] for r in rec] == [1.0, 1.0, 0.5, 0.0, 0.0]
    assert 'pretrain_g_loss' in rec[0] and all(np.isfinite(r['g_loss']) for r in rec[1:])


def test_cli_train_with_scheduled_sampling_then_evaluate(tmp_path):
    out, ev = tmp_path / 'run', tmp_path / 'eval'
    T.main(['synthetic', str(out), '--dna', '--adv', 'True', '--rollout_steps', '3', '--sched_sampling', 'linear', '--ss_decay_iters', '4',
            '--batch_size', '8', '--pretrain_iter', '1', '--train_iter', '4'])
    rec = [json.loads(l) for l in open(out / 'logs' / 'train.jsonl')]
    probs = [r['ss_prob'] for r in rec]
    assert rec and all(a >= b for a, b in zip(probs, probs[1:])), probs
    assert all(r['ss_prob'] == 1.0 for r in rec if r['iteration'] <= 1)                  # the offset: pretraining is teacher-forced
    assert all(np.isfinite(v) for r in rec for k, v in r.items() if 'loss' in k)
    E.main([str(out / 'models'), 'synthetic', str(ev), '--dna', '--num_sequences', '16'])
    got = json.load(open(ev / 'metrics.json'))
    assert got['sequences'] == 16 and all(np.isfinite(got[k]).all() for k in ('ssim', 'psnr'))


def test_library_exports_the_new_entries():
    lib = _lib.get()
    assert all(hasattr(lib, n) for n in ('sched_sample_draw', 'sched_sample_fwd', 'sched_sample_bwd'))
    assert {'acg_sched_sample_draw', 'acg_sched_sample_fwd', 'acg_sched_sample_bwd'} <= set(_lib.EXTENSIONS['rollout'].signatures)
    assert lib.version() == 8 == _lib.ABI_VERSION
