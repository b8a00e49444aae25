"""GPU: planning with the generator (include/acgan_rollout.h acg_plan_sample / acg_plan_cost / acg_plan_refit; plan.Planner and
its CLI).  The three kernels against the float64 restatement of tests/plan_ref.py, their replay in one captured graph, and the
Planner end to end.  Every output buffer is sentinel-filled with a guard band behind it.

SAMPLE: compared absolutely.  z is within 1e-5 of its float64 value (the bound derived in test_gpu_noise.py); the fused multiply-add
and the float32 inputs add 2.4e-7 relative to |mean| + |std z|: |delta| <= 1e-5 std + 2.4e-7 (|mean| + |std z|) per element.
Measured on an MI355X over the four shapes: 1.22e-6 at most ((1024, 16, 8); 6.0e-7 at (64, 5, 5), 2.5e-7 at (3, 2, 5)); asserted:
min(4 x that, the bound).  An element whose float64
value lies beyond lo / hi by more than the tolerance must equal the bound bitwise.

COST: relative 1e-5 against float64 of the same (stored) inputs.  Per thread at most 64 sequential fused multiply-adds of
non-negative terms, then a tree over 64 lanes and 4 waves: (64 + 6 + 4 + 3) * 2^-24 < 5e-6 at worst, about 2e-6 with the
squares' own rounding in practice.  Measured over the four shapes, both storage types, four weight pairs and both accumulate
modes: 1.50e-7 at most ((130, 16, 16, 3, 3, 0), bf16); asserted: the 1e-5.

REFIT: elite_idx exactly; mean and std within min(4 x measured, 2e-4 max|action|): two sequential float32 sums of at most 1024
terms, 1024 * 2^-24 = 6.1e-5 relative at worst.  Measured: 2.71e-7 at most (the std of N = E = 1000; 1.47e-7 at N = 1024, E = 100)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import noise_ref
import plan_ref as R

from action_conditioned_gans_amd import _lib
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import plan as P
from action_conditioned_gans_amd import train as T

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = np.float32(-7.25)
GUARD = 64
MEASURED_SAMPLE = 1.22e-6     # the largest errors seen on an MI355X (the docstring)
MEASURED_COST = 1.50e-7
MEASURED_REFIT = 2.71e-7
COST_RTOL = 1e-5
Z_BOUND = 1e-5 + 2.4e-7 * 5.77          # the sample bound at mean 0, std 1: |z| <= 5.77


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV).to(dtype).contiguous()


def _guarded(n, dtype=torch.float32, fill=float(SENTINEL)):
    """-> (the whole buffer, its first n elements): n elements to write and GUARD sentinels behind them."""
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[:n]


def _guard_intact(buf, n, fill=float(SENTINEL)):
    tail = buf[n:].cpu().numpy()
    return np.array_equal(tail, np.full(GUARD, fill, tail.dtype))


def _i64(v):
    return v - 2 ** 64 if v >= 2 ** 63 else v


def _state(seed, counter):
    return torch.tensor([_i64(seed), _i64(counter)], dtype=torch.int64, device=DEV)


def _read_state(state):
    return tuple(int(v) % 2 ** 64 for v in state.cpu().numpy())


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _differ(a, b):
    """Two independent draws: (almost) no element in common."""
    return float((np.asarray(a) != np.asarray(b)).mean()) > 0.99


# ---- sample ----------------------------------------------------------------------------------------------------------------------
SEED, COUNTER = 0x123456789abcdef, 2 ** 32 + 5


def _sample_inputs(h, a, seed=0):
    rng = np.random.default_rng(300 + seed)
    mean = rng.uniform(-0.5, 0.5, (h, a)).astype(np.float32)
    std = rng.uniform(0.1, 1.0, (h, a)).astype(np.float32)
    lo = rng.uniform(-0.9, -0.6, a).astype(np.float32)
    hi = rng.uniform(0.5, 0.8, a).astype(np.float32)
    return mean, std, lo, hi


def _draw(shape, mean, std, lo, hi, seed=SEED, counter=COUNTER, stream_id=3, keep_mean=True, state=None):
    n = int(np.prod(shape))
    buf, out = _guarded(n)
    state = _state(seed, counter) if state is None else state
    P.sample_actions(_dev(mean), _dev(std), _dev(lo), _dev(hi), state, out.view(shape), keep_mean=keep_mean, stream_id=stream_id)
    torch.cuda.synchronize()
    assert _guard_intact(buf, n), 'written behind the candidates'
    return out.cpu().numpy().reshape(shape), state


@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 2, 5), (64, 5, 5), (1024, 16, 8)], ids=str)
@pytest.mark.parametrize('keep_mean', [True, False])
def test_sample_matches_the_restatement(shape, keep_mean):
    n, h, a = shape
    mean, std, lo, hi = _sample_inputs(h, a, seed=n)
    got, state = _draw(shape, mean, std, lo, hi, keep_mean=keep_mean)
    assert _read_state(state) == (SEED, COUNTER + 1)                       # the counter advanced, the seed is untouched
    want, noise = R.unclamped(mean, std, SEED, COUNTER, shape, stream_id=3, keep_mean=keep_mean)
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    bound = 1e-5 * std.astype(np.float64)[None] + 2.4e-7 * (np.abs(mean.astype(np.float64))[None] + np.abs(noise))
    err = np.abs(got.astype(np.float64) - np.clip(want, lo64, hi64))
    print('plan_sample %s keep_mean=%s: max |delta| = %.3e (bound at that element %.3e, measured constant %r)'
          % (shape, keep_mean, err.max(), bound.reshape(-1)[err.argmax()], MEASURED_SAMPLE))
    tol = np.minimum(4 * MEASURED_SAMPLE, bound)
    assert (err <= tol).all(), (shape, err.max())
    above, below = want > hi64 + tol, want < lo64 - tol
    assert np.array_equal(_bits(got[above]), _bits(np.broadcast_to(hi, shape)[above]))
    assert np.array_equal(_bits(got[below]), _bits(np.broadcast_to(lo, shape)[below]))
    if n >= 64:
        assert above.any() and below.any() and (~above & ~below).any()
    if keep_mean:
        assert np.array_equal(_bits(got[0]), _bits(np.minimum(np.maximum(mean, lo), hi)))
    # the same state again: the same bits
    again, _ = _draw(shape, mean, std, lo, hi, keep_mean=keep_mean)
    assert np.array_equal(_bits(again), _bits(got))


def test_sample_counter_stream_id_and_tag():
    shape = (64, 5, 5)
    mean, std = np.zeros((5, 5), np.float32), np.ones((5, 5), np.float32)
    lo, hi = np.full(5, -1e30, np.float32), np.full(5, 1e30, np.float32)
    state = _state(7, 0)
    outs = [_draw(shape, mean, std, lo, hi, keep_mean=False, stream_id=0, state=state)[0] for _ in range(3)]
    assert _read_state(state) == (7, 3)
    for i, out in enumerate(outs):                       # launch i drew with counter i
        want = R.sample(mean, std, lo, hi, 7, i, shape, stream_id=0, keep_mean=False)
        assert np.abs(out - want).max() <= Z_BOUND, i
    assert _differ(outs[0], outs[1]) and _differ(outs[1], outs[2]) and _differ(outs[0], outs[2])
    other, _ = _draw(shape, mean, std, lo, hi, seed=7, counter=0, keep_mean=False, stream_id=1)
    assert _differ(other, outs[0])                       # two stream ids: different draws
    # the noise input's draw for the same {seed, counter, stream_id}: other values - what ACG_PLAN_STREAM_TAG is for
    n = int(np.prod(shape))
    b, z, a = 25, 64, 1
    noise_out = torch.zeros(b, a + z, device=DEV)
    nstate = _state(7, 0)
    _lib.get().noise_concat(_p(torch.zeros(b, a, device=DEV)), _p(nstate), _p(torch.ones(1, device=DEV)), _p(noise_out), b, a, z, 0, _stream())
    torch.cuda.synchronize()
    noise_z = noise_out[:, a:].cpu().numpy().reshape(-1)
    assert np.abs(noise_z - noise_ref.normals(7, 0, 0, n)).max() <= Z_BOUND       # (the noise draw is what it always was)
    assert _differ(noise_z, outs[0].reshape(-1))


# ---- cost ------------------------------------------------------------------------------------------------------------------------
COST_SHAPES = [(1, 1, 1, 1, 1, 0), (3, 5, 7, 3, 3, 5), (2, 64, 64, 3, 4, 5), (130, 16, 16, 3, 3, 0)]


def _cost_inputs(shape, dtype):
    n, h, w, c, pitch, s = shape
    rng = np.random.default_rng(sum(shape))
    frames = rng.uniform(-1, 1, (n, h, w, pitch)).astype(np.float32)
    frames[..., c:] = 1e30                                # garbage in the pad channels: never scored
    goal = rng.uniform(-1, 1, (h, w, c)).astype(np.float32)
    states = rng.standard_normal((n, s)).astype(np.float32) if s else None
    goal_state = rng.standard_normal(s).astype(np.float32) if s else None
    ft = _dev(frames, dtype)
    stored = ft.float().cpu().numpy().astype(np.float64)           # bf16: the restatement reads the rounded values
    return ft, stored, goal, states, goal_state


@pytest.mark.parametrize('shape', COST_SHAPES, ids=str)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_cost_matches_float64(shape, dtype):
    n, h, w, c, pitch, s = shape
    ft, stored, goal, states, goal_state = _cost_inputs(shape, dtype)
    gt, st, gst = _dev(goal), (_dev(states) if s else None), (_dev(goal_state) if s else None)
    old = np.random.default_rng(5).uniform(1.0, 50.0, n).astype(np.float32)
    worst = 0.0
    for fw, sw in ((1.0, 0.0), (0.5, 2.0), (0.0, 1.5), (0.0, 0.0)):
        for accumulate in (False, True):
            buf, cost = _guarded(n, fill=float('nan'))             # accumulate = 0: the NaNs in the buffer must not survive
            if accumulate:
                cost.copy_(_dev(old))
            P.accumulate_cost(ft, gt, cost, states=st, goal_state=gst, frame_weight=fw, state_weight=sw, accumulate=accumulate, channels=c)
            first = cost.cpu().numpy().copy()
            assert np.isnan(buf[n:].cpu().numpy()).all(), 'written behind the costs'
            want = R.cost(stored, goal, states, goal_state, fw, sw, old=old if accumulate else None, channels=c)
            err = np.abs(first.astype(np.float64) - want)
            rel = float((err / np.maximum(np.abs(want), 1e-300)).max()) if (want != 0).any() else 0.0
            worst = max(worst, rel)
            assert (err <= COST_RTOL * np.abs(want)).all(), (shape, fw, sw, accumulate, rel)
            if accumulate:
                cost.copy_(_dev(old))
            P.accumulate_cost(ft, gt, cost, states=st, goal_state=gst, frame_weight=fw, state_weight=sw, accumulate=accumulate, channels=c)
            assert np.array_equal(_bits(cost.cpu().numpy()), _bits(first))                # two launches, the same bits
    print('plan_cost %s %s: max relative error %.3e (asserted %.0e, measured constant %r)' % (shape, dtype, worst, COST_RTOL, MEASURED_COST))


def test_cost_loader_paths_agree_to_the_bit():
    """One frame set through the dense 16-byte loader (pitch 3, 64 x 64), the pitch-4 pixel loader and the scalar loader (pitch 5)
    gives the same terms in another order, so each is held to the float64 value, as is the dense layout at a base address that
    is no multiple of 16 bytes (the scalar loader again)."""
    rng = np.random.default_rng(77)
    frames, goal = rng.uniform(-1, 1, (5, 64, 64, 3)).astype(np.float32), rng.uniform(-1, 1, (64, 64, 3)).astype(np.float32)
    want = R.cost(frames, goal)
    gt = _dev(goal)
    for pitch in (3, 4, 5):
        padded = np.concatenate([frames, np.full((5, 64, 64, pitch - 3), 1e30, np.float32)], axis=-1)
        cost = torch.empty(5, device=DEV)
        P.accumulate_cost(_dev(padded), gt, cost, channels=3)
        assert (np.abs(cost.cpu().numpy() - want) <= COST_RTOL * want).all(), pitch
    shifted = torch.empty(frames.size + 1, device=DEV)[1:]            # 4 bytes off a 16-byte boundary
    shifted.copy_(_dev(frames).view(-1))
    cost = torch.empty(5, device=DEV)
    P.accumulate_cost(shifted.view(5, 64, 64, 3), gt, cost)
    assert (np.abs(cost.cpu().numpy() - want) <= COST_RTOL * want).all()


# ---- refit -----------------------------------------------------------------------------------------------------------------------
class Refit:
    """One call site of acg_plan_refit: guarded device buffers and the float64 restatement on the same inputs."""

    def __init__(self, n, e, h, a, costs=None, seed=0):
        rng = np.random.default_rng(900 + seed + n)
        self.n, self.e, self.h, self.a = n, e, h, a
        self.actions = rng.uniform(-1, 1, (n, h, a)).astype(np.float32)
        self.costs = rng.uniform(0, 10, n).astype(np.float32) if costs is None else np.asarray(costs, np.float32)
        self.mean0 = rng.uniform(-0.5, 0.5, (h, a)).astype(np.float32)
        self.std0 = rng.uniform(0.2, 1.0, (h, a)).astype(np.float32)
        ha = h * a
        self.bufs = {k: _guarded(m) for k, m in (('mean', ha), ('std', ha), ('best_cost', 1), ('best_actions', ha), ('history', 1))}
        self.elite_buf, self.elite = _guarded(e, dtype=torch.int32, fill=-7)
        self.d_actions, self.d_costs = _dev(self.actions), _dev(self.costs)
        self.reset()

    def reset(self, best_cost=np.inf, best_actions=None):
        self.bufs['mean'][1].copy_(_dev(self.mean0).view(-1))
        self.bufs['std'][1].copy_(_dev(self.std0).view(-1))
        self.bufs['best_cost'][1].fill_(float(best_cost))
        self.best0 = np.full((self.h, self.a), 0.125, np.float32) if best_actions is None else best_actions
        self.bufs['best_actions'][1].copy_(_dev(self.best0).view(-1))
        self.best_cost0 = best_cost

    def launch(self, alpha, min_std, history=True):
        v = {k: b[1] for k, b in self.bufs.items()}
        P.refit(self.d_costs, self.d_actions, v['mean'], v['std'], v['best_cost'], v['best_actions'], self.elite, alpha, min_std,
                history=v['history'] if history else None)
        torch.cuda.synchronize()
        for k, (buf, view) in self.bufs.items():
            assert _guard_intact(buf, view.numel()), 'written behind ' + k
        assert _guard_intact(self.elite_buf, self.e, fill=-7), 'written behind elite_idx'
        out = {k: view.cpu().numpy().copy() for k, (_, view) in self.bufs.items()}
        out['elite_idx'] = self.elite.cpu().numpy().copy()
        return out

    def want(self, alpha, min_std):
        return R.refit(self.costs, self.actions, self.mean0, self.std0, self.e, alpha, min_std, self.best_cost0, self.best0)


TIES = [3.0, 1.0, np.nan, 1.0, np.inf, 0.5, 3.0]
REFIT_CASES = [(1, 1, 1, 1, None), (7, 3, 2, 5, TIES), (1024, 100, 16, 8, None), (1000, 1000, 3, 5, None)]


@pytest.mark.parametrize('n,e,h,a,costs', REFIT_CASES, ids=lambda v: str(v) if isinstance(v, int) else ('ties' if v else 'random'))
@pytest.mark.parametrize('alpha', [0.0, 0.5])
def test_refit_matches_the_restatement(n, e, h, a, costs, alpha):
    call = Refit(n, e, h, a, costs)
    min_std = 0.3                                       # above some of the refitted deviations, below others
    got, want = call.launch(alpha, min_std), call.want(alpha, min_std)
    assert np.array_equal(got['elite_idx'], want['elite_idx'])
    if costs is TIES:
        assert got['elite_idx'].tolist() == [5, 1, 3]                      # equal costs: the lower index first
    scale = float(np.abs(call.actions).max())
    err_m = np.abs(got['mean'].reshape(h, a) - want['mean']).max()
    err_s = np.abs(got['std'].reshape(h, a) - want['std']).max()
    print('plan_refit N=%d E=%d H=%d A=%d alpha=%g: max |mean - float64| = %.3e, |std - float64| = %.3e (bound %.3e, measured constant %r)'
          % (n, e, h, a, alpha, err_m, err_s, 2e-4 * scale, MEASURED_REFIT))
    tol = min(4 * MEASURED_REFIT, 2e-4 * scale)
    assert err_m <= tol and err_s <= tol
    # the floor is exact: where the float64 value before the floor is clearly below it, the result IS min_std
    free = R.refit(call.costs, call.actions, call.mean0, call.std0, e, alpha, 0.0)['std']
    floored = free < min_std - tol
    assert np.array_equal(_bits(got['std'].reshape(h, a)[floored]), _bits(np.full(int(floored.sum()), min_std, np.float32)))
    if n == 1 and alpha == 0.0:
        assert floored.all()                                               # one elite has no deviation
    # the best plan: the candidate of rank 0, its cost and its actions bit for bit; history holds the cost
    first = int(want['elite_idx'][0])
    assert np.array_equal(_bits(got['best_cost']), _bits(call.costs[first:first + 1]))
    assert np.array_equal(_bits(got['best_actions']), _bits(call.actions[first].reshape(-1)))
    assert np.array_equal(_bits(got['history']), _bits(got['best_cost']))
    call.reset()
    again = call.launch(alpha, min_std)
    for k in got:                                                          # two launches, the same bits
        assert np.array_equal(got[k].view(np.uint32) if got[k].dtype == np.float32 else got[k],
                              again[k].view(np.uint32) if again[k].dtype == np.float32 else again[k]), k


def test_refit_updates_the_best_plan_on_strict_improvement_only():
    call = Refit(7, 3, 2, 5, TIES)
    marker = np.full((2, 5), 0.375, np.float32)
    prev_history = np.array([SENTINEL])
    for best, takes in ((0.5, False), (0.25, False), (0.75, True), (np.inf, True), (np.nan, False)):
        call.reset(best_cost=best, best_actions=marker)
        got = call.launch(0.5, 0.05, history=(best != 0.25))               # (once without a history pointer)
        if takes:
            assert got['best_cost'][0] == np.float32(0.5) and np.array_equal(_bits(got['best_actions']), _bits(call.actions[5].reshape(-1)))
        else:
            assert np.array_equal(_bits(got['best_cost']), _bits(np.array([best], np.float32)))
            assert np.array_equal(_bits(got['best_actions']), _bits(marker.reshape(-1)))
        if best != 0.25:
            assert np.array_equal(_bits(got['history']), _bits(got['best_cost']))
        else:
            assert np.array_equal(_bits(got['history']), _bits(prev_history))      # not written
        prev_history = got['history']
    # every cost NaN: the first E candidates by index, a finite refit, the best plan untouched
    nan_call = Refit(7, 3, 2, 5, [np.nan] * 7)
    nan_call.reset(best_actions=marker)
    got, want = nan_call.launch(0.5, 0.05), nan_call.want(0.5, 0.05)
    assert got['elite_idx'].tolist() == [0, 1, 2] and np.isfinite(got['mean']).all() and np.isfinite(got['std']).all()
    assert np.abs(got['mean'].reshape(2, 5) - want['mean']).max() <= 2e-4 and np.abs(got['std'].reshape(2, 5) - want['std']).max() <= 2e-4
    assert np.isposinf(got['best_cost'][0]) and np.isposinf(got['history'][0])
    assert np.array_equal(_bits(got['best_actions']), _bits(marker.reshape(-1)))


# ---- refused arguments: AcgError, nothing launched -------------------------------------------------------------------------------
def _untouched(*bufs):
    torch.cuda.synchronize()
    return all(np.array_equal(_bits(b.cpu().numpy()), _bits(np.full(b.numel(), SENTINEL))) for b in bufs)


@pytest.mark.parametrize('over', [dict(n=0), dict(n=1025), dict(h=0), dict(h=17), dict(a=0), dict(a=9), dict(mean=None), dict(state=None),
                                  dict(actions=None), dict(lo=None)], ids=str)
def test_sample_refuses_out_of_range_arguments(over):
    lib = _lib.get()
    out = torch.full((1024,), float(SENTINEL), device=DEV)
    vec = torch.full((128,), float(SENTINEL), device=DEV)
    state = _state(7, 5)
    kw = dict(mean=vec, std=vec, lo=vec, hi=vec, state=state, actions=out, n=2, h=2, a=5)
    kw.update(over)
    with pytest.raises(_lib.AcgError, match='plan_sample'):
        lib.plan_sample(_p(kw['mean']), _p(kw['std']), _p(kw['lo']), _p(kw['hi']), _p(kw['state']), _p(kw['actions']), kw['n'], kw['h'],
                        kw['a'], 1, 0, _stream())
    assert _untouched(out) and _read_state(state) == (7, 5)


@pytest.mark.parametrize('over', [dict(n=0), dict(n=1025), dict(h=0), dict(w=0), dict(c=0), dict(c=4, pitch=3), dict(pitch=65, c=3),
                                  dict(s=17), dict(s=0), dict(states=None), dict(goal_state=None), dict(dtype=2), dict(frames=None),
                                  dict(goal=None), dict(cost=None)], ids=str)
def test_cost_refuses_out_of_range_arguments(over):
    lib = _lib.get()
    cost = torch.full((8,), float(SENTINEL), device=DEV)
    x = torch.zeros(4096, device=DEV)
    kw = dict(frames=x, goal=x, states=x, goal_state=x, cost=cost, n=2, h=4, w=4, c=3, pitch=3, s=5, dtype=_lib.ACG_F32)
    kw.update(over)
    with pytest.raises(_lib.AcgError, match='plan_cost'):
        lib.plan_cost(_p(kw['frames']), _p(kw['goal']), _p(kw['states']), _p(kw['goal_state']), 1.0, 1.0, _p(kw['cost']), 0, kw['n'],
                      kw['h'], kw['w'], kw['c'], kw['pitch'], kw['s'], kw['dtype'], _stream())
    assert _untouched(cost)


@pytest.mark.parametrize('over', [dict(n=0), dict(n=1025), dict(h=0), dict(h=17), dict(a=0), dict(a=9), dict(e=0), dict(e=8), dict(alpha=-0.1),
                                  dict(alpha=1.5), dict(alpha=float('nan')), dict(min_std=-1.0), dict(min_std=float('inf')), dict(cost=None),
                                  dict(actions=None), dict(mean=None), dict(std=None), dict(best_cost=None), dict(best_actions=None),
                                  dict(elite_idx=None)], ids=str)
def test_refit_refuses_out_of_range_arguments(over):
    lib = _lib.get()
    outs = {k: torch.full((128,), float(SENTINEL), device=DEV) for k in ('mean', 'std', 'best_cost', 'best_actions', 'history')}
    elite = torch.full((1024,), -7, dtype=torch.int32, device=DEV)
    x = torch.zeros(1024 * 128, device=DEV)
    kw = dict(cost=x, actions=x, elite_idx=elite, n=7, h=2, a=5, e=3, alpha=0.5, min_std=0.1, **outs)
    kw.update(over)
    with pytest.raises(_lib.AcgError, match='plan_refit'):
        lib.plan_refit(_p(kw['cost']), _p(kw['actions']), _p(kw['mean']), _p(kw['std']), _p(kw['best_cost']), _p(kw['best_actions']),
                       _p(kw['elite_idx']), _p(kw['history']), kw['n'], kw['h'], kw['a'], kw['e'], kw['alpha'], kw['min_std'], _stream())
    assert _untouched(*outs.values()) and bool((elite == -7).all())


# ---- replay ----------------------------------------------------------------------------------------------------------------------
def test_three_replays_of_one_captured_round_equal_three_eager_rounds():
    """sample -> cost -> refit as one linear captured graph on one stream.  The candidates themselves are the 'frames' the cost
    reads (an H x A image of one channel), so every launch depends on the one before it."""
    N, H, A, E = 64, 5, 5, 8
    rng = np.random.default_rng(41)
    lo, hi = _dev(np.full(A, -1.0)), _dev(np.full(A, 1.0))
    goal = _dev(rng.uniform(-0.5, 0.5, (H, A, 1)))
    mean, std = torch.empty(H, A, device=DEV), torch.empty(H, A, device=DEV)
    best_cost, best_actions = torch.empty(1, device=DEV), torch.empty(H, A, device=DEV)
    actions, cost = torch.empty(N, H, A, device=DEV), torch.empty(N, device=DEV)
    elite, history = torch.empty(E, dtype=torch.int32, device=DEV), torch.empty(1, device=DEV)
    state = _state(11, 0)
    outputs = (actions, cost, mean, std, best_cost, best_actions, elite, history)

    def reset():
        mean.zero_(), std.fill_(0.5), best_cost.fill_(float('inf')), best_actions.zero_(), state.copy_(_state(11, 0))

    def one_round():
        P.sample_actions(mean, std, lo, hi, state, actions)
        P.accumulate_cost(actions.view(N, H, A, 1), goal, cost)
        P.refit(cost, actions, mean, std, best_cost, best_actions, elite, 0.25, 0.05, history=history)

    def snapshot():
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in outputs]

    reset()
    eager = []
    for _ in range(3):
        one_round()
        eager.append(snapshot())
    assert _read_state(state) == (11, 3)
    reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one_round()
    reset()                                  # (capturing launches nothing; reset again all the same)
    torch.cuda.synchronize()
    for i in range(3):
        graph.replay()
        for got, want in zip(snapshot(), eager[i]):
            assert np.array_equal(got.view(np.uint32) if got.dtype == np.float32 else got,
                                  want.view(np.uint32) if want.dtype == np.float32 else want), i
    assert _read_state(state) == (11, 3)
    assert eager[2][7][0] <= eager[1][7][0] <= eager[0][7][0] and not np.array_equal(eager[0][0], eager[1][0])


# ---- Planner end to end ------------------------------------------------------------------------------------------------------
B, S, H, E, I = 4, 64, 2, 2, 3


def _trainer(model, **kw):
    G.reset_default_graph()
    sess = G.Session(device=DEV)
    tr = T.Trainer(sess, False, 'bce', 'adam', {'dna': True, 'plain': False, 'cdna': 'cdna'}[model], batch_size=B, img_size=S, lookahead=False,
                   **kw)
    sess.run(G.global_variables_initializer())
    return sess, tr


def _scene(seed=51):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (S, S, 3)).astype(np.float32), rng.standard_normal(5).astype(np.float32),
            rng.uniform(-1, 1, (S, S, 3)).astype(np.float32), rng.standard_normal(5).astype(np.float32))


def _check_history(res):
    h = res['history']
    assert h.shape == (I,) and np.isfinite(h).all() and (np.diff(h) <= 0).all() and res['cost'] == h[-1]


def test_planner_end_to_end_dna():
    sess, tr = _trainer('dna')
    frame, state, goal, goal_state = _scene()
    kw = dict(init_std=0.5, min_std=0.05, alpha=0.25, state_weight=0.5, seed=77)
    planner = P.Planner(tr, H, E, I, **kw)
    res = planner.plan(frame, state, goal, goal_state=goal_state, keep_candidates=True)
    assert planner.plan_state() == (77, I)                                  # one draw per iteration
    assert res['candidates'].shape == (I, B, H, 5) and res['costs'].shape == (I, B) and res['elites'].shape == (I, E)
    assert res['means'].shape == res['stds'].shape == (I, H, 5) and res['actions'].shape == res['mean'].shape == res['std'].shape == (H, 5)
    _check_history(res)
    assert np.array_equal(_bits(res['mean']), _bits(res['means'][-1])) and np.array_equal(_bits(res['std']), _bits(res['stds'][-1]))
    assert np.array_equal(_bits(res['history']), _bits(np.minimum.accumulate(res['costs'].min(axis=1))))
    assert res['history'][0] <= res['costs'][0][0]                          # the mean row of the first round is a candidate
    assert not res['candidates'][0][0].any()                                # ... and it is the zero sequence
    it, row = np.unravel_index(np.argmin(res['costs']), res['costs'].shape)      # the first to attain the minimum (C order)
    assert np.float32(res['cost']) == res['costs'].min() and np.array_equal(_bits(res['actions']), _bits(res['candidates'][it][row]))
    mean, std = np.zeros((H, 5)), np.full((H, 5), 0.5)
    zeros = np.zeros((B, 1, S, S, 3), np.float32)
    for i in range(I):
        # the same batch through the same kernels, without the sampling: the same bits
        again, frames = planner.evaluate_actions(frame, state, res['candidates'][i], goal, goal_state=goal_state, return_frames=True)
        assert np.array_equal(_bits(again), _bits(res['costs'][i])), i
        assert frames.shape == (B, H, S, S, 3) and np.isfinite(frames).all()
        # the host loop - Trainer.test step by step, as test_sequence(device_loop=False) - and the float64 cost of ITS frames
        cur, st, want = np.broadcast_to(frame, (B, S, S, 3)).copy(), np.broadcast_to(state, (B, 5)).copy(), np.zeros(B)
        for t in range(H):
            acs = np.concatenate([res['candidates'][i][:, t], st], axis=1).astype(np.float32)
            cur, st, _ = tr.test(cur, zeros[:, 0], acs)
            want += R.cost(cur, goal, st, goal_state, 1.0, 0.5)
        assert (np.abs(res['costs'][i] - want) <= 1e-5 * want).all(), (i, np.abs(res['costs'][i] - want) / want)
        ref = R.refit(res['costs'][i], res['candidates'][i], mean, std, E, 0.25, 0.05)
        assert np.array_equal(res['elites'][i], ref['elite_idx']), i
        scale = float(np.abs(res['candidates'][i]).max())
        tol = min(4 * MEASURED_REFIT, 2e-4 * scale)
        assert np.abs(res['means'][i] - ref['mean']).max() <= tol and np.abs(res['stds'][i] - ref['std']).max() <= tol, i
        mean, std = res['means'][i].astype(np.float64), res['stds'][i].astype(np.float64)
        # the candidates are the restatement's draw around the distribution the round started from
        prev_m, prev_s = (np.zeros((H, 5), np.float32), np.full((H, 5), 0.5, np.float32)) if i == 0 else (res['means'][i - 1], res['stds'][i - 1])
        drawn = R.sample(prev_m, prev_s, np.full(5, -1.0), np.full(5, 1.0), 77, i, (B, H, 5))
        assert np.abs(res['candidates'][i] - drawn).max() <= Z_BOUND, i        # (std <= 1, |mean| <= 1: the bound of std 1 covers it)
    # the same seed again: the same bits; another seed: other candidates
    twin = P.Planner(tr, H, E, I, **kw).plan(frame, state, goal, goal_state=goal_state, keep_candidates=True)
    for k in res:
        assert np.array_equal(res[k], twin[k]), k
    other = P.Planner(tr, H, E, I, **dict(kw, seed=78)).plan(frame, state, goal, goal_state=goal_state, keep_candidates=True)
    assert not np.array_equal(other['candidates'][0][1:], res['candidates'][0][1:])
    # the stream goes on: a second plan of the same Planner draws with the next counters
    planner.plan(frame, state, goal, goal_state=goal_state)
    assert planner.plan_state() == (77, 2 * I)
    # cost_steps='last' scores the last frame only
    last = P.Planner(tr, H, E, 1, **dict(kw, cost_steps='last', state_weight=0.0))
    lres = last.plan(frame, state, goal, keep_candidates=True)
    _, frames = last.evaluate_actions(frame, state, lres['candidates'][0], goal, return_frames=True)
    want = R.cost(frames[:, -1], goal)
    assert (np.abs(lres['costs'][0] - want) <= COST_RTOL * want).all()
    with pytest.raises(ValueError, match='goal_state'):
        planner.plan(frame, state, goal)
    with pytest.raises(ValueError, match='frame'):
        planner.plan(frame[:32], state, goal, goal_state=goal_state)
    sess.close()


@pytest.mark.parametrize('model', ['cdna', 'plain'])
def test_planner_runs_with_the_other_generators(model):
    sess, tr = _trainer(model)
    frame, state, goal, goal_state = _scene(52)
    if model == 'plain':
        with pytest.raises(ValueError, match='state_weight'):
            P.Planner(tr, H, E, I, state_weight=1.0)
    res = P.Planner(tr, H, E, I, seed=3).plan(frame, state, goal, goal_state=goal_state)           # (goal_state is not read at weight 0)
    _check_history(res)
    assert np.abs(res['actions']).max() <= 1.0
    sess.close()


def test_planner_with_stored_batchnorm_statistics():
    sess, tr = _trainer('dna', bn_inference=True)
    frame, state, goal, _ = _scene(53)
    with pytest.raises(RuntimeError, match='uncalibrated'):
        P.Planner(tr, H, E, I, bn='stored').plan(frame, state, goal)
    rng = np.random.default_rng(54)
    for _ in range(2):
        tr.calibrate_bn(rng.uniform(-1, 1, (B, S, S, 3)).astype(np.float32), rng.standard_normal((B, 10)).astype(np.float32))
    planner = P.Planner(tr, H, E, I, bn='stored', seed=5)
    res = planner.plan(frame, state, goal, keep_candidates=True)
    _check_history(res)
    # stored statistics: a row's cost does not depend on its companions - the best plan alone in another batch costs the same
    rows = np.zeros((B, H, 5), np.float32)
    rows[B - 1] = res['actions']
    alone = planner.evaluate_actions(frame, state, rows, goal)
    assert abs(alone[B - 1] - res['cost']) <= 1e-5 * res['cost']
    sess_plain, tr_plain = _trainer('dna')
    with pytest.raises(RuntimeError, match='bn_inference'):
        P.Planner(tr_plain, H, E, I, bn='stored')
    sess.close()
    sess_plain.close()


def test_planner_with_the_averaged_weights():
    sess, tr = _trainer('dna', ema_decay=0.5)
    frame, state, goal, _ = _scene(55)
    with pytest.raises(RuntimeError, match='0 updates'):
        P.Planner(tr, H, E, I, weights='ema').plan(frame, state, goal)
    rng = np.random.default_rng(56)
    for _ in range(2):
        x = rng.uniform(-1, 1, (2, B, S, S, 3)).astype(np.float32)
        a = rng.standard_normal((B, 10)).astype(np.float32)
        tr.pretrain_g(x[0], x[1], a, a[:, 5:])
    raw = P.Planner(tr, H, E, I, seed=9).plan(frame, state, goal, keep_candidates=True)
    ema = P.Planner(tr, H, E, I, seed=9, weights='ema').plan(frame, state, goal, keep_candidates=True)
    _check_history(ema)
    assert np.array_equal(ema['candidates'][0], raw['candidates'][0]) and not np.array_equal(ema['costs'][0], raw['costs'][0])
    with tr.ema_weights():                               # the same call inside the context, as Trainer.test defines 'ema'
        inside = P.Planner(tr, H, E, I, seed=9).plan(frame, state, goal, keep_candidates=True)
    for k in ema:
        assert np.array_equal(ema[k], inside[k]), k
    again = P.Planner(tr, H, E, I, seed=9).plan(frame, state, goal, keep_candidates=True)      # the raw weights are back
    assert np.array_equal(_bits(again['costs']), _bits(raw['costs']))
    sess_plain, tr_plain = _trainer('dna')
    with pytest.raises(RuntimeError, match='ema_decay'):
        P.Planner(tr_plain, H, E, I, weights='ema')
    sess.close()
    sess_plain.close()


# ---- CLI -------------------------------------------------------------------------------------------------------------------------
def _train_checkpoint(root, dna, iters=2):
    model_dir = str(root / ('models_dna' if dna else 'models_plain'))
    os.makedirs(model_dir)
    tr = T.train('synthetic', None, None, None, model_dir, False, 'bce', 'adam', dna, batch_size=4, seq_len=5, train_iter=iters,
                 pretrain_iter=0, device=DEV, quiet=True, eval_every=0, log_every=1)
    tr.sess.close()
    return model_dir


def test_plan_cli_end_to_end(tmp_path):
    model_dir = _train_checkpoint(tmp_path, dna=True)
    out = tmp_path / 'plan'
    res = P.main([model_dir, 'synthetic', str(out), '--dna', '--candidates', '4', '--elites', '2', '--iterations', '2', '--horizon', '2',
                  '--num_sequences', '2', '--seq_len', '4', '--seed', '3', '--dump'])
    got = json.load(open(out / 'plan.json'))
    assert got == json.loads(json.dumps(res))
    assert got['model'] == 'dna' and got['ksize'] == 5 and got['num_masks'] is None
    assert os.path.basename(got['checkpoint']).startswith('model')
    assert got['sequences'] == 2 and len(got['plans']) == 2 and got['rollout_s'] > 0 and 0.0 <= got['share_not_worse_than_recorded'] <= 1.0
    s = got['settings']
    assert (s['candidates'], s['elites'], s['iterations'], s['horizon'], s['goal_step'], s['seed']) == (4, 2, 2, 2, 2, 3)
    assert s['cost_steps'] == 'all' and s['bn_stats'] == 'batch' and s['weights'] == 'raw' and s['state_weight'] == 0.0
    for p in got['plans']:
        assert np.asarray(p['actions']).shape == (2, 5) and len(p['history']) == 2 and p['history'][-1] == p['cost']
        assert p['history'][1] <= p['history'][0] and np.isfinite([p['cost'], p['recorded_cost'], p['zero_cost']]).all()
        assert p['cost'] <= p['zero_cost']               # zero is the mean row of the first round
    plans, frames = np.load(out / 'plans.npy'), np.load(out / 'plan_frames.npy')
    assert plans.shape == (2, 2, 5) and frames.shape == (2, 2, 64, 64, 3) and np.isfinite(frames).all()
    assert np.array_equal(plans, np.asarray([p['actions'] for p in got['plans']], np.float32))
    # a checkpoint of the other generator is refused, as evaluate refuses it
    plain_dir = _train_checkpoint(tmp_path, dna=False, iters=1)
    with pytest.raises(ValueError, match='checkpoint'):
        P.main([plain_dir, 'synthetic', str(tmp_path / 'bad'), '--dna', '--candidates', '4', '--elites', '2', '--horizon', '2', '--num_sequences', '1',
                '--seq_len', '4'])
    with pytest.raises(ValueError, match='calibrated'):
        P.main([model_dir, 'synthetic', str(tmp_path / 'bad2'), '--dna', '--bn_stats', 'stored', '--candidates', '4', '--elites', '2',
                '--horizon', '2', '--num_sequences', '1', '--seq_len', '4'])
