"""Plan actions with the generator: ``python -m action_conditioned_gans_amd.plan MODEL_PATH INPUT OUTPUT [options]``.

What an action-conditioned predictor is for (visual model-predictive control, the use the push dataset was recorded for): find
the commands that lead from a start frame to a goal frame.  The optimiser is the cross-entropy method (CEM): draw N candidate
command sequences of H steps from a diagonal Gaussian, roll each through the generator, score the predicted frames against the
goal, refit the Gaussian to the E best, repeat.  The N candidates are the rows of ONE batch of the Trainer's generator, and
everything around the generator forwards runs on the device too (include/acgan_rollout.h: acg_plan_sample / acg_plan_cost /
acg_plan_refit, csrc/plan.hip): no frame, no cost and no candidate comes to the host inside the loop.  There is no host
fallback: a library without the entries raises.

``sample_actions`` / ``accumulate_cost`` / ``refit`` are the three launches on torch device tensors; ``Planner`` is the loop
around a ``train.Trainer``; ``main`` plans for the sequences of a dataset and writes OUTPUT/plan.json.

INPUT is evaluate's: a frames ``.npy`` with ``--actions``, a push TFRecord directory, or ``synthetic``.  For each sequence the
start is frame 0 with the recorded state 0 and the goal is frame ``--goal_step`` (default: ``--horizon``) with its recorded
state (read when ``--state_weight`` > 0).  plan.json holds per sequence ``actions`` [horizon, 5], ``cost``, ``history`` (the
best cost after every iteration), ``recorded_cost`` (the dataset's own first ``horizon`` commands, row 0 of one
``evaluate_actions`` batch whose other rows are zero commands) and ``zero_cost`` (the all-zero command sequence: the mean row
of the first round, the initial mean being 0 - scored in the batch the plan competed in, so ``cost <= zero_cost`` always);
and ``share_not_worse_than_recorded``, every setting, ``model`` / ``num_masks`` / ``ksize`` / ``checkpoint`` as evaluate's
metrics.json records them, and ``rollout_s``, the time spent in ``plan``.  With ``--bn_stats batch`` a row's prediction depends
on the other rows of its batch, so costs of different batches compare only roughly; ``--bn_stats stored`` makes them exact.
``--dump`` also writes ``plans.npy`` [n, horizon, 5] and ``plan_frames.npy`` [n, horizon, H, W, 3], the frames predicted for
each plan (row 0 of a batch whose other rows are zero commands).

Not covered: a designated-pixel or mask cost (the cost is the squared error of whole frames, plus the state's); replanning
against a simulator or a robot (one open-loop plan per call); sampling the generator's noise (z = 0 always); gradient-based
refinement of the plan; more than one rank; bf16 end to end (the cost kernel reads bf16 frames, a bf16 Planner was never run).
"""
import argparse
import ctypes
import json
import math
import os
import time

import numpy as np
import torch

from . import _lib
from .metrics import _stream_handle
from .ops import read_draw_state, write_draw_state

COMMAND_DIM = 5             # the commanded half of the 10-dim action vector; columns 5..9 are the state
COST_STEPS = ('all', 'last')
DEFAULTS = {'init_std': 0.5, 'min_std': 0.05, 'alpha': 0.1, 'lo': -1.0, 'hi': 1.0}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _device_f32(what, **tensors):
    dev = None
    for name, t in tensors.items():
        if t is None:
            continue
        if not torch.is_tensor(t):
            raise TypeError('%s takes device tensors (%s is %s)' % (what, name, type(t).__name__))
        if t.device.type != 'cuda' or (dev is not None and t.device != dev):
            raise ValueError('%s: every tensor must be on one GPU (%s is on %s)' % (what, name, t.device))
        if not t.is_contiguous():
            raise ValueError('%s: %s must be contiguous' % (what, name))
        dev = t.device
    return dev


def _want(what, name, t, dtype, numel):
    if t.dtype != dtype or t.numel() != numel:
        raise ValueError('%s: %s must be %s with %d elements, got %s %s' % (what, name, dtype, numel, t.dtype, tuple(t.shape)))


def sample_actions(mean, std, lo, hi, state, actions, keep_mean=True, stream_id=0, stream=None, lib=None):
    """``actions`` [N, H, A] (float32, written) = clamp(mean + std * z, lo, hi) with z ~ N(0, 1) drawn on the device from
    ``state`` (int64 [2] = {seed, counter}; the launch stores counter + 1).  ``mean`` / ``std`` [H, A] (or flat), ``lo`` / ``hi``
    [A].  ``keep_mean``: row 0 is clamp(mean) without noise.  One launch of acg_plan_sample on ``stream`` (default: the current
    torch stream); a pure function of (seed, counter, stream_id): bit-identical across launches."""
    run = _lib.entry(lib or _lib.get(), 'plan_sample')
    _device_f32('sample_actions', mean=mean, std=std, lo=lo, hi=hi, state=state, actions=actions)
    if actions.dim() != 3:
        raise ValueError('sample_actions: actions must be [N, H, A], got %s' % (tuple(actions.shape),))
    n, h, a = actions.shape
    for name, t, k in (('mean', mean, h * a), ('std', std, h * a), ('lo', lo, a), ('hi', hi, a), ('actions', actions, n * h * a)):
        _want('sample_actions', name, t, torch.float32, k)
    _want('sample_actions', 'state', state, torch.int64, 2)
    run(_p(mean), _p(std), _p(lo), _p(hi), _p(state), _p(actions), n, h, a, 1 if keep_mean else 0, int(stream_id),
        _stream_handle(stream, actions.device))
    return actions


def accumulate_cost(frames, goal, cost, states=None, goal_state=None, frame_weight=1.0, state_weight=0.0, accumulate=False,
                    channels=None, stream=None, lib=None):
    """``cost`` [N] (float32, written) = (``accumulate``: its old value, else 0) + frame_weight * the squared error of
    ``frames`` [N, H, W, pitch] (float32 or bfloat16; the channels < ``channels``, default all, are scored) against ``goal``
    [H, W, channels] (float32) + state_weight * the squared error of ``states`` [N, S] against ``goal_state`` [S] (both or
    neither).  One launch of acg_plan_cost, one block per candidate, fixed summation order: bit-identical across launches."""
    run = _lib.entry(lib or _lib.get(), 'plan_cost')
    _device_f32('accumulate_cost', frames=frames, goal=goal, cost=cost, states=states, goal_state=goal_state)
    if frames.dim() != 4 or goal.dim() != 3:
        raise ValueError('accumulate_cost: frames [N, H, W, pitch] and goal [H, W, C] expected, got %s and %s'
                         % (tuple(frames.shape), tuple(goal.shape)))
    n, h, w, pitch = frames.shape
    c = pitch if channels is None else int(channels)
    if tuple(goal.shape) != (h, w, c):
        raise ValueError('accumulate_cost: goal must be %s, got %s' % ((h, w, c), tuple(goal.shape)))
    _want('accumulate_cost', 'goal', goal, torch.float32, h * w * c)
    _want('accumulate_cost', 'cost', cost, torch.float32, n)
    if (states is None) != (goal_state is None):
        raise ValueError('accumulate_cost: states and goal_state go together')
    s = 0
    if states is not None:
        if states.dim() != 2 or states.shape[0] != n:
            raise ValueError('accumulate_cost: states must be [%d, S], got %s' % (n, tuple(states.shape)))
        s = states.shape[1]
        _want('accumulate_cost', 'states', states, torch.float32, n * s)
        _want('accumulate_cost', 'goal_state', goal_state, torch.float32, s)
    run(_p(frames), _p(goal), _p(states), _p(goal_state), float(frame_weight), float(state_weight), _p(cost), 1 if accumulate else 0,
        n, h, w, c, pitch, s, _lib.code(frames.dtype), _stream_handle(stream, frames.device))
    return cost


def refit(cost, actions, mean, std, best_cost, best_actions, elite_idx, alpha, min_std, history=None, stream=None, lib=None):
    """One CEM update on the device (acg_plan_refit): rank the N candidates by ``cost`` (NaN as +inf; ties by index),
    ``elite_idx`` [E] (int32, written) = the E best in rank order, ``mean`` / ``std`` [H, A] move to the elites' mean and
    population standard deviation by ``alpha`` (the weight of the OLD value) with ``std`` floored at ``min_std``, and
    ``best_cost`` [1] / ``best_actions`` [H, A] take the best candidate when it is strictly better.  ``history`` (float32 [1],
    optional) receives ``best_cost`` after the update.  One launch of one block; bit-identical across launches."""
    run = _lib.entry(lib or _lib.get(), 'plan_refit')
    _device_f32('refit', cost=cost, actions=actions, mean=mean, std=std, best_cost=best_cost, best_actions=best_actions,
                elite_idx=elite_idx, history=history)
    if actions.dim() != 3:
        raise ValueError('refit: actions must be [N, H, A], got %s' % (tuple(actions.shape),))
    n, h, a = actions.shape
    for name, t, k in (('cost', cost, n), ('actions', actions, n * h * a), ('mean', mean, h * a), ('std', std, h * a),
                       ('best_cost', best_cost, 1), ('best_actions', best_actions, h * a)):
        _want('refit', name, t, torch.float32, k)
    _want('refit', 'elite_idx', elite_idx, torch.int32, elite_idx.numel())
    if history is not None:
        _want('refit', 'history', history, torch.float32, 1)
    run(_p(cost), _p(actions), _p(mean), _p(std), _p(best_cost), _p(best_actions), _p(elite_idx), _p(history), n, h, a,
        elite_idx.numel(), float(alpha), float(min_std), _stream_handle(stream, actions.device))


# ---- argument checks (before any graph op or launch) -----------------------------------------------------------------------------
def _finite(v):
    return isinstance(v, (int, float, np.floating, np.integer)) and not isinstance(v, bool) and math.isfinite(float(v))


def _bounds(value, what):
    arr = np.asarray(value, np.float64)
    if arr.ndim == 0:
        arr = np.full(COMMAND_DIM, float(arr))
    if arr.shape != (COMMAND_DIM,) or not np.isfinite(arr).all():
        raise ValueError('%s must be a finite number or %d of them, got %r' % (what, COMMAND_DIM, value))
    return arr.astype(np.float32)


def check_plan(candidates, horizon, elites, iterations, init_std=DEFAULTS['init_std'], min_std=DEFAULTS['min_std'],
               alpha=DEFAULTS['alpha'], lo=DEFAULTS['lo'], hi=DEFAULTS['hi'], frame_weight=1.0, state_weight=0.0, cost_steps='all',
               seed=0, has_state_head=True):
    """ValueError for settings the planner does not take, each naming its argument; -> the checked values as a dict."""
    from .train import check_noise_seed
    for name, v, top in (('horizon', horizon, _lib.PLAN_HORIZON_MAX), ('elites', elites, _lib.PLAN_CANDIDATES_MAX),
                         ('iterations', iterations, 1 << 20)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= top:
            raise ValueError('%s must be an integer in 1..%d, got %r' % (name, top, v))
    if not 1 <= candidates <= _lib.PLAN_CANDIDATES_MAX:
        raise ValueError('the batch size is the number of candidates: 1..%d, got %r' % (_lib.PLAN_CANDIDATES_MAX, candidates))
    if elites > candidates:
        raise ValueError('elites must be <= the %d candidates (the batch size), got %r' % (candidates, elites))
    if not _finite(init_std) or init_std <= 0:
        raise ValueError('init_std must be finite and > 0, got %r' % (init_std,))
    if not _finite(min_std) or min_std < 0:
        raise ValueError('min_std must be finite and >= 0, got %r' % (min_std,))
    if not _finite(alpha) or not 0 <= alpha <= 1:
        raise ValueError('alpha (the weight of the old mean and std) must be in [0, 1], got %r' % (alpha,))
    lo, hi = _bounds(lo, 'lo'), _bounds(hi, 'hi')
    if (lo > hi).any():
        raise ValueError('lo must be <= hi in every dimension, got lo %s, hi %s' % (lo.tolist(), hi.tolist()))
    if not _finite(frame_weight) or frame_weight < 0:
        raise ValueError('frame_weight must be finite and >= 0, got %r' % (frame_weight,))
    if not _finite(state_weight) or state_weight < 0:
        raise ValueError('state_weight must be finite and >= 0, got %r' % (state_weight,))
    if state_weight != 0 and not has_state_head:
        raise ValueError('state_weight %r: the plain generator predicts no state (state_weight must be 0)' % (state_weight,))
    if cost_steps not in COST_STEPS:
        raise ValueError("cost_steps must be 'all' or 'last', got %r" % (cost_steps,))
    return {'horizon': int(horizon), 'elites': int(elites), 'iterations': int(iterations), 'init_std': float(init_std),
            'min_std': float(min_std), 'alpha': float(alpha), 'lo': lo, 'hi': hi, 'frame_weight': float(frame_weight),
            'state_weight': float(state_weight), 'cost_steps': cost_steps, 'seed': check_noise_seed(seed, 'seed')}


class Planner:
    """CEM over the rows of a Trainer's batch (module docstring).  ``trainer``: a ``train.Trainer`` on a GPU session; its batch
    size is the number of candidates N.  ``horizon`` H steps, the ``elites`` E best refit the Gaussian, ``iterations`` rounds.
    ``init_std``: the standard deviation every plan starts from (around mean 0); ``min_std``: its floor;
    ``alpha``: the weight of the OLD mean and std in an update; ``lo`` / ``hi``: the bounds of a command (a number or 5).
    ``frame_weight`` / ``state_weight``: the weights of the two squared errors (the state term needs a generator with a state
    head and a ``goal_state``); ``cost_steps``: 'all' sums the cost over the H predicted frames, 'last' scores the last one.
    ``seed``: the candidates' stream, {seed, counter} on the device, one draw per iteration.  ``bn`` / ``weights``: as
    ``Trainer.test`` takes them ('stored' needs ``bn_inference`` and a calibration, 'ema' an average).  The generator's noise,
    where it has one, is zero.  Builds nothing in the graph: the steps are the Trainer's own predict program."""

    def __init__(self, trainer, horizon, elites, iterations, init_std=DEFAULTS['init_std'], min_std=DEFAULTS['min_std'],
                 alpha=DEFAULTS['alpha'], lo=DEFAULTS['lo'], hi=DEFAULTS['hi'], frame_weight=1.0, state_weight=0.0, cost_steps='all',
                 seed=0, bn='batch', weights='raw'):
        self.args = check_plan(trainer.batch_size, horizon, elites, iterations, init_std, min_std, alpha, lo, hi, frame_weight,
                               state_weight, cost_steps, seed, has_state_head=trainer.model != 'plain')
        if bn not in ('batch', 'stored'):
            raise ValueError("bn must be 'batch' or 'stored', got %r" % (bn,))
        if weights not in ('raw', 'ema'):
            raise ValueError("weights must be 'raw' or 'ema', got %r" % (weights,))
        sess = trainer.sess
        for name in ('plan_sample', 'plan_cost', 'plan_refit'):
            _lib.entry(sess.rt.lib, name)                # (the C oracle: the AcgError that names the entry and its header)
        if not sess.rt.is_cuda:
            raise RuntimeError('the planner runs on the GPU: the session has no GPU device')
        if bn == 'stored':
            trainer._require_bn_inference()
        if weights == 'ema':
            trainer._require_ema()
        self.trainer, self.sess, self.bn, self.weights = trainer, sess, bn, weights
        a = self.args
        self.N, self.H, self.A, self.E, self.I = trainer.batch_size, a['horizon'], COMMAND_DIM, a['elites'], a['iterations']
        dev, f32 = sess.rt.device, torch.float32
        self.state = torch.empty(2, dtype=torch.int64, device=dev)
        write_draw_state(self.state, a['seed'])
        self.lo, self.hi = torch.from_numpy(a['lo']).to(dev), torch.from_numpy(a['hi']).to(dev)
        self.mean = torch.zeros(self.H, self.A, dtype=f32, device=dev)
        self.std = torch.full((self.H, self.A), a['init_std'], dtype=f32, device=dev)
        self.best_cost = torch.full((1,), math.inf, dtype=f32, device=dev)
        self.best_actions = torch.zeros(self.H, self.A, dtype=f32, device=dev)
        self.history = torch.zeros(self.I, dtype=f32, device=dev)
        self.actions = torch.zeros(self.N, self.H, self.A, dtype=f32, device=dev)
        self.cost = torch.zeros(self.N, dtype=f32, device=dev)
        self.elite_idx = torch.zeros(self.E, dtype=torch.int32, device=dev)

    # ---- the candidates' stream
    def plan_state(self):
        """-> (seed, counter) as Python ints in [0, 2^64): the counter is the number of draws (iterations) so far."""
        return read_draw_state(self.state)

    # ---- inputs
    def _frame(self, value, what):
        S = self.trainer.img_size
        t = self.sess.upload(value)
        if tuple(t.shape) != (S, S, 3):
            raise ValueError('%s must be [%d, %d, 3], got %s' % (what, S, S, tuple(t.shape)))
        return t.contiguous()

    def _vector(self, value, what, n):
        t = self.sess.upload(value)
        if tuple(t.shape) != (n,):
            raise ValueError('%s must be [%d], got %s' % (what, n, tuple(t.shape)))
        return t.contiguous()

    def _goal(self, goal_frame, goal_state):
        goal = self._frame(goal_frame, 'goal_frame')
        use_state = self.args['state_weight'] != 0
        return goal, (self._vector(goal_state, 'goal_state', 5) if use_state else None)

    def _start(self, frame, state):
        N = self.N
        f0 = self._frame(frame, 'frame').unsqueeze(0).expand(N, -1, -1, -1).contiguous()
        s0 = self._vector(state, 'state', 5).unsqueeze(0).expand(N, -1).contiguous()
        return f0, s0

    # ---- the rollout: the predict program and the feeding of Trainer._rollout_on_device, from step 0 on
    def _rollout(self, f0, s0, actions, goal, goal_state, cost, keep_frames=False):
        """Roll ``actions`` [N, H, A] out from (f0, s0) and leave the cost of every row in ``cost``; nothing comes to the host.
        -> the predicted frames [N, H, ...] on the device with ``keep_frames``."""
        tr, a = self.trainer, self.args
        stored = self.bn == 'stored'
        has_state = tr.g_state_out is not None
        fetches = [tr.g_out_stored] + ([tr.g_state_stored] if has_state else []) if stored else \
                  [tr.g_next_frame] + ([tr.g_state_out] if has_state else [])
        frame, state, kept = f0, s0, []
        every = a['cost_steps'] == 'all'
        for t in range(self.H):
            acs = torch.cat([actions[:, t], state], dim=1)
            tr._announced = None
            res = self.sess.run(fetches, tr._feed(frame, frame, acs), device_fetch=True)       # (next_frame is not read by this program)
            out = res[0] if res[0].is_contiguous() else res[0].contiguous()
            if has_state:
                state = res[1].float().contiguous()
            if every or t == self.H - 1:
                accumulate_cost(out, goal, cost, states=state if goal_state is not None else None, goal_state=goal_state,
                                frame_weight=a['frame_weight'], state_weight=a['state_weight'], accumulate=every and t > 0,
                                lib=self.sess.rt.lib)
            # the fetch is the tensor's own buffer and the next step overwrites it - after the feed has copied it into the
            # placeholders, so only a frame that is kept needs a copy of its own
            frame = out.float().clone() if keep_frames else out.float()
            if keep_frames:
                kept.append(frame)
        return torch.stack(kept, dim=1) if keep_frames else None

    def plan(self, frame, state, goal_frame, goal_state=None, keep_candidates=False):
        """One open-loop plan from ``frame`` [H, W, 3] / ``state`` [5] towards ``goal_frame`` [H, W, 3] (and ``goal_state`` [5]
        when ``state_weight`` > 0), starting from mean 0 and ``init_std``.  -> {'actions' [H, 5], 'cost', 'history' [iterations]
        (the best cost after each iteration), 'mean', 'std' [H, 5]} as numpy arrays and a float, copied to the host once, after the
        last iteration; with
        ``keep_candidates`` also 'candidates' [I, N, H, 5], 'costs' [I, N], 'elites' [I, E], 'means' / 'stds' [I, H, 5] (what
        each round drew, scored and refitted to; device-side copies per round, and one more host copy each at the end)."""
        a = self.args
        if a['state_weight'] != 0 and goal_state is None:
            raise ValueError('state_weight %r needs a goal_state' % (a['state_weight'],))
        with self.trainer._predicting(self.bn, self.weights):      # (the mode checks come before anything is uploaded or launched)
            goal, gstate = self._goal(goal_frame, goal_state)
            f0, s0 = self._start(frame, state)
            self.mean.zero_()
            self.std.fill_(a['init_std'])
            self.best_cost.fill_(math.inf)
            self.best_actions.zero_()
            rank = self.sess.rt.rank
            lib = self.sess.rt.lib
            log = None
            if keep_candidates:
                dev, I = self.sess.rt.device, self.I
                log = {'candidates': torch.empty((I,) + tuple(self.actions.shape), device=dev), 'costs': torch.empty(I, self.N, device=dev),
                       'elites': torch.empty(I, self.E, dtype=torch.int32, device=dev), 'means': torch.empty(I, self.H, self.A, device=dev),
                       'stds': torch.empty(I, self.H, self.A, device=dev)}
            for i in range(self.I):
                sample_actions(self.mean, self.std, self.lo, self.hi, self.state, self.actions, keep_mean=True, stream_id=rank, lib=lib)
                self._rollout(f0, s0, self.actions, goal, gstate, self.cost)
                refit(self.cost, self.actions, self.mean, self.std, self.best_cost, self.best_actions, self.elite_idx, a['alpha'],
                      a['min_std'], history=self.history[i:i + 1], lib=lib)
                if log is not None:
                    for k, src in (('candidates', self.actions), ('costs', self.cost), ('elites', self.elite_idx), ('means', self.mean),
                                   ('stds', self.std)):
                        log[k][i].copy_(src)
        ha = self.H * self.A
        flat = torch.cat([self.history, self.best_cost, self.best_actions.view(-1), self.mean.view(-1), self.std.view(-1)]).cpu().numpy()
        I = self.I
        out = {'history': flat[:I].copy(), 'cost': float(flat[I]), 'actions': flat[I + 1:I + 1 + ha].reshape(self.H, self.A).copy(),
               'mean': flat[I + 1 + ha:I + 1 + 2 * ha].reshape(self.H, self.A).copy(),
               'std': flat[I + 1 + 2 * ha:].reshape(self.H, self.A).copy()}
        if log is not None:
            out.update({k: v.cpu().numpy() for k, v in log.items()})
        return out

    def evaluate_actions(self, frame, state, actions, goal_frame, goal_state=None, return_frames=False):
        """The cost of given command sequences ``actions`` [N, H, 5]: the rollout and the cost kernel of ``plan`` without the
        sampling.  -> costs [N] (numpy); with ``return_frames`` also the predicted frames [N, H, H, W, 3]."""
        if self.args['state_weight'] != 0 and goal_state is None:
            raise ValueError('state_weight %r needs a goal_state' % (self.args['state_weight'],))
        with self.trainer._predicting(self.bn, self.weights):
            goal, gstate = self._goal(goal_frame, goal_state)
            f0, s0 = self._start(frame, state)
            acts = self.sess.upload(np.asarray(actions, np.float32) if not torch.is_tensor(actions) else actions)
            if tuple(acts.shape) != (self.N, self.H, self.A):
                raise ValueError('actions must be [%d, %d, %d], got %s' % (self.N, self.H, self.A, tuple(acts.shape)))
            cost = torch.empty_like(self.cost)
            frames = self._rollout(f0, s0, acts.contiguous(), goal, gstate, cost, keep_frames=return_frames)
        if return_frames:
            return cost.cpu().numpy(), frames.cpu().numpy()
        return cost.cpu().numpy()


# ---- CLI -----------------------------------------------------------------------------------------------------------------------------
def plan_sequences(model_path, input_path, output_path, actions_path=None, dna=False, cdna=False, num_masks=10, ksize=5, img_size=64,
                   dtype='f32', device='cuda:0', bn_stats='batch', weights='raw', candidates=64, elites=8, iterations=3, horizon=5,
                   goal_step=None, init_std=DEFAULTS['init_std'], min_std=DEFAULTS['min_std'], alpha=DEFAULTS['alpha'], state_weight=0.0,
                   cost_steps='all', seed=0, num_sequences=None, seq_len=8, dump=False):
    """Restore ``model_path`` as evaluate.evaluate does and plan for the sequences of ``input_path`` (module docstring).
    -> the dict written to ``output_path``/plan.json."""
    from .evaluate import _batches, predicting_trainer
    from .saver import latest_checkpoint
    from .train import model_kind
    if dna and cdna:
        raise ValueError('dna and cdna name two different generators')
    if bn_stats not in ('batch', 'stored'):
        raise ValueError("bn_stats must be 'batch' or 'stored', got %r" % (bn_stats,))
    if weights not in ('raw', 'ema'):
        raise ValueError("weights must be 'raw' or 'ema', got %r" % (weights,))
    transform = 'cdna' if cdna else dna
    goal_step = horizon if goal_step is None else goal_step
    checked = check_plan(candidates, horizon, elites, iterations, init_std, min_std, alpha, state_weight=state_weight, cost_steps=cost_steps,
                         seed=seed, has_state_head=model_kind(transform) != 'plain')
    if isinstance(goal_step, bool) or not isinstance(goal_step, (int, np.integer)) or goal_step < 1:
        raise ValueError('goal_step must be an integer >= 1, got %r' % (goal_step,))
    need = max(goal_step + 1, horizon)
    ckpt = latest_checkpoint(model_path) if os.path.isdir(model_path) else model_path
    if ckpt is None:
        raise FileNotFoundError('no checkpoint under %s' % model_path)
    os.makedirs(output_path, exist_ok=True)
    trainer, ema_updates, _ = predicting_trainer(ckpt, transform, candidates, ksize, img_size, dtype, device, num_masks, bn_stats, weights,
                                                 calibrate_with='evaluate --bn_stats calibrate')
    sess = trainer.sess
    try:
        planner = Planner(trainer, horizon, elites, iterations, init_std=init_std, min_std=min_std, alpha=alpha, state_weight=state_weight,
                          cost_steps=cost_steps, seed=seed, bn=bn_stats)
        per_seq, plans, plan_frames, rollout_s = [], [], [], 0.0
        for frames, acts in _batches(input_path, actions_path, 16, img_size, max(seq_len, need), num_sequences):
            if frames.shape[2:4] != (img_size, img_size):
                raise ValueError('frames of %s x %s, the model is built for --img_size %d' % (frames.shape[2], frames.shape[3], img_size))
            if frames.shape[1] < need:
                raise ValueError('sequences of %d frames: --goal_step %d and --horizon %d need %d' % (frames.shape[1], goal_step, horizon, need))
            for f, ac in zip(frames, acts):
                start, state0, goal, gstate = f[0], ac[0, COMMAND_DIM:], f[goal_step], ac[goal_step, COMMAND_DIM:]
                gs = gstate if checked['state_weight'] != 0 else None
                t0 = time.perf_counter()
                res = planner.plan(start, state0, goal, goal_state=gs, keep_candidates=True)
                rollout_s += time.perf_counter() - t0
                rows = np.zeros((candidates, horizon, COMMAND_DIM), np.float32)
                rows[0] = ac[:horizon, :COMMAND_DIM]
                recorded = planner.evaluate_actions(start, state0, rows, goal, goal_state=gs)
                per_seq.append({'actions': res['actions'].tolist(), 'cost': res['cost'], 'history': [float(v) for v in res['history']],
                                'recorded_cost': float(recorded[0]), 'zero_cost': float(res['costs'][0, 0])})
                if dump:
                    rows[0] = res['actions']
                    _, pf = planner.evaluate_actions(start, state0, rows, goal, goal_state=gs, return_frames=True)
                    plans.append(res['actions'])
                    plan_frames.append(pf[0])
        if not per_seq:
            raise ValueError('%s holds no sequences' % input_path)
        result = {
            'checkpoint': os.path.abspath(ckpt),
            'model': trainer.model,
            'num_masks': num_masks if trainer.model == 'cdna' else None,
            'ksize': ksize if trainer.model != 'plain' else None,
            'sequences': len(per_seq),
            'share_not_worse_than_recorded': float(np.mean([s['cost'] <= s['recorded_cost'] for s in per_seq])),
            'settings': {'candidates': candidates, 'elites': elites, 'iterations': iterations, 'horizon': horizon, 'goal_step': int(goal_step),
                         'init_std': checked['init_std'], 'min_std': checked['min_std'], 'alpha': checked['alpha'],
                         'lo': checked['lo'].tolist(), 'hi': checked['hi'].tolist(), 'frame_weight': checked['frame_weight'],
                         'state_weight': checked['state_weight'], 'cost_steps': cost_steps, 'seed': checked['seed'], 'bn_stats': bn_stats,
                         'weights': weights, 'dtype': dtype, 'img_size': img_size},
            'rollout_s': rollout_s,
            'plans': per_seq,
        }
        if weights == 'ema':
            result['ema_updates'] = int(ema_updates)
        with open(os.path.join(output_path, 'plan.json'), 'w') as fh:
            json.dump(result, fh, indent=1)
        if dump:
            np.save(os.path.join(output_path, 'plans.npy'), np.stack(plans))
            np.save(os.path.join(output_path, 'plan_frames.npy'), np.stack(plan_frames))
        return result
    finally:
        sess.close()


def main(argv=None):
    parser = argparse.ArgumentParser(description='plan actions towards a goal frame with a trained generator (cross-entropy method)')
    parser.add_argument('model_path', type=str, help='checkpoint directory (its latest checkpoint) or checkpoint prefix')
    parser.add_argument('input', type=str, help="frames .npy [N,T,H,W,3], push TFRecord directory, or 'synthetic'")
    parser.add_argument('output', type=str)
    parser.add_argument('--actions', type=str, default=None, help='actions .npy [N,T,10] (with a frames .npy)')
    from .evaluate import ACTION_DIM, load_frames
    from .train import add_model_args, check_model_args
    add_model_args(parser)
    parser.add_argument('--ksize', type=int, default=5)
    parser.add_argument('--img_size', type=int, default=64)
    parser.add_argument('--dtype', type=str, default='f32', choices=['f32', 'bf16'])
    parser.add_argument('--device', type=str, default='cuda:0')
    parser.add_argument('--bn_stats', type=str, default='batch', choices=['batch', 'stored'],
                        help='BatchNorm statistics of the generator: of each batch of candidates, or stored in the checkpoint')
    parser.add_argument('--weights', type=str, default='raw', choices=['raw', 'ema'])
    parser.add_argument('--candidates', type=int, default=64, help='candidate sequences per iteration (the batch size)')
    parser.add_argument('--elites', type=int, default=8)
    parser.add_argument('--iterations', type=int, default=3)
    parser.add_argument('--horizon', type=int, default=5)
    parser.add_argument('--goal_step', type=int, default=None, help='the frame of the sequence that is the goal (default: --horizon)')
    parser.add_argument('--init_std', type=float, default=DEFAULTS['init_std'])
    parser.add_argument('--min_std', type=float, default=DEFAULTS['min_std'])
    parser.add_argument('--alpha', type=float, default=DEFAULTS['alpha'], help='weight of the old mean / std in a refit')
    parser.add_argument('--state_weight', type=float, default=0.0)
    parser.add_argument('--cost_steps', type=str, default='all', choices=list(COST_STEPS))
    parser.add_argument('--seed', type=int, default=0)
    parser.add_argument('--num_sequences', type=int, default=None)
    parser.add_argument('--seq_len', type=int, default=8, help='sequence length of the synthetic source')
    parser.add_argument('--dump', action='store_true', help='save the plans and their predicted frames as .npy')
    args = parser.parse_args(argv)
    transform = check_model_args(parser, args)
    from .train import model_kind
    goal_step = args.horizon if args.goal_step is None else args.goal_step
    try:
        check_plan(args.candidates, args.horizon, args.elites, args.iterations, args.init_std, args.min_std, args.alpha,
                   state_weight=args.state_weight, cost_steps=args.cost_steps, seed=args.seed, has_state_head=model_kind(transform) != 'plain')
    except ValueError as e:
        parser.error(str(e))
    if goal_step < 1:
        parser.error('--goal_step must be >= 1')
    if args.num_sequences is not None and args.num_sequences < 1:
        parser.error('--num_sequences must be >= 1')
    need = max(goal_step + 1, args.horizon)
    if args.input == 'synthetic':
        if args.num_sequences is None:
            parser.error('the synthetic source needs --num_sequences')
    elif not os.path.isdir(args.input):
        if args.actions is None:
            parser.error('a frames .npy needs --actions ACTIONS.npy')
        try:
            frames, actions = load_frames(args.input), np.load(args.actions, mmap_mode='r')
        except (OSError, ValueError) as e:
            parser.error(str(e))
        if actions.ndim != 3 or actions.shape[2] != ACTION_DIM:
            parser.error('%s: expected actions [N, T, %d], got %s' % (args.actions, ACTION_DIM, actions.shape))
        if actions.shape[:2] != frames.shape[:2]:
            parser.error('frames %s and actions %s disagree in N or T' % (frames.shape[:2], actions.shape[:2]))
        if frames.shape[1] < need:
            parser.error('sequences of %d frames: --goal_step %d and --horizon %d need %d' % (frames.shape[1], goal_step, args.horizon, need))
    return plan_sequences(args.model_path, args.input, args.output, actions_path=args.actions, dna=args.dna, cdna=args.cdna,
                          num_masks=args.num_masks, ksize=args.ksize, img_size=args.img_size, dtype=args.dtype, device=args.device,
                          bn_stats=args.bn_stats, weights=args.weights, candidates=args.candidates, elites=args.elites,
                          iterations=args.iterations, horizon=args.horizon, goal_step=goal_step, init_std=args.init_std,
                          min_std=args.min_std, alpha=args.alpha, state_weight=args.state_weight, cost_steps=args.cost_steps, seed=args.seed,
                          num_sequences=args.num_sequences, seq_len=args.seq_len, dump=args.dump)


if __name__ == '__main__':
    main()
