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

The designated-pixel cost (Finn & Levine, "Deep Visual Foresight"; ``Planner(pixel_weight=W)``, ``--pixel Y,X --goal_pixel Y,X``):
the user marks up to 4 pixels of the start frame and says where each should end up.  Every candidate carries a probability map per
marked pixel, one-hot at the start; each step the DNA generator moves the maps with the per-pixel kernels it predicts for the frame
(``Trainer(pixel_maps=D)``: a twin of the DNA gather on the same logits, the maps as its image), and ``accumulate_pixel_cost``
(acg_plan_pixel_cost, the fourth launch) adds the expected distance of every map to its goal position and divides the map by its
mass - the gather loses what it pushes over the border and does not sum to one otherwise either.  A whole-frame squared error
mostly measures the arm and the background and needs a goal image; this cost needs none: with ``--frame_weight 0`` the goal frame
is not scored (``goal_frame=None``).  The DNA generator only: the plain generator predicts no flow, and the CDNA generator is
declined - its channel split, kept as written from the reference, transforms the colour channels of one mask with different
kernels, so there is no single flow that a map could follow consistently with the frame.  One goal set serves all candidates.
The map path is float32 in a bf16 graph too (as the DNA image is); it was not run in one.

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
each plan (row 0 of a batch whose other rows are zero commands).  With pixels (``--pixel`` / ``--goal_pixel``, repeatable, for
every sequence; or ``--pixels`` / ``--goal_pixels`` FILE.npy [n, D, 2] per sequence; ``--pixel_weight``, default 1) the settings
gain ``pixels`` / ``goal_pixels`` / ``pixel_weight``, every plan ``pixel_expected`` [D, 2] (the expected positions after the
plan's last step), ``pixel_distance`` [D] (their distances to the goals) and ``recorded_pixel_distance`` (the same for the
dataset's own commands), and ``--dump`` also writes ``plan_maps.npy`` [n, horizon, H, W, D].

Not covered: a mask cost, per-candidate goal pixels, CDNA maps (above), a gather that moves frame and maps in one launch (the maps
cost one more DNA launch per step); replanning
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
from . import models as M
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


def accumulate_pixel_cost(maps, goals, cost, pixel_weight=1.0, accumulate=False, expected=None, mass=None, stream=None, lib=None):
    """``cost`` [N] (float32, written) = (``accumulate``: its old value, else 0) + pixel_weight * sum_j of the expected distance of
    map j of ``maps`` [N, H, W, D] (float32, D in 1..4) to ``goals`` [D, 2] (float32, (y, x), may be fractional): sum P * dist /
    sum P.  ``maps`` is rewritten in place, every map divided by its mass.  ``expected`` [N, D, 2] / ``mass`` [N, D] (float32,
    optional) receive the maps' expected positions and their masses before the division.  A map whose mass is not finite or not
    > 0 makes the row's cost +inf and stays as it is.  One launch of acg_plan_pixel_cost, one block per candidate, fixed
    summation order: bit-identical across launches."""
    run = _lib.entry(lib or _lib.get(), 'plan_pixel_cost')
    _device_f32('accumulate_pixel_cost', maps=maps, goals=goals, cost=cost, expected=expected, mass=mass)
    if maps.dim() != 4:
        raise ValueError('accumulate_pixel_cost: maps [N, H, W, D] expected, got %s' % (tuple(maps.shape),))
    n, h, w, d = maps.shape
    if tuple(goals.shape) != (d, 2):
        raise ValueError('accumulate_pixel_cost: goals must be %s, got %s' % ((d, 2), tuple(goals.shape)))
    for name, t, k in (('maps', maps, n * h * w * d), ('goals', goals, 2 * d), ('cost', cost, n), ('expected', expected, 2 * n * d),
                       ('mass', mass, n * d)):
        if t is not None:
            _want('accumulate_pixel_cost', name, t, torch.float32, k)
    run(_p(maps), _p(goals), float(pixel_weight), _p(cost), 1 if accumulate else 0, _p(expected), _p(mass), n, h, w, d,
        _stream_handle(stream, maps.device))
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
               seed=0, has_state_head=True, pixel_weight=0.0):
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
    if not _finite(pixel_weight) or pixel_weight < 0:
        raise ValueError('pixel_weight must be finite and >= 0, got %r' % (pixel_weight,))
    return {'horizon': int(horizon), 'elites': int(elites), 'iterations': int(iterations), 'init_std': float(init_std),
            'min_std': float(min_std), 'alpha': float(alpha), 'lo': lo, 'hi': hi, 'frame_weight': float(frame_weight),
            'state_weight': float(state_weight), 'cost_steps': cost_steps, 'seed': check_noise_seed(seed, 'seed'),
            'pixel_weight': float(pixel_weight)}


class Planner:
    """CEM over the rows of a Trainer's batch (module docstring).  ``trainer``: a ``train.Trainer`` on a GPU session; its batch
    size is the number of candidates N.  ``horizon`` H steps, the ``elites`` E best refit the Gaussian, ``iterations`` rounds.
    ``init_std``: the standard deviation every plan starts from (around mean 0); ``min_std``: its floor;
    ``alpha``: the weight of the OLD mean and std in an update; ``lo`` / ``hi``: the bounds of a command (a number or 5).
    ``frame_weight`` / ``state_weight``: the weights of the two squared errors (the state term needs a generator with a state
    head and a ``goal_state``); ``cost_steps``: 'all' sums the cost over the H predicted frames, 'last' scores the last one.
    ``seed``: the candidates' stream, {seed, counter} on the device, one draw per iteration.  ``bn`` / ``weights``: as
    ``Trainer.test`` takes them ('stored' needs ``bn_inference`` and a calibration, 'ema' an average).  The generator's noise,
    where it has one, is zero.  Builds nothing in the graph: the steps are the Trainer's own predict program.
    ``pixel_weight`` W (0: nothing new is built or launched, ``plan`` is the one without the argument bit for bit; > 0 needs a
    Trainer built with ``pixel_maps`` >= 1): adds W times the designated-pixel cost (acg_plan_pixel_cost) - ``plan`` and
    ``evaluate_actions`` then take ``pixels`` and ``goal_pixels``, each step also moves the pixels' probability maps through the
    Trainer's map twin, and the maps are scored (and renormalised) at the steps ``cost_steps`` names, after the frame / state cost
    of the step."""

    def __init__(self, trainer, horizon, elites, iterations, init_std=DEFAULTS['init_std'], min_std=DEFAULTS['min_std'],
                 alpha=DEFAULTS['alpha'], lo=DEFAULTS['lo'], hi=DEFAULTS['hi'], frame_weight=1.0, state_weight=0.0, cost_steps='all',
                 seed=0, bn='batch', weights='raw', pixel_weight=0.0):
        self.args = check_plan(trainer.batch_size, horizon, elites, iterations, init_std, min_std, alpha, lo, hi, frame_weight,
                               state_weight, cost_steps, seed, has_state_head=M.KINDS[trainer.model].state_head, pixel_weight=pixel_weight)
        pixel = self.args['pixel_weight'] > 0
        if pixel and not getattr(trainer, 'pixel_maps', 0):
            raise ValueError('pixel_weight %r needs a Trainer built with pixel_maps >= 1 (the DNA generator\'s map path)' % (pixel_weight,))
        if bn not in ('batch', 'stored'):
            raise ValueError("bn must be 'batch' or 'stored', got %r" % (bn,))
        if weights not in ('raw', 'ema'):
            raise ValueError("weights must be 'raw' or 'ema', got %r" % (weights,))
        sess = trainer.sess
        for name in (('plan_pixel_cost',) if pixel else ()) + ('plan_sample', 'plan_cost', 'plan_refit'):
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

    def _check_pixels(self, goal_frame, pixels, goal_pixels):
        """The designated pixels of a call against the Planner's weights, before anything is uploaded or launched.
        -> (pixels int64 [D, 2], goal_pixels float32 [D, 2]) as numpy arrays, or (None, None) without a pixel cost."""
        a = self.args
        if a['pixel_weight'] == 0:
            if pixels is not None or goal_pixels is not None:
                raise ValueError('pixels / goal_pixels: this Planner was built with pixel_weight 0, it scores no pixels')
            if goal_frame is None:
                raise ValueError('goal_frame may be None only with a pixel cost (pixel_weight > 0)')
            return None, None
        if pixels is None or goal_pixels is None:
            raise ValueError('pixel_weight %r needs pixels and goal_pixels' % (a['pixel_weight'],))
        if goal_frame is None and (a['frame_weight'] != 0 or a['state_weight'] != 0):
            raise ValueError('goal_frame may be None only when frame_weight and state_weight are 0 (they are %r and %r)'
                             % (a['frame_weight'], a['state_weight']))
        D, S = self.trainer.pixel_maps, self.trainer.img_size
        px, gp = np.asarray(pixels), np.asarray(goal_pixels)
        if px.shape != (D, 2) or px.dtype.kind not in 'iu':
            raise ValueError('pixels must be an integer [%d, 2] array of (y, x) (the Trainer has pixel_maps=%d), got %s %s'
                             % (D, D, px.dtype, px.shape))
        if (px < 0).any() or (px >= S).any():
            raise ValueError('pixels must lie inside the %d x %d image, got %s' % (S, S, px.tolist()))
        if gp.shape != (D, 2) or gp.dtype.kind not in 'iuf':
            raise ValueError('goal_pixels must be a float [%d, 2] array of (y, x), got %s %s' % (D, gp.dtype, gp.shape))
        gp = gp.astype(np.float32)
        if not np.isfinite(gp).all() or (gp < 0).any() or (gp > S - 1).any():
            raise ValueError('goal_pixels must lie within [0, %d], got %s' % (S - 1, gp.tolist()))
        return px.astype(np.int64), gp

    def _start_maps(self, px, gp):
        """-> (one-hot maps [N, S, S, D] at ``px``, the same in every row; the goals [D, 2]) on the device."""
        S, D = self.trainer.img_size, len(px)
        maps = torch.zeros(self.N, S, S, D, dtype=torch.float32, device=self.sess.rt.device)
        for j, (y, x) in enumerate(px.tolist()):
            maps[:, y, x, j] = 1.0
        return maps, self.sess.upload(gp).contiguous()

    def _goal(self, goal_frame, goal_state):
        if goal_frame is None:               # (_check_pixels: the frame and the state are not scored)
            return None, None
        goal = self._frame(goal_frame, 'goal_frame')
        use_state = self.args['state_weight'] != 0
        return goal, (self._vector(goal_state, 'goal_state', 5) if use_state else None)

    def _start(self, frame, state):
        N = self.N
        f0 = self._frame(frame, 'frame').unsqueeze(0).expand(N, -1, -1, -1).contiguous()
        s0 = self._vector(state, 'state', 5).unsqueeze(0).expand(N, -1).contiguous()
        return f0, s0

    # ---- the rollout: the predict program and the feeding of Trainer._rollout_on_device, from step 0 on
    def _rollout(self, f0, s0, actions, goal, goal_state, cost, keep_frames=False, maps=None, goal_pixels=None, keep_maps=False,
                 expected=None):
        """Roll ``actions`` [N, H, A] out from (f0, s0) and leave the cost of every row in ``cost``; nothing comes to the host.
        ``goal`` None: the frames and states are not scored.  ``maps`` [N, S, S, D] / ``goal_pixels`` [D, 2]: the designated pixels'
        maps go through the map twin at every step and are scored - and renormalised in place - where the frames are, after
        them; ``expected`` [N, D, 2] receives the last step's expected positions.
        -> (the predicted frames [N, H, ...] with ``keep_frames`` else None, the maps [N, H, S, S, D] with ``keep_maps`` else None)
        on the device."""
        tr, a = self.trainer, self.args
        stored = self.bn == 'stored'
        has_state = tr.g_state_out is not None
        fetches = [tr.g_out_stored] + ([tr.g_state_stored] if has_state else []) if stored else \
                  [tr.g_next_frame] + ([tr.g_state_out] if has_state else [])
        if maps is not None:
            fetches = fetches + [tr.g_map_stored if stored else tr.g_map_out]
        frame, state, kept, kept_maps = f0, s0, [], []
        every = a['cost_steps'] == 'all'
        wrote = False                        # whether a launch of this rollout has written ``cost`` already
        lib = self.sess.rt.lib
        for t in range(self.H):
            acs = torch.cat([actions[:, t], state], dim=1)
            tr._announced = None
            feed = tr._feed(frame, frame, acs)                                                 # (next_frame is not read by this program)
            if maps is not None:
                feed[tr.pixel_map_ph] = maps
            res = self.sess.run(fetches, feed, device_fetch=True)
            out = res[0] if res[0].is_contiguous() else res[0].contiguous()
            if has_state:
                state = res[1].float().contiguous()
            if maps is not None:
                maps = res[-1]               # the twin's own buffer: scaled in place below, copied into the placeholder by the next feed
            if every or t == self.H - 1:
                if goal is not None:
                    accumulate_cost(out, goal, cost, states=state if goal_state is not None else None, goal_state=goal_state,
                                    frame_weight=a['frame_weight'], state_weight=a['state_weight'], accumulate=every and t > 0, lib=lib)
                    wrote = True
                if maps is not None:
                    accumulate_pixel_cost(maps, goal_pixels, cost, pixel_weight=a['pixel_weight'], accumulate=wrote,
                                          expected=expected if t == self.H - 1 else None, lib=lib)
                    wrote = True
            if keep_maps:
                kept_maps.append(maps.clone())
            # the fetch is the tensor's own buffer and the next step overwrites it - after the feed has copied it into the
            # placeholders, so only a frame that is kept needs a copy of its own
            frame = out.float().clone() if keep_frames else out.float()
            if keep_frames:
                kept.append(frame)
        return (torch.stack(kept, dim=1) if keep_frames else None), (torch.stack(kept_maps, dim=1) if keep_maps else None)

    def plan(self, frame, state, goal_frame, goal_state=None, keep_candidates=False, pixels=None, goal_pixels=None):
        """One open-loop plan from ``frame`` [H, W, 3] / ``state`` [5] towards ``goal_frame`` [H, W, 3] (and ``goal_state`` [5]
        when ``state_weight`` > 0), starting from mean 0 and ``init_std``.  -> {'actions' [H, 5], 'cost', 'history' [iterations]
        (the best cost after each iteration), 'mean', 'std' [H, 5]} as numpy arrays and a float, copied to the host once, after the
        last iteration; with
        ``keep_candidates`` also 'candidates' [I, N, H, 5], 'costs' [I, N], 'elites' [I, E], 'means' / 'stds' [I, H, 5] (what
        each round drew, scored and refitted to; device-side copies per round, and one more host copy each at the end).
        With a pixel cost (``pixel_weight`` > 0): ``pixels`` [D, 2], integer (y, x) inside the image, one per map of the Trainer, and
        ``goal_pixels`` [D, 2], float (y, x) within [0, S - 1], where each should end up; ``goal_frame`` may then be None when
        ``frame_weight`` and ``state_weight`` are 0 (acg_plan_cost is not launched).  Every candidate starts from one-hot maps at
        ``pixels``.  The result gains 'pixel_expected' [D, 2] and 'pixel_distance' [D]: the expected positions after the last
        step of the best plan and their distances to the goals, from one more batch whose row 0 is the plan and whose other rows
        are zero commands (``evaluate_actions``'s rollout)."""
        a = self.args
        if a['state_weight'] != 0 and goal_state is None:
            raise ValueError('state_weight %r needs a goal_state' % (a['state_weight'],))
        px, gp = self._check_pixels(goal_frame, pixels, goal_pixels)
        expected = None
        with self.trainer._predicting(self.bn, self.weights):      # (the mode checks come before anything is uploaded or launched)
            goal, gstate = self._goal(goal_frame, goal_state)
            f0, s0 = self._start(frame, state)
            maps0, gpix = self._start_maps(px, gp) if px is not None else (None, None)
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
                self._rollout(f0, s0, self.actions, goal, gstate, self.cost, maps=maps0, goal_pixels=gpix)
                refit(self.cost, self.actions, self.mean, self.std, self.best_cost, self.best_actions, self.elite_idx, a['alpha'],
                      a['min_std'], history=self.history[i:i + 1], lib=lib)
                if log is not None:
                    for k, src in (('candidates', self.actions), ('costs', self.cost), ('elites', self.elite_idx), ('means', self.mean),
                                   ('stds', self.std)):
                        log[k][i].copy_(src)
            if px is not None:
                rows = torch.zeros_like(self.actions)
                rows[0].copy_(self.best_actions)
                expected = torch.empty(self.N, len(px), 2, dtype=torch.float32, device=self.sess.rt.device)
                self._rollout(f0, s0, rows, goal, gstate, torch.empty_like(self.cost), maps=maps0, goal_pixels=gpix, expected=expected)
        ha = self.H * self.A
        flat = torch.cat([self.history, self.best_cost, self.best_actions.view(-1), self.mean.view(-1), self.std.view(-1)]).cpu().numpy()
        I = self.I
        out = {'history': flat[:I].copy(), 'cost': float(flat[I]), 'actions': flat[I + 1:I + 1 + ha].reshape(self.H, self.A).copy(),
               'mean': flat[I + 1 + ha:I + 1 + 2 * ha].reshape(self.H, self.A).copy(),
               'std': flat[I + 1 + 2 * ha:].reshape(self.H, self.A).copy()}
        if log is not None:
            out.update({k: v.cpu().numpy() for k, v in log.items()})
        if expected is not None:
            out['pixel_expected'] = expected[0].cpu().numpy()
            out['pixel_distance'] = np.sqrt(((out['pixel_expected'].astype(np.float64) - gp) ** 2).sum(axis=1))
        return out

    def evaluate_actions(self, frame, state, actions, goal_frame, goal_state=None, return_frames=False, pixels=None, goal_pixels=None,
                         return_maps=False, return_expected=False):
        """The cost of given command sequences ``actions`` [N, H, 5]: the rollout and the cost kernels of ``plan`` without the
        sampling; ``pixels`` / ``goal_pixels`` as ``plan`` takes them.  -> costs [N] (numpy); then, in this order, with
        ``return_frames`` the predicted frames [N, H, H, W, 3], with ``return_maps`` the pixels' maps [N, H, H, W, D] (after every
        scored step normalised to mass 1; with ``cost_steps='last'`` the earlier steps are as the gather left them), with
        ``return_expected`` the expected positions after the last step [N, D, 2]."""
        if self.args['state_weight'] != 0 and goal_state is None:
            raise ValueError('state_weight %r needs a goal_state' % (self.args['state_weight'],))
        px, gp = self._check_pixels(goal_frame, pixels, goal_pixels)
        if (return_maps or return_expected) and px is None:
            raise ValueError('return_maps / return_expected need a pixel cost (pixel_weight > 0)')
        with self.trainer._predicting(self.bn, self.weights):
            goal, gstate = self._goal(goal_frame, goal_state)
            f0, s0 = self._start(frame, state)
            maps0, gpix = self._start_maps(px, gp) if px is not None else (None, None)
            acts = self.sess.upload(np.asarray(actions, np.float32) if not torch.is_tensor(actions) else actions)
            if tuple(acts.shape) != (self.N, self.H, self.A):
                raise ValueError('actions must be [%d, %d, %d], got %s' % (self.N, self.H, self.A, tuple(acts.shape)))
            cost = torch.empty_like(self.cost)
            expected = torch.empty(self.N, len(px), 2, dtype=torch.float32, device=cost.device) if return_expected else None
            frames, maps = self._rollout(f0, s0, acts.contiguous(), goal, gstate, cost, keep_frames=return_frames, maps=maps0,
                                         goal_pixels=gpix, keep_maps=return_maps, expected=expected)
        extra = [t.cpu().numpy() for t, asked in ((frames, return_frames), (maps, return_maps), (expected, return_expected)) if asked]
        return (cost.cpu().numpy(),) + tuple(extra) if extra else cost.cpu().numpy()


def check_pixel_args(pixels, goal_pixels, pixel_weight, model, img_size):
    """The designated pixels of a run - [D, 2] for every sequence or [n, D, 2] per sequence - against the generator ``model``.
    ValueError for what the planner does not take; -> (pixels int64, goal_pixels float32, pixel_weight), or (None, None, 0.0)
    without pixels."""
    if pixels is None and goal_pixels is None:
        if pixel_weight:
            raise ValueError('pixel_weight %r without pixels' % (pixel_weight,))
        return None, None, 0.0
    if pixels is None or goal_pixels is None:
        raise ValueError('pixels and goal_pixels go together')
    from .train import check_pixel_maps
    check_pixel_maps(1, model)                           # (the Trainer's own refusal, with its reason)
    px, gp = np.asarray(pixels), np.asarray(goal_pixels)
    if px.dtype.kind not in 'iu' or px.ndim not in (2, 3) or px.shape[-1] != 2:
        raise ValueError('pixels must be integer (y, x) pairs, [D, 2] or [n, D, 2], got %s %s' % (px.dtype, px.shape))
    if gp.dtype.kind not in 'iuf' or gp.shape != px.shape:
        raise ValueError('goal_pixels must be float (y, x) pairs of the shape of pixels %s, got %s %s' % (px.shape, gp.dtype, gp.shape))
    if not 1 <= px.shape[-2] <= _lib.PLAN_PIXEL_MAPS_MAX:
        raise ValueError('1..%d pixels per sequence, got %d' % (_lib.PLAN_PIXEL_MAPS_MAX, px.shape[-2]))
    if px.ndim == 3 and len(px) < 1:
        raise ValueError('pixels for no sequence')
    gp = gp.astype(np.float32)
    if (px < 0).any() or (px >= img_size).any():
        raise ValueError('pixels must lie inside the %d x %d image' % (img_size, img_size))
    if not np.isfinite(gp).all() or (gp < 0).any() or (gp > img_size - 1).any():
        raise ValueError('goal_pixels must lie within [0, %d]' % (img_size - 1))
    weight = 1.0 if pixel_weight is None else pixel_weight
    if not _finite(weight) or weight <= 0:
        raise ValueError('pixel_weight must be finite and > 0 with pixels, got %r' % (pixel_weight,))
    return px.astype(np.int64), gp, float(weight)


# ---- CLI -----------------------------------------------------------------------------------------------------------------------------
def plan_sequences(model_path, input_path, output_path, actions_path=None, dna=False, cdna=False, num_masks=10, ksize=5, img_size=64,
                   dtype='f32', device='cuda:0', bn_stats='batch', weights='raw', candidates=64, elites=8, iterations=3, horizon=5,
                   goal_step=None, init_std=DEFAULTS['init_std'], min_std=DEFAULTS['min_std'], alpha=DEFAULTS['alpha'], state_weight=0.0,
                   cost_steps='all', seed=0, num_sequences=None, seq_len=8, dump=False, pixels=None, goal_pixels=None, pixel_weight=None,
                   frame_weight=1.0, affine=False, canvas=False):
    """Restore ``model_path`` as evaluate.evaluate does and plan for the sequences of ``input_path`` (module docstring).
    ``pixels`` (int) / ``goal_pixels`` (float): [D, 2] for every sequence or [n, D, 2], one set per sequence - the designated-pixel
    cost, weighted ``pixel_weight`` (None: 1.0 with pixels, 0 without); ``frame_weight`` 0 with ``state_weight`` 0: the goal frame
    is not scored.  ``canvas``: as evaluate.evaluate takes it; plan.json then holds ``canvas: true``.
    -> the dict written to ``output_path``/plan.json."""
    from .evaluate import _batches, predicting_trainer
    from .saver import latest_checkpoint
    from .train import check_canvas
    transform = M.transform_argument(dict(dna=dna, cdna=cdna, affine=affine))
    kind = M.KINDS[M.model_kind(transform)]
    canvas = check_canvas(canvas, kind.name, ksize, num_masks)
    if bn_stats not in ('batch', 'stored'):
        raise ValueError("bn_stats must be 'batch' or 'stored', got %r" % (bn_stats,))
    if weights not in ('raw', 'ema'):
        raise ValueError("weights must be 'raw' or 'ema', got %r" % (weights,))
    goal_step = horizon if goal_step is None else goal_step
    pixels, goal_pixels, pixel_weight = check_pixel_args(pixels, goal_pixels, pixel_weight, kind.name, img_size)
    checked = check_plan(candidates, horizon, elites, iterations, init_std, min_std, alpha, frame_weight=frame_weight,
                         state_weight=state_weight, cost_steps=cost_steps, seed=seed, has_state_head=kind.state_head,
                         pixel_weight=pixel_weight)
    if pixels is None and checked['frame_weight'] == 0 and checked['state_weight'] == 0:
        raise ValueError('frame_weight 0 and state_weight 0 without pixels: nothing is scored')
    if pixels is not None and pixels.ndim == 3 and num_sequences is not None and len(pixels) < num_sequences:
        raise ValueError('pixels for %d sequences, %d are planned' % (len(pixels), num_sequences))
    score_frames = pixels is None or checked['frame_weight'] != 0 or checked['state_weight'] != 0
    if isinstance(goal_step, bool) or not isinstance(goal_step, (int, np.integer)) or goal_step < 1:
        raise ValueError('goal_step must be an integer >= 1, got %r' % (goal_step,))
    need = max(goal_step + 1, horizon)
    ckpt = latest_checkpoint(model_path) if os.path.isdir(model_path) else model_path
    if ckpt is None:
        raise FileNotFoundError('no checkpoint under %s' % model_path)
    os.makedirs(output_path, exist_ok=True)
    trainer, ema_updates, _ = predicting_trainer(ckpt, transform, candidates, ksize, img_size, dtype, device, num_masks, bn_stats, weights,
                                                 calibrate_with='evaluate --bn_stats calibrate',
                                                 pixel_maps=0 if pixels is None else pixels.shape[-2],
                                                 **({'canvas': True} if canvas else {}))
    sess = trainer.sess
    try:
        planner = Planner(trainer, horizon, elites, iterations, init_std=init_std, min_std=min_std, alpha=alpha, frame_weight=frame_weight,
                          state_weight=state_weight, cost_steps=cost_steps, seed=seed, bn=bn_stats, pixel_weight=pixel_weight)
        per_seq, plans, plan_frames, plan_maps, used_pixels, used_goals, rollout_s = [], [], [], [], [], [], 0.0
        for frames, acts in _batches(input_path, actions_path, 16, img_size, max(seq_len, need), num_sequences):
            if frames.shape[2:4] != (img_size, img_size):
                raise ValueError('frames of %s x %s, the model is built for --img_size %d' % (frames.shape[2], frames.shape[3], img_size))
            if frames.shape[1] < need:
                raise ValueError('sequences of %d frames: --goal_step %d and --horizon %d need %d' % (frames.shape[1], goal_step, horizon, need))
            for f, ac in zip(frames, acts):
                start, state0, goal, gstate = f[0], ac[0, COMMAND_DIM:], f[goal_step], ac[goal_step, COMMAND_DIM:]
                gs = gstate if checked['state_weight'] != 0 else None
                pkw = {}
                if pixels is not None:
                    k = len(per_seq)
                    if pixels.ndim == 3 and k >= len(pixels):
                        raise ValueError('pixels for %d sequences, %s holds more' % (len(pixels), input_path))
                    pkw = {'pixels': pixels[k] if pixels.ndim == 3 else pixels, 'goal_pixels': goal_pixels[k] if pixels.ndim == 3 else goal_pixels}
                    used_pixels.append(pkw['pixels'].tolist())
                    used_goals.append(pkw['goal_pixels'].tolist())
                    if not score_frames:
                        goal = None
                t0 = time.perf_counter()
                res = planner.plan(start, state0, goal, goal_state=gs, keep_candidates=True, **pkw)
                rollout_s += time.perf_counter() - t0
                rows = np.zeros((candidates, horizon, COMMAND_DIM), np.float32)
                rows[0] = ac[:horizon, :COMMAND_DIM]
                if pixels is None:
                    recorded = planner.evaluate_actions(start, state0, rows, goal, goal_state=gs)
                else:
                    recorded, rec_exp = planner.evaluate_actions(start, state0, rows, goal, goal_state=gs, return_expected=True, **pkw)
                per_seq.append({'actions': res['actions'].tolist(), 'cost': res['cost'], 'history': [float(v) for v in res['history']],
                                'recorded_cost': float(recorded[0]), 'zero_cost': float(res['costs'][0, 0])})
                if pixels is not None:
                    rec_dist = np.sqrt(((rec_exp[0].astype(np.float64) - pkw['goal_pixels']) ** 2).sum(axis=1))
                    per_seq[-1].update({'pixel_expected': res['pixel_expected'].tolist(), 'pixel_distance': res['pixel_distance'].tolist(),
                                        'recorded_pixel_distance': rec_dist.tolist()})
                if dump:
                    rows[0] = res['actions']
                    got = planner.evaluate_actions(start, state0, rows, goal, goal_state=gs, return_frames=True, return_maps=pixels is not None,
                                                   **pkw)
                    plans.append(res['actions'])
                    plan_frames.append(got[1][0])
                    if pixels is not None:
                        plan_maps.append(got[2][0])
        if not per_seq:
            raise ValueError('%s holds no sequences' % input_path)
        result = {
            'checkpoint': os.path.abspath(ckpt),
            'model': trainer.model,
            **kind.result_fields(ksize, num_masks, canvas),
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
        if pixels is not None:
            per_sequence = pixels.ndim == 3
            result['settings'].update({'pixels': used_pixels if per_sequence else used_pixels[0],
                                       'goal_pixels': used_goals if per_sequence else used_goals[0], 'pixel_weight': checked['pixel_weight']})
        with open(os.path.join(output_path, 'plan.json'), 'w') as fh:
            json.dump(result, fh, indent=1)
        if dump:
            np.save(os.path.join(output_path, 'plans.npy'), np.stack(plans))
            np.save(os.path.join(output_path, 'plan_frames.npy'), np.stack(plan_frames))
            if pixels is not None:
                np.save(os.path.join(output_path, 'plan_maps.npy'), np.stack(plan_maps))
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
    parser.add_argument('--dump', action='store_true', help='save the plans and their predicted frames (and pixel maps) as .npy')
    parser.add_argument('--pixel', type=str, action='append', default=None, metavar='Y,X',
                        help='a designated pixel of frame 0, for every sequence (repeatable, up to 4; needs --dna)')
    parser.add_argument('--goal_pixel', type=str, action='append', default=None, metavar='Y,X',
                        help='where the --pixel of the same position should end up (may be fractional)')
    parser.add_argument('--pixels', type=str, default=None, metavar='FILE.npy', help='designated pixels per sequence, int [n, D, 2]')
    parser.add_argument('--goal_pixels', type=str, default=None, metavar='FILE.npy', help='their goals, float [n, D, 2]')
    parser.add_argument('--pixel_weight', type=float, default=None, help='weight of the designated-pixel cost (default 1.0 once pixels are given)')
    parser.add_argument('--frame_weight', type=float, default=1.0, help='weight of the frame cost; 0 (with --state_weight 0): the goal frame is not scored')
    args = parser.parse_args(argv)
    kind = M.KINDS[M.model_kind(check_model_args(parser, args))]
    goal_step = args.horizon if args.goal_step is None else args.goal_step
    pixels = goal_pixels = None
    if (args.pixel or args.goal_pixel) and (args.pixels or args.goal_pixels):
        parser.error('--pixel / --goal_pixel and --pixels / --goal_pixels exclude each other')
    try:
        if args.pixel or args.goal_pixel:
            if len(args.pixel or []) != len(args.goal_pixel or []):
                parser.error('%d --pixel and %d --goal_pixel: the counts must be equal' % (len(args.pixel or []), len(args.goal_pixel or [])))
            pixels = np.array([[int(v) for v in p.split(',')] for p in args.pixel], np.int64).reshape(len(args.pixel), -1)
            goal_pixels = np.array([[float(v) for v in p.split(',')] for p in args.goal_pixel], np.float64).reshape(len(args.pixel), -1)
        elif args.pixels or args.goal_pixels:
            if not (args.pixels and args.goal_pixels):
                parser.error('--pixels and --goal_pixels go together')
            pixels, goal_pixels = np.load(args.pixels), np.load(args.goal_pixels)
            if pixels.ndim != 3:
                parser.error('%s: expected pixels [n, D, 2], got %s' % (args.pixels, pixels.shape))
        pixels, goal_pixels, pixel_weight = check_pixel_args(pixels, goal_pixels, args.pixel_weight, kind.name, args.img_size)
        checked = check_plan(args.candidates, args.horizon, args.elites, args.iterations, args.init_std, args.min_std, args.alpha,
                             frame_weight=args.frame_weight, state_weight=args.state_weight, cost_steps=args.cost_steps, seed=args.seed,
                             has_state_head=kind.state_head, pixel_weight=pixel_weight)
    except (OSError, ValueError) as e:
        parser.error(str(e))
    if pixels is None and checked['frame_weight'] == 0 and checked['state_weight'] == 0:
        parser.error('--frame_weight 0 and --state_weight 0 without pixels: nothing is scored')
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
        if pixels is not None and pixels.ndim == 3 and args.num_sequences is None and len(pixels) < frames.shape[0]:
            parser.error('%s holds pixels for %d sequences, %d are planned' % (args.pixels, len(pixels), frames.shape[0]))
    if pixels is not None and pixels.ndim == 3 and args.num_sequences is not None and len(pixels) < args.num_sequences:
        parser.error('%s holds pixels for %d sequences, %d are planned' % (args.pixels, len(pixels), args.num_sequences))
    return plan_sequences(args.model_path, args.input, args.output, actions_path=args.actions,
                          num_masks=args.num_masks, ksize=args.ksize, img_size=args.img_size, dtype=args.dtype, device=args.device,
                          bn_stats=args.bn_stats, weights=args.weights, candidates=args.candidates, elites=args.elites,
                          iterations=args.iterations, horizon=args.horizon, goal_step=goal_step, init_std=args.init_std,
                          min_std=args.min_std, alpha=args.alpha, state_weight=args.state_weight, cost_steps=args.cost_steps, seed=args.seed,
                          num_sequences=args.num_sequences, seq_len=args.seq_len, dump=args.dump, pixels=pixels, goal_pixels=goal_pixels,
                          pixel_weight=pixel_weight if pixels is not None else None, frame_weight=args.frame_weight,
                          **{flag: getattr(args, flag) for flag in M.flags()}, **({'canvas': True} if args.canvas else {}))


if __name__ == '__main__':
    main()
