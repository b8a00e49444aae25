"""Optimizers, the discriminator weight clip and the data-parallel gradient all-reduce.

``AdamOptimizer(lr, name).minimize(loss, var_list)`` / ``RMSPropOptimizer`` keep the reference's call
shape (train.py:91-102) and TensorFlow-1.0's update formulas.  ``minimize``:

1. lays the scope's variables out in one flat parameter buffer and allocates one flat gradient buffer
   with the same layout (graph.py), so wgrad kernels write gradients in place;
2. builds the backward ops (graph.build_gradients) - only along paths that reach ``var_list``;
3. with world_size > 1, cuts the flat gradient buffer into contiguous buckets in backward-completion
   order and inserts one RCCL all-reduce per bucket right after the op that completes it - on the
   compute stream in program order, or on a side HIP stream overlapping the rest of backward
   (``collectives='side'``; see DataParallel) - captured into the step's HIP graph either way; the
   optimizer step runs behind all of them;
4. appends ONE fused update launch over the flat buffers (+ the weight clip when it is fetched with it); with ``ema=`` that
   launch also updates the scope's weight average (WeightAverage); with ``clip_norm=`` one ClipNormOp in front of it measures
   the gradient's global norm and scales the flat gradient buffer to a bound (GradNorm); with ``lr_schedule=`` the launch
   evaluates its learning rate itself, from an update counter on the device that it advances (LrSchedule).
"""
import math

import torch

from . import _lib
from . import graph as G
from . import ops as O

_p = G._ptr


def _f32(v):
    """TF-1.0 holds optimizer hyper-parameters as float32 constants."""
    import numpy as np
    return float(np.float32(v))


class DataParallel:
    """Per-graph data-parallel configuration (one process per GPU; this process's own RCCL communicator, comm.py)."""

    def __init__(self, world_size=1, n_buckets=None, force=False, sync_bn=False, exact_global_batch=False, collectives='stream'):
        self.world_size, self.force = int(world_size), bool(force)
        # Every bucket's all-reduce is a plain ncclAllReduce on a HIP stream, captured into the step's HIP graph:
        # 'stream': on the compute stream, in program order right behind the op that completes the bucket;
        # 'side':   on the session's second stream, behind one fork edge, overlapping the rest of backward; one join
        #           edge in front of the optimizer update (north_star: "overlapped with backward on a side HIP stream").
        if collectives not in ('stream', 'side'):
            raise ValueError("collectives must be 'stream' or 'side'")
        self.collectives = collectives
        # buckets per optimizer: an in-order all-reduce hides nothing, so ONE large message per optimizer is best there;
        # the side-stream form sends the layers that finish first (the last-created, for D 69 % of the bytes) while the
        # rest of backward still runs, in two messages
        self.n_buckets = int(n_buckets) if n_buckets else (1 if collectives == 'stream' else 2)
        # exact_global_batch: the run reproduces ONE device at the global batch - BatchNorm over the global batch,
        # the GDL sum scaled by the world size, the state-loss norm taken over all ranks (SURVEY 8(e) caveats 1-3)
        self.exact_global_batch = bool(exact_global_batch)
        self.sync_bn = bool(sync_bn) or self.exact_global_batch   # BatchNorm over the GLOBAL batch (ops.batch_norm)

    @property
    def active(self):
        return self.world_size > 1 or self.force


def set_data_parallel(world_size, n_buckets=None, graph=None, force=False, sync_bn=False, exact_global_batch=False, collectives='stream'):
    """``force`` inserts the bucketed all-reduce even at world_size 1 (a one-rank communicator): lets a single GPU
    exercise the collective / side-stream / graph-capture machinery the multi-GPU runs depend on."""
    (graph or G.get_default_graph()).collections['data_parallel'] = DataParallel(world_size, n_buckets, force, sync_bn, exact_global_batch, collectives)


def _dp(graph):
    return graph.collections.get('data_parallel') or DataParallel(1)


def _chain(*launches):
    """The launches that are not None as one launch, in order (a single one: itself)."""
    live = [f for f in launches if f is not None]
    if len(live) == 1:
        return live[0]

    def launch(s):
        for f in live:
            f(s)
    return launch


class AllReduceOp(G.Op):
    """Sum-all-reduce of one contiguous gradient bucket, in place: ``ncclAllReduce`` on the stream the launch list
    hands it - the compute stream (collectives='stream') or the session's side stream (collectives='side',
    ``side_stream`` makes graph._launch_segment fork and join around it).  A device op like any kernel launch."""

    is_collective = True     # never part of a hoisted side chain; forks behind EVERY main op enqueued so far (its bucket's writers)
    joins_side = True        # on the main stream: side-chain weight gradients of its bucket must have landed

    def __init__(self, flat_grad, start, end, after, name, side):
        super().__init__(flat_grad.graph, name, [], [], control_inputs=after)
        self.flat_grad, self.start, self.end = flat_grad, start, end
        self.index = max(o.index for o in after) + 0.5     # right behind the op that completes the bucket
        self.side_stream = bool(side)

    def bind(self, rt):
        comm = rt.comm
        view = self.flat_grad.buf[self.start:self.end]
        self.no_graph = rt.is_cuda and not comm.capturable
        if hasattr(comm, 'all_reduce_ptr'):
            from . import comm as C
            ptr, n, call = _p(view), view.numel(), comm.all_reduce_ptr
            return lambda s: call(ptr, n, C.NCCL_FLOAT32, C.NCCL_SUM, s)
        return lambda s: comm.all_reduce(view)


class WeightAverage:
    """The exponential moving average of one scope's weights (tf.train.ExponentialMovingAverage(decay, num_updates)): what
    ``Optimizer.minimize(..., ema=)`` takes.  Every StepOp given the same object updates the same average.

    State - graph state (Graph.new_state), no variable, no part of a flat parameter / gradient buffer, no optimizer slot:
    ``<scope>/ema/shadow`` float32 [total] with the layout of the scope's flat parameter buffer (float32 master weights in bf16
    graphs too), ``<scope>/ema/num_updates`` int64 [1] on the device, and one unnamed 32-bit word (the retired-block count of
    the in-launch counter advance, include/acgan_ema.h - unnamed, so no checkpoint holds it).

    The update runs behind every parameter update, in the same program.  With k = the counter before it and p = the parameter
    after the optimizer update (and the clip folded into it): k == 0: shadow = p; else d = min(decay, (1 + k) / (10 + k)) in
    double and shadow -= float32(1 - d) * (shadow - p) in three float32 roundings; then the counter is k + 1.
    DEVIATION from TensorFlow, which seeds the shadow with the variable's INITIAL value: here the first update copies the
    updated parameter, so that a counter of 0 - after ``reset``, or after restoring a checkpoint written before the average
    existed - starts cleanly from the weights as they stand.  The average never feeds back into training.

    The state is created by ``build`` (at the latest when the first StepOp that carries it is compiled), not by the
    constructor: a caller that builds more graph after ``minimize`` can create it last and leave every other op where it was."""

    def __init__(self, decay, scope, graph=None):
        d = float(decay)
        if not 0.0 < d < 1.0 or not 0.0 < _f32(d) < 1.0:
            raise ValueError('WeightAverage: decay must lie in (0, 1), got %r' % (decay,))
        self.decay, self.scope, self.graph = _f32(d), scope, graph or G.get_default_graph()
        self.shadow = self.num_updates = self.done = None

    def build(self):
        if self.shadow is None:
            _, total, _ = self.graph.layout(self.scope)
            self.shadow = self.graph.new_state((total,), 0.0, self.scope + '/ema/shadow')
            self.num_updates = self.graph.new_state((1,), 0, self.scope + '/ema/num_updates', dtype=torch.int64)
            self.done = self.graph.new_state((1,), 0, None, dtype=torch.int32)
        return self

    def tensors(self):
        self.build()
        return [self.shadow, self.num_updates, self.done]

    def args(self):
        """(shadow, decay, counter, state word): the tail of the acg_*_step_ema argument lists."""
        return (_p(self.shadow.buf), self.decay, _p(self.num_updates.buf), _p(self.done.buf))


class GradNorm:
    """The global norm of one scope's gradient and the bound it is clipped to (tf.clip_by_global_norm): what
    ``Optimizer.minimize(..., clip_norm=)`` takes.  ``max_norm`` > 0, or ``math.inf`` to measure only.  Every StepOp of the scope
    given the same object gets a ClipNormOp that writes the same statistics, so they hold the last update of the scope that ran.

    State - graph state, no variable, no optimizer slot: ONE unnamed float32 [2 + V] (V = the scope's variables in layout
    order): the norm of the averaged gradient, the scale it was multiplied by (1: it fitted, or it was not finite), and each
    variable's norm before scaling (include/acgan_rollout.h acg_grad_clip_norm ``stats``).  Unnamed, so no checkpoint holds it.
    Created by ``build`` (at the latest when the first ClipNormOp is compiled), like WeightAverage's, so that a caller can create
    it last and leave every other state where it was."""

    def __init__(self, max_norm, scope, graph=None):
        try:
            m = float(max_norm)
        except (TypeError, ValueError):
            raise ValueError('GradNorm: max_norm must be a number > 0 (math.inf: measure only), got %r' % (max_norm,))
        if isinstance(max_norm, bool) or not m > 0.0 or (math.isfinite(m) and not 0.0 < _f32(m) < math.inf):
            raise ValueError('GradNorm: max_norm must be > 0 (math.inf: measure only), got %r' % (max_norm,))
        self.max_norm, self.scope, self.graph = _f32(m), scope, graph or G.get_default_graph()
        self.stats = None
        self.names = None           # the scope's variables in layout order: stats[2 + i] belongs to names[i]

    def segments(self):
        """-> (names, [(offset, numel)]) of the scope's variables in the flat buffers, layout order."""
        offsets, _, _ = self.graph.layout(self.scope)
        names = sorted(offsets, key=offsets.get)
        if len(names) > _lib.NORM_SEGMENTS_MAX:
            raise ValueError('GradNorm: scope %r has %d variables, acg_grad_clip_norm takes at most %d segments'
                             % (self.scope, len(names), _lib.NORM_SEGMENTS_MAX))
        return names, [(offsets[n], self.graph.variables[n].numel) for n in names]

    def build(self):
        if self.stats is None:
            self.names, _ = self.segments()
            self.stats = self.graph.new_state((2 + len(self.names),), 0.0, None)
        return self

    def tensors(self):
        return [self.build().stats]


class LrSchedule:
    """A learning-rate schedule of one scope's updates - linear warmup, then a constant, linear, cosine or exponential decay - that
    the optimizer's launch evaluates on the device: what ``Optimizer.minimize(..., lr_schedule=)`` takes.  Every StepOp given the
    same object advances the same update counter (acg_adam_step_lr / acg_rmsprop_step_lr, include/acgan_rollout.h, which states
    the formulas): with k the counter as an update finds it and ``lr`` the optimizer's rate, the update uses
    float32(lr * w(k) * f(k)), w = (k + 1) / warmup while k < warmup, f the decay from 1 towards ``final`` over ``decay_steps``
    updates behind the warmup (exponential: final ** (j / decay_steps), not clamped), and leaves the counter at k + 1.  The rate is
    no kernel argument, so a captured HIP graph of the step follows the schedule as it is replayed, with no host in the loop.

    State - graph state, no variable, no optimizer slot: ``<scope>/lr/updates`` int64 [1] (named: a checkpoint key, a restored
    run continues its schedule; a checkpoint without it leaves the counter at 0), one unnamed 32-bit word (the retired-block count
    of the counter advance) and one unnamed float32 [1], the rate the last update used (0 before the first).  Created by ``build``
    (at the latest when the first StepOp that carries it is compiled), like WeightAverage's, so that a caller can create it last
    and leave every other state where it was."""

    def __init__(self, kind, scope, warmup=0, decay_steps=0, final=0.0, graph=None):
        if kind not in _lib.LrSched.KINDS:
            raise ValueError('LrSchedule: kind must be one of %s, got %r' % (', '.join(_lib.LrSched.KINDS), kind))
        for what, v in (('warmup', warmup), ('decay_steps', decay_steps)):
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < 2 ** 63:
                raise ValueError('LrSchedule: %s must be an integer >= 0, got %r' % (what, v))
        try:
            f = float(final)
        except (TypeError, ValueError):
            raise ValueError('LrSchedule: final must be a number in [0, 1], got %r' % (final,))
        if kind != 'constant':
            if int(decay_steps) < 1:
                raise ValueError('LrSchedule: a %s schedule needs decay_steps >= 1, got %r' % (kind, decay_steps))
            low_ok = 0.0 < _f32(f) if kind == 'exponential' else 0.0 <= f
            if isinstance(final, bool) or not (low_ok and f <= 1.0):
                raise ValueError('LrSchedule: final must lie in %s for a %s schedule, got %r'
                                 % ('(0, 1]' if kind == 'exponential' else '[0, 1]', kind, final))
        self.kind, self.scope, self.graph = kind, scope, graph or G.get_default_graph()
        self.warmup, self.decay_steps, self.final = int(warmup), int(decay_steps), _f32(f)
        self.updates = self.done = self.lr = None

    def build(self):
        if self.updates is None:
            self.updates = self.graph.new_state((1,), 0, self.scope + '/lr/updates', dtype=torch.int64)
            self.done = self.graph.new_state((1,), 0, None, dtype=torch.int32)
            self.lr = self.graph.new_state((1,), 0.0, None)
        return self

    def tensors(self):
        self.build()
        return [self.updates, self.done, self.lr]

    def args(self):
        """(schedule, counter, state word, lr_out): what the acg_*_step_lr argument lists hold behind the plain entry's; the
        first is the ctypes struct itself (the call reads it on the host), to be passed by reference and kept alive."""
        self.build()
        sched = _lib.LrSched(_lib.LrSched.KINDS.index(self.kind), self.warmup, self.decay_steps, self.final)
        return (sched, _p(self.updates.buf), _p(self.done.buf), _p(self.lr.buf))


class ClipNormOp(G.Op):
    """acg_grad_clip_norm over a scope's flat gradient buffer, immediately in front of the StepOp it was made for: measures
    grad_scale * g per variable and in all, and multiplies g by min(1, max_norm / norm) in place (never with max_norm = inf).
    Its control inputs are what the StepOp waited for - the gradient writers, the deferred weight-gradient reductions and, under
    data parallelism, the all-reduces: every rank then scales the same summed gradient by the same factor."""
    joins_side = True        # reads every gradient of its scope, whichever stream produced it

    def __init__(self, norm, flat_grad, deps, grad_scale, name):
        super().__init__(flat_grad.graph, name, [flat_grad], [], control_inputs=deps)
        self.norm, self.grad_scale = norm, grad_scale

    @property
    def extras(self):
        return self.norm.tensors()

    def bind(self, rt):
        import ctypes
        fn, size = _lib.entry(rt.lib, 'grad_clip_norm'), _lib.entry(rt.lib, 'grad_clip_norm_workspace_bytes')
        g, norm = self.inputs[0], self.norm.build()
        _, windows = norm.segments()
        segs = _lib.NormSegments()
        segs.count = len(windows)
        for i, (off, numel) in enumerate(windows):
            segs.offset[i], segs.length[i] = off, numel
        ws, n = rt.workspace(size(g.numel, ctypes.byref(segs)))
        self._keep = (ws, segs)
        args = (_p(g.buf), g.numel, ctypes.byref(segs), float(self.grad_scale), norm.max_norm, _p(norm.stats.buf), _p(ws), n)
        return lambda s: fn(*args, s)


class StepOp(G.Op):
    """One fused optimizer launch over the flat buffers of a scope.  ``ema`` (a WeightAverage of the scope, or None): the
    scope's weight average is updated from the new parameters behind the update -
    float32 graph, Adam / RMSProp: inside the optimizer's launch (acg_adam_step_ema / acg_rmsprop_step_ema);
    bf16 graph: acg_ema_update behind the update-and-refresh launch(es), which stay as they are;
    where the fused entry is declined (Session(fuse_ema=False)): acg_ema_update behind the plain step.
    ``lr_schedule`` (an LrSchedule of the scope, or None): the flat entry is the scheduled one (acg_adam_step_lr /
    acg_rmsprop_step_lr), which also carries the average where the plain one would; a bf16 graph then takes the two-launch form
    (the scheduled flat entry, then the refresh of the filter copies) - the one-launch update-and-refresh has no scheduled form."""
    is_optimizer_step = True
    joins_side = True        # reads every gradient of its scope, whichever stream produced it

    def __init__(self, opt, scope, var_names, flat_param, flat_grad, slots, deps, grad_scale, ema=None, lr_schedule=None):
        super().__init__(flat_param.graph, opt.name + '/update', [flat_param, flat_grad] + slots, [], control_inputs=deps)
        self.opt, self.scope, self.var_names, self.grad_scale = opt, scope, list(var_names), grad_scale
        self.program_clip = None
        self.ema, self.lr_schedule = ema, lr_schedule
        self._copies = [t for t3 in flat_param.graph.weight_copies.get(scope, []) for t in t3[1:]]

    @property
    def extras(self):
        """What the launch touches besides its inputs (the session materialises it): the bf16 filter copies, the average's state,
        the schedule's."""
        return (self._copies + (self.ema.tensors() if self.ema is not None else [])
                + (self.lr_schedule.tensors() if self.lr_schedule is not None else []))

    def bind(self, rt):
        opt, ema, clip, update = self.opt, self.ema, self.program_clip, None
        if ema is not None:
            fn, p = _lib.entry(rt.lib, 'ema_update'), self.inputs[0]
            args = (_p(ema.shadow.buf), _p(p.buf), p.numel, ema.decay, _p(ema.num_updates.buf), _p(ema.done.buf))
            update = lambda s: fn(*args, s)
            if not self.graph.weight_copies.get(self.scope) and getattr(rt, 'fuse_ema', True):
                return opt._bind_flat(rt, self, clip, ema)
        # bf16 pipeline: the conv kernels read bf16 copies of the filters, which follow the update.  Round 4: update and
        # refresh are ONE launch (acg_opt_step_prepare_bf16: the blocks that write a filter's copies update its elements) where
        # every copy of the scope fits one list; else two launches as before (also with a learning-rate schedule)
        step = opt._bind_prepared(rt, self, clip) if rt.fuse_weight_refresh else None
        if step is None:
            step = _chain(opt._bind_flat(rt, self, clip), O.prepare_weights_launch(rt, self.graph, self.scope))
        return _chain(step, update)


class ClipOp(G.Op):
    """p.assign(tf.clip_by_value(p, lo, hi)) (train.py:89).  Ordered after the update of the same
    program (defect D6), and folded into the optimizer kernel when it covers the optimizer's scope."""
    joins_side = True
    is_clip = True
    run_last = True

    def __init__(self, var, lo, hi):
        super().__init__(var.graph, 'clip/' + var.name, [var], [])
        self.var, self.lo, self.hi = var, _f32(lo), _f32(hi)

    def bind(self, rt):
        args = (_p(self.var.buf), self.var.numel, self.lo, self.hi)
        fn = rt.lib.clip
        if getattr(self.var, 'copies', None) is None:
            return lambda s: fn(*args, s)
        prep = O.prepare_weights_launch(rt, self.graph, self.var.scope)    # a standalone clip changes a filter: refresh

        def launch(s):
            fn(*args, s)
            prep(s)
        return launch


def clip_by_value_assign(var, lo, hi):
    return ClipOp(var, lo, hi)


class Optimizer:
    def __init__(self, learning_rate, name):
        self.lr, self.name = _f32(learning_rate), name

    def _make_slots(self, graph, total):
        raise NotImplementedError

    def _describe(self, op):
        """What the optimizer is, said once: -> (kind of acg_opt_args, the flat entry's name - ``<entry>_ema`` carries a weight
        average -, (lr, beta1 | decay, beta2 | None, eps), [slot, ...], step counter | None)."""
        raise NotImplementedError

    def _before(self, rt, op, step):
        """The launch that must precede the update of this program, or None."""
        return None

    def _bind_flat(self, rt, op, clip, ema=None):
        """The flat entry over the scope's buffers; with ``ema`` the one that updates that weight average in the same launch.
        An op with a learning-rate schedule takes ``<entry>_lr``, whose tail holds the average's arguments or NULLs."""
        _, entry, hyper, slots, step = self._describe(op)
        p, g = op.inputs[:2]
        lo, hi = clip if clip else (0.0, 0.0)
        buffers = [p, g] + slots + ([step] if step is not None else [])
        args = tuple(_p(t.buf) for t in buffers) + (p.numel,) + tuple(h for h in hyper if h is not None)
        args += (op.grad_scale, 1 if clip else 0, lo, hi)
        if op.lr_schedule is not None:
            import ctypes
            sched, *state = op.lr_schedule.args()
            args += (ctypes.byref(sched),) + tuple(state) + (ema.args() if ema is not None else (None, 0.0, None, None))
            fn = _lib.entry(rt.lib, entry + '_lr')
            return _chain(self._before(rt, op, step), lambda s, _keep=sched: fn(*args, s))
        args += ema.args() if ema is not None else ()
        fn = _lib.entry(rt.lib, entry + ('_ema' if ema is not None else ''))
        return _chain(self._before(rt, op, step), lambda s: fn(*args, s))

    def _bind_prepared(self, rt, op, clip):
        """One launch for the update of the scope and the refresh of its bf16 filter copies, or None (no copies: a float32
        graph; more filters than one list holds; an update with a learning-rate schedule - acg_opt_args is ABI and holds none)."""
        import ctypes
        entries = op.graph.weight_copies.get(op.scope) or []
        if not entries or len(entries) > _lib.PREP_MAX or op.lr_schedule is not None:
            return None
        kind, _, hyper, slots, step = self._describe(op)
        pl = _lib.PrepList()
        for i, (w, rm, tr) in enumerate(entries):
            kh, kw, a, b = w.shape
            pl.src[i], pl.rm[i], pl.tr[i] = w.buf.data_ptr(), rm.buf.data_ptr(), tr.buf.data_ptr()
            pl.taps[i], pl.a[i], pl.b[i] = kh * kw, a, b
        lo, hi = clip if clip else (0.0, 0.0)
        oa = _lib.OptArgs(kind, *(h or 0.0 for h in hyper), op.grad_scale, 1 if clip else 0, lo, hi)
        p, g = op.inputs[:2]
        s1, s2 = (slots + [None])[:2]
        args = tuple(_p(t.buf) if t is not None else None for t in (p, g, s1, s2, step)) + (p.numel, ctypes.byref(oa), ctypes.byref(pl), len(entries))
        fn = rt.lib.opt_step_prepare_bf16
        launch = _chain(self._before(rt, op, step), lambda s: fn(*args, s))
        launch._keep = (oa, pl)
        return launch

    def minimize(self, loss, var_list=None, slots_of=None, ema=None, clip_norm=None, lr_schedule=None):
        """``ema``: a WeightAverage of the variables' scope; the update then also advances it (StepOp).
        ``clip_norm``: a GradNorm of the variables' scope; a ClipNormOp then sits between the gradients and the update
        (``step_op.clip_norm_op``) and the update waits for it alone.  None: nothing is built.
        ``lr_schedule``: an LrSchedule of the variables' scope; the update then takes its rate from it and advances its counter
        (StepOp).  Every StepOp given the same object shares the counter.  None: the rate is this optimizer's constant.
        ``slots_of``: the StepOp of an earlier ``minimize`` by an optimizer of this kind over the same scope; this update then
        continues that one's state (moments, step counter) instead of owning slots of its own - a second loss of one training
        run (train.Trainer's rollout G step continues the one-step G step's optimizer, and checkpoints hold one set of slots)."""
        if not isinstance(loss, O.Scalar):
            raise TypeError('minimize expects a loss built from this package\'s loss functions')
        g = G.get_default_graph()
        if var_list is None:
            var_list = g.trainable_variables()
        if not var_list:
            raise ValueError('No variables to optimize.')
        scopes = {v.scope for v in var_list}
        if len(scopes) != 1:
            raise ValueError('minimize: var_list must come from one top-level scope, got %s' % sorted(scopes))
        scope = scopes.pop()
        if ema is not None and (ema.scope != scope or ema.graph is not g):
            raise ValueError('minimize: ema averages scope %r, the variables are of scope %r' % (ema.scope, scope))
        if clip_norm is not None:
            if clip_norm.scope != scope or clip_norm.graph is not g:
                raise ValueError('minimize: clip_norm measures scope %r, the variables are of scope %r' % (clip_norm.scope, scope))
            clip_norm.segments()         # (more variables than one segment list holds: ValueError before anything is built)
        if lr_schedule is not None and (lr_schedule.scope != scope or lr_schedule.graph is not g):
            raise ValueError('minimize: lr_schedule counts the updates of scope %r, the variables are of scope %r' % (lr_schedule.scope, scope))
        offsets, total, flat_param = g.layout(scope)
        flat_grad = g.new_state((total,), 0.0, self.name + '/flat_grad')
        heads = {}
        for head, idx, w in loss.terms:
            heads.setdefault(head, {})
            heads[head][idx] = heads[head].get(idx, 0.0) + w
        ctx = G.build_gradients(g, heads, var_list, flat_grad, offsets, O._add)
        missing = [v.name for v in var_list if v.name not in ctx.writers]
        if len(missing) == len(var_list):
            raise ValueError('No gradients provided for any variable: %s' % missing)
        dp = _dp(g)
        buckets = self._buckets(dp, var_list, offsets, total) if dp.active else [(0, total)]
        reduce_ops = self._defer_wgrad_reductions(var_list, ctx, offsets, buckets)
        writers = [op for ops_ in ctx.writers.values() for op in ops_]
        deps = list(dict.fromkeys(writers))
        if dp.active:
            deps += self._insert_allreduce(var_list, ctx, flat_grad, offsets, buckets, dp.collectives == 'side')
        if slots_of is not None:
            if type(slots_of.opt) is not type(self) or slots_of.scope != scope:
                raise ValueError('minimize: slots_of is a %s update of scope %r' % (type(slots_of.opt).__name__, slots_of.scope))
            slots = list(slots_of.inputs[2:])
        else:
            slots = self._make_slots(g, total)
        clip_op = None
        if clip_norm is not None:
            clip_op = ClipNormOp(clip_norm, flat_grad, deps, 1.0 / dp.world_size, self.name + '/clip_norm')
            deps = [clip_op]
        step_op = StepOp(self, scope, [v.name for v in var_list], flat_param, flat_grad, slots, deps, 1.0 / dp.world_size, ema=ema,
                         lr_schedule=lr_schedule)
        step_op.clip_norm_op = clip_op
        step_op.reduce_ops = reduce_ops        # one of them can carry the step counter's increment (_step_inc_launch)
        return step_op

    @staticmethod
    def _buckets(dp, var_list, offsets, total):
        # Buckets are contiguous windows of the flat gradient buffer, cut from the END of the layout
        # (the last-created layers finish their wgrad first), each reduced as soon as its last writer ran.
        order = sorted(var_list, key=lambda v: offsets[v.name])
        target = max(total // max(dp.n_buckets, 1), 1)
        buckets, hi, acc = [], total, 0
        for v in reversed(order):
            acc = hi - offsets[v.name]
            if acc >= target:
                buckets.append((offsets[v.name], hi))
                hi, acc = offsets[v.name], 0
        if hi > 0:
            buckets.append((0, hi))
        return buckets

    def _defer_wgrad_reductions(self, var_list, ctx, offsets, buckets):
        """Per bucket (one bucket = the whole buffer without data parallelism), the conv weight gradients with a single
        writer hand their split-K slab reduction to ONE WgradReduceOp, which becomes the gradient's writer."""
        made = []
        for k, (lo, hi) in enumerate(buckets):
            group = [ctx.writers[v.name][0] for v in var_list
                     if lo <= offsets[v.name] < hi and len(ctx.writers.get(v.name, ())) == 1
                     and isinstance(ctx.writers[v.name][0], O.ConvWgradOp)]
            if len(group) < 2:
                continue
            red = O.WgradReduceOp(group, '%s/wgrad_reduce_%d' % (self.name, k))
            made.append(red)
            for v in var_list:
                if ctx.writers.get(v.name) and ctx.writers[v.name][0] in group:
                    ctx.writers[v.name] = [red]
        return made

    def _insert_allreduce(self, var_list, ctx, flat_grad, offsets, buckets, side):
        order = sorted(var_list, key=lambda v: offsets[v.name])
        reduces = []
        for k, (lo, hi_) in enumerate(buckets):
            after = list(dict.fromkeys(op for v in order if lo <= offsets[v.name] < hi_ for op in ctx.writers.get(v.name, [])))
            if not after:
                continue
            reduces.append(AllReduceOp(flat_grad, lo, hi_, after, '%s/allreduce_%d' % (self.name, k), side))
        return reduces


class AdamOptimizer(Optimizer):
    """tf.train.AdamOptimizer: lr_t = lr*sqrt(1-b2^t)/(1-b1^t); p -= lr_t*m/(sqrt(v)+eps)."""

    def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8, name='Adam'):
        super().__init__(learning_rate, name)
        self.b1, self.b2, self.eps = _f32(beta1), _f32(beta2), _f32(epsilon)

    def _make_slots(self, graph, total):
        return [graph.new_state((total,), 0.0, self.name + '/m'), graph.new_state((total,), 0.0, self.name + '/v'),
                graph.new_state((1,), 0, self.name + '/step', dtype=torch.int32)]

    @staticmethod
    def _step_inc_launch(rt, op, step):
        """The launch that advances the device step counter in front of the update, or None when a deferred weight-gradient
        reduction of this optimizer runs in the same program: that launch (acg_splitk_reduce_many, always ahead of the update on
        the main stream) then carries the increment in its acg_reduce_list::step_inc - one tiny launch less per step."""
        for red in getattr(op, 'reduce_ops', ()):
            lists = getattr(red, '_keep', None)
            # the hand-off is explicit: the reduce op must have been bound for THIS compile (WgradReduceOp.bind stamps the program
            # it built its lists for - a stale list of an earlier program, or a reduce op bound after this step op, never matches,
            # and the counter then gets its own launch below), and one list carries ONE counter
            if id(red) in rt.program_ops and lists and not red.side_stream and getattr(red, '_bound_for', None) is rt.program_ops:
                if red.carries_step_inc:
                    raise RuntimeError('%s already advances another optimizer step counter' % red.name)
                lists[0][0].step_inc = step.buf.data_ptr()
                red.carries_step_inc = True
                return None
        inc, ps = rt.lib.step_inc, _p(step.buf)
        return lambda s: inc(ps, s)

    _before = _step_inc_launch

    def _describe(self, op):
        m, v, step = op.inputs[2:]
        return 0, 'adam_step', (self.lr, self.b1, self.b2, self.eps), [m, v], step


class RMSPropOptimizer(Optimizer):
    """tf.train.RMSPropOptimizer (momentum 0): ms starts at ONE; p -= lr*g/sqrt(ms+eps)."""

    def __init__(self, learning_rate, decay=0.9, momentum=0.0, epsilon=1e-10, name='RMSProp'):
        super().__init__(learning_rate, name)
        if momentum != 0.0:
            raise ValueError('RMSPropOptimizer: momentum is not used by the reference and is not implemented')
        self.decay, self.eps = _f32(decay), _f32(epsilon)

    def _make_slots(self, graph, total):
        return [graph.new_state((total,), 1.0, self.name + '/ms')]

    def _describe(self, op):
        return 1, 'rmsprop_step', (self.lr, self.decay, None, self.eps), [op.inputs[2]], None
