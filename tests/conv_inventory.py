"""The conv launches of the benchmark's programs, taken from the model itself (not from a hand-typed table).

``record(monkeypatch, make_session, cfg)`` builds the Trainer the way bench.py does (default Session options, look-ahead
on), compiles the programs of the bench's call pair - ``train_d(..., next_g=...)`` then ``train_g`` (and, with n_critic > 1,
the D step that follows an announcing D step) - and those of the plain call path, and records what every conv op's ``bind``
chose: the full descriptor, the ABI entry (path) and its flags, ``accumulate``, the consuming BatchNorm's parameters and the
planner's tile / split choice.  Test-side only: ``bind`` is wrapped through pytest's monkeypatch, production behaviour is
unchanged.  Shared by the CPU suite (C-oracle session: the descriptors) and the GPU suite (libacgan_hip.so: the paths)."""
import ctypes
from collections import OrderedDict

from action_conditioned_gans_amd import _lib as L
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import ops as O
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T

# per-GPU sizes of the BASELINE configurations (bench.py defaults: batch 32 per GPU)
CONFIGS = OrderedDict([
    ('c2', dict(dtype='f32', batch=32, img=64, ksize=5, loss='bce', opt='adam', dna=True)),
    ('c4', dict(dtype='f32', batch=32, img=64, ksize=5, loss='wass', opt='rmsprop', dna=True)),
    ('c3', dict(dtype='bf16', batch=32, img=64, ksize=5, loss='bce', opt='adam', dna=True)),
    ('c5', dict(dtype='bf16', batch=32, img=128, ksize=11, loss='bce', opt='adam', dna=True)),
    ('plain', dict(dtype='f32', batch=32, img=64, ksize=5, loss='bce', opt='adam', dna=False)),
])

ACTS = {None: L.ACT_NONE, 'relu': L.ACT_RELU, 'lrelu': L.ACT_LRELU, 'tanh': L.ACT_TANH}


def build(make_session, cfg):
    c = CONFIGS[cfg]
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = make_session(dtype=c['dtype'])
    tr = T.Trainer(sess, True, c['loss'], c['opt'], c['dna'], batch_size=c['batch'], img_size=c['img'], ksize=c['ksize'], seed=0,
                   lookahead=True)
    sess.run(G.global_variables_initializer())
    return sess, tr


def programs(tr, cfg):
    """(name, fetches, feed keys, skip ops) of every program the bench's step and the plain call path compile."""
    fd = list(tr._feed(None, None, None, None).keys())
    pair = fd + [tr.pair_img_ph, tr._pair_img_pad, tr.pair_action_ph]
    out = [('d_lookahead', [tr.d_opt_op, tr.clip_d, tr._pair_concat], pair, tr._skip_d),
           ('g_after_lookahead', [tr.g_opt_op, tr.g_next_frame] + tr._g_extra, fd, tr._skip_g)]
    if CONFIGS[cfg]['loss'] == 'wass':        # n_critic 5: the D step behind an announcing D step
        out.append(('d_after_lookahead', [tr.d_opt_op, tr.clip_d] + tr._g_extra, fd, tr._skip_g))
    out += [('d_plain', [tr.d_opt_op, tr.clip_d], fd, None), ('g_plain', [tr.g_opt_op, tr.g_next_frame], fd, None)]
    return out


def plan(lib, d, which, dtype):
    rows, cols = ctypes.c_int32(0), ctypes.c_int32(0)
    tiles = lib.conv2d_tile(ctypes.byref(d), which, dtype, ctypes.byref(rows), ctypes.byref(cols))
    return (rows.value, cols.value, tiles, lib.conv2d_splits(ctypes.byref(d), which, dtype))


def _bn(bn):
    if bn is None:
        return None
    return dict(groups=bn.groups, act=bn.act, leak=bn.leak, eps=bn.eps, rows=bn.rows, c=bn.c, xp=bn.xp, yp=bn.yp,
                y_f32=bn.outputs[0].dtype != bn.inputs[0].dtype)


class Inventory:
    def __init__(self, cfg, conv_dtype, opt):
        self.cfg, self.conv_dtype, self.opt = cfg, conv_dtype, opt
        self.entries = OrderedDict()        # dedup key -> entry (with the ops / programs it was bound for)
        self.reduces = []                   # (program, [(entry key, splits, accumulate)])
        self._wgrad_key = {}                # id(dw tensor) -> entry key of the contraction that leaves its slabs
        self.program = None

    def add(self, op, role, path, d, which, rt, **kw):
        e = dict(role=role, transposed=op.transposed, which=which, dtype=rt.conv_dtype, desc=d.key(), path=path,
                 flags=kw.pop('flags', 0), layout=kw.pop('layout', None), accumulate=kw.pop('accumulate', None),
                 bn=kw.pop('bn', None), bias_act=kw.pop('bias_act', None), plan=plan(rt.lib, d, which, rt.conv_dtype))
        e.update(kw)
        key = (role, e['transposed'], e['dtype'], e['desc'], path, e['flags'], e['layout'], e['accumulate'],
               tuple(sorted(e['bn'].items())) if e['bn'] else None, e['bias_act'])
        if key not in self.entries:
            e['ops'], e['programs'], e['key'] = [], [], key
            self.entries[key] = e
        ent = self.entries[key]
        if op.name not in ent['ops']:
            ent['ops'].append(op.name)
        if self.program not in ent['programs']:
            ent['programs'].append(self.program)
        return key

    def kinds(self):
        """path kinds present: stats, fwd_slabs, bwd_slabs, pair, deferred, fused_bias, f32_head, plain_*"""
        out = set()
        for e in self.entries.values():
            out.add(e['path'])
            if e['path'] == 'pair':
                if e['flags'] & 1:
                    out.add('deferred')
                if e['flags'] & 2:
                    out.add('bwd_slabs')
        return out


def _record_conv(inv, op, rt):
    d = op.desc
    if op._fused_bias:
        bc = op.bias_consumer
        inv.add(op, 'fwd', 'fused_bias', op._keep[0], op.which, rt, bias_act=(bc.act, bc.leak))
    elif op.out_f32:
        inv.add(op, 'fwd', 'f32_head', d, op.which, rt)
    elif op._stats is not None:
        inv.add(op, 'fwd', 'stats', d, op.which, rt, bn=_bn(op.bn_consumer), bn_flags=op.bn_consumer.launch_flags(rt, False))
    elif op._slab is not None:
        inv.add(op, 'fwd', 'fwd_slabs', d, op.which, rt, layout=op._slab[2], bn=_bn(op.bn_consumer),
                bn_flags=op.bn_consumer.launch_flags(rt, False))
    else:
        inv.add(op, 'fwd', 'plain', d, op.which, rt)


def _record_dgrad(inv, op, rt):
    d, bn = op.desc, op.bn_bwd_consumer
    slab = op._slab
    kw = {}
    if slab is not None:
        kw = dict(layout=slab[2], bn=_bn(bn.fwd), bn_flags=bn.fwd.launch_flags(rt, True))
    if not op.pair_active:
        inv.add(op, 'dgrad', 'bwd_slabs' if slab is not None else 'plain', d, op.which, rt, **kw)
        return
    wg = op.pair_w
    flags = op._keep_flags
    key = inv.add(op, 'dgrad', 'pair', d, op.which, rt, flags=flags, accumulate=wg.accumulate, wplan=plan(rt.lib, d, L.CONV_WGRAD, rt.conv_dtype),
                  **kw)
    if flags & 1:
        inv._wgrad_key[id(wg.outputs[0])] = key


def _record_wgrad(inv, op, rt, fn):
    if op.paired or fn is None:
        return
    d = op.desc
    deferred = op.deferred_to is not None and rt.lib.conv2d_splits(ctypes.byref(d), L.CONV_WGRAD, rt.conv_dtype) > 1
    key = inv.add(op, 'wgrad', 'deferred' if deferred else 'plain', d, L.CONV_WGRAD, rt, accumulate=op.accumulate)
    if deferred:
        inv._wgrad_key[id(op.outputs[0])] = key


def record(monkeypatch, make_session, cfg):
    """-> (Inventory, session, trainer): every conv bind of the bench's programs and the plain call path."""
    sess, tr = build(make_session, cfg)
    inv = Inventory(cfg, sess.rt.conv_dtype, CONFIGS[cfg]['opt'])

    def wrap(cls, after):
        orig = cls.bind

        def bind(self, rt):
            fn = orig(self, rt)
            after(self, rt, fn)
            return fn
        monkeypatch.setattr(cls, 'bind', bind)

    wrap(O.Conv2dOp, lambda op, rt, fn: _record_conv(inv, op, rt))

    orig_dgrad = O.ConvDgradOp.bind

    def dgrad_bind(self, rt):
        fn = orig_dgrad(self, rt)
        self._keep_flags = 0
        if self.pair_active:                       # the flag word the paired launch was bound with (its last argument before the stream)
            cells = dict(zip(fn.__code__.co_freevars, (c.cell_contents for c in fn.__closure__)))
            self._keep_flags = int(cells['args'][-1])
        _record_dgrad(inv, self, rt)
        return fn
    monkeypatch.setattr(O.ConvDgradOp, 'bind', dgrad_bind)
    wrap(O.ConvWgradOp, lambda op, rt, fn: _record_wgrad(inv, op, rt, fn))

    orig_reduce = O.WgradReduceOp.bind

    def reduce_bind(self, rt):
        pending = [(inv._wgrad_key[id(dst)], splits, acc) for ws, dst, splits, acc in self.pending]
        fn = orig_reduce(self, rt)
        if pending:
            inv.reduces.append((inv.program, pending))
        return fn
    monkeypatch.setattr(O.WgradReduceOp, 'bind', reduce_bind)

    for name, fetches, feeds, skip in programs(tr, cfg):
        inv.program = name
        sess._compile(sess._flatten(fetches), feeds, tuple(skip) if skip else ())
    return inv, sess, tr


def describe(e):
    d = L.ConvDesc(*e['desc'])
    geo = 'B%d %dx%dx%d->%dx%dx%d k%dx%d s%d p%d,%d pitch %d/%d dgrad_c %d/%d' % (
        d.batch, d.in_h, d.in_w, d.in_c, d.out_h, d.out_w, d.out_c, d.kh, d.kw, d.stride_h, d.pad_top, d.pad_left, d.in_pitch, d.out_pitch,
        d.dgrad_c, d.adj_dgrad_c)
    rows, cols, tiles, splits = e['plan']
    return '%s %s%s [%s] path %s flags %d layout %s acc %s | tile %dx%d x%d splits %d | %s' % (
        '/'.join(e['ops'][:2]) + ('+%d' % (len(e['ops']) - 2) if len(e['ops']) > 2 else ''), e['role'], ' (transposed)' if e['transposed'] else '',
        geo, e['path'], e['flags'], e['layout'], e['accumulate'], rows, cols, tiles, splits, ','.join(e['programs']))
