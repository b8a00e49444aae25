"""Every conv launch of the benchmark's programs, at its exact descriptor and through its exact ABI entry, elementwise against
float64 (oracle/tf_ops.py, on the device).

tests/conv_inventory.py records what the model binds - the look-ahead call pair bench.py times and the plain call path - for
BASELINE configs 2, 3, 4, 5 and a plain-generator model at per-GPU size.  Each distinct entry is replayed here on seeded inputs
through the same entry point with the same descriptor, flags and accumulate value:
  * values: fp32 outputs at TOL_CONV; bf16 outputs at TOL_BF16 against the fp64 result of the bf16-rounded operands; weight
    gradients (float32 in both pipelines) at TOL_CONV; BatchNorm y / mean / rstd behind the epilogue statistics and the slab
    hand-offs at the bars of op_cases.case_conv_bn_stats / case_slab_handoff;
  * bitwise, where acgan_hip.h promises it: the paired launch equals the separate entries, the conv written back by a slab
    hand-off equals the separate reduction, one acg_splitk_reduce_many over all deferred layers of a program equals the per-layer
    reductions;
  * contract edges: fp32 x pad channels hold a non-zero value that must not matter; dx pad channels and the channels at or beyond
    dgrad_c / adj_dgrad_c start at a sentinel and must come back bit-identical - for bf16 outputs too, whose zero pad channels
    (read by the next layer's gather) are stored once by the caller and never written by a conv entry; every workspace keeps its
    canary."""
import ctypes

import pytest
import torch

import conv_inventory as CI
from abi_call import Abi
from op_cases import close
from oracle import tf_ops as T
from test_gpu_ops import TOL_BF16, TOL_CONV

from action_conditioned_gans_amd import _lib as L
from action_conditioned_gans_amd import graph as G

pytestmark = pytest.mark.gpu

X_PAD = 3.0              # fp32 x pad channels: finite and non-zero - they must not reach the result
SENTINEL = -777.0        # outputs start here: channels a call must not write come back bit-identical
BN_TOL = {False: dict(stat=1e-4, y=TOL_CONV, dx=8 * 2e-5, dbeta=8 * 2e-5),          # case_conv_bn_stats / case_slab_handoff bars
          True: dict(stat=2e-3, y=4 * TOL_BF16, dx=8e-3, dbeta=2e-3)}
# the path kinds test_gpu_train.py asserts the model takes (statistics out of the epilogue, split-K slabs handed to BatchNorm
# forward and backward, the paired dgrad + wgrad launch, deferred weight-gradient slabs, the fused deconv bias + tanh): each
# config's inventory must show them, or an empty or degenerate inventory would pass
REQUIRED = {'c2': {'stats', 'fwd_slabs', 'bwd_slabs', 'pair', 'deferred'},
            'c4': {'stats', 'fwd_slabs', 'bwd_slabs', 'pair', 'deferred'},
            'c3': {'stats', 'fwd_slabs', 'bwd_slabs', 'pair', 'deferred', 'f32_head'},
            'c5': {'stats', 'fwd_slabs', 'bwd_slabs', 'pair', 'deferred', 'f32_head'},
            'plain': {'stats', 'pair', 'deferred', 'fused_bias'}}


def _gen(seed):
    return torch.Generator(device='cuda:0').manual_seed(seed)


def _r8(c):
    return (c + 7) // 8 * 8


class Layer:
    """Seeded operands of one conv geometry and their float64 images under the descriptor's conv C (x on the in side, y on the
    out side; a transposed layer's descriptor is its adjoint):  C(A), C^T(B) and dW(A, B) = d<C_w(A), B>/dw.  A conv's fwd /
    dgrad / wgrad are C(A), C^T(B), dW(A, B); a transposed layer's are C^T(B), C(A), dW(A, B) with x = B, dy = A."""

    def __init__(self, d, half, seed):
        self.d, self.half = d, half
        dev = torch.device('cuda:0')
        r = (lambda t: t.bfloat16().float()) if half else (lambda t: t)
        g = _gen(seed)
        self.A = r(torch.rand((d.batch, d.in_h, d.in_w, d.in_c), generator=g, device=dev) * 2 - 1)
        self.B = r(torch.randn((d.batch, d.out_h, d.out_w, d.out_c), generator=g, device=dev))
        self.w = r(torch.randn((d.kh, d.kw, d.in_c, d.out_c), generator=g, device=dev) * 0.1)
        pad = None
        for p in ('SAME', 'VALID'):
            oh, ow, pt, _, pl, _ = T.conv_geometry(d.in_h, d.in_w, d.kh, d.kw, d.stride_h, d.stride_w, p)
            if (oh, ow, pt, pl) == (d.out_h, d.out_w, d.pad_top, d.pad_left):
                pad = p
        assert pad is not None and d.stride_h == d.stride_w, 'descriptor is neither SAME nor VALID: %s' % (d.key(),)
        a, w = self.A.double().requires_grad_(True), self.w.double().requires_grad_(True)
        y = T.conv2d(a, w, d.stride_h, pad)
        self.CA = y.detach()
        self.CtB, self.dW = torch.autograd.grad(y, [a, w], self.B.double())
        del y, a, w


def _lay(t, pitch, dtype, pad_fill=0.0):
    out = torch.full(t.shape[:-1] + (pitch,), pad_fill, dtype=dtype, device=t.device)
    out[..., :t.shape[-1]] = t.to(dtype)
    return out


class Replay:
    def __init__(self, abi, inv):
        self.abi, self.inv, self.half = abi, inv, inv.conv_dtype == L.ACG_BF16
        self.store = torch.bfloat16 if self.half else torch.float32
        self.layers, self.checks, self.ws = {}, 0, []

    # ---- operands
    def layer(self, d):
        geo = L.ConvDesc(*d.key())
        geo.in_pitch = geo.out_pitch = geo.dgrad_c = geo.adj_dgrad_c = 0
        k = geo.key()
        if k not in self.layers:
            self.layers[k] = Layer(geo, self.half, 7 + len(self.layers))
        return self.layers[k]

    def pitch(self, d, side):
        c, p = (d.in_c, d.in_pitch) if side == 'in' else (d.out_c, d.out_pitch)
        if self.half:
            assert p in (0, _r8(c)), 'bf16 tensor at pitch %d for %d channels' % (p, c)
            return _r8(c)
        return p or c

    def tensor(self, d, side, t, pad_fill=0.0):
        return _lay(t, self.pitch(d, side), self.store, 0.0 if self.half else pad_fill)

    def output(self, d, side, dtype=None):
        c = d.in_c if side == 'in' else d.out_c
        shape = (d.batch, d.in_h, d.in_w) if side == 'in' else (d.batch, d.out_h, d.out_w)
        return torch.full(shape + (self.pitch(d, side),), SENTINEL, dtype=dtype or self.store, device='cuda:0'), c

    def keep(self, *ws):
        self.ws += [w for w in ws if w is not None]

    # ---- checks
    def check_out(self, got, ref, c, n, tag, tol=None):
        """``got`` [.., pitch] started at SENTINEL: channels [0, n) against ``ref``; [n, c) and the pad channels [c, pitch) untouched."""
        tol = tol if tol is not None else (TOL_BF16 if (self.half and got.dtype == torch.bfloat16) else TOL_CONV)
        close(got[..., :n].float(), ref[..., :n], tol, tag)
        sent = torch.tensor(SENTINEL, dtype=got.dtype)
        if n < c:
            assert bool((got[..., n:c].cpu() == sent).all()), '%s: channels [%d, %d) beyond dgrad_c were written' % (tag, n, c)
        if got.shape[-1] > c:          # (bf16 too: the zero pad channels the next gather reads are the caller's, never written)
            assert bool((got[..., c:].cpu() == sent).all()), '%s: pad channels [%d, %d) were written' % (tag, c, got.shape[-1])
        self.checks += 1

    @staticmethod
    def bitwise(a, b, tag):
        a, b = a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)
        assert a.shape == b.shape and bool(torch.equal(a, b)), '%s: not bit-identical (%d bytes differ)' % (tag, int((a != b).sum()))

    def bn_fwd_ref(self, conv, bn, beta, tag, y, mean, rstd):
        """y / mean / rstd against float64 BatchNorm + activation of the conv output as stored."""
        c, g = bn['c'], bn['groups']
        rows = conv[..., :c].double().reshape(g, -1, c)
        m, v = rows.mean(1), rows.var(1, unbiased=False)
        t = BN_TOL[self.half]
        close(mean, m.reshape(-1), t['stat'], tag + ' bn mean')
        close(rstd, (1.0 / torch.sqrt(v + bn['eps'])).reshape(-1), t['stat'], tag + ' bn rstd')
        pre = (rows - m[:, None]) / torch.sqrt(v[:, None] + bn['eps']) + beta.double()
        want = _act(pre, bn['act'], bn['leak']).reshape(conv[..., :c].shape)
        close(y[..., :c].float(), want, t['y'], tag + ' bn y')
        self.checks += 1

    @staticmethod
    def beta(c, seed):
        return torch.randn((c,), generator=_gen(seed), device='cuda:0') * 0.5

    # ---- entries
    def run(self, e):
        d = L.ConvDesc(*e['desc'])
        getattr(self, 'do_' + e['role'])(e, d, self.layer(d), CI.describe(e) + ' (%s)' % self.inv.cfg)
        self.abi.sync()
        for w in self.ws:
            Abi.canary_intact(w)
        self.ws = []

    def _fwd_io(self, e, d, lay):
        """(x laid out, reference, output side)"""
        if e['transposed']:
            return self.tensor(d, 'out', lay.B), lay.CtB, 'in'
        return self.tensor(d, 'in', lay.A, X_PAD), lay.CA, 'out'

    def do_fwd(self, e, d, lay, tag):
        abi, path = self.abi, e['path']
        x, ref, side = self._fwd_io(e, d, lay)
        if path == 'fused_bias':
            act, leak = e['bias_act']
            bias = torch.randn((d.in_c,), generator=_gen(5), device='cuda:0') * 0.5
            y = torch.full((d.batch, d.in_h, d.in_w, d.in_pitch or d.in_c), SENTINEL, device='cuda:0')
            abi.fwd_bias_act_d(d, x, lay.w, bias, y, act, leak)
            abi.sync()
            self.check_out(y, _act(ref + bias.double(), act, leak), d.in_c, d.in_c, tag + ' fused bias+act', tol=TOL_CONV)
            return
        if path == 'f32_head':
            y, c = self.output(d, side, torch.float32)
            self.keep(abi.fwd_d(d, e['transposed'], x, lay.w, y, L.dtype2(L.ACG_BF16, L.ACG_F32)))
            abi.sync()
            close(y[..., :c], ref, TOL_CONV, tag + ' bf16->fp32 head')
            self.checks += 1
            return
        y_plain, c = self.output(d, side)
        self.keep(abi.fwd_d(d, e['transposed'], x, lay.w, y_plain))
        abi.sync()
        self.check_out(y_plain, ref, c, c, tag + ' plain entry')
        if path == 'plain':
            return
        bn = e['bn']
        beta = self.beta(c, 11)
        y_dtype = torch.float32 if bn['y_f32'] else self.store
        yb = torch.zeros(y_plain.shape[:-1] + (bn['yp'],), dtype=y_dtype, device='cuda:0')
        mean, rstd = abi.empty(bn['groups'] * c), abi.empty(bn['groups'] * c)
        code = L.dtype2(L.code(self.store), L.code(y_dtype))
        conv, _ = self.output(d, side)
        assert conv.shape[-1] == bn['xp'], (conv.shape, bn)
        if path == 'stats':
            got = abi.fwd_stats_d(d, e['transposed'], x, lay.w, conv, bn['groups'])
            assert got is not None, tag + ': bound to the statistics epilogue but acg_conv2d_stats_layout says no'
            part, nblk, brows, rrows, ws = got
            self.keep(ws)
            abi.lib.bn_act_fwd_partials(_p(conv), _p(beta), _p(part), nblk, brows, rrows, _p(yb), _p(mean), _p(rstd), bn['rows'], c, bn['xp'],
                                        bn['yp'], bn['groups'], bn['eps'], CI.ACTS[bn['act']], bn['leak'], code, abi.stream())
            abi.sync()
            self.check_out(conv, ref, c, c, tag + ' stats conv')
        else:
            ws, splits = abi.fwd_slabs_d(d, e['transposed'], x, lay.w, e['layout'])
            bws, n = abi.bn_ws(bn['rows'], c, bn['groups'])
            self.keep(ws)
            abi.lib.bn_act_fwd_slabs(_p(ws), splits, _p(conv), _p(beta), _p(yb), _p(mean), _p(rstd), bn['rows'], c, bn['xp'], bn['yp'],
                                     bn['groups'], bn['eps'], CI.ACTS[bn['act']], bn['leak'], code, e['layout'], e['bn_flags'], _p(bws), n,
                                     abi.stream())
            abi.sync()
            Abi.no_timeout(bws)
            # the write-back is what the separate reduction stores; the pad channels are not part of the promise
            self.bitwise(conv[..., :c], y_plain[..., :c], tag + ' slab write-back vs separate reduction')
        self.bn_fwd_ref(conv, bn, beta, tag, yb, mean, rstd)

    def _dgrad_io(self, e, d, lay):
        """(dy laid out, reference, dx side, computed channels)"""
        if e['transposed']:
            return self.tensor(d, 'in', lay.A), lay.CA, 'out', d.adj_dgrad_c or d.out_c
        return self.tensor(d, 'out', lay.B), lay.CtB, 'in', d.dgrad_c or d.in_c

    def _wgrad_io(self, e, d, lay):
        """(x, dy) of the layer's weight gradient, laid out"""
        if e['transposed']:
            return self.tensor(d, 'out', lay.B), self.tensor(d, 'in', lay.A)
        return self.tensor(d, 'in', lay.A, X_PAD), self.tensor(d, 'out', lay.B)

    def dw0(self, lay, seed):
        return torch.randn(lay.w.shape, generator=_gen(seed), device='cuda:0')

    def check_dw(self, dw, lay, dw0, acc, tag):
        close(dw, acc * dw0.double() + lay.dW, TOL_CONV, tag)
        self.checks += 1

    def do_dgrad(self, e, d, lay, tag):
        abi, path = self.abi, e['path']
        dy, ref, side, n = self._dgrad_io(e, d, lay)
        dx_plain, c = self.output(d, side)
        self.keep(abi.dgrad_d(d, e['transposed'], dy, lay.w, dx_plain))
        abi.sync()
        self.check_out(dx_plain, ref, c, n, tag + ' dgrad plain entry')
        slabs = None
        if e['layout'] is not None:
            slabs = abi.dgrad_slabs_d(d, e['transposed'], dy, lay.w, e['layout'])
            self.keep(slabs[0])
        if path == 'pair':
            f, acc = e['flags'], e['accumulate']
            x, dyw = self._wgrad_io(e, d, lay)
            dw0 = self.dw0(lay, 13)
            dx, _ = self.output(d, side)
            dw = dw0.clone()
            wsd, wsw = abi.bwd_pair_d(d, e['transposed'], dy, lay.w, x, None if f & 2 else dx, None if f & 1 else dw, acc, f)
            self.keep(wsd, wsw)
            abi.sync()
            if f & 2:
                self.bitwise(wsd, slabs[0], tag + ' pair input-gradient slabs vs acg_*_dgrad_slabs')
            else:
                self.bitwise(dx, dx_plain, tag + ' pair dx vs separate dgrad')
            if f & 1:
                ws_sep, splits = abi.wgrad_slabs_d(d, e['transposed'], x, dyw)
                self.keep(ws_sep)
                abi.sync()
                self.bitwise(wsw, ws_sep, tag + ' pair weight-gradient slabs vs acg_*_wgrad_slabs')
            else:
                dw_sep = dw0.clone()
                self.keep(abi.wgrad_d(d, e['transposed'], x, dyw, dw_sep, acc))
                abi.sync()
                self.bitwise(dw, dw_sep, tag + ' pair dw vs separate wgrad')
                self.check_dw(dw, lay, dw0, acc, tag + ' pair dw')
        if slabs is None:
            return
        # BatchNorm backward reading the input-gradient slabs (acg_bn_act_bwd_slabs) against float64 BatchNorm backward of the
        # plain entry's dx (checked above against float64)
        bn = e['bn']
        assert dx_plain.shape[-1] == bn['xp'], (dx_plain.shape, bn)
        g = _gen(17)
        xb64 = torch.randn(dx_plain.shape[:-1] + (c,), generator=g, device='cuda:0') * 1.5 + 0.7
        xb = _lay(xb64, bn['xp'], self.store)
        beta = self.beta(c, 19)
        xs = xb[..., :c].double()
        rows = xs.reshape(bn['groups'], -1, c)
        m, v = rows.mean(1), rows.var(1, unbiased=False)
        mean, rstd = m.reshape(-1).float(), (1.0 / torch.sqrt(v + bn['eps'])).reshape(-1).float()
        dxb = torch.zeros_like(xb)
        dbeta = abi.empty(c)
        bws, nb = abi.bn_ws(bn['rows'], c, bn['groups'])
        abi.lib.bn_act_bwd_slabs(_p(xb), _p(slabs[0]), slabs[1], _p(beta), _p(mean), _p(rstd), _p(dxb), _p(dbeta), 0.0, bn['rows'], c, bn['xp'],
                                 bn['yp'], bn['groups'], CI.ACTS[bn['act']], bn['leak'], L.dtype2(L.code(self.store), L.code(self.store)),
                                 e['layout'], e['bn_flags'], _p(bws), nb, abi.stream())
        abi.sync()
        Abi.no_timeout(bws)
        xr = xs.clone().requires_grad_(True)
        br = beta.double().requires_grad_(True)
        rr = xr.reshape(bn['groups'], -1, c)
        mu = rr.mean(1, keepdim=True)          # batch statistics as functions of x: slim batch_norm's gradient flows through them
        pre = (rr - mu) / torch.sqrt(((rr - mu) ** 2).mean(1, keepdim=True) + bn['eps']) + br
        out = _act(pre, bn['act'], bn['leak']).reshape(xs.shape)
        dx_ref, db_ref = torch.autograd.grad(out, [xr, br], dx_plain[..., :c].double())
        t = BN_TOL[self.half]
        close(dxb[..., :c].float(), dx_ref, t['dx'], tag + ' bn bwd from slabs dx')
        close(dbeta, db_ref, t['dbeta'], tag + ' bn bwd from slabs dbeta')
        self.checks += 1

    def do_wgrad(self, e, d, lay, tag):
        abi, acc = self.abi, e['accumulate']
        x, dy = self._wgrad_io(e, d, lay)
        dw0 = self.dw0(lay, 23)
        dw = dw0.clone()
        self.keep(abi.wgrad_d(d, e['transposed'], x, dy, dw, acc))
        abi.sync()
        self.check_dw(dw, lay, dw0, acc, tag + ' wgrad')
        if e['path'] == 'deferred':
            ws, splits = abi.wgrad_slabs_d(d, e['transposed'], x, dy)
            self.keep(ws)
            out = dw0.clone()
            abi.splitk_reduce_many([(ws, out, splits, acc)])
            abi.sync()
            self.bitwise(out, dw, tag + ' slabs + acg_splitk_reduce_many vs acg_*_wgrad')

    def reduce_list(self, program, items):
        """One acg_splitk_reduce_many over every deferred layer of a program, in the list shape WgradReduceOp builds (chunks of
        ACG_REDUCE_MAX, accumulate per entry, the optimizer's step counter on the first launch), against per-layer reductions."""
        abi = self.abi
        entries, singles, refs = [], [], []
        for i, (key, splits, acc) in enumerate(items):
            e = self.inv.entries[key]
            d = L.ConvDesc(*e['desc'])
            lay = self.layer(d)
            x, dy = self._wgrad_io(e, d, lay)
            ws, s = abi.wgrad_slabs_d(d, e['transposed'], x, dy)
            assert s == splits, (CI.describe(e), s, splits)
            self.keep(ws)
            dw0 = self.dw0(lay, 29 + i)
            entries.append((ws, dw0.clone(), splits, acc))
            singles.append((ws, dw0.clone(), splits, acc))
            refs.append((lay, dw0, acc))
        step = torch.zeros(4, dtype=torch.int32, device='cuda:0')
        for lo in range(0, len(entries), L.REDUCE_MAX):
            abi.splitk_reduce_many(entries[lo:lo + L.REDUCE_MAX], step=step[:1] if lo == 0 else None)
        for s in singles:
            abi.splitk_reduce_many([s])
        abi.sync()
        assert int(step[0]) == 1 and bool((step[1:] == 0).all()), 'step counter %s' % step.tolist()
        for (key, _, _), a, b, (lay, dw0, acc) in zip(items, entries, singles, refs):
            tag = '%s (%s, %s)' % (CI.describe(self.inv.entries[key]), self.inv.cfg, program)
            self.bitwise(a[1], b[1], '%s: reduce list of %d vs per-layer reduction' % (tag, len(items)))
            self.check_dw(a[1], lay, dw0, acc, tag + ' reduced dw')
        for w in self.ws:
            Abi.canary_intact(w)
        self.ws = []
        self.checks += 1


def _act(t, act, leak):
    if act == 'relu':
        return torch.relu(t)
    if act == 'lrelu':
        return torch.where(t > 0, t, leak * t)
    if act == 'tanh':
        return torch.tanh(t)
    assert act is None, act
    return t


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _summary(inv):
    counts = {}
    for e in inv.entries.values():
        counts[(e['role'], e['path'])] = counts.get((e['role'], e['path']), 0) + 1
    return ', '.join('%s/%s %d' % (r, p, n) for (r, p), n in sorted(counts.items()))


_DONE = set()        # entries already verified by an earlier config of this run (c2 and c4 share most of their launches)


@pytest.mark.timeout(900)
@pytest.mark.parametrize('cfg', list(CI.CONFIGS))
def test_every_conv_launch_of_the_bench_step(cfg, monkeypatch, hip_abi):
    inv, sess, tr = CI.record(monkeypatch, lambda **kw: G.Session(device='cuda:0', **kw), cfg)
    monkeypatch.undo()
    missing = REQUIRED[cfg] - inv.kinds()
    assert not missing, '%s: the inventory has no %s launches (%s)' % (cfg, sorted(missing), _summary(inv))
    assert inv.reduces, cfg + ': no deferred weight-gradient reduction in any program'
    abi = Abi(hip_abi.lib, 'cuda:0', conv_dtype=inv.conv_dtype)
    rep = Replay(abi, inv)
    failures, ran = [], 0
    for key, e in inv.entries.items():
        if key in _DONE:
            continue
        try:
            rep.run(e)
            _DONE.add(key)
            ran += 1
        except (AssertionError, L.AcgError) as exc:
            failures.append('%s (%s): %s' % (CI.describe(e), cfg, str(exc).split('\n')[0]))
    for program, items in inv.reduces:
        try:
            rep.reduce_list(program, items)
        except (AssertionError, L.AcgError) as exc:
            failures.append('%s reduce list %s: %s' % (cfg, program, str(exc).split('\n')[0]))
    print('%s: %d entries (%d replayed here), %d reduce lists, %d checks: %s' % (cfg, len(inv.entries), ran, len(inv.reduces), rep.checks,
                                                                               _summary(inv)))
    sess.close()
    del rep, sess, tr
    torch.cuda.empty_cache()
    assert not failures, '%d of %d conv launches off:\n  %s' % (len(failures), len(inv.entries), '\n  '.join(failures))
