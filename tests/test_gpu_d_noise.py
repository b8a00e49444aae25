"""GPU: instance noise on the discriminator's inputs (include/acgan_rollout.h: acg_inst_noise_prepare / acg_inst_noise_add;
ops.InstNoisePrepareOp / InstNoiseOp; Trainer d_noise) and the D statistics (acg_logit_stats; Trainer d_stats).  The kernels
against the float64 restatement of tests/d_noise_ref.py with guard bands on both sides of every buffer, and a Trainer with noise
against the fp64 oracle that judges the same noisy frames.

Tolerances.  Copied channels, pad channels, keys, counters and sigma are compared bitwise.  A noisy float32 value is one float32
fused multiply-add of (sigma, z, in): against float64 it may be off by sigma * |z32 - z64| plus half an ulp of the result, so the
bar is sigma * Z_TOL + 2^-24 * |out| with Z_TOL the bound tests/test_gpu_noise.py derived and measured for the same normals()
(4 x 1.66e-6).  A bf16 value is that float32 result rounded to nearest even: it equals the rounded float64 reference except
where the reference lies within the float32 bar of a rounding boundary, where either neighbour - one bf16 ulp apart - is right;
so the bar is [round(ref - bar), round(ref + bar)]."""
import ctypes
import json

import numpy as np
import pytest
import torch

import d_noise_ref as R
import train_cases as TC
from action_conditioned_gans_amd import _lib
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T
from action_conditioned_gans_amd.saver import Saver
from oracle import models as OM

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
Z_TOL = min(4 * 1.66e-6, 2e-5)       # tests/test_gpu_noise.py
GUARD = 64                           # elements on either side of every buffer (256 bytes of float32: the payload stays aligned)
SENTINEL = -7.25                     # exact in bf16 too
I64_SENTINEL = -0x0123456789abcdef


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _i64(v):
    return v - 2 ** 64 if v >= 2 ** 63 else v


_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.int64: torch.int64}


class Band:
    """A device buffer of n elements with a guard band on both sides; ``shift`` elements move the payload off its alignment."""

    def __init__(self, n, dtype=torch.float32, shift=0, values=None):
        self.fill = I64_SENTINEL if dtype == torch.int64 else SENTINEL
        self.full = torch.full((GUARD + shift + n + GUARD,), self.fill, dtype=dtype, device=DEV)
        self.lo, self.hi = GUARD + shift, GUARD + shift + n
        self.t = self.full[self.lo:self.hi]
        if values is not None:
            self.t.copy_(torch.as_tensor(values, dtype=dtype).reshape(-1))

    def bits(self):
        """The payload's bits on the host; asserts the guards are untouched."""
        torch.cuda.synchronize()
        host = self.full.view(_INT[self.full.dtype]).cpu().numpy()
        want = torch.full((1,), self.fill, dtype=self.full.dtype).view(_INT[self.full.dtype]).numpy()[0]
        assert (host[:self.lo] == want).all() and (host[self.hi:] == want).all(), 'written outside the buffer'
        return host[self.lo:self.hi].copy()

    def untouched(self):
        torch.cuda.synchronize()
        host = self.full.view(_INT[self.full.dtype]).cpu().numpy()
        want = torch.full((1,), self.fill, dtype=self.full.dtype).view(_INT[self.full.dtype]).numpy()[0]
        return bool((host == want).all())

    def values(self):
        self.bits()
        return self.t.cpu()


# ---- acg_inst_noise_prepare ---------------------------------------------------------------------------------------------------
class Prepare:
    def __init__(self, seed, counter, updates):
        self.lib = _lib.get()
        self.state, self.updates = Band(2, torch.int64, values=[_i64(seed), _i64(counter)]), Band(1, torch.int64, values=[_i64(updates)])
        self.key, self.sigma = Band(2, torch.int64), Band(1)

    def launch(self, start, final, offset, decay, advance, **over):
        kw = dict(state=_p(self.state.t), updates=_p(self.updates.t), key=_p(self.key.t), sigma=_p(self.sigma.t))
        kw.update(over)
        self.lib.inst_noise_prepare(kw['state'], kw['updates'], kw['key'], kw['sigma'], start, final, offset, decay, advance, _stream())

    def read(self):
        u64 = lambda band: tuple(int(v) % 2 ** 64 for v in band.bits())      # noqa: E731
        return u64(self.state), u64(self.updates)[0], u64(self.key), self.sigma.bits().view(np.float32)[0]


@pytest.mark.parametrize('advance', [1, 0], ids=['advance', 'hold'])
def test_prepare_is_exact_and_a_second_call_moves_on(advance):
    """Both halves of seed and counter are non-zero; the counter wraps at 2^64 in the second case."""
    for seed, counter in ((0x123456789abcdef, 2 ** 32 + 5), (2 ** 64 - 3, 2 ** 64 - 1)):
        call = Prepare(seed, counter, 5)
        sched = (0.8, 0.1, 2, 7)
        state, updates = (seed, counter), 5
        for n in range(3):
            call.launch(*sched, advance)
            key, sigma, state, updates = R.prepare(state, updates, *sched, advance)
            got = call.read()
            assert got[0] == state and got[1] == updates and got[2] == key, (n, got)
            assert got[3].view(np.uint32) == sigma.view(np.uint32), (n, got[3], sigma)
        assert state == (seed, (counter + 3) % 2 ** 64) and updates == 5 + 3 * advance


@pytest.mark.parametrize('sched', [(0.8, 0.1, 2, 7), (0.1, 0.0, 0, 3), (0.25, 1.5, 1, 4), (0.3, 0.9, 5, 0), (0.0, 0.0, 0, 0),
                                   (1e-3, 3.0e38, 0, 2 ** 40)], ids=str)
def test_sigma_matches_the_restatement_bitwise(sched):
    call = Prepare(7, 0, 0)
    for k in (0, 1, 2, 3, 6, 9, 10, 2 ** 40 + 1, 2 ** 64 - 1):
        call.updates.t.fill_(_i64(k))
        call.launch(*sched, 0)
        got = call.read()
        want = R.sigma(k, *sched)
        assert got[3].view(np.uint32) == want.view(np.uint32), (k, got[3], want)
        assert got[1] == k


@pytest.mark.parametrize('over', [dict(state=None), dict(updates=None), dict(key=None), dict(sigma=None), dict(start=-0.5), dict(start=float('nan')),
                                  dict(start=float('inf')), dict(final=-1e-3), dict(final=float('nan')), dict(final=float('inf')),
                                  dict(offset=-1), dict(decay=-1)], ids=str)
def test_prepare_refusals_launch_nothing(over):
    call, over = Prepare(7, 5, 3), dict(over)
    kw = dict(start=0.5, final=0.1, offset=0, decay=4)
    kw.update({k: over.pop(k) for k in list(over) if k in kw})
    with pytest.raises(_lib.AcgError, match='inst_noise_prepare'):
        call.launch(kw['start'], kw['final'], kw['offset'], kw['decay'], 1, **over)
    assert call.read()[:2] == ((7, 5), 3) and call.key.untouched() and call.sigma.untouched()


# ---- acg_inst_noise_add -------------------------------------------------------------------------------------------------------
# (pixels, c, pitch, c0, cn): the issue's five, and one above 2048 blocks x 256 threads, where the grid-stride loop comes round
SHAPES = [(1, 1, 1, 0, 1), (5, 6, 8, 3, 3), (257, 4, 4, 0, 4), (12288, 6, 8, 3, 3), (70001, 3, 3, 1, 2), (2048 * 256 + 4097, 4, 4, 1, 2)]
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}
KEY = (0x123456789abcdef, 2 ** 32 + 5)
SPECIALS = np.array([-0.0, 1e-40, 3.0e38], np.float32)


def _input(shape, dtype, seed=0):
    """[pixels, pitch] stored values (float32 array holding what the storage type holds): N(0, 1), and -0.0, a denormal and
    3e38 among the channels that are copied (pad channels included)."""
    pixels, c, pitch, c0, cn = shape
    rng = np.random.default_rng(seed + pixels)
    x = rng.standard_normal((pixels, pitch)).astype(np.float32)
    copied = [ch for ch in range(pitch) if not c0 <= ch < c0 + cn]
    for i, ch in enumerate(copied):
        rows = np.arange(i % 3, pixels, 3)
        x[rows, ch] = SPECIALS[(rows // 3 + i) % 3]
    return torch.from_numpy(x).to(dtype)


class Add:
    def __init__(self, shape, dtype, x, sigma, key=KEY, shift=0):
        self.lib = _lib.get()
        self.shape, self.dtype = shape, dtype
        pixels, c, pitch, c0, cn = shape
        self.src, self.dst = Band(pixels * pitch, dtype, shift, x), Band(pixels * pitch, dtype, shift)
        self.key, self.sigma = Band(2, torch.int64, values=[_i64(key[0]), _i64(key[1])]), Band(1, values=[sigma])

    def launch(self, stream_id=0, **over):
        pixels, c, pitch, c0, cn = self.shape
        kw = dict(src=_p(self.src.t), dst=_p(self.dst.t), key=_p(self.key.t), sigma=_p(self.sigma.t), pixels=pixels, c=c, pitch=pitch, c0=c0,
                  cn=cn, dtype=_lib.code(self.dtype))
        kw.update(over)
        self.lib.inst_noise_add(kw['src'], kw['dst'], kw['key'], kw['sigma'], kw['pixels'], kw['c'], kw['pitch'], kw['c0'], kw['cn'], kw['dtype'],
                                stream_id, _stream())

    def result(self):
        """-> (bits of the output, its values as float64 [pixels, pitch]); key, sigma and the input are read, never written."""
        pixels, c, pitch, c0, cn = self.shape
        bits = self.dst.bits().reshape(pixels, pitch)
        return bits, self.dst.values().double().numpy().reshape(pixels, pitch)


def _check_noisy(got, got_bits, x, shape, dtype, key, sigma, stream_id, what):
    """Copied channels bitwise, noisy channels against float64 by the module's rule; -> the largest error seen (bf16: against the
    rounded reference)."""
    pixels, c, pitch, c0, cn = shape
    x_bits = x.view(_INT[dtype]).numpy().reshape(pixels, pitch)
    copied = [ch for ch in range(pitch) if not c0 <= ch < c0 + cn]
    assert np.array_equal(got_bits[:, copied], x_bits[:, copied]), what
    sig = np.float64(np.float32(sigma))
    ref = R.add(x.double().numpy().reshape(pixels, pitch), key, sigma, c0, cn, stream_id)[:, c0:c0 + cn]
    out = got[:, c0:c0 + cn]
    err = float(np.abs(out - ref).max())
    if dtype == torch.float32:
        bar = sig * Z_TOL + 2.0 ** -24 * np.abs(out)
        assert (np.abs(out - ref) <= bar).all(), (what, err)
    else:
        bar = sig * Z_TOL + 2.0 ** -24 * np.abs(ref)
        lo, hi = R.round_bf16(ref - bar), R.round_bf16(ref + bar)
        assert ((lo <= out) & (out <= hi)).all(), (what, err)
        exact = R.round_bf16(ref)
        err = float(np.abs(out - exact).max())
        print('%s: %d of %d bf16 values sit on the other side of a rounding boundary' % (what, int((out != exact).sum()), out.size))
    print('inst_noise_add %s %s sigma=%g: max |out - reference| = %.3e' % (what, shape, sigma, err))
    return err


@pytest.mark.parametrize('name', list(DTYPES))
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_add_matches_the_restatement_on_both_paths(shape, name):
    """Aligned buffers take the 16-byte path where the pitch allows it, buffers 4 bytes off the element path: the same bits.
    The same call twice gives the same bits."""
    dtype, sigma, sid = DTYPES[name], 0.75, 66
    x = _input(shape, dtype)
    runs = []
    for shift in (0, 4 // x.element_size(), 0):
        call = Add(shape, dtype, x, sigma, shift=shift)
        call.launch(sid)
        runs.append(call.result())
        assert np.array_equal(call.src.bits(), x.view(_INT[dtype]).numpy().reshape(-1))          # inputs are read only
        assert tuple(int(v) % 2 ** 64 for v in call.key.bits()) == KEY and call.sigma.values()[0] == np.float32(sigma)
    _check_noisy(runs[0][1], runs[0][0], x, shape, dtype, KEY, sigma, sid, name)
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][0], runs[2][0])
    call.dst.t.fill_(SENTINEL)
    call.launch(sid)                                                                  # the same call site again
    assert np.array_equal(call.result()[0], runs[0][0])


@pytest.mark.parametrize('name', list(DTYPES))
def test_stream_ids_and_counters_give_different_noise(name):
    dtype, shape = DTYPES[name], (257, 4, 4, 0, 4)
    x = _input(shape, dtype)
    outs = {}
    for key, sid in ((KEY, 0), (KEY, 1), ((KEY[0], KEY[1] + 1), 0), ((KEY[0] + 1, KEY[1]), 0), (KEY, 64)):
        call = Add(shape, dtype, x, 1.0, key=key)
        call.launch(sid)
        bits, vals = call.result()
        _check_noisy(vals, bits, x, shape, dtype, key, 1.0, sid, '%s key %r stream %d' % (name, key, sid))
        outs[(key, sid)] = vals - x.double().numpy().reshape(vals.shape)
    keys = list(outs)
    for i, a in enumerate(keys):
        for b in keys[:i]:
            assert np.mean(np.isclose(outs[a], outs[b], rtol=0, atol=1e-2)) < 0.05, (a, b)       # unrelated normals rarely meet


@pytest.mark.parametrize('name', list(DTYPES))
@pytest.mark.parametrize('shape', [(5, 6, 8, 3, 3), (70001, 3, 3, 1, 2)], ids=str)
def test_sigma_0_is_a_bitwise_copy(shape, name):
    dtype = DTYPES[name]
    x = _input(shape, dtype).view(-1, shape[2]).clone()
    x[::2, shape[3]] = -0.0                                   # -0.0 in a noisy channel stays -0.0
    x[1::2, shape[3]] = 1e-40
    for shift in (0, 4 // x.element_size()):
        call = Add(shape, dtype, x, 0.0, shift=shift)
        call.launch(3)
        assert np.array_equal(call.result()[0].reshape(-1), x.view(_INT[dtype]).numpy().reshape(-1))


@pytest.mark.parametrize('over', [dict(src=None), dict(dst=None), dict(key=None), dict(sigma=None), dict(dst='src'), dict(c0=4, cn=3), dict(c0=6, cn=1),
                                  dict(c=9), dict(c=0), dict(cn=5, c0=0), dict(cn=0), dict(c0=-1), dict(pixels=0), dict(pixels=-3),
                                  dict(pixels=2 ** 32), dict(dtype=2), dict(dtype=0x110)], ids=str)
def test_add_refusals_write_nothing(over):
    shape = (5, 6, 8, 3, 3)
    call = Add(shape, torch.float32, _input(shape, torch.float32), 0.5)
    if over.get('dst') == 'src':
        over = dict(dst=_p(call.src.t))
    with pytest.raises(_lib.AcgError, match='inst_noise_add'):
        call.launch(0, **over)
    assert call.dst.untouched()
    assert np.array_equal(call.src.bits(), _input(shape, torch.float32).view(torch.int32).numpy().reshape(-1))


# ---- acg_logit_stats ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 7, 64])
def test_logit_stats(n):
    lib = _lib.get()
    rng = np.random.default_rng(n)
    for trial in range(3):
        fake, real = (rng.standard_normal(n) * 3).astype(np.float32), (rng.standard_normal(n) * 3 + 0.5).astype(np.float32)
        fake[::3], real[1::4] = 0.0, 0.0                      # a zero is neither fake < 0 nor real > 0
        if trial == 1:
            fake, real = -np.abs(fake) - 1, np.abs(real) + 1  # D is right everywhere
        if trial == 2:
            real[0] = -0.0
        f, r, out = Band(n, values=fake), Band(n, values=real), Band(4)
        lib.logit_stats(_p(f.t), _p(r.t), n, _p(out.t), _stream())
        got = out.bits().view(np.float32)
        want = R.logit_stats(fake, real)
        print('logit_stats n=%d: %s vs %s' % (n, got, want))
        for k in (0, 1):
            assert abs(float(got[k]) - want[k]) <= 1e-6 * abs(want[k]), (k, got, want)
        assert got[2] == np.float32(want[2]) and got[3] == np.float32(want[3])
        assert np.array_equal(f.bits().view(np.float32).view(np.uint32), fake.view(np.uint32))
    for bad in (dict(f=None), dict(r=None), dict(o=None), dict(n=0), dict(n=-1)):
        kw = dict(dict(f=_p(f.t), r=_p(r.t), o=_p(out.t), n=n), **bad)
        out.full.fill_(SENTINEL)
        with pytest.raises(_lib.AcgError, match='logit_stats'):
            lib.logit_stats(kw['f'], kw['r'], kw['n'], kw['o'], _stream())
        assert out.untouched()


# ---- Trainer ------------------------------------------------------------------------------------------------------------------
B, S, K, SEED = 4, 64, 5, 0xfeedface12345678
NOISE = dict(d_noise=0.5, d_noise_final=0.125, d_noise_decay_steps=4, d_noise_offset=1, d_noise_seed=SEED)
SCHED = (0.5, 0.125, 1, 4)


def _inputs(seed=21):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (B, S, S, 3)).astype(np.float32)
    y = np.clip(np.roll(x, 2, axis=2) + 0.05 * rng.standard_normal(x.shape).astype(np.float32), -1, 1)
    return x, y, rng.standard_normal((B, 10)).astype(np.float32), rng.standard_normal((B, 5)).astype(np.float32)


_PARAMS = {}


def _params(transform):
    """Computed once per generator and shared; never modified (the sessions copy them)."""
    if transform not in _PARAMS:
        _PARAMS[transform] = OM.init_params(transform, batch=B, img=S, ksize=K, seed=3, dtype=torch.float32)
    return _PARAMS[transform]


def _trainer(transform, params=None, dtype='f32', sess_kw=None, **kw):
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device=DEV, dtype=dtype, **(sess_kw or {}))
    tr = T.Trainer(sess, True, 'bce', 'adam', transform, batch_size=B, img_size=S, ksize=K, **kw)
    sess.run(G.global_variables_initializer())
    g = G.get_default_graph()
    if params is not None:
        assert set(params) == set(g.variables)
        for n, v in g.variables.items():
            sess.set_value(v, params[n])
    return sess, tr, g


def _check_d_input(noisy, clean, last, slot, dtype, what):
    """The fetched noisy D input against the restatement from the fetched key and sigma and the fetched clean input; -> sigma * z
    [rows, S, S, 3] float64 for the oracle."""
    rows = clean.shape[0]
    xs = torch.from_numpy(np.ascontiguousarray(clean)).to(dtype).reshape(-1, 8)
    got = torch.from_numpy(np.ascontiguousarray(noisy)).to(dtype).reshape(-1, 8)
    assert not xs[:, 6:].any() and float(xs[:, :6].abs().max()) > 0.1, what            # pad channels zero, the rest fed / generated
    _check_noisy(got.double().numpy(), got.view(_INT[dtype]).numpy(), xs.reshape(-1), (rows * S * S, 6, 8, 3, 3), dtype, last['key'], last['sigma'],
                 slot, what)
    return (np.float64(np.float32(last['sigma'])) * R.z(last['key'], slot, rows * S * S, 3)).reshape(rows, S, S, 3)


@pytest.mark.parametrize('transform', [True, False], ids=['dna', 'plain'])
def test_d_and_g_step_match_the_oracle_on_the_same_noisy_input(transform):
    """One D step and one G step (bce / Adam): the noisy D inputs against the restatement, then loss, frame and every variable's
    gradient norm within 1e-3 of the fp64 oracle whose discriminator judges frame + the same sigma * z."""
    params = _params(transform)
    sess, tr, g = _trainer(transform, params, **NOISE)
    ot = R.DNoiseOracleTrainer({k: v.double() for k, v in params.items()}, True, 'bce', 'adam', transform, K)
    x, y, a, s = _inputs()
    td = lambda t: torch.from_numpy(t).double()     # noqa: E731
    norms = lambda: {'n/' + k: v.norm() for k, v in ot.last_grads.items()}     # noqa: E731
    assert tr.d_noise_state() == (SEED, 0, 0)

    noisy_t = tr.d_noisy['both']
    res = sess.run([tr.d_opt_op, tr.d_loss, tr.g_next_frame, noisy_t, noisy_t.op.inputs[0], tr.clip_d], tr._feed(x, y, a))
    last = tr.d_noise_last()
    assert last['key'] == (SEED, 0) and np.float32(last['sigma']) == R.sigma(0, *SCHED) and tr.d_noise_state() == (SEED, 1, 1)
    add = _check_d_input(res[3], res[4], last, R.SLOT['both'], torch.float32, 'D(both) input')
    assert np.array_equal(res[4][:B, ..., :3], x) and np.array_equal(res[4][B:, ..., :3], x) and np.array_equal(res[4][B:, ..., 3:6], y)
    ot.d_add = [add[:B], add[B:]]
    od = ot.train_d(td(x), td(y), td(a), return_all=True)
    print('train_d frame rel %.3e, d_loss %.6g vs %.6g' % (TC.rel(res[2], od['frame'].numpy()), res[1][0], float(od['d_loss'])))
    assert TC.rel(res[2], od['frame'].numpy()) <= 1e-3
    assert abs(res[1][0] - float(od['d_loss'])) <= 1e-3 * max(abs(float(od['d_loss'])), 1.0)
    TC.check_norms(TC.flat_grad_norms(sess, tr.d_opt_op), norms(), 'n/', 1e-3, 'D grad')
    for n, v in g.variables.items():                 # every step is compared from one starting point
        ot.p[n] = sess.get_value(v).double()

    noisy_t = tr.d_noisy['gen']
    fetch = [tr.g_opt_op, tr.g_loss, tr.g_next_frame, noisy_t, noisy_t.op.inputs[0]] + ([tr.g_state_out] if transform else [])
    res = sess.run(fetch, tr._feed(x, y, a, s))
    last = tr.d_noise_last()
    assert last['key'] == (SEED, 1) and np.float32(last['sigma']) == R.sigma(1, *SCHED) and tr.d_noise_state() == (SEED, 2, 1)
    add = _check_d_input(res[3], res[4], last, R.SLOT['gen'], torch.float32, 'D(fake) input of the G step')
    assert np.array_equal(res[4][..., 3:6], res[2])
    ot.d_add = [add]
    og = ot.train_g(td(x), td(y), td(a), td(s), return_all=True)
    print('train_g frame rel %.3e, g_loss %.6g vs %.6g' % (TC.rel(res[2], og['frame'].numpy()), res[1][0], float(og['g_loss'])))
    assert TC.rel(res[2], og['frame'].numpy()) <= 1e-3
    if transform:
        assert TC.rel(res[5], og['state'].numpy()) <= 1e-3
    assert abs(res[1][0] - float(og['g_loss'])) <= 1e-3 * abs(float(og['g_loss']))
    TC.check_norms(TC.flat_grad_norms(sess, tr.g_opt_op), norms(), 'n/', 1e-3, 'G grad')
    sess.close()


def test_two_instance_d_step_draws_per_instance():
    """batched_d=False: D(fake) and D(real) of the D step read their own noisy copies under one key and two stream ids."""
    sess, tr, g = _trainer(True, _params(True), batched_d=False, **NOISE)
    x, y, a, s = _inputs(3)
    ng, nr = tr.d_noisy['gen'], tr.d_noisy['real']
    res = sess.run([tr.d_opt_op, ng, ng.op.inputs[0], nr, nr.op.inputs[0], tr.clip_d], tr._feed(x, y, a))
    last = tr.d_noise_last()
    assert last['key'] == (SEED, 0) and tr.d_noise_state() == (SEED, 1, 1)
    zg = _check_d_input(res[1], res[2], last, R.SLOT['gen'], torch.float32, 'D(fake) input')
    zr = _check_d_input(res[3], res[4], last, R.SLOT['real'], torch.float32, 'D(real) input')
    assert not np.isclose(zg, zr).all() and np.array_equal(res[4][..., 3:6], y)
    tr.train_g(x, y, a, s)                           # the shared D(fake) instance in the G step: the schedule stays
    assert tr.d_noise_state() == (SEED, 2, 1) and tr.d_noise_last()['key'] == (SEED, 1)
    sess.close()


def test_schedule_replay_equals_eager_and_g_steps_leave_the_schedule():
    """Run 1 of a program is eager, run 2 captures, runs 3+ replay; against a session that never captures, from the same state and
    weights: sigma and key of every program, the frames and the final weights bit for bit - and sigma follows the schedule of the D
    updates while the G steps draw at the level they find."""
    params = _params(True)
    x, y, a, s = _inputs(7)
    finals = []
    for use_graphs in (False, True):
        sess, tr, g = _trainer(True, params, sess_kw=dict(use_hip_graphs=use_graphs), **NOISE)
        rec = []
        for i in range(6):
            tr.train_d(x, y, a)
            last = tr.d_noise_last()
            assert last['key'] == (SEED, 2 * i) and np.float32(last['sigma']) == R.sigma(i, *SCHED), (i, last)
            assert tr.d_noise_state() == (SEED, 2 * i + 1, i + 1)
            frames = tr.train_g(x, y, a, s)
            last = tr.d_noise_last()
            assert last['key'] == (SEED, 2 * i + 1) and np.float32(last['sigma']) == R.sigma(i + 1, *SCHED), (i, last)
            assert tr.d_noise_state() == (SEED, 2 * i + 2, i + 1)
            rec.append(tr.d_noisy['gen'].buf.detach().cpu().numpy().copy())
        torch.cuda.synchronize()
        finals.append(({n: sess.get_value(v) for n, v in g.variables.items()}, frames, np.stack(rec)))
        if use_graphs:
            assert all(p.graphs is not None for p in sess._programs.values() if p.runs >= 2)
        sess.close()
    (pe, fe, re_), (pg, fg, rg) = finals
    assert np.array_equal(re_.view(np.uint32), rg.view(np.uint32)) and len({r.tobytes() for r in rg}) == 6
    assert np.array_equal(fe.view(np.uint32), fg.view(np.uint32))
    for n in pe:
        assert torch.equal(pe[n], pg[n]), n


def test_a_restored_checkpoint_continues_the_key_and_the_schedule(tmp_path):
    sess, tr, g = _trainer(True, _params(True), **NOISE)
    x, y, a, s = _inputs(9)
    for _ in range(2):
        tr.train_d(x, y, a)
        tr.train_g(x, y, a, s)
    path = Saver().save(sess, str(tmp_path / 'ckpt'))
    saved = np.load(path)
    assert [int(v) % 2 ** 64 for v in saved['state:d/inst_noise/state']] == [SEED, 4] and saved['state:d/inst_noise/updates'].tolist() == [2]
    assert sorted(k for k in saved.files if 'inst_noise' in k) == ['state:d/inst_noise/state', 'state:d/inst_noise/updates']

    def two_iterations():
        rec = []
        for _ in range(2):
            tr.train_d(x, y, a)
            rec.append(tr.d_noise_last())
            tr.train_g(x, y, a, s)
            rec.append(tr.d_noise_last())
        return rec, {n: sess.get_value(v) for n, v in g.variables.items()}
    rec_a, w_a = two_iterations()
    Saver().restore(sess, path)
    assert tr.d_noise_state() == (SEED, 4, 2)
    rec_b, w_b = two_iterations()
    assert rec_a == rec_b and [r['key'][1] for r in rec_a] == [4, 5, 6, 7]
    assert [np.float32(r['sigma']) for r in rec_a] == [R.sigma(k, *SCHED) for k in (2, 3, 3, 4)]
    for n in w_a:
        assert torch.equal(w_a[n], w_b[n]), n
    sess.close()


@pytest.mark.parametrize('transform', [True, False], ids=['dna', 'plain'])
def test_d_noise_0_is_bit_identical_to_a_trainer_without_the_arguments(transform):
    x, y, a, s = _inputs(11)
    got = []
    for kw in ({}, dict(d_noise=0.0, d_noise_final=0.7, d_noise_decay_steps=9, d_noise_offset=2, d_noise_seed=5, d_stats=False)):
        sess, tr, g = _trainer(transform, _params(transform), **kw)
        tr.train_d(x, y, a)
        frames = tr.train_g(x, y, a, s)
        got.append((frames, {n: sess.get_value(v) for n, v in g.variables.items()}, [type(o).__name__ for o in g.ops]))
        sess.close()
    assert got[0][2] == got[1][2]
    assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32))
    for n in got[0][1]:
        assert torch.equal(got[0][1][n], got[1][1][n]), n


def test_a_bf16_d_step_reads_the_noisy_bf16_input():
    sess, tr, g = _trainer(True, dtype='bf16', **NOISE)
    x, y, a, s = _inputs(8)
    noisy_t = tr.d_noisy['both']
    assert noisy_t.dtype == torch.bfloat16
    res = sess.run([tr.d_opt_op, tr.d_loss, noisy_t, noisy_t.op.inputs[0], tr.clip_d], tr._feed(x, y, a))
    last = tr.d_noise_last()
    assert last['key'] == (SEED, 0) and np.float32(last['sigma']) == R.sigma(0, *SCHED)
    _check_d_input(res[2], res[3], last, R.SLOT['both'], torch.bfloat16, 'bf16 D(both) input')
    assert np.isfinite(res[1][0])
    frames = tr.train_g(x, y, a, s)
    assert np.isfinite(frames).all() and all(bool(torch.isfinite(sess.get_value(v)).all()) for v in g.variables.values())
    sess.close()


@pytest.mark.parametrize('transform', ['cdna', True], ids=['cdna', 'dna'])
def test_the_other_training_options_take_it(transform):
    """The weight average, the SSIM term, both clip norms, a learning-rate schedule and the generator's noise input beside the
    instance noise: two replayed iterations, everything finite, key and schedule where they belong."""
    sess, tr, g = _trainer(transform, ema_decay=0.99, ssim_weight=10.0, g_clip_norm=5.0, d_clip_norm=5.0, lr_schedule='cosine', lr_decay_steps=10,
                           noise_dim=4, d_stats=True, **NOISE)
    x, y, a, s = _inputs(15)
    for i in range(3):
        tr.train_d(x, y, a)
        frames = tr.train_g(x, y, a, s)
        assert tr.d_noise_state() == (SEED, 2 * i + 2, i + 1) and np.float32(tr.d_noise_last()['sigma']) == R.sigma(i + 1, *SCHED)
    summ = tr.train_d(x, y, a, summarize=True)
    assert np.isfinite(frames).all() and np.isfinite(list(summ.values())).all() and summ['d_noise_sigma'] == float(R.sigma(3, *SCHED))
    assert all(bool(torch.isfinite(sess.get_value(v)).all()) for v in g.variables.values())
    assert tr.noise_state()[1] == 7 and tr.ema_updates() == 3 and tr.grad_norm_stats('d')['norm'] > 0
    sess.close()


@pytest.mark.parametrize('batched', [True, False], ids=['batched', 'two_instances'])
def test_d_stats_summaries_match_numpy_on_the_fetched_logits(batched):
    sess, tr, g = _trainer(True, _params(True), batched_d=batched, d_stats=True, d_noise=0.25)
    x, y, a, s = _inputs(13)
    for _ in range(2):
        summ = tr.train_d(x, y, a, summarize=True)
        fake = (tr.d_out_both.buf[:B] if batched else tr.d_out_gen.buf).detach().double().cpu().numpy().reshape(-1)
        real = tr.d_out_real.buf.detach().double().cpu().numpy().reshape(-1)
        want = R.logit_stats(fake, real)
        print('d_stats %s vs numpy %s' % ({k: summ[k] for k in summ if k.startswith('d_')}, want))
        assert fake.size == real.size == B * 4
        for k, name in enumerate(('d_fake_logit', 'd_real_logit')):
            assert abs(summ[name] - want[k]) <= 1e-6 * abs(want[k]), (name, summ[name], want[k])
        assert summ['d_fake_acc'] == float(np.float32(want[2])) and summ['d_real_acc'] == float(np.float32(want[3]))
        assert summ['d_noise_sigma'] == tr.d_noise_last()['sigma'] == 0.25
    assert np.isfinite(list(summ.values())).all()
    sess.close()


def test_cli_logs_sigma_and_the_statistics(tmp_path):
    out2 = tmp_path / 'run'
    T.main(['synthetic', str(out2), '--adv', 'True', '--dna', '--d_noise', '0.5', '--d_noise_final', '0.125', '--d_noise_decay_iters', '2',
            '--d_noise_seed', '5', '--log_d_stats', '--batch_size', '4', '--seq_len', '4', '--pretrain_iter', '0', '--train_iter', '2'])
    rec = [json.loads(line) for line in open(out2 / 'logs' / 'train.jsonl')]
    assert len(rec) == 1 and rec[0]['d_noise_sigma'] == 0.5
    assert all(np.isfinite(rec[0][k]) for k in ('d_fake_logit', 'd_real_logit')) and all(0.0 <= rec[0][k] <= 1.0 for k in ('d_fake_acc', 'd_real_acc'))
    saved = np.load(str(out2 / 'models' / 'model0.npz'))
    assert int(saved['state:d/inst_noise/state'][0]) == 5 and int(saved['state:d/inst_noise/state'][1]) == 2 and saved['state:d/inst_noise/updates'].tolist() == [1]
    plain = tmp_path / 'plain'
    T.main(['synthetic', str(plain), '--adv', 'True', '--dna', '--batch_size', '4', '--seq_len', '4', '--pretrain_iter', '0', '--train_iter', '1'])
    rec = [json.loads(line) for line in open(plain / 'logs' / 'train.jsonl')]
    assert rec and not any(k.startswith('d_noise') or k in ('d_fake_logit', 'd_real_logit', 'd_fake_acc', 'd_real_acc') for k in rec[0])
    assert not any('inst_noise' in k for k in np.load(str(plain / 'models' / 'model0.npz')).files)
