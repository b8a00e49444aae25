"""GPU: differentiable augmentation of the discriminator's inputs (include/acgan_rollout.h: acg_d_augment_draw / _fwd / _bwd;
ops.DAugmentDrawOp / DAugmentOp / DAugmentBwdOp; Trainer d_augment).  The kernels against the float64 restatement of
tests/d_augment_ref.py with guard bands around every buffer, and a Trainer with augmentation against the fp64 oracle whose
discriminator judges the same transformed pairs.

Tolerances.  The draw, the pad channels, the counters and everything that is compared between two launches are compared
bitwise.  The forward map is four terms of at most three float32 factors each, of magnitude at most 3 max|x|, with three
additions of partial sums of at most 5.5 max|x|: at most 52 roundings' worth, so |delta| <= 64 * 2^-24 * max(1, max|x|); the
adjoint holds the same bound with max|dout|, and 1e-4 normwise, the project's bar for backward kernels.  The Trainer steps hold
1e-3 against the oracle, the project's step bar."""
import ctypes
import json

import numpy as np
import pytest
import torch

import d_augment_ref as R
import d_noise_ref as DN
import train_cases as TC
from action_conditioned_gans_amd import _lib
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import ops as O
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T
from action_conditioned_gans_amd.saver import Saver
from oracle import models as OM

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GUARD = 64                           # float32 elements on either side of every buffer (256 bytes: the payload stays aligned)
SENTINEL = -7.25


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _i64(v):
    return v - 2 ** 64 if v >= 2 ** 63 else v


class Band:
    """A device buffer of n float32 between two guard bands; ``shift`` elements move the payload off its 16-byte alignment; the
    payload starts as ``values`` or as NaN."""

    def __init__(self, n, shift=0, values=None):
        self.full = torch.full((GUARD + shift + n + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.lo, self.hi = GUARD + shift, GUARD + shift + n
        self.t = self.full[self.lo:self.hi]
        self.t.fill_(float('nan'))
        if values is not None:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(values), dtype=torch.float32).reshape(-1))

    def get(self):
        """The payload on the host; asserts the guards are untouched."""
        torch.cuda.synchronize()
        host = self.full.cpu().numpy()
        assert (host[:self.lo] == SENTINEL).all() and (host[self.hi:] == SENTINEL).all(), 'written outside the buffer'
        return host[self.lo:self.hi].copy()


def _launch(mode, x, params, shape, shift=0):
    """One acg_d_augment_fwd / _bwd on guarded buffers -> the output [rows, h, w, pitch]; the workspace is followed by a guard."""
    lib = _lib.get()
    rows, h, w, pitch, frames, cf = shape
    n = rows * h * w * pitch
    src, dst, par = Band(n, shift, x), Band(n, shift), Band(rows * 8, 0, params)
    nbytes = lib.d_augment_workspace_bytes(rows, h, w, frames, cf)
    assert nbytes > 0 and nbytes % 8 == 0
    ws = Band(nbytes // 4)
    fn = lib.d_augment_fwd if mode == 'fwd' else lib.d_augment_bwd
    fn(_p(src.t), _p(par.t), _p(dst.t), rows, h, w, pitch, frames, cf, _p(ws.t), nbytes, _stream())
    out = dst.get().reshape(rows, h, w, pitch)
    ws.get()
    assert np.array_equal(src.get().view(np.uint32), np.asarray(x, np.float32).reshape(-1).view(np.uint32))
    assert np.array_equal(par.get().view(np.uint32), np.asarray(params, np.float32).reshape(-1).view(np.uint32))
    return out


def _param_rows(h, w):
    """The explicit rows of the issue and a drawn row for each of the eight policies, float64 [18, 8]."""
    m = max(h, w)
    rows = [R.IDENTITY,
            (0.5, 0.0, 0.5, 0, 0, 0, 0, 0), (-0.5, 2.0, 1.5, 0, 0, 0, 0, 0),              # the extreme colour factors
            (0.25, 1.5, 0.75, h, 0, 0, 0, 0), (0.25, 1.5, 0.75, -h, 0, 0, 0, 0), (0.25, 1.5, 0.75, 0, w, 0, 0, 0),   # a shift of exactly +-H, W
            (0.25, 1.5, 0.75, 0, 0, 0, 0, m),                                                # a cut covering the image
            (0.25, 1.5, 0.75, 0, 0, h, w, 3), (0.25, 1.5, 0.75, 0, 0, -5, -5, 5),        # cuts wholly outside
            (0.25, 1.5, 0.75, 1 if h > 1 else 0, 0, -1, 1, 3)]                              # a negative cy0
    rows += [tuple(R.draw(11 + policy, policy, 3, 1, h, w, policy)[0]) for policy in range(8)]
    return np.array(rows, np.float64)


def _check(mode, got, x, params, shape):
    rows, h, w, pitch, frames, cf = shape
    nv = frames * cf
    ref = (R.apply if mode == 'fwd' else R.adjoint)(x[..., :nv].astype(np.float64), params, frames, cf).numpy()
    scale = max(1.0, float(np.abs(x[..., :nv]).max()))
    err = float(np.abs(got[..., :nv].astype(np.float64) - ref).max())
    print('%s %s: max err %.3e (bar %.3e), max|ref| %.3g' % (mode, shape, err, 64 * 2.0 ** -24 * scale, np.abs(ref).max()))
    assert err <= 64 * 2.0 ** -24 * scale
    if mode == 'fwd':
        assert np.array_equal(got[..., nv:].view(np.uint32), x[..., nv:].view(np.uint32))      # pad channels: the input's bits
    else:
        assert not got[..., nv:].view(np.uint32).any()                                         # +0
        assert np.linalg.norm(got[..., :nv].astype(np.float64) - ref) <= 1e-4 * np.linalg.norm(ref)


# (rows, h, w, pitch, frames, cf), the smallest at which each path can go wrong
SHAPES = [(1, 1, 1, 1, 1, 1), (2, 5, 7, 8, 2, 3), (3, 16, 16, 8, 2, 3), (2, 64, 64, 8, 2, 3), (1, 128, 128, 8, 2, 3), (2, 9, 6, 4, 1, 3), (2, 8, 8, 4, 1, 4),
          (1024, 2, 2, 8, 2, 3)]


@pytest.mark.parametrize('shape,scale', [(s, 1.0) for s in SHAPES] + [((3, 16, 16, 8, 2, 3), 1e3)], ids=str)
def test_forward_and_adjoint_against_float64(shape, scale):
    rows, h, w, pitch, frames, cf = shape
    nv = frames * cf
    rng = np.random.default_rng(rows + 10 * h + pitch)
    table = _param_rows(h, w)
    x = (rng.uniform(-1, 1, (rows, h, w, pitch)) * scale).astype(np.float32)
    x[..., nv:] = (rng.standard_normal((rows, h, w, pitch - nv)) * 1e6).astype(np.float32)        # pad: anything
    for k in range(-(-len(table) // rows)):
        params = table[(k * rows + np.arange(rows)) % len(table)]
        for mode in ('fwd', 'bwd'):
            got = _launch(mode, x, params, shape)
            _check(mode, got, x, params, shape)
            if k == 0:
                again = _launch(mode, x, params, shape)
                assert np.array_equal(got.view(np.uint32), again.view(np.uint32))                 # two launches: the same bits
                off = _launch(mode, x, params, shape, shift=1)
                assert np.array_equal(got.view(np.uint32), off.view(np.uint32))                   # a base 4 bytes off: the same bits


def test_the_identity_returns_the_frame_bit_for_bit():
    """What the header says: 1 * X + 0 - the valid channels of a finite frame bit for bit, except that -0.0 becomes +0.0."""
    shape = (2, 9, 6, 8, 2, 3)
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, shape[:3] + (8,)).astype(np.float32)
    x[0, 0, 0, :3] = (1e-40, -1e-40, 3e38)
    params = np.array([R.IDENTITY] * 2)
    got = _launch('fwd', x, params, shape)
    assert np.array_equal(got.view(np.uint32), x.view(np.uint32))
    x[1, 2, 3, 1] = -0.0
    got = _launch('fwd', x, params, shape)
    assert got[1, 2, 3, 1] == 0.0 and not np.signbit(got[1, 2, 3, 1])
    x[1, 2, 3, 1] = 0.0
    assert np.array_equal(got.view(np.uint32), x.view(np.uint32))
    dout = rng.standard_normal(shape[:3] + (8,)).astype(np.float32)
    din = _launch('bwd', dout, params, shape)
    assert np.array_equal(din[..., :6].view(np.uint32), dout[..., :6].view(np.uint32)) and not din[..., 6:].view(np.uint32).any()


@pytest.mark.parametrize('seed,counter,sid,rows,h,w', [(1, 0, 0, 64, 64, 64), (2 ** 64 - 2, 2 ** 32 + 7, 130, 1024, 5, 7), (77, 2 ** 64 - 1, 2, 3, 128, 96)])
def test_the_draw_bit_for_bit_and_its_counter(seed, counter, sid, rows, h, w):
    lib = _lib.get()
    state = torch.full((2 + 2 * 8,), -0x0123456789abcdef, dtype=torch.int64, device=DEV)
    state[8:10] = torch.tensor([_i64(seed), _i64(counter)], dtype=torch.int64)
    par = Band(rows * 8)
    for step, policy in enumerate((7, 5)):
        lib.d_augment_draw(_p(state[8:10]), _p(par.t), rows, h, w, policy, sid, _stream())
        got = par.get().reshape(rows, 8)
        want = R.draw(seed, counter + step, sid, rows, h, w, policy).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (step, got[:2], want[:2])
        host = [int(v) % 2 ** 64 for v in state.cpu().numpy()]
        assert host[8:10] == [seed, (counter + step + 1) % 2 ** 64]                               # advanced by exactly one
        assert all(v == (-0x0123456789abcdef) % 2 ** 64 for v in host[:8] + host[10:])


# ---- Trainer ------------------------------------------------------------------------------------------------------------------
B, S, K, SEED = 2, 64, 5, 0xfeedface12345678
AUG = dict(d_augment='color,translation,cutout', d_augment_seed=SEED)


def _inputs(seed=21):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (B, S, S, 3)).astype(np.float32)
    y = np.clip(np.roll(x, 2, axis=2) + 0.05 * rng.standard_normal(x.shape).astype(np.float32), -1, 1)
    return x, y, rng.standard_normal((B, 10)).astype(np.float32), rng.standard_normal((B, 5)).astype(np.float32)


_PARAMS = {}


def _params():
    """Computed once and shared; never modified (the sessions copy them)."""
    if not _PARAMS:
        _PARAMS[True] = OM.init_params(True, batch=B, img=S, ksize=K, seed=3, dtype=torch.float32)
    return _PARAMS[True]


def _trainer(params=None, loss='bce', opt='adam', sess_kw=None, **kw):
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device=DEV, **(sess_kw or {}))
    tr = T.Trainer(sess, True, loss, opt, True, batch_size=B, img_size=S, ksize=K, **kw)
    sess.run(G.global_variables_initializer())
    g = G.get_default_graph()
    if params is not None:
        assert set(params) == set(g.variables)
        for n, v in g.variables.items():
            sess.set_value(v, params[n])
    return sess, tr, g


def _noise_add(tr, slot, rows):
    last = tr.d_noise_last()
    return (np.float64(np.float32(last['sigma'])) * DN.z(last['key'], DN.SLOT[slot], rows * S * S, 3)).reshape(rows, S, S, 3)


@pytest.mark.parametrize('loss,opt,batched,noise', [('bce', 'adam', True, False), ('bce', 'adam', False, False), ('wass', 'rmsprop', True, False),
                                                    ('bce', 'adam', True, True)], ids=str)
def test_d_and_g_step_match_the_oracle_on_the_same_augmented_pairs(loss, opt, batched, noise):
    """One D step and one G step: loss, frame and every variable's gradient norm within 1e-3 of the fp64 oracle whose discriminator
    judges the pairs transformed under the parameters the programs drew (d_augment_last, in call order); with d_noise the oracle
    adds the same noise behind the augmentation."""
    params = _params()
    kw = dict(AUG, batched_d=batched, **(dict(d_noise=0.5, d_noise_seed=9) if noise else {}))
    sess, tr, g = _trainer(params, loss, opt, **kw)
    ot = R.DAugOracleTrainer({k: v.double() for k, v in params.items()}, True, loss, opt, True, K)
    x, y, a, s = _inputs()
    td = lambda t: torch.from_numpy(t).double()     # noqa: E731
    norms = lambda: {'n/' + k: v.norm() for k, v in ot.last_grads.items()}     # noqa: E731
    assert tr.d_augment_state() == (SEED, 0)

    res = sess.run([tr.d_opt_op, tr.d_loss, tr.g_next_frame, tr.clip_d], tr._feed(x, y, a))
    last = tr.d_augment_last()
    draws = 1 if batched else 2
    assert tr.d_augment_state() == (SEED, draws)
    if batched:
        want = R.draw(SEED, 0, R.SLOT['both'], 2 * B, S, S, 7)
        assert np.array_equal(last['both'].astype(np.float64), want) and not last['gen'].any()
        ot.d_params = [last['both'][:B], last['both'][B:]]
        if noise:
            add = _noise_add(tr, 'both', 2 * B)
            ot.d_add = [add[:B], add[B:]]
    else:
        # two draws in one program, stream-ordered in the program's order: each took the counter it found
        assert np.array_equal(last['gen'].astype(np.float64), R.draw(SEED, 0, R.SLOT['gen'], B, S, S, 7))
        assert np.array_equal(last['real'].astype(np.float64), R.draw(SEED, 1, R.SLOT['real'], B, S, S, 7))
        ot.d_params = [last['gen'], last['real']]
    od = ot.train_d(td(x), td(y), td(a), return_all=True)
    print('train_d frame rel %.3e, d_loss %.6g vs %.6g' % (TC.rel(res[2], od['frame'].numpy()), res[1][0], float(od['d_loss'])))
    assert TC.rel(res[2], od['frame'].numpy()) <= 1e-3
    assert abs(res[1][0] - float(od['d_loss'])) <= 1e-3 * max(abs(float(od['d_loss'])), 1.0)
    TC.check_norms(TC.flat_grad_norms(sess, tr.d_opt_op), norms(), 'n/', 1e-3, 'D grad')
    for n, v in g.variables.items():                 # every step is compared from one starting point
        ot.p[n] = sess.get_value(v).double()

    res = sess.run([tr.g_opt_op, tr.g_loss, tr.g_next_frame, tr.g_state_out], tr._feed(x, y, a, s))
    last = tr.d_augment_last()
    assert tr.d_augment_state() == (SEED, draws + 1)
    assert np.array_equal(last['gen'].astype(np.float64), R.draw(SEED, draws, R.SLOT['gen'], B, S, S, 7))
    ot.d_params = [last['gen']]
    if noise:
        ot.d_add = [_noise_add(tr, 'gen', B)]
    og = ot.train_g(td(x), td(y), td(a), td(s), return_all=True)
    print('train_g frame rel %.3e, g_loss %.6g vs %.6g' % (TC.rel(res[2], og['frame'].numpy()), res[1][0], float(og['g_loss'])))
    assert TC.rel(res[2], og['frame'].numpy()) <= 1e-3 and TC.rel(res[3], og['state'].numpy()) <= 1e-3
    assert abs(res[1][0] - float(og['g_loss'])) <= 1e-3 * abs(float(og['g_loss']))
    TC.check_norms(TC.flat_grad_norms(sess, tr.g_opt_op), norms(), 'n/', 1e-3, 'G grad')
    sess.close()


def test_the_g_step_launches_no_slice_or_add_the_parent_lacks():
    x, y, a, s = _inputs()
    kinds = []
    for kw in (dict(lookahead=False), AUG):
        sess, tr, g = _trainer(**kw)
        names = TC.program_op_names(sess, [tr.g_opt_op], tr._feed(x, y, a, s))
        kinds.append(sorted(k for _, k, _ in names if k in ('SliceOp', 'AddOp')))
        assert any(k == 'DAugmentBwdOp' for _, k, _ in names) == ('d_augment' in kw)
        sess.close()
    assert kinds[0] == kinds[1]


def test_without_the_arguments_the_steps_are_bit_identical_to_the_parent():
    x, y, a, s = _inputs(11)
    got = []
    for kw in ({}, dict(d_augment=None, d_augment_seed=5), dict(d_augment='', d_augment_seed=0)):
        sess, tr, g = _trainer(_params(), **kw)
        tr.train_d(x, y, a)
        frames = tr.train_g(x, y, a, s)
        got.append((frames, {n: sess.get_value(v) for n, v in g.variables.items()}, [type(o).__name__ for o in g.ops]))
        sess.close()
    for other in got[1:]:
        assert got[0][2] == other[2]
        assert np.array_equal(got[0][0].view(np.uint32), other[0].view(np.uint32))
        for n in got[0][1]:
            assert torch.equal(got[0][1][n], other[1][n]), n


def test_replay_equals_eager_and_every_program_draws_afresh():
    """Run 1 of a program is eager, run 2 captures, runs 3+ replay; against a session that never captures, from the same state and
    weights: the parameters of every program, the frames and the final weights bit for bit; the counter counts the draws."""
    params = _params()
    x, y, a, s = _inputs(7)
    finals = []
    for use_graphs in (False, True):
        sess, tr, g = _trainer(params, sess_kw=dict(use_hip_graphs=use_graphs), **AUG)
        rec = []
        for i in range(4):
            tr.train_d(x, y, a)
            assert tr.d_augment_state() == (SEED, 2 * i + 1)
            both = tr.d_augment_last()['both']
            assert np.array_equal(both.astype(np.float64), R.draw(SEED, 2 * i, R.SLOT['both'], 2 * B, S, S, 7)), i
            frames = tr.train_g(x, y, a, s)
            assert tr.d_augment_state() == (SEED, 2 * i + 2)
            gen = tr.d_augment_last()['gen']
            assert np.array_equal(gen.astype(np.float64), R.draw(SEED, 2 * i + 1, R.SLOT['gen'], B, S, S, 7)), i
            rec.append(np.concatenate([both.reshape(-1), gen.reshape(-1)]))
        torch.cuda.synchronize()
        finals.append(({n: sess.get_value(v) for n, v in g.variables.items()}, frames, np.stack(rec)))
        if use_graphs:
            assert all(p.graphs is not None for p in sess._programs.values() if p.runs >= 2)
        sess.close()
    (pe, fe, re_), (pg, fg, rg) = finals
    assert np.array_equal(re_.view(np.uint32), rg.view(np.uint32)) and len({r.tobytes() for r in rg}) == 4
    assert np.array_equal(fe.view(np.uint32), fg.view(np.uint32))
    for n in pe:
        assert torch.equal(pe[n], pg[n]), n


def test_a_checkpoint_round_trip_continues_the_draws_and_an_old_one_restores(tmp_path):
    sess0, tr0, g0 = _trainer(_params())
    old = Saver().save(sess0, str(tmp_path / 'old'))                           # a checkpoint of a run without the arguments
    assert 'state:d/augment/state' not in np.load(old).files
    sess0.close()
    sess, tr, g = _trainer(_params(), **AUG)
    x, y, a, s = _inputs(9)
    tr.train_d(x, y, a)
    tr.train_g(x, y, a, s)
    path = Saver().save(sess, str(tmp_path / 'ckpt'))
    saved = np.load(path)
    assert [int(v) % 2 ** 64 for v in saved['state:d/augment/state']] == [SEED, 2]
    assert sorted(k for k in saved.files if 'augment' in k) == ['state:d/augment/state']

    def one_iteration():
        tr.train_d(x, y, a)
        both = tr.d_augment_last()['both']
        tr.train_g(x, y, a, s)
        return both, tr.d_augment_last()['gen'], {n: sess.get_value(v) for n, v in g.variables.items()}
    b_a, g_a, w_a = one_iteration()
    assert tr.d_augment_state() == (SEED, 4)
    Saver().restore(sess, path)
    assert tr.d_augment_state() == (SEED, 2)
    b_b, g_b, w_b = one_iteration()
    assert np.array_equal(b_a.view(np.uint32), b_b.view(np.uint32)) and np.array_equal(g_a.view(np.uint32), g_b.view(np.uint32))
    for n in w_a:
        assert torch.equal(w_a[n], w_b[n]), n
    Saver().restore(sess, old)                       # the key is missing: the state stays, the variables are the old run's
    assert tr.d_augment_state() == (SEED, 4)
    for n, v in g.variables.items():
        assert torch.equal(sess.get_value(v).cpu(), _params()[n].cpu()), n
    sess.close()


def test_cli_trains_and_records_the_policy(tmp_path):
    out = tmp_path / 'run'
    T.main(['synthetic', str(out), '--adv', 'True', '--dna', '--d_augment', 'cutout,color', '--d_augment_seed', '5', '--batch_size', '4',
            '--seq_len', '4', '--pretrain_iter', '0', '--train_iter', '3'])
    rec = [json.loads(line) for line in open(out / 'logs' / 'train.jsonl')]
    assert len(rec) == 1 and rec[0]['d_augment'] == 'color,cutout' and np.isfinite(rec[0]['g_loss'])
    saved = np.load(str(out / 'models' / 'model0.npz'))
    assert int(saved['state:d/augment/state'][0]) == 5 and int(saved['state:d/augment/state'][1]) >= 2
    plain = tmp_path / 'plain'
    T.main(['synthetic', str(plain), '--adv', 'True', '--dna', '--batch_size', '4', '--seq_len', '4', '--pretrain_iter', '0', '--train_iter', '1'])
    rec = [json.loads(line) for line in open(plain / 'logs' / 'train.jsonl')]
    assert rec and 'd_augment' not in rec[0] and 'state:d/augment/state' not in np.load(str(plain / 'models' / 'model0.npz')).files
