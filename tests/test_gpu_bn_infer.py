"""GPU: BatchNorm with stored statistics (include/acgan_bn_infer.h) - the two kernels against float64, the calibrated generators
against the float64 restatement (tests/bn_infer_ref.py), the property the feature exists for (a row's prediction does not depend
on its batch), and the consistency of the stored-statistics programs with the batch-statistics ones.

Bars.  Kernels: the per-op bars of this suite - op_cases.close at 2e-5 for float32 results, one bf16 rounding (4e-3 on the scale
of test_bn_bf16's 4e-3 to 6e-3) for bf16 results; pooled moments of an input with mean / std ~ 1e3 at the bars of
test_conv_bn_stats_large_mean (mean 1e-6, rstd 2e-3).  Models: the north_star 1e-3 (max abs error over the reference's scale);
bf16: BF16_TOL's frame and state bars."""
import ctypes
import json

import numpy as np
import pytest
import torch

import bn_infer_ref as R
import cdna_ref
import op_cases as C
import train_cases as TC
from action_conditioned_gans_amd import _lib
from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T
from action_conditioned_gans_amd.saver import Saver
from oracle import models as OM
from oracle import tf_ops as OT
from test_gpu_train import BF16_TOL

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
EPS = 1e-3
ACTS = {'none': _lib.ACT_NONE, 'relu': _lib.ACT_RELU, 'lrelu': _lib.ACT_LRELU}
TDT = {'f32': torch.float32, 'bf16': torch.bfloat16}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pitched(rows, c, pitch, dtype, seed, scale=1.0, shift=0.0):
    """[rows, pitch] with random channels [0, c) and a sentinel in the pad channels; -> (device tensor, float64 [rows, c] as stored)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((rows, pitch), 7.0)
    x[:, :c] = torch.randn(rows, c, generator=g) * scale + shift
    x = x.to(dtype)
    return x.to(DEV), x[:, :c].double()


def _act64(u, act, leak=0.2):
    if act == 'relu':
        return torch.relu(u)
    if act == 'lrelu':
        return 0.5 * (1 + leak) * u + 0.5 * (1 - leak) * u.abs()
    return u


# (rows, channels, x pitch, y pitch, x type, y type, activation)
def _round(c, u):
    return -(-c // u) * u


INFER_CASES = []
for b in (1, 2, 32):        # the BatchNorm layers of the generators at 64 x 64 (DNA / CDNA widths, then the plain generator's)
    for hw, c in ((32, 32), (16, 64), (8, 128), (4, 256), (16, 128), (8, 32), (4, 16), (32, 128), (32, 64), (4, 512), (8, 256)):
        INFER_CASES.append((b * hw * hw, c, c, c, 'f32', 'f32', 'relu'))
        if c % 8 == 0 and b != 2:
            INFER_CASES.append((b * hw * hw, c, c, c, 'bf16', 'bf16', 'relu'))
INFER_CASES += [(32 * 16, 256, 256, 268, 'f32', 'f32', 'relu'), (16, 256, 256, 268, 'f32', 'f32', 'relu'),      # conv4 inside its concatenation
                (32 * 16, 256, 256, 272, 'bf16', 'bf16', 'relu'), (2 * 16, 512, 512, 524, 'f32', 'f32', 'relu')]
for c in (3, 138, 266):     # ragged channel counts at their float32 (round4) and bf16 (round8) pitches
    for act in ('none', 'relu', 'lrelu'):
        INFER_CASES.append((50, c, _round(c, 4), _round(c, 4), 'f32', 'f32', act))
        INFER_CASES.append((50, c, _round(c, 8), _round(c, 8), 'bf16', 'bf16', act))
    INFER_CASES.append((1, c, _round(c, 4), _round(c, 4), 'f32', 'f32', 'relu'))
    INFER_CASES.append((1, c, _round(c, 8), _round(c, 8), 'bf16', 'bf16', 'lrelu'))
    INFER_CASES.append((33, c, _round(c, 8), c, 'bf16', 'f32', 'none'))          # a bf16 network's float32 dense head
INFER_CASES += [(1, 32, 32, 32, 'f32', 'f32', 'none'), (1, 256, 256, 256, 'bf16', 'bf16', 'relu'), (3, 64, 64, 64, 'f32', 'f32', 'lrelu'),
                (4099, 32, 32, 32, 'f32', 'f32', 'lrelu'), (70001, 64, 64, 64, 'bf16', 'bf16', 'none'), (640, 1, 1, 1, 'f32', 'f32', 'relu'),
                (40000, 256, 256, 256, 'f32', 'f32', 'relu'), (300000, 8, 8, 8, 'f32', 'f32', 'relu')]    # (40000 x 256: a block walks two batches)


def _infer(lib, x, beta, mean, var, rows, c, xp, yp, xt, yt, act, y=None):
    if y is None:
        y = torch.full((rows, yp), 7.0, dtype=TDT[yt], device=DEV)
    lib.bn_act_infer(_p(x), _p(beta), _p(mean), _p(var), _p(y), rows, c, xp, yp, EPS, ACTS[act], 0.2,
                     _lib.dtype2(_lib.code(TDT[xt]), _lib.code(TDT[yt])), _stream())
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize('case', INFER_CASES, ids=str)
def test_bn_act_infer_matches_float64(hip_abi, case):
    rows, c, xp, yp, xt, yt, act = case
    lib = hip_abi.lib
    x, x64 = _pitched(rows, c, xp, TDT[xt], seed=rows + c, scale=1.5, shift=0.3)
    g = torch.Generator().manual_seed(c)
    beta, mean = torch.randn(c, generator=g) * 0.5, torch.randn(c, generator=g)
    var = torch.rand(c, generator=g) * 2 + 0.05
    var[0] = 0.0                                   # a dead channel: eps alone under the root
    want = _act64((x64 - mean.double()) * torch.rsqrt(var.double() + EPS) + beta.double(), act)
    y = _infer(lib, x, beta.to(DEV), mean.to(DEV), var.to(DEV), rows, c, xp, yp, xt, yt, act)
    C.close(y[:, :c], want, 2e-5 if yt == 'f32' else 4e-3, 'bn_act_infer %s' % (case,))
    assert bool((y[:, c:] == 7.0).all()), 'channels at or beyond `channels` were written'
    y2 = _infer(lib, x, beta.to(DEV), mean.to(DEV), var.to(DEV), rows, c, xp, yp, xt, yt, act)
    assert torch.equal(y2, y), 'a second launch gives other bits'


def test_bn_act_infer_rows_are_independent_and_arguments_are_checked(hip_abi):
    lib = hip_abi.lib
    rows, c = 96, 64
    x, _ = _pitched(rows, c, c, torch.float32, seed=1)
    g = torch.Generator().manual_seed(2)
    beta, mean, var = (t.to(DEV) for t in (torch.randn(c, generator=g), torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.1))
    y = _infer(lib, x, beta, mean, var, rows, c, c, c, 'f32', 'f32', 'relu')
    y1 = _infer(lib, x[5:6].contiguous(), beta, mean, var, 1, c, c, c, 'f32', 'f32', 'relu')
    assert torch.equal(y1[0], y[5])
    for bad in (dict(rows=0), dict(c=0), dict(xp=c - 1), dict(act=_lib.ACT_TANH)):
        a = dict(rows=rows, c=c, xp=c, act=_lib.ACT_RELU)
        a.update(bad)
        with pytest.raises(_lib.AcgError):
            lib.bn_act_infer(_p(x), _p(beta), _p(mean), _p(var), _p(y), a['rows'], a['c'], a['xp'], c, EPS, a['act'], 0.2, _lib.ACG_F32, _stream())
    with pytest.raises(_lib.AcgError):
        lib.bn_act_infer(_p(x), _p(beta), None, _p(var), _p(y), rows, c, c, c, EPS, _lib.ACT_RELU, 0.2, _lib.ACG_F32, _stream())
    ws = torch.zeros(16, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(_lib.AcgError):          # workspace too small
        lib.bn_collect(_p(x), _p(cnt), _p(mean), _p(var), rows, c, c, _lib.ACG_F32, _p(ws), 16, _stream())


# (row counts of the three calls, channels, pitch, type, scale, shift)
COLLECT_CASES = [((2048, 32, 8192), 32, 32, 'f32', 1.0, 0.2), ((2048, 32, 8192), 32, 32, 'bf16', 1.0, 0.2),
                 ((32768, 32768, 2048), 128, 128, 'f32', 2.0, -0.5), ((32768, 4096, 32768), 128, 128, 'bf16', 2.0, -0.5),
                 ((16, 16, 512), 256, 256, 'f32', 1.0, 0.0), ((16, 32, 16), 512, 512, 'bf16', 1.0, 0.0),
                 ((1, 1, 1), 16, 16, 'f32', 1.0, 0.0), ((1, 7, 300001), 8, 8, 'f32', 1.0, 1.0),
                 ((50, 3, 999), 3, 4, 'f32', 1.0, 0.1), ((50, 3, 999), 3, 8, 'bf16', 1.0, 0.1),
                 ((64, 640, 65), 138, 140, 'f32', 1.0, 0.1), ((64, 640, 65), 138, 144, 'bf16', 1.0, 0.1),
                 ((64, 640, 65), 266, 268, 'f32', 1.0, 0.1), ((64, 640, 65), 266, 272, 'bf16', 1.0, 0.1),
                 ((8192, 4096, 1024), 64, 64, 'f32', 1.0, 1000.0), ((600, 9000, 20), 40, 40, 'f32', 0.5, -700.0),
                 ((8192, 4096, 1024), 64, 64, 'bf16', 8.0, 8000.0)]          # mean / std ~ 1e3 (bf16: in units of its spacing at 8000)


def _collect_run(lib, chunks, c, pitch):
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    mean = torch.full((c,), 5.0, device=DEV)            # whatever the state held is ignored by the first merge
    var = torch.full((c,), 9.0, device=DEV)
    seen = []
    for x in chunks:
        rows = x.shape[0]
        nb = lib.bn_collect_workspace_bytes(rows, c)
        ws = torch.zeros(nb + 512, dtype=torch.uint8, device=DEV)
        ws[nb:] = 0xA5
        lib.bn_collect(_p(x), _p(cnt), _p(mean), _p(var), rows, c, pitch, _lib.code(x.dtype), _p(ws), nb, _stream())
        torch.cuda.synchronize()
        assert bool((ws[nb:] == 0xA5).all()), 'bn_collect wrote past its workspace'
        seen.append(int(cnt.item()))
    return seen, mean.clone(), var.clone()


@pytest.mark.parametrize('case', COLLECT_CASES, ids=str)
def test_bn_collect_pools_the_moments_of_the_concatenation(hip_abi, case):
    row_counts, c, pitch, dt, scale, shift = case
    lib = hip_abi.lib
    chunks, rows64 = [], []
    for i, n in enumerate(row_counts):
        x, x64 = _pitched(n, c, pitch, TDT[dt], seed=31 * i + c + n % 97, scale=scale, shift=shift + 0.25 * i * scale)
        chunks.append(x)
        rows64.append(x64)
    seen, mean, var = _collect_run(lib, chunks, c, pitch)
    assert seen == list(np.cumsum(row_counts))
    allr = torch.cat(rows64)
    m, v = allr.mean(0), allr.var(0, unbiased=False)
    large = abs(shift) >= 100
    if large:
        ratio = (m.abs() / v.sqrt()).min().item()
        assert ratio > 100, 'test premise: mean / std = %.1f' % ratio
        C.close(mean, m, 1e-6, 'pooled mean %s' % (case,))
        C.close(1.0 / torch.sqrt(var.double().cpu() + EPS), 1.0 / torch.sqrt(v + EPS), 2e-3, 'pooled rstd %s' % (case,))
    else:
        # float32 sums of centred values: the per-op 2e-5, of the spread (and of the mean's own size)
        err = (mean.double().cpu() - m).abs()
        assert bool((err <= 2e-5 * (v.sqrt() + m.abs()) + 1e-30).all()), (case, float(err.max()))
        if sum(row_counts) > 3:
            C.close(var, v, 2e-5, 'pooled variance %s' % (case,))
        else:
            assert bool(((var.double().cpu() - v).abs() <= 2e-5 * v + 1e-12).all())
    # the first merge alone: the batch's own moments, whatever the state held
    seen1, mean1, var1 = _collect_run(lib, chunks[:1], c, pitch)
    m1, v1 = rows64[0].mean(0), rows64[0].var(0, unbiased=False)
    assert bool(((mean1.double().cpu() - m1).abs() <= (1e-6 if large else 2e-5) * (m1.abs() + v1.sqrt()) + 1e-30).all())
    assert bool(((var1.double().cpu() - v1).abs() <= 2e-3 * v1 + 1e-12).all())
    # the same calls, the same bits
    seen2, mean2, var2 = _collect_run(lib, chunks, c, pitch)
    assert seen2 == seen and torch.equal(mean2, mean) and torch.equal(var2, var)


# ---- models ----------------------------------------------------------------------------------------------------------------------
def _oracle_params(model, seed=5):
    p = cdna_ref.init_params_cdna(batch=2, seed=seed) if model == 'cdna' else OM.init_params(model == 'dna', batch=2, seed=seed, dtype=torch.float32)
    g = torch.Generator().manual_seed(seed + 100)
    return {k: (torch.randn(v.shape, generator=g) * 0.2 if k.endswith('/beta') else v) for k, v in p.items()}


def _trainer(model, B, dtype='f32', params=None, bn_inference=True, **sess_kw):
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device=DEV, dtype=dtype, **sess_kw)
    tr = T.Trainer(sess, False, 'bce', 'adam', {'plain': False, 'dna': True, 'cdna': 'cdna'}[model], batch_size=B, img_size=64, ksize=5,
                   lookahead=False, bn_inference=bn_inference)
    sess.run(G.global_variables_initializer())
    params = params if params is not None else _oracle_params(model)
    for n, v in G.get_default_graph().variables.items():
        sess.set_value(v, params[n])
    return sess, tr, params


def _pairs(B, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (B, 64, 64, 3)).astype(np.float32), rng.standard_normal((B, 10)).astype(np.float32)


def _td(x):
    return torch.from_numpy(np.asarray(x)).double()


def _p64(params):
    return {k: v.double() for k, v in params.items()}


def _calibrate_both(tr, params, model, B, n_batches=4, seed=40):
    """Calibrate the Trainer and the restatement on the same batches; -> pooled float64 moments."""
    record = {}
    tr.reset_bn_statistics()
    for i in range(n_batches):
        x, a = _pairs(B, seed + i)
        assert tr.calibrate_bn(x, a) == (i + 1) * B
        R.run_recording(model, _p64(params), _td(x), _td(a), record)
    return R.pooled_moments(record)


def _check_statistics(tr, want, tol):
    got = tr.bn_statistics()
    assert len(got) == 3 * len(want)
    worst = 0.0
    for scope, (mean, var, rows) in want.items():
        assert int(got[scope + '/calibration_rows'][0]) == rows, scope
        # on the scale of the layer's spread: a mean is an average of values of that size
        em = np.abs(got[scope + '/moving_mean'] - mean.numpy()).max() / max(float(var.sqrt().max()), float(mean.abs().max()))
        ev = TC.rel(got[scope + '/moving_variance'], var.numpy())
        worst = max(worst, em, ev)
        assert em <= tol and ev <= tol, (scope, em, ev)
    return worst


@pytest.mark.timeout(1200)
@pytest.mark.parametrize('model', ['plain', 'dna', 'cdna'])
@pytest.mark.parametrize('B', [2, 32])
def test_calibrated_generator_matches_the_restatement(model, B):
    torch.set_num_threads(16)
    sess, tr, params = _trainer(model, B)
    stats = _calibrate_both(tr, params, model, B)
    worst = _check_statistics(tr, stats, 1e-3)
    x, a = _pairs(B, 99)
    frame, state, summ = tr.test(x, x, a, bn='stored')
    wf, ws = R.run_stored(model, _p64(params), _td(x), _td(a), stats)
    ef = TC.rel(frame, wf.numpy())
    es = TC.rel(state, ws.numpy()) if ws is not None else 0.0
    print('stored %s B=%d: statistics %.2e frame %.2e state %.2e' % (model, B, worst, ef, es))
    assert ef <= 1e-3 and es <= 1e-3, (ef, es)
    assert (state is None) == (model == 'plain') and set(summ) == {'g_psnr'} and np.isfinite(summ['g_psnr'])
    sess.close()


@pytest.mark.timeout(1200)
@pytest.mark.parametrize('B', [2, 32])
def test_calibrated_dna_generator_in_bf16_matches_the_bf16_storage_oracle(B):
    torch.set_num_threads(16)
    sess, tr, params = _trainer('dna', B, dtype='bf16')
    assert G.get_default_graph().act_dtype == torch.bfloat16
    with OT.bf16_storage():
        stats = _calibrate_both(tr, params, 'dna', B)
        worst = _check_statistics(tr, stats, BF16_TOL['frame'])
        x, a = _pairs(B, 99)
        frame, state, _ = tr.test(x, x, a, bn='stored')
        wf, ws = R.run_stored('dna', _p64(params), _td(x), _td(a), stats)
    ef, es = TC.rel(frame, wf.numpy()), TC.rel(state, ws.numpy())
    print('stored dna bf16 B=%d: statistics %.2e frame %.2e state %.2e' % (B, worst, ef, es))
    assert ef <= BF16_TOL['frame'] and es <= BF16_TOL['state'], (ef, es)
    sess.close()


# ---- the property the feature exists for ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_a_row_does_not_depend_on_its_companions(dtype):
    """Row 0 of a batch, same B, same position, other sequences in rows 1..B-1: bitwise equal with stored statistics; with batch
    statistics the same comparison differs grossly (asserted: more than ten times the whole-model bar of 1e-3)."""
    B = 8
    sess, tr, _ = _trainer('dna', B, dtype=dtype)
    for i in range(4):
        tr.calibrate_bn(*_pairs(B, 60 + i))
    x1, a1 = _pairs(B, 70)
    x2, a2 = _pairs(B, 71)
    x2[1:] = 0.9 * np.sign(x2[1:])          # companions of another kind altogether: saturated frames, large actions
    a2[1:] *= 4.0
    x2[0], a2[0] = x1[0], a1[0]
    f1, s1, _ = tr.test(x1, x1, a1, bn='stored')
    f2, s2, _ = tr.test(x2, x2, a2, bn='stored')
    assert np.array_equal(f1[0], f2[0]) and np.array_equal(s1[0], s2[0]), 'stored statistics: row 0 depends on its companions'
    assert not np.array_equal(f1[1], f2[1])
    b1, t1, _ = tr.test(x1, x1, a1)
    b2, t2, _ = tr.test(x2, x2, a2, bn='batch')
    df = np.abs(b1[0] - b2[0]).max() / np.abs(b1[0]).max()
    ds = np.abs(t1[0] - t2[0]).max() / np.abs(t1[0]).max()
    print('batch statistics (%s): row 0 moves by %.3e (frame) / %.3e (state) with its companions' % (dtype, df, ds))
    assert max(df, ds) > 1e-2, (df, ds)
    sess.close()


@pytest.mark.timeout(1200)
def test_one_sequence_at_batch_1_2_and_32(tmp_path):
    """Calibrated at batch 32, saved, restored into graphs of batch 1, 2 and 32: the same sequence in row 0 meets the 1e-3 bar
    against the restatement (which is a function of the row alone) at every batch size."""
    torch.set_num_threads(16)
    sess, tr, params = _trainer('dna', 32)
    stats = _calibrate_both(tr, params, 'dna', 32)
    Saver().save(sess, str(tmp_path / 'cal'))
    sess.close()
    x, a = _pairs(32, 123)
    wf, ws = R.run_stored('dna', _p64(params), _td(x[:1]), _td(a[:1]), stats)
    out = {}
    for B in (1, 2, 32):
        sess, tr, _ = _trainer('dna', B, params=_oracle_params('dna', seed=77))          # other weights: the checkpoint brings its own
        Saver().restore(sess, str(tmp_path / 'cal'))
        assert tr.bn_calibration_rows() == 4 * 32
        frame, state, _ = tr.test(x[:B], x[:B], a[:B], bn='stored')
        assert frame.shape == (B, 64, 64, 3) and state.shape == (B, 5)
        ef, es = TC.rel(frame[0], wf[0].numpy()), TC.rel(state[0], ws[0].numpy())
        print('B=%d: frame %.2e state %.2e' % (B, ef, es))
        assert ef <= 1e-3 and es <= 1e-3, (B, ef, es)
        out[B] = (frame[0], state[0])
        if B == 1:          # the device loop and the metrics at a batch of one
            seq = np.stack([x[:1]] * 4, axis=1)
            acts = np.stack([a[:1]] * 4, axis=1)
            m = tr.rollout_metrics(seq, acts, bn='stored', return_frames=True)
            assert m['frames'].shape == (1, 3, 64, 64, 3) and np.isfinite(m['ssim']).all()
            assert np.array_equal(m['frames'][0, 0], frame[0])
        sess.close()
    assert TC.rel(out[1][0], out[32][0]) <= 2e-3 and TC.rel(out[2][0], out[32][0]) <= 2e-3


# ---- consistency between the two modes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', ['plain', 'dna', 'cdna'])
def test_stored_equals_batch_on_the_batch_it_was_calibrated_on(model):
    """Calibrated on exactly one batch, the stored statistics ARE that batch's: the two programs then differ by how the same
    moments were summed (one-pass kernels against the pooled Chan merge) - 2e-5 per BatchNorm layer, through a chain of up to eight
    of them; the whole-model 1e-3 is the ceiling asserted.  The measured value is printed; none is recorded here yet (this test
    had not run on a GPU when it was written)."""
    B = 32
    sess, tr, _ = _trainer(model, B)
    x, a = _pairs(B, 17)
    assert tr.calibrate_bn(x, a) == B
    fs, ss, _ = tr.test(x, x, a, bn='stored')
    fb, sb, _ = tr.test(x, x, a, bn='batch')
    ef = TC.rel(fs, fb)
    es = TC.rel(ss, sb) if ss is not None else 0.0
    print('stored vs batch on the calibration batch (%s): frame %.2e state %.2e' % (model, ef, es))
    assert ef <= 1e-3 and es <= 1e-3, (ef, es)
    sess.close()


def test_hip_graph_replay_equals_eager_launches():
    def run(graphs):
        sess, tr, _ = _trainer('dna', 8, use_hip_graphs=graphs)
        for rep in range(2):                 # the second round resets and replays the captured calibration program
            tr.reset_bn_statistics()
            for i in range(4):
                tr.calibrate_bn(*_pairs(8, 80 + i))
        stats = tr.bn_statistics()
        outs = []
        for i in range(4):
            x, a = _pairs(8, 90 + i)
            outs.append(tr.test(x, x, a, bn='stored')[:2])
        seq = np.stack([_pairs(8, 95 + t)[0] for t in range(4)], axis=1)
        acts = np.stack([_pairs(8, 95 + t)[1] for t in range(4)], axis=1)
        pred, _ = tr.test_sequence(seq, seq, acts, bn='stored')
        if graphs:
            progs = [p for p in sess._programs.values() if p.runs >= 2]
            assert progs and all(p.graphs is not None for p in progs)
        sess.close()
        return stats, outs, pred
    s0, o0, p0 = run(False)
    s1, o1, p1 = run(True)
    assert all(np.array_equal(s0[k], s1[k]) for k in s0), 'calibration: HIP-graph replay differs from eager launches'
    assert int(s1['g/conv1/BatchNorm/calibration_rows'][0]) == 4 * 8 * 32 * 32
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(o0, o1)), 'stored program: replay differs'
    assert np.array_equal(p0, p1)


@pytest.mark.timeout(1200)
@pytest.mark.parametrize('model', ['dna', 'plain'])
def test_device_rollout_matches_the_restatement_rollout(model):
    torch.set_num_threads(16)
    B, Tn = 4, 5
    sess, tr, params = _trainer(model, B)
    stats = _calibrate_both(tr, params, model, B)
    rng = np.random.default_rng(8)
    frames = rng.uniform(-1, 1, (B, Tn, 64, 64, 3)).astype(np.float32)
    acts = rng.standard_normal((B, Tn, 10)).astype(np.float32)
    pred, summ = tr.test_sequence(frames, frames, acts, bn='stored')
    host, _ = tr.test_sequence(frames, frames, acts, bn='stored', device_loop=False)
    assert np.array_equal(pred, host), 'the device loop and the step-by-step loop differ'
    want = R.rollout_stored(model, _p64(params), stats, _td(frames), _td(acts), Tn - 1)
    errs = [TC.rel(pred[:, j], want[:, j].numpy()) for j in range(Tn - 1)]
    print('stored rollout (%s): per-step error %s' % (model, ' '.join('%.2e' % e for e in errs)))
    assert pred.shape == (B, Tn - 1, 64, 64, 3) and max(errs) <= 1e-3, errs
    m = tr.rollout_metrics(frames, acts, bn='stored', return_frames=True)
    assert np.array_equal(m['frames'], pred) and set(summ) == {'g_psnr'}
    sess.close()


def test_checkpoint_round_trip_gives_the_same_bits(tmp_path):
    sess, tr, params = _trainer('dna', 8)
    for i in range(3):
        tr.calibrate_bn(*_pairs(8, 50 + i))
    x, a = _pairs(8, 55)
    want_f, want_s, _ = tr.test(x, x, a, bn='stored')
    want_stats = tr.bn_statistics()
    Saver().save(sess, str(tmp_path / 'm'))
    sess.close()
    sess, tr, _ = _trainer('dna', 8, params=_oracle_params('dna', seed=78))
    with pytest.raises(RuntimeError, match='uncalibrated'):
        tr.test(x, x, a, bn='stored')
    Saver().restore(sess, str(tmp_path / 'm'))
    got = tr.bn_statistics()
    assert all(np.array_equal(got[k], want_stats[k]) for k in want_stats) and tr.bn_calibration_rows() == 24
    f, s, _ = tr.test(x, x, a, bn='stored')
    assert np.array_equal(f, want_f) and np.array_equal(s, want_s)
    # a plain graph takes that checkpoint, and a bn_inference graph takes a plain checkpoint (statistics left uncalibrated)
    sess.close()
    sess, tr, _ = _trainer('dna', 8, bn_inference=False)
    Saver().restore(sess, str(tmp_path / 'm'))
    with pytest.raises(RuntimeError, match='bn_inference'):
        tr.test(x, x, a, bn='stored')
    Saver().save(sess, str(tmp_path / 'plain'))
    sess.close()
    sess, tr, _ = _trainer('dna', 8)
    Saver().restore(sess, str(tmp_path / 'plain'))
    assert tr.bn_calibration_rows() == 0
    sess.close()


def _train_briefly(out):
    T.main(['synthetic', str(out), '--adv', 'True', '--dna', '--batch_size', '8', '--pretrain_iter', '0', '--train_iter', '3'])
    return str(out / 'models')


def _sequences(path, n=5, t=8, seed=4):
    """n sequences as a frames / actions .npy pair (the synthetic source draws other sequences at another batch size)."""
    rng = np.random.default_rng(seed)
    np.save(path / 'frames.npy', rng.uniform(-1, 1, (n, t, 64, 64, 3)).astype(np.float32))
    np.save(path / 'actions.npy', rng.standard_normal((n, t, 10)).astype(np.float32))
    return [str(path / 'frames.npy'), '--actions', str(path / 'actions.npy')]


def test_evaluate_stored_on_a_checkpoint_without_statistics_raises(tmp_path):
    models = _train_briefly(tmp_path / 'run')
    with pytest.raises(ValueError, match='model'):
        E.main([models, 'synthetic', str(tmp_path / 'ev'), '--dna', '--num_sequences', '4', '--batch_size', '4', '--bn_stats', 'stored'])
    assert not (tmp_path / 'ev' / 'metrics.json').exists()


@pytest.mark.timeout(1200)
def test_cli_calibrated_predictions_do_not_move_with_the_batch_size(tmp_path):
    """train briefly; evaluate 5 sequences at batch 4 (4 + 1 real row and 3 padding rows) and at batch 5 (no padding).  With
    --bn_stats calibrate the dumped predictions agree within twice the 1e-3 bar; with --bn_stats batch they do not."""
    models = _train_briefly(tmp_path / 'run')
    src = _sequences(tmp_path)
    pred, metrics = {}, {}
    for mode in ('calibrate', 'batch'):
        for b in (4, 5):
            ev = tmp_path / ('%s_%d' % (mode, b))
            extra = ['--calibrate_batch_size', '16', '--calibrate_batches', '4', '--calibrate_input', 'synthetic'] if mode == 'calibrate' else []
            E.main([models, src[0], str(ev), '--dna', '--batch_size', str(b), '--samples', '0', '--dump', '--bn_stats', mode] + src[1:] + extra)
            pred[mode, b] = np.load(ev / 'predictions.npy')
            metrics[mode, b] = json.load(open(ev / 'metrics.json'))
            assert pred[mode, b].shape == (5, 7, 64, 64, 3)
    for b in (4, 5):
        m = metrics['calibrate', b]
        assert m['bn_statistics'] == 'calibrate' and m['calibration_rows'] == 64 and m['sequences'] == 5
        assert 'bn_statistics' not in metrics['batch', b] and 'calibration_rows' not in metrics['batch', b]
        assert (tmp_path / ('calibrate_%d' % b) / 'calibrated.npz').exists() and not (tmp_path / ('batch_%d' % b) / 'calibrated.npz').exists()
    stored = TC.rel(pred['calibrate', 4], pred['calibrate', 5])
    batch = TC.rel(pred['batch', 4], pred['batch', 5])
    print('predictions at batch 4 against batch 5: stored %.3e, batch statistics %.3e' % (stored, batch))
    assert stored <= 2e-3, stored
    assert batch > 2e-3, batch
    # the calibrated checkpoint is a normal checkpoint: --bn_stats stored takes it, at a batch of one
    ev = tmp_path / 'stored_1'
    got = E.main([str(tmp_path / 'calibrate_4' / 'calibrated'), src[0], str(ev), '--dna', '--num_sequences', '2', '--batch_size', '1',
                  '--samples', '0', '--dump', '--bn_stats', 'stored'] + src[1:])
    assert got['bn_statistics'] == 'stored' and got['calibration_rows'] == 64
    assert TC.rel(np.load(ev / 'predictions.npy'), pred['calibrate', 5][:2]) <= 2e-3


def test_library_exports_the_bn_infer_table():
    lib = _lib.get()
    assert all(hasattr(lib, n[4:]) for n in _lib.EXTENSIONS['bn_infer'].signatures)
