"""GPU: the SSIM training loss.  acg_ssim_loss (include/acgan_ssim_loss.h) against the float64 restatements of
tests/ssim_loss_ref.py - the gradient held to 8 x the larger error of two float32 CPU evaluations of the same case, the value
to tests/test_gpu_eval.py's SSIM bar per frame - and its determinism properties; then the term through the runtime: live G
steps against the oracle with the term added, the K-step rollout, the look-ahead and HIP-graph call paths, and the CLI."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import ssim_loss_ref as R
import train_cases as TC
from action_conditioned_gans_amd import _lib
from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import metrics as M
from action_conditioned_gans_amd import ops as O
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FACTOR = 8.0              # summation order and FMA contraction on top of the float32 floor; a wrong tap, halo or normalisation
                          # is off by 1e-2 .. 1 of max|g|
VALUE_BAR = 1e-5          # per frame: test_gpu_eval.py's SSIM bar
GUARD = 64                # sentinel floats on either side of the gradient buffer

# one map position | tiny and ragged | the map narrower than the window: the adjoint halo clips on both sides | crosses a
# 64-column strip, odd sizes | the product's shape | several bands and tiles
SHAPES = [(1, 11, 11, 1), (2, 12, 13, 3), (1, 21, 27, 4), (2, 33, 75, 3), (3, 64, 64, 3), (1, 128, 128, 3)]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(x, y, value=True, grad=True, gw=1.0):
    """One acg_ssim_loss call on NaN-filled outputs -> (value tensor [1] or None, gradient tensor or None); the gradient buffer and
    the workspace sit between sentinels that the call must leave alone."""
    lib = _lib.get()
    n, h, w, c = x.shape
    xd, yd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(np.ascontiguousarray(y)).to(DEV)
    nbytes = lib.ssim_loss_workspace_bytes(n, h, w, c)
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    val = torch.full((1,), float('nan'), device=DEV) if value else None
    buf = torch.full((x.size + 2 * GUARD,), -12345.0, device=DEV) if grad else None
    dp = buf[GUARD:GUARD + x.size] if grad else None
    if grad:
        dp.fill_(float('nan'))
    lib.ssim_loss(_p(xd), _p(yd), _p(val), _p(dp), float(gw), n, h, w, c, 2.0, 0.01, 0.03, _p(ws), nbytes, _stream())
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all()), 'the call wrote past its workspace'
    if grad:
        assert bool((buf[:GUARD] == -12345.0).all()) and bool((buf[GUARD + x.size:] == -12345.0).all()), 'the call wrote outside dpred'
        dp = dp.reshape(x.shape).clone()
    return val, dp


@functools.lru_cache(maxsize=None)
def _reference(kind, shape):
    """Computed once per case and shared: inputs, float64 gradient and value, and the errors of the two float32 CPU evaluations."""
    x, y = R.case(kind, shape, seed=sum(shape))
    g64 = R.grad_autograd(x, y)
    e_a = float(np.abs(R.grad_autograd(x, y, torch.float32) - g64).max())
    e_b = float(np.abs(R.grad_closed32(x, y) - g64).max())
    for a in (x, y, g64):
        a.setflags(write=False)
    return dict(x=x, y=y, g64=g64, e_a=e_a, e_b=e_b, value=R.value64(x, y), scale=float(np.abs(g64).max()))


def measure(kind, shape):
    """-> dict of what one case measures (also what tools/bench_ssim_loss.py --parity writes to profiles/ssim_loss/parity.txt)."""
    ref = _reference(kind, shape)
    val, dp = _call(ref['x'], ref['y'])
    val2, dp2 = _call(ref['x'], ref['y'])
    err = float(np.abs(dp.double().cpu().numpy() - ref['g64']).max())
    bar = FACTOR * max(ref['e_a'], ref['e_b'])
    return dict(ref, err=err, bar=bar, ratio=err / bar, got_value=float(val.item()), value_err=abs(float(val.item()) - ref['value']),
                repeat_equal=torch.equal(dp, dp2) and torch.equal(val, val2), finite=bool(torch.isfinite(dp).all()))


@pytest.mark.parametrize('shape', SHAPES, ids=str)
@pytest.mark.parametrize('kind', R.CLASSES)
def test_gradient_and_value_against_float64(kind, shape):
    m = measure(kind, shape)
    print('%s %s: |g_gpu - g64| %.3e = %.3f of the bar %.3e (e_a %.2e, e_b %.2e, max|g| %.3e); value %.7f vs %.7f'
          % (kind, shape, m['err'], m['ratio'], m['bar'], m['e_a'], m['e_b'], m['scale'], m['got_value'], m['value']))
    assert m['finite'], 'an element of dpred was not written (or is not finite)'
    assert m['err'] <= m['bar']
    assert m['value_err'] <= shape[0] * VALUE_BAR
    assert m['repeat_equal'], 'a second launch gave other bits'


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_pred_equal_to_truth(shape):
    ref = _reference('near_identical', shape)
    val, dp = _call(ref['y'], ref['y'])
    assert abs(float(val.item())) <= shape[0] * VALUE_BAR
    assert float(dp.abs().max().item()) <= FACTOR * max(ref['e_a'], ref['e_b'])     # the near-identical bar of the same shape


@pytest.mark.parametrize('shape', [(2, 12, 13, 3), (3, 64, 64, 3)], ids=str)
def test_grad_weight_scales_to_the_last_bit(shape):
    ref = _reference('smooth', shape)
    _, base = _call(ref['x'], ref['y'], value=False)
    for k in (0.25, 8.0, -2.0):
        _, got = _call(ref['x'], ref['y'], value=False, gw=k)
        assert torch.equal(got, base * k), k
    _, zero = _call(ref['x'], ref['y'], value=False, gw=0.0)
    assert not bool(zero.any())


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_value_only_and_gradient_only_equal_the_combined_call(shape):
    ref = _reference('uniform', shape)
    val, dp = _call(ref['x'], ref['y'])
    v_only, none = _call(ref['x'], ref['y'], grad=False)
    none2, g_only = _call(ref['x'], ref['y'], value=False)
    assert none is None and none2 is None
    assert torch.equal(v_only, val) and torch.equal(g_only, dp)


@pytest.mark.parametrize('shape', [(2, 33, 75, 3), (1, 21, 27, 4)], ids=str)
def test_trained_ssim_is_the_reported_ssim(shape):
    """The loss value against sum_n (1 - ssim_n) of frame_metrics on the same float32 frames: each side is held to float64 at
    1e-5 per frame (VALUE_BAR above, SSIM_BAR in tests/test_gpu_eval.py), so the two are within the sum of the two bars."""
    ref = _reference('smooth', shape)
    val, _ = _call(ref['x'], ref['y'], grad=False)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    ssim, _ = M.frame_metrics(to_dev(ref['x']), to_dev(ref['y']))
    reported = float((1.0 - ssim.double()).sum().item())
    print('%s: loss value %.7f, from the metric %.7f' % (shape, float(val.item()), reported))
    assert abs(float(val.item()) - reported) <= 2 * shape[0] * VALUE_BAR


def test_invalid_arguments_are_errors():
    lib = _lib.get()
    assert lib.ssim_loss_workspace_bytes(1, 10, 64, 3) == 0 and lib.ssim_loss_workspace_bytes(1, 64, 10, 3) == 0
    assert lib.ssim_loss_workspace_bytes(0, 64, 64, 3) == 0 and lib.ssim_loss_workspace_bytes(1, 64, 64, 5) == 0
    assert lib.ssim_loss_workspace_bytes(32, 64, 64, 3) >= 32 * 3 * 3 * 54 * 54 * 4
    x = torch.zeros(1, 16, 16, 3, device=DEV)
    out, ws = torch.zeros_like(x), torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    for n, h, w, c in [(1, 10, 16, 3), (1, 16, 10, 3), (1, 16, 16, 5), (0, 16, 16, 3)]:
        with pytest.raises(_lib.AcgError, match='acg_ssim_loss'):
            lib.ssim_loss(_p(x), _p(x), None, _p(out), 1.0, n, h, w, c, 2.0, 0.01, 0.03, _p(ws), ws.numel(), _stream())
    with pytest.raises(_lib.AcgError, match='neither'):
        lib.ssim_loss(_p(x), _p(x), None, None, 1.0, 1, 16, 16, 3, 2.0, 0.01, 0.03, _p(ws), ws.numel(), _stream())
    with pytest.raises(_lib.AcgError, match='workspace'):
        lib.ssim_loss(_p(x), _p(x), None, _p(out), 1.0, 1, 16, 16, 3, 2.0, 0.01, 0.03, _p(ws), 8, _stream())
    torch.cuda.synchronize()


def test_library_exports_the_table():
    lib = _lib.get()
    assert all(hasattr(lib, n[4:]) for n in _lib.EXTENSIONS['ssim_loss'].signatures)


# ---- through the runtime ---------------------------------------------------------------------------------------------------
def _trainer(dna, B=2, loss='bce', opt='adam', weight=0.0, ksize=5, seed=TC.MG.PARAM_SEED, **kw):
    from oracle import models as OM
    sess_kw = {k: kw.pop(k) for k in ('dtype', 'use_hip_graphs') if k in kw}
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device=DEV, **sess_kw)
    tr = T.Trainer(sess, True, loss, opt, dna, batch_size=B, img_size=64, ksize=ksize, ssim_weight=weight, **kw)
    sess.run(G.global_variables_initializer())
    params = None
    if dna != 'cdna':
        params = OM.init_params(bool(dna), batch=B, ksize=ksize, seed=seed, dtype=torch.float32)
        for n, v in G.get_default_graph().variables.items():
            sess.set_value(v, params[n])
    return sess, tr, params


def _td(t):
    return torch.from_numpy(np.ascontiguousarray(t)).double()


def _ssim_share(ref, key, x, y, a, s):
    """In the oracle alone: |d (W g_ssim_loss) / d frame| over |d loss / d frame|."""
    p = ref._with_grad(ref.g_names)
    out = ref._g_losses(p, x, y, a, s)
    total, = torch.autograd.grad(out[key], out['frame'], retain_graph=True)
    part, = torch.autograd.grad(ref.ssim_weight * out['g_ssim_loss'], out['frame'])
    return float(part.norm() / total.norm())


# the GDL and L1 terms are unnormalised sums over the frame: on these random frames their frame gradient has a norm of 358
# (DNA G loss) and 78 (plain pretraining loss) against 9e-3 W / 8e-3 W for the SSIM term (oracle, float64)
@pytest.mark.parametrize('dna,step,weight', [(True, 'train_g', 5000.0), (False, 'pretrain_g', 2000.0)], ids=['dna_train_g', 'plain_pretrain_g'])
def test_g_step_matches_the_oracle_with_the_term(dna, step, weight):
    x, y, a, s = TC.MG.inputs(2)
    sess, tr, params = _trainer(dna, weight=weight, lookahead=False)
    opt_op = tr.g_opt_op if step == 'train_g' else tr.g_pretrain_opt_op
    key = 'g_loss' if step == 'train_g' else 'g_l2_loss'
    res = sess.run([opt_op, tr.g_loss, tr.g_l2_loss, tr.g_ssim_loss, tr.g_next_frame], tr._feed(x, y, a, s))
    torch.set_num_threads(16)
    ref = R.SsimOracleTrainer({k: v.double() for k, v in params.items()}, True, 'bce', 'adam', dna, 5, ssim_weight=weight)
    share = _ssim_share(ref, key, _td(x), _td(y), _td(a), _td(s))
    print('%s: the SSIM term carries %.3f of the frame gradient in the oracle' % (step, share))
    assert share >= 0.10
    p = ref._with_grad(ref.g_names)
    out = ref._g_losses(p, _td(x), _td(y), _td(a), _td(s))
    grads = torch.autograd.grad(out[key], [p[n] for n in ref.g_names], allow_unused=True)
    want = {'g/' + n: g.norm() for n, g in zip(ref.g_names, grads) if g is not None}
    assert TC.rel(res[4], out['frame'].detach().numpy()) <= 1e-3
    for got, k in ((res[1], 'g_loss'), (res[2], 'g_l2_loss'), (res[3], 'g_ssim_loss')):
        assert abs(float(got[0]) - float(out[k])) <= 1e-3 * abs(float(out[k])), (k, float(got[0]), float(out[k]))
    TC.check_norms(TC.flat_grad_norms(sess, opt_op), want, 'g/', 1e-3, step + ' grad')
    sess.close()


def _rollout_inputs(B, K, S=64, seed=21):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (B, K + 1, S, S, 3)).astype(np.float32)
    for j in range(1, K + 1):                 # frames that follow from their predecessors: a shift plus noise
        x[:, j] = np.clip(np.roll(x[:, j - 1], 2, axis=2) + 0.05 * rng.standard_normal(x[:, j].shape).astype(np.float32), -1, 1)
    return x, rng.standard_normal((B, K, 10)).astype(np.float32), rng.standard_normal((B, K, 5)).astype(np.float32)


def test_rollout_g_step_matches_the_restatement_with_the_term():
    B, K, W = 2, 2, 5000.0
    sess, tr, params = _trainer(True, B=B, weight=W, rollout_steps=K, lookahead=False, seed=9)
    x, a, s = _rollout_inputs(B, K)
    res = sess.run([tr.g_rollout_opt_op, tr.rollout_losses, tr.rollout_frames, tr.rollout_states], tr._rollout_feed(x, a, s))
    torch.set_num_threads(16)
    ref = R.SsimRolloutOracle({k: v.double() for k, v in params.items()}, True, 'bce', 'adam', True, 5, ssim_weight=W)
    out = ref.train_g(_td(x), _td(a), _td(s))
    for j in range(K):
        assert TC.rel(res[2][j], out['frames'][j].numpy()) <= 1e-3, 'frame of step %d' % j
        assert TC.rel(res[3][j], out['states'][j].numpy()) <= 1e-3, 'state of step %d' % j
        assert abs(float(res[1][j][0]) - float(out['step_loss'][j])) <= 1e-3 * abs(float(out['step_loss'][j])), j
    TC.check_norms(TC.flat_grad_norms(sess, tr.g_rollout_opt_op), {'g/' + k: v.norm() for k, v in ref.last_grads.items()},
                   'g/', 1e-3, 'rollout G grad')
    sess.close()


def test_lookahead_equals_the_plain_call_path_at_iteration_0():
    """tests/test_gpu_train.py's look-ahead comparison (float32 DNA, batch 8, distinct D-step and G-step samples) with the term,
    at its bars after one iteration: frames 1e-5, D gradient 1e-4, G gradient 5e-3."""
    x, y, a, s = TC.MG.inputs(8)
    xb, yb, ab, sb = [np.ascontiguousarray(np.roll(t, 3, axis=0)[::-1]) for t in (y, x, a, s)]
    nrel = lambda got, want: float(np.linalg.norm(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / np.linalg.norm(np.asarray(want, np.float64)))  # noqa: E731

    def run(use):
        G.reset_default_graph()
        optim.set_data_parallel(1)
        sess = G.Session(device=DEV)
        tr = T.Trainer(sess, True, 'bce', 'rmsprop', True, batch_size=8, ksize=5, ssim_weight=5000.0)
        sess.run(G.global_variables_initializer())
        grad = lambda name: [sess._materialize(t).clone().cpu().double() for t in G.get_default_graph().state if t.name == name][0]   # noqa: E731
        tr.train_d(x, y, a, next_g=(xb, ab) if use else None)
        dg = grad('d_opt/flat_grad')
        frames = np.array(tr.train_g(xb, yb, ab, sb), copy=True)
        gg = grad('g_opt/flat_grad')
        sess.close()
        return frames, dg, gg
    f0, dg0, gg0 = run(False)
    f1, dg1, gg1 = run(True)
    assert np.isfinite(f1).all()
    assert nrel(f1, f0) <= 1e-5 and nrel(dg1, dg0) <= 1e-4 and nrel(gg1, gg0) <= 5e-3, (nrel(f1, f0), nrel(dg1, dg0), nrel(gg1, gg0))


@pytest.mark.parametrize('dna,dtype', [(True, 'f32'), (True, 'bf16'), ('cdna', 'f32')], ids=['dna_f32', 'dna_bf16', 'cdna_f32'])
def test_hip_graph_replay_equals_eager(dna, dtype):
    """Run 1 is eager, run 2 captures, run 3+ replays: weights and frames must match an all-eager session bit for bit."""
    x, y, a, s = TC.MG.inputs(2)
    finals = []
    for use_graphs in (False, True):
        sess, tr, _ = _trainer(dna, weight=50.0, dtype=dtype, use_hip_graphs=use_graphs)
        tr.pretrain_g(x, y, a, s)
        for _ in range(4):
            tr.train_d(x, y, a)
            frames = tr.train_g(x, y, a, s)
        torch.cuda.synchronize()
        finals.append(({n: sess.get_value(v) for n, v in G.get_default_graph().variables.items()}, frames))
        if use_graphs:
            assert all(p.graphs is not None for p in sess._programs.values() if p.runs >= 2)
        sess.close()
    (pe, fe), (pg, fg) = finals
    assert np.isfinite(fe).all()
    for n in pe:
        assert torch.equal(pe[n], pg[n]), n
    assert np.array_equal(fe, fg)


def test_bf16_graph_runs_the_entry_on_the_float32_frame():
    """In a bf16 graph the generated frame is float32: the head's gradient op gives the bits of the stand-alone entry called on
    the fetched frame."""
    x, y, a, s = TC.MG.inputs(2)
    W = 50.0
    sess, tr, _ = _trainer(True, weight=W, dtype='bf16', lookahead=False)
    grad_op = [o for o in G.get_default_graph().ops if isinstance(o, O.SsimLossOp) and o.dgen is not None][0]     # the G step's
    assert grad_op.inputs[0] is tr.g_out and tr.g_out.dtype == torch.float32 and grad_op.grad_weight == W / 2
    res = sess.run([tr.g_opt_op, tr.g_next_frame, grad_op.dgen], tr._feed(x, y, a, s), device_fetch=True)
    frame, got = res[1].clone(), res[2].clone()
    assert frame.dtype == torch.float32 and got.dtype == torch.float32
    _, want = _call(frame.cpu().numpy(), y, value=False, gw=W / 2)
    assert torch.equal(got.reshape(want.shape), want)
    sess.close()


def test_cli_train_with_the_term_then_evaluate(tmp_path):
    out, ev = tmp_path / 'run', tmp_path / 'eval'
    T.main(['synthetic', str(out), '--adv', 'True', '--dna', '--ssim_weight', '50', '--batch_size', '8', '--pretrain_iter', '0',
            '--train_iter', '3'])
    rec = [json.loads(l) for l in open(out / 'logs' / 'train.jsonl')]
    assert rec and all(r['ssim_weight'] == 50.0 and np.isfinite(r['g_loss']) and np.isfinite(r['g_ssim_loss']) for r in rec)
    assert all(0.0 <= r['g_ssim_loss'] <= 2.0 for r in rec)
    E.main([str(out / 'models'), 'synthetic', str(ev), '--dna', '--num_sequences', '16'])
    got = json.load(open(ev / 'metrics.json'))
    assert got['sequences'] == 16 and all(np.isfinite(got[k]).all() for k in ('ssim', 'psnr'))
