"""GPU: the affine (STP) generator and its fused warp-and-composite kernels (include/acgan_cdna.h) against the float64
restatement (tests/affine_ref.py), through the call paths the CDNA generator runs on.

Which staging path runs: there is one.  The kernels read every tap from global memory under a per-tap bounds check, for every
theta (csrc/affine_composite.hip and DESIGN.md say why the LDS box was measured and dropped), so all the cases below - near the
identity, wide, ragged tiles, 64x64 and 128x128 - run the same code; what differs between them is how many taps fall outside."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import affine_ref as R
import train_cases as TC
from action_conditioned_gans_amd import _lib
from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import models as MB
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T
from action_conditioned_gans_amd.saver import Saver

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SHAPES = [(1, 20, 36, 3, 1), (3, 17, 33, 4, 32), (2, 64, 64, 3, 10), (2, 24, 40, 1, 6), (2, 128, 128, 3, 10)]
# (shape, seed, spread): every shape near the identity with two seeds, two of them wide; and 128x128 wide
CASES = [(s, seed, 1) for s in SHAPES for seed in (0, 1)] + [((2, 64, 64, 3, 10), 0, 8), ((2, 24, 40, 1, 6), 0, 8),
                                                             ((2, 128, 128, 3, 10), 0, 8)]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def d(t):
    return t.to(DEV)


def fwd(lib, params, z, bias, img, m, pitch=0, c=None):
    b, h, w = img.shape[:3]
    c = c or img.shape[3]
    out = torch.empty(b, h, w, c, device=DEV)
    lib.affine_composite_fwd(_p(params), _p(z), _p(bias), _p(img), pitch, _p(out), b, h, w, c, m, _stream())
    torch.cuda.synchronize()
    return out


def bwd(lib, params, z, bias, img, dout, m, dbias=None, acc=0.0):
    b, h, w, c = img.shape
    dpar, dz = torch.empty_like(params), torch.empty_like(z)
    nb = lib.affine_composite_workspace_bytes(b, h, w, c, m)
    assert nb > 0
    ws = torch.zeros(nb + 512, dtype=torch.uint8, device=DEV)
    ws[nb:] = 0xA5
    lib.affine_composite_bwd(_p(params), _p(z), _p(bias), _p(img), 0, _p(dout), _p(dpar), _p(dz), _p(dbias), acc, b, h, w, c, m,
                             _p(ws), nb, _stream())
    torch.cuda.synchronize()
    assert bool((ws[nb:] == 0xA5).all()), 'the backward wrote past its workspace'
    return dpar, dz


def nrel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / max(float(want.norm()), 1e-30))


@functools.lru_cache(maxsize=None)
def _case(shape, seed, spread):
    """The shared case (affine_ref.case) with a bias and logits of +-30 in a row each."""
    b, h, w, c, m = shape
    params, z, img, dout = R.case(shape, seed, spread)
    z[:, 0, :, 0], z[:, -1, :, -1] = 30.0, -30.0
    bias = torch.randn(m + 1, generator=torch.Generator().manual_seed(seed + 2000))
    return params, z, bias, img, dout


@functools.lru_cache(maxsize=None)
def _forward_reference(shape, seed, spread):
    """The forward case: mask 0 of every sample has exactly zero parameters and its logit at +30 in row 1.  -> (params, z,
    float64 out)."""
    params, z, bias, img, _ = _case(shape, seed, spread)
    params, z = params.clone(), z.clone()
    params[:, :6] = 0.0
    z[:, 1, :, 1] = 30.0
    with torch.no_grad():
        want = R.composite(z.double() + bias.double(), img.double(), params.double(), shape[4])
    return params, z, want


@functools.lru_cache(maxsize=None)
def _backward_reference(shape, seed, spread):
    """-> (dout under the kink rule, the zeroed share, float64 dparams, dz, dbias)."""
    params, z, bias, img, dout = _case(shape, seed, spread)
    dout, share = R.apply_kink_rule(params, dout)
    pd, zd, bd = (t.double().requires_grad_(True) for t in (params, z, bias))
    R.composite(zd + bd, img.double(), pd, shape[4]).backward(dout.double())
    return dout, share, pd.grad, zd.grad, bd.grad


def _outside_masks(params, h, w):
    """[B, M] bool: every tap of every pixel falls outside the image (by a margin no float32 rounding crosses)."""
    px, py = R.coords(params.double(), h, w)
    out = (px < -1.001) | (px > w + 0.001) | (py < -1.001) | (py > h + 0.001)
    return out.flatten(2).all(dim=2)


@pytest.mark.parametrize('shape,seed,spread', CASES, ids=str)
def test_composite_forward_matches_float64(hip_abi, shape, seed, spread):
    """max|out - want| <= 1e-5 + 2^-20 * max(H, W): a few ulps of a coordinate of magnitude about the image size times a slope
    of at most 2 (the float32 torch restatement stays within 2.1e-5 at 128 and 8.7e-6 at 64)."""
    b, h, w, c, m = shape
    lib = hip_abi.lib
    _, _, bias, img, _ = _case(shape, seed, spread)
    params, z, want = _forward_reference(shape, seed, spread)
    out = fwd(lib, d(params), d(z), d(bias), d(img), m)
    err = (out.cpu().double() - want).abs().max().item()
    print('forward', shape, seed, spread, 'max abs err', err)
    assert err <= 1e-5 + 2.0 ** -20 * max(h, w)
    # the zero-parameter mask under a logit of +30 gives the image in row 1
    assert (out[:, 1].cpu() - img[:, 1]).abs().max().item() <= 1e-5
    if c == 3:                 # the image at a channel pitch of 4 gives the same bits
        img4 = torch.zeros(b, h, w, 4)
        img4[..., :3] = img
        assert torch.equal(fwd(lib, d(params), d(z), d(bias), d(img4), m, pitch=4, c=3), out)
    # without a bias
    with torch.no_grad():
        want0 = R.composite(z.double(), img.double(), params.double(), m)
    out0 = fwd(lib, d(params), d(z), None, d(img), m)
    assert (out0.cpu().double() - want0).abs().max().item() <= 1e-5 + 2.0 ** -20 * max(h, w)


@pytest.mark.parametrize('shape,seed,spread', CASES, ids=str)
def test_composite_backward_matches_float64(hip_abi, shape, seed, spread):
    """nrel <= 1e-4 for dmask_logits, dparams and dmask_bias against float64 under the kink rule (the float32 torch restatement
    agrees with float64 to 7.5e-6 or better on these cases)."""
    b, h, w, c, m = shape
    lib = hip_abi.lib
    params, z, bias, img, _ = _case(shape, seed, spread)
    dout, share, want_p, want_z, want_b = _backward_reference(shape, seed, spread)
    assert share <= R.KINK_SHARE, share
    dbias = torch.full((m + 1,), 123.0, device=DEV)
    dpar, dz = bwd(lib, d(params), d(z), d(bias), d(img), d(dout), m, dbias=dbias, acc=0.0)
    errs = (nrel(dz, want_z), nrel(dpar, want_p), nrel(dbias, want_b))
    print('backward', shape, seed, spread, 'kink share', share, 'nrel dz, dparams, dbias', errs)
    assert max(errs) <= 1e-4, errs
    outside = _outside_masks(params, h, w)
    assert (dpar.cpu().view(b, m, 6)[outside] == 0).all(), 'a mask whose samples all fall outside must have zero gradient'
    dbias2 = dbias.clone()
    dpar2, dz2 = bwd(lib, d(params), d(z), d(bias), d(img), d(dout), m, dbias=dbias2, acc=1.0)
    assert torch.equal(dpar2, dpar) and torch.equal(dz2, dz), 'two launches differ'
    assert torch.equal(dbias2, dbias + dbias), 'accumulate = 1 must add'
    dpar3, dz3 = bwd(lib, d(params), d(z), d(bias), d(img), d(dout), m)       # no bias gradient asked for
    assert torch.equal(dpar3, dpar) and torch.equal(dz3, dz)


def test_a_mask_that_samples_outside_has_zero_gradient_and_adds_nothing(hip_abi):
    shape = (2, 24, 40, 1, 6)
    b, h, w, c, m = shape
    params, z, bias, img, dout = _case(shape, 0, 1)
    params = params.clone()
    params[0, :6] = torch.tensor([0.0, 0.0, 3.0, 0.0, 0.0, 0.0])        # xs = u + 3 >= 2: every px >= 1.5 (W - 1)
    params[1, 6:12] = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, -2.5])      # ys = v - 2.5 <= -1.5: every py <= -(H - 1) / 4
    outside = _outside_masks(params, h, w)
    assert outside[0, 0] and outside[1, 1]
    dpar, dz = bwd(hip_abi.lib, d(params), d(z), d(bias), d(img), d(dout), m)
    assert (dpar.cpu().view(b, m, 6)[outside] == 0).all()
    assert bool(torch.isfinite(dpar).all()) and bool(torch.isfinite(dz).all())
    with torch.no_grad():
        want = R.composite(z.double() + bias.double(), img.double(), params.double(), m)
    out = fwd(hip_abi.lib, d(params), d(z), d(bias), d(img), m)
    assert (out.cpu().double() - want).abs().max().item() <= 1e-5 + 2.0 ** -20 * max(h, w)


def test_unsupported_geometry_is_an_error_and_a_workspace_of_zero(hip_abi):
    lib = hip_abi.lib
    for b, h, w, c, m in [(1, 16, 16, 5, 2), (1, 16, 16, 3, 33), (1, 1, 16, 3, 2), (1, 16, 1, 3, 2)]:
        assert lib.affine_composite_workspace_bytes(b, h, w, c, m) == 0
        t = torch.zeros(b * h * w * 40, device=DEV)
        with pytest.raises(_lib.AcgError):
            lib.affine_composite_fwd(_p(t), _p(t), None, _p(t), 0, _p(t), b, h, w, c, m, _stream())
    t = torch.zeros(4096, device=DEV)
    with pytest.raises(_lib.AcgError):
        lib.affine_composite_fwd(_p(t), _p(t), None, _p(t), 2, _p(t), 1, 16, 16, 3, 2, _stream())      # pitch < C


def _gen_graph(B, S, M=10, seed=3):
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device=DEV)
    img, act = G.placeholder((B, S, S, 3), name='img'), G.placeholder((B, 10), name='act')
    frame, state = MB.build_generator_affine(img, act, num_masks=M)
    sess.run(G.global_variables_initializer())
    params = R.init_params_affine(batch=B, img=S, num_masks=M, seed=seed)
    for n, v in G.get_default_graph().variables.items():
        sess.set_value(v, params[n])
    return sess, img, act, frame, state, params


@pytest.mark.parametrize('B,S', [(2, 64), (2, 128)])
def test_generator_forward_matches_float64(B, S):
    sess, img, act, frame, state, params = _gen_graph(B, S)
    rng = np.random.default_rng(B + S)
    x = rng.uniform(-1, 1, (B, S, S, 3)).astype(np.float32)
    a = rng.standard_normal((B, 10)).astype(np.float32)
    got_f, got_s = sess.run([frame, state], {img: x, act: a})
    with torch.no_grad():
        wf, ws = R.generator_affine({k: v.double() for k, v in params.items()}, torch.from_numpy(x).double(), torch.from_numpy(a).double())
    assert TC.rel(got_f, wf.numpy()) <= 1e-3 and TC.rel(got_s, ws.numpy()) <= 1e-3, (TC.rel(got_f, wf.numpy()), TC.rel(got_s, ws.numpy()))
    sess.close()


STEP_SEED = 9          # of the weights; the frames are affine_ref.smooth_frames(4, seed=21)


def _trainer(B, loss='bce', opt='adam', seed=STEP_SEED, num_masks=4, **kw):
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device=DEV, **{k: v for k, v in kw.items() if k == 'use_hip_graphs'})
    tr = T.Trainer(sess, True, loss, opt, 'affine', batch_size=B, img_size=64, num_masks=num_masks,
                   **{k: v for k, v in kw.items() if k != 'use_hip_graphs'})
    sess.run(G.global_variables_initializer())
    params = R.init_params_affine(batch=B, num_masks=num_masks, seed=seed)
    if not kw.get('noise_dim'):
        for n, v in G.get_default_graph().variables.items():
            sess.set_value(v, params[n])
    return sess, tr, params


def test_one_d_step_and_one_g_step_match_the_oracle():
    """Batch 4, 64x64, 4 masks, bce / adam, smooth frames: the test pass, one D step and one G step against AffineOracleTrainer
    in float64 - losses and per-variable gradient norms to 1e-3.  The oracle trainer itself, run in float32 against float64 on
    the CPU for this seed, stays within 9.1e-5 on every variable's gradient norm (worst: g/conv1/weights; D: 5.7e-5), 4.8e-5 on
    the frame and 6e-8 on the losses - a third of 1e-3 is the limit."""
    B = 4
    sess, tr, params = _trainer(B)
    x, y, a, s = R.smooth_frames(B, seed=21)
    td = lambda t: torch.from_numpy(t).double()     # noqa: E731
    ot = R.AffineOracleTrainer({k: v.double() for k, v in params.items()}, True, 'bce', 'adam', num_masks=4)
    frame, state, _ = tr.test(x, y, a)
    oframe, ostate, _ = ot.test(td(x), td(y), td(a))
    assert TC.rel(frame, oframe.numpy()) <= 1e-3 and TC.rel(state, ostate.numpy()) <= 1e-3
    dsumm = tr.train_d(x, y, a, summarize=True)
    od = ot.train_d(td(x), td(y), td(a), return_all=True)
    assert abs(dsumm['discriminator_loss'] - float(od['d_loss'])) <= 1e-3 * max(abs(float(od['d_loss'])), 1.0)
    TC.check_norms(TC.flat_grad_norms(sess, tr.d_opt_op), {'dgrad_norm/' + k: v.norm() for k, v in ot.last_grads.items()},
                   'dgrad_norm/', 1e-3, 'D grad')
    res = sess.run([tr.g_opt_op, tr.g_loss], tr._feed(x, y, a, s))
    og = ot.train_g(td(x), td(y), td(a), td(s), return_all=True)
    assert abs(res[1][0] - float(og['g_loss'])) <= 1e-3 * abs(float(og['g_loss']))
    TC.check_norms(TC.flat_grad_norms(sess, tr.g_opt_op), {'ggrad_norm/' + k: v.norm() for k, v in ot.last_grads.items()},
                   'ggrad_norm/', 1e-3, 'G grad')
    sess.close()


def test_pretrain_steps_stay_finite_and_lower_the_loss():
    """With the default initialiser the transforms start far from the identity and Adam's first updates of g/affine_params
    overshoot: the float64 oracle's loss on these frames rises for three or four steps before it falls, whatever the seed
    (weights of seed 0, chosen from the oracle's run: 2957, 3662, 5040, 5125, 4484, 3661, 2966, 2282; seed 9: 3100 ... 5791 ...
    3687, below the first value only after 9 steps).  An initialiser nearer the identity is out of scope."""
    sess, tr, _ = _trainer(4, seed=0)
    x, y, a, s = R.smooth_frames(4, seed=7)
    losses = [tr.pretrain_g(x, y, a, s) for _ in range(8)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    sess.close()


def test_hip_graph_replay_equals_eager_launches():
    x, y, a, s = R.smooth_frames(4, seed=5)

    def run(graphs):
        sess, tr, _ = _trainer(4, 'bce', 'rmsprop', use_hip_graphs=graphs)
        for _ in range(3):
            tr.train_d(x, y, a)
            frames = np.array(tr.train_g(x, y, a, s), copy=True)
        final = {k: sess.get_value(v).clone() for k, v in G.get_default_graph().variables.items()}
        if graphs:
            assert all(p.graphs is not None for p in sess._programs.values())
        sess.close()
        return frames, final
    f1, w1 = run(True)
    f2, w2 = run(False)
    assert np.array_equal(f1, f2) and all(torch.equal(w1[k], w2[k]) for k in w1), 'HIP-graph replay differs from eager launches'


def test_checkpoint_round_trip_and_cross_model_restore(tmp_path):
    x, y, a, s = R.smooth_frames(4, seed=3)
    sess, tr, _ = _trainer(4)
    for _ in range(2):
        tr.train_d(x, y, a)
        tr.train_g(x, y, a, s)
    path = str(tmp_path / 'affine')
    Saver().save(sess, path)
    tr.train_d(x, y, a)
    want = tr.train_g(x, y, a, s)
    sess.close()
    sess, tr, _ = _trainer(4, seed=1)
    Saver().restore(sess, path)
    tr.train_d(x, y, a)
    assert np.array_equal(tr.train_g(x, y, a, s), want), 'the restored run does not continue bit-identically'
    sess.close()
    # a CDNA and a DNA checkpoint into the affine graph, and the affine checkpoint into theirs
    for kind, kw in (('cdna', {'num_masks': 4}), (True, {})):
        G.reset_default_graph()
        optim.set_data_parallel(1)
        sess = G.Session(device=DEV)
        T.Trainer(sess, True, 'bce', 'adam', kind, batch_size=4, **kw)
        sess.run(G.global_variables_initializer())
        other = str(tmp_path / ('other_%s' % kind))
        Saver().save(sess, other)
        with pytest.raises(ValueError):
            Saver().restore(sess, path)
        sess.close()
        sess, tr, _ = _trainer(4)
        with pytest.raises(ValueError):
            Saver().restore(sess, other)
        sess.close()


def test_noise_dim_builds_and_steps():
    sess, tr, _ = _trainer(4, noise_dim=4)
    assert G.get_default_graph().variables['g/affine_params/weights'].shape == (4, 4, 270, 24)
    x, y, a, s = R.smooth_frames(4, seed=2)
    tr.train_d(x, y, a)
    frames = tr.train_g(x, y, a, s)
    assert np.isfinite(frames).all()
    sess.close()


def test_cli_train_then_evaluate(tmp_path):
    out, ev = tmp_path / 'run', tmp_path / 'eval'
    T.main(['synthetic', str(out), '--adv', 'True', '--affine', '--batch_size', '8', '--pretrain_iter', '0', '--train_iter', '3'])
    E.main([str(out / 'models'), 'synthetic', str(ev), '--affine', '--num_sequences', '16'])
    got = json.load(open(ev / 'metrics.json'))
    assert got['model'] == 'affine' and got['num_masks'] == 10 and got['ksize'] is None and got['sequences'] == 16
    assert all(np.isfinite(got[k]).all() for k in ('ssim', 'psnr', 'identity_ssim', 'identity_psnr'))


def test_library_exports_the_affine_entries():
    lib = _lib.get()
    assert all(hasattr(lib, n) for n in ('affine_composite_workspace_bytes', 'affine_composite_fwd', 'affine_composite_bwd'))
