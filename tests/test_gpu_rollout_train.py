"""GPU: training through the generator's own K-step rollouts (train.Trainer rollout_steps).  The two new kernels
(include/acgan_rollout.h) against float64 brute force, live K-step G steps against the float64 restatement
(tests/rollout_train_ref.py), the K = 1 and HIP-graph call paths, and the CLI end to end."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import rollout_train_ref as R
import train_cases as TC
from dna_cases import dimage_f64 as _dimage_f64
from action_conditioned_gans_amd import _lib
from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


IMG_CASES = [(1, 19, 37, 3, 3), (2, 33, 21, 1, 5), (1, 40, 70, 4, 6), (2, 29, 45, 3, 11), (3, 64, 64, 3, 5), (1, 17, 17, 4, 11),
             # the other kernel sizes (each ACG_DIMAGE_CASE is an instantiation of its own), ragged against the 32 x 32 tile; C = 2;
             # (1, 5, 3, 2, 8): an image narrower than k - 1
             (1, 5, 9, 3, 1), (2, 6, 35, 2, 2), (1, 9, 33, 1, 4), (1, 7, 40, 3, 7), (1, 5, 3, 2, 8), (2, 4, 34, 4, 9), (1, 3, 66, 3, 10)]


@pytest.mark.parametrize('case', IMG_CASES, ids=str)
@pytest.mark.parametrize('bias_on,dout2_on,acc', [(False, False, 0.0), (True, True, 0.0), (True, False, 1.0), (False, True, 0.5)],
                         ids=['plain', 'bias_dout2', 'bias_acc1', 'dout2_acc05'])
def test_image_gradient_matches_float64(case, bias_on, dout2_on, acc):
    b, h, w, c, k = case
    gen = torch.Generator().manual_seed(b * 1000 + h + w + k)
    z = torch.randn(b, h, w, k * k, generator=gen, dtype=torch.float64) * 3
    z[0, :2] = 30.0 * torch.sign(torch.randn(2, w, k * k, generator=gen, dtype=torch.float64))     # extreme logits
    bias = torch.randn(k * k, generator=gen, dtype=torch.float64) if bias_on else None
    dout = torch.randn(b, h, w, c, generator=gen, dtype=torch.float64)
    pitch, off = 8, 4 - (c == 4) * 4
    d2 = torch.randn(b, h, w, pitch, generator=gen, dtype=torch.float64) if dout2_on else None
    prev = torch.randn(b, h, w, c, generator=gen, dtype=torch.float64)
    g = dout + (d2[..., off:off + c] if dout2_on else 0.0)
    want = _dimage_f64(z, bias, g, k) + (acc * prev if acc else 0.0)
    f = lambda t: None if t is None else t.float().to(DEV).contiguous()     # noqa: E731
    zd, bd, dd, d2d = f(z), f(bias), f(dout), f(d2)
    lib = _lib.get()
    outs = []
    for _ in range(2):
        out = f(prev)
        lib.dna_bwd_image(_p(zd), _p(bd), _p(dd), _p(d2d), pitch if dout2_on else 0, off if dout2_on else 0, _lib.ACG_F32, _p(out), acc,
                          b, h, w, c, k, _lib.ACG_F32, _stream())
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]), 'two launches differ'
    got = outs[0].double().cpu()
    scale = max(want.abs().max().item(), 1e-30)
    assert (got - want).abs().max().item() <= 1e-5 * scale


@pytest.mark.parametrize('rows_hw,batch,groups,pitch,c_off,n', [(16, 2, 1, 268, 256, 10), (256, 32, 2, 140, 133, 5), (7, 3, 1, 12, 0, 12),
                                                               (256, 1, 1, 140, 128, 10), (1, 5, 2, 300, 1, 299)], ids=str)
def test_action_gradient_matches_float64(rows_hw, batch, groups, pitch, c_off, n):
    """Rows of ``groups`` stacked sub-batches of ``batch`` samples x ``rows_hw`` pixels; the (div, mod) mapping is (hw, batch):
    sample q of every sub-batch feeds row q of the [batch, n] gradient (a joined batch when groups == 2)."""
    gen = torch.Generator().manual_seed(rows_hw + batch + n)
    rows = groups * batch * rows_hw
    dcat = torch.randn(rows, pitch, generator=gen, dtype=torch.float64)
    prev = torch.randn(batch, n, generator=gen, dtype=torch.float64)
    want = dcat[:, c_off:c_off + n].reshape(groups, batch, rows_hw, n).sum(dim=(0, 2))
    lib = _lib.get()
    for acc in (0.0, 1.0):
        outs = []
        for _ in range(2):
            out = prev.float().to(DEV).contiguous()
            dd = dcat.float().to(DEV).contiguous()
            lib.action_grad(_p(dd), rows, pitch, c_off, n, rows_hw, batch, _p(out), acc, _stream())
            outs.append(out)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1])
        ref = want + (prev if acc else 0.0)
        assert (outs[0].double().cpu() - ref).abs().max().item() <= 1e-5 * max(ref.abs().max().item(), 1.0)


def _inputs(B, K, S=64, seed=21):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (B, K + 1, S, S, 3)).astype(np.float32)
    for j in range(1, K + 1):                 # frames that follow from their predecessors: a shift plus noise
        x[:, j] = np.clip(np.roll(x[:, j - 1], 2, axis=2) + 0.05 * rng.standard_normal(x[:, j].shape).astype(np.float32), -1, 1)
    a = rng.standard_normal((B, K, 10)).astype(np.float32)
    s = rng.standard_normal((B, K, 5)).astype(np.float32)
    return x, a, s


def _trainer(B, K, loss='bce', opt='adam', dna=True, seed=9, **sess_kw):
    from oracle import models as OM
    params = OM.init_params(dna, batch=B, img=64, ksize=5, seed=seed, dtype=torch.float32)
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device=DEV, **sess_kw)
    tr = T.Trainer(sess, True, loss, opt, dna, batch_size=B, img_size=64, ksize=5, rollout_steps=K)
    sess.run(G.global_variables_initializer())
    for n, v in G.get_default_graph().variables.items():
        sess.set_value(v, params[n])
    return sess, tr, params


LIVE = [(2, 2, 'bce', 'adam', True), (2, 3, 'wass', 'rmsprop', True), (32, 3, 'bce', 'adam', True), (32, 2, 'wass', 'rmsprop', True),
        (2, 3, 'bce', 'adam', False), (32, 2, 'bce', 'adam', False)]


@pytest.mark.parametrize('B,K,loss,opt,dna', LIVE, ids=str)
def test_rollout_g_step_matches_float64_restatement(B, K, loss, opt, dna):
    """A live K-step G step against the float64 restatement at config 2's 1e-3 bars: the frames (and states) of every step,
    the G loss, the per-variable gradient norms and, for RMSProp, the weights after the update."""
    sess, tr, params = _trainer(B, K, loss, opt, dna)
    x, a, s = _inputs(B, K)
    fetch = [tr.g_rollout_opt_op, tr.rollout_losses, tr.rollout_frames] + ([tr.rollout_states] if dna else [])
    res = sess.run(fetch, tr._rollout_feed(x, a, s))
    td = lambda t: torch.from_numpy(np.ascontiguousarray(t)).double()     # noqa: E731
    torch.set_num_threads(16)
    ref = R.RolloutOracle({k: v.double() for k, v in params.items()}, True, loss, opt, dna, 5)
    out = ref.train_g(td(x), td(a), td(s))
    for j in range(K):
        assert TC.rel(res[2][j], out['frames'][j].numpy()) <= 1e-3, 'frame of step %d' % j
        if dna:
            assert TC.rel(res[3][j], out['states'][j].numpy()) <= 1e-3, 'state of step %d' % j
    g_loss = float(np.mean([v[0] for v in res[1]]))
    want = float(out['g_loss'])
    assert abs(g_loss - want) <= 1e-3 * max(abs(want), 1e-2), (g_loss, want)
    TC.check_norms(TC.flat_grad_norms(sess, tr.g_rollout_opt_op), {'g/' + k: v.norm() for k, v in ref.last_grads.items()},
                   'g/', 1e-3, 'rollout G grad')
    if opt == 'rmsprop':
        for n, v in G.get_default_graph().variables.items():
            if n.startswith('g/'):
                got, w = sess.get_value(v).double().cpu(), ref.p[n]
                assert (got - w).abs().max().item() <= 1e-3 * max(w.abs().max().item(), 1e-3) + 2e-6, n
    sess.close()


def test_rollout_pretrain_matches_float64_restatement():
    sess, tr, params = _trainer(2, 3, 'bce', 'rmsprop', True)
    x, a, s = _inputs(2, 3, seed=5)
    got = tr.pretrain_g_rollout(x, a, s)
    td = lambda t: torch.from_numpy(np.ascontiguousarray(t)).double()     # noqa: E731
    ref = R.RolloutOracle({k: v.double() for k, v in params.items()}, True, 'bce', 'rmsprop', True, 5)
    out = ref.pretrain_g(td(x), td(a), td(s))
    assert abs(got - float(out['step_loss'][-1])) <= 1e-3 * abs(float(out['step_loss'][-1]))
    TC.check_norms(TC.flat_grad_norms(sess, tr.g_rollout_pretrain_opt_op), {'g/' + k: v.norm() for k, v in ref.last_grads.items()},
                   'g/', 1e-3, 'rollout pretrain grad')
    sess.close()


def test_k1_rollout_is_train_g_bit_for_bit():
    x, a, s = _inputs(4, 1, seed=3)
    got = {}
    for how in ('rollout', 'plain'):
        sess, tr, _ = _trainer(4, 1)
        for _ in range(3):
            frames = tr.train_g_rollout(x, a, s) if how == 'rollout' else tr.train_g(x[:, 0], x[:, 1], a[:, 0], s[:, 0])
        got[how] = (frames, {n: sess.get_value(v).cpu().clone() for n, v in G.get_default_graph().variables.items()})
        sess.close()
    assert np.array_equal(got['rollout'][0], got['plain'][0])
    assert all(torch.equal(got['rollout'][1][n], got['plain'][1][n]) for n in got['plain'][1])


def test_hip_graph_replay_equals_eager_launches():
    x, a, s = _inputs(4, 3, seed=4)
    got = {}
    for graphs in (False, True):
        sess, tr, _ = _trainer(4, 3, 'wass', 'rmsprop', True, use_hip_graphs=graphs)
        tr.pretrain_g_rollout(x, a, s)
        for _ in range(3):                      # eager -> capture -> replay
            frames = tr.train_g_rollout(x, a, s)
        got[graphs] = (frames, {n: sess.get_value(v).cpu().clone() for n, v in G.get_default_graph().variables.items()})
        sess.close()
    assert np.array_equal(got[False][0], got[True][0])
    assert all(torch.equal(got[False][1][n], got[True][1][n]) for n in got[True][1])


def test_cli_train_with_rollouts_then_evaluate(tmp_path):
    out, ev = tmp_path / 'run', tmp_path / 'eval'
    T.main(['synthetic', str(out), '--dna', '--adv', 'True', '--rollout_steps', '3', '--batch_size', '8', '--pretrain_iter', '0',
            '--train_iter', '3'])
    rec = [json.loads(l) for l in open(out / 'logs' / 'train.jsonl')]
    assert rec and all(r['rollout_steps'] == 3 and np.isfinite(r['g_loss']) for r in rec)
    E.main([str(out / 'models'), 'synthetic', str(ev), '--dna', '--num_sequences', '16'])
    got = json.load(open(ev / 'metrics.json'))
    assert got['sequences'] == 16 and all(np.isfinite(got[k]).all() for k in ('ssim', 'psnr'))
    assert os.path.isfile(os.path.join(str(out), 'logs', 'test.jsonl'))


def test_library_exports_the_rollout_table():
    lib = _lib.get()
    assert all(hasattr(lib, n[4:]) for n in _lib.EXTENSIONS['rollout'].signatures)
