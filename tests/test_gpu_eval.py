"""Checkpoint evaluation on the GPU: the SSIM / squared-error kernel (include/acgan_metrics.h) against the float64 restatement
(tests/ssim_ref.py), Trainer.rollout_metrics against test_sequence, the evaluate CLI end to end, and the SSIM curve of
train()'s eval block."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

import ssim_ref as R

from action_conditioned_gans_amd import _lib
from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import metrics as M
from action_conditioned_gans_amd import train as T

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SSIM_BAR, SQ_BAR = 1e-5, 1e-6


def _inputs(kind, shape, rng):
    if kind == 'uniform':
        return rng.uniform(-1, 1, shape), rng.uniform(-1, 1, shape)
    if kind == 'noise':                                  # SSIM near 1: where the moments cancel
        y = rng.uniform(-1, 1, shape)
        return y + 1e-3 * rng.standard_normal(shape), y
    if kind == 'constant':                               # one value per frame
        lead = shape[:-3] + (1, 1, 1)
        return np.broadcast_to(rng.uniform(-1, 1, lead), shape), np.broadcast_to(rng.uniform(-1, 1, lead), shape)
    if kind == 'extremes':
        return rng.choice([-1.0, 1.0], shape), rng.choice([-1.0, 1.0], shape)
    raise ValueError(kind)


def _stored(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV).to(dt)


def _check(x, y, tag):
    ssim, sq = M.frame_metrics(x, y)
    xs, ys = x.double().cpu().numpy(), y.double().cpu().numpy()
    want_s, want_q = R.ssim(xs, ys), R.sqerr(xs, ys)
    got_s, got_q = ssim.cpu().numpy().astype(np.float64), sq.cpu().numpy().astype(np.float64)
    assert got_s.shape == want_s.shape and got_q.shape == want_q.shape
    err_s = np.abs(got_s - want_s).max()
    err_q = (np.abs(got_q - want_q) / np.maximum(want_q, 1e-30)).max()
    assert err_s <= SSIM_BAR, (tag, err_s)
    assert err_q <= SQ_BAR or np.abs(got_q - want_q).max() <= 1e-30, (tag, err_q)
    return ssim, sq


SHAPES = [(1, 11, 11, 3), (7, 37, 53, 3), (224, 64, 64, 3), (224, 128, 128, 3), (5, 40, 70, 1), (3, 23, 150, 2)]
KINDS = ['uniform', 'noise', 'constant', 'extremes']
STORAGE = {'f32': (torch.float32, torch.float32), 'bf16': (torch.bfloat16, torch.bfloat16), 'mixed': (torch.bfloat16, torch.float32),
           'mixed_rev': (torch.float32, torch.bfloat16)}


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', KINDS)
def test_kernel_matches_float64_f32(shape, kind):
    rng = np.random.default_rng(zlib.crc32(repr((shape, kind)).encode()))
    x, y = _inputs(kind, shape, rng)
    _check(_stored(x, torch.float32), _stored(y, torch.float32), (shape, kind))


@pytest.mark.parametrize('storage', ['bf16', 'mixed', 'mixed_rev'])
@pytest.mark.parametrize('shape', [(1, 11, 11, 3), (7, 37, 53, 3), (224, 64, 64, 3)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', KINDS)
def test_kernel_matches_float64_bf16(shape, kind, storage):
    """Storage in bf16 (one input or both; the restatement reads the same stored values), arithmetic in float32."""
    rng = np.random.default_rng(zlib.crc32(repr((shape, kind, storage)).encode()))
    x, y = _inputs(kind, shape, rng)
    ta, tb = STORAGE[storage]
    _check(_stored(x, ta), _stored(y, tb), (shape, kind, storage))


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
def test_channel_pitch_and_determinism(dt):
    rng = np.random.default_rng(11)
    x, y = _inputs('uniform', (9, 64, 64, 3), rng)
    a, b = _stored(x, dt), _stored(y, dt)
    s3, q3 = M.frame_metrics(a, b)
    pad = lambda t: torch.cat([t, torch.zeros_like(t[..., :1])], dim=-1).contiguous()     # the pitch-4 copies (images.padded)
    s4, q4 = M.frame_metrics(pad(a), pad(b), channels=3)
    assert torch.equal(s3, s4) and torch.equal(q3, q4)
    s3b, q3b = M.frame_metrics(a, b)
    assert torch.equal(s3, s3b) and torch.equal(q3, q3b)            # two launches, same bits
    # the stream argument: the session's (= torch's current) stream handle or a torch stream
    s5, _ = M.frame_metrics(a, b, stream=torch.cuda.current_stream())
    assert torch.equal(s3, s5)


@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
def test_loader_paths_agree_to_the_bit(dt):
    """The four cases of the row loader on one input.  (2, 23, 75, 3) is two strips, the second ragged; a row is 225 elements at
    pitch 3 (scalar loads, unpitched), 300 at pitch 4 (vector loads, pitched) and 375 at pitch 5 (scalar loads, pitched); the
    vector loader without a pitch is what every 64 x 64 x 3 case above runs."""
    rng = np.random.default_rng(23)
    x, y = _inputs('uniform', (2, 23, 75, 3), rng)
    a, b = _stored(x, dt), _stored(y, dt)
    s3, q3 = _check(a, b, ('pitch 3', dt))
    for pitch in (4, 5):
        pad = lambda t: torch.cat([t, torch.zeros(t.shape[:-1] + (pitch - 3,), dtype=t.dtype, device=t.device)], dim=-1).contiguous()   # noqa: E731
        s, q = M.frame_metrics(pad(a), pad(b), channels=3)
        assert torch.equal(s, s3) and torch.equal(q, q3), pitch


def test_too_small_frames_raise():
    x = torch.zeros(2, 10, 64, 3, device=DEV)
    with pytest.raises(_lib.AcgError, match='smaller than the 11 x 11'):
        M.frame_metrics(x, x)
    y = torch.zeros(2, 64, 10, 3, device=DEV)
    with pytest.raises(_lib.AcgError):
        M.frame_metrics(y, y)
    assert _lib.get().frame_metrics_workspace_bytes(2, 10, 64) == 0


# ---- Trainer.rollout_metrics ------------------------------------------------------------------------------------------
def _trainer(dna, dtype, batch=4, ksize=5):
    G.reset_default_graph()
    sess = G.Session(device=DEV, dtype=dtype)
    tr = T.Trainer(sess, False, 'bce', 'adam', dna, batch_size=batch, img_size=64, ksize=ksize)
    sess.run(G.global_variables_initializer())
    return sess, tr


@pytest.mark.parametrize('dna,dtype', [(True, 'f32'), (True, 'bf16'), (False, 'f32')])
def test_rollout_metrics_matches_restatement(dna, dtype):
    sess, tr = _trainer(dna, dtype)
    rng = np.random.default_rng(21)
    frames = rng.uniform(-1, 1, (4, 6, 64, 64, 3)).astype(np.float32)
    acts = rng.standard_normal((4, 6, 10)).astype(np.float32)
    m = tr.rollout_metrics(frames, acts, return_frames=True)
    pred, _ = tr.test_sequence(frames, frames, acts)
    assert np.array_equal(m['frames'], pred)                      # the same rollout, the same bits
    truth = frames[:, 1:].astype(np.float64)
    ident = np.broadcast_to(frames[:, :1], truth.shape)
    for key, src in (('', pred), ('identity_', ident)):
        assert m[key + 'ssim'].shape == (4, 5) and m[key + 'sqerr'].shape == (4, 5)
        assert np.abs(m[key + 'ssim'] - R.ssim(src, truth)).max() <= 1e-5, key
        want_q = R.sqerr(src, truth)
        assert (np.abs(m[key + 'sqerr'] - want_q) / want_q).max() <= 1e-5, key
    # single-batch PSNR from the kernel's sums = the train loop's rollout_psnr formula
    psnr = E.set_psnr(m['sqerr'], np.ones(4, bool), 64 * 64 * 3)
    loop = [10.0 * np.log10(1.0 / max(np.mean((pred[:, j] - frames[:, j + 1]) ** 2), 1e-30)) for j in range(5)]
    assert np.abs(psnr - np.array(loop)).max() <= 1e-4
    # no frames unless asked for, and the identity half can be skipped
    m2 = tr.rollout_metrics(frames, acts, steps=2, identity=False)
    assert sorted(m2) == ['sqerr', 'ssim'] and np.abs(m2['ssim'] - m['ssim'][:, :2]).max() <= 1e-6
    sess.close()


# ---- evaluate CLI end to end -------------------------------------------------------------------------------------------
def _train_checkpoint(root, dna, iters=3):
    model_dir = str(root / ('models_dna' if dna else 'models_plain'))
    os.makedirs(model_dir)
    tr = T.train('synthetic', None, None, None, model_dir, False, 'bce', 'adam', dna, batch_size=4, seq_len=5, train_iter=iters,
                 pretrain_iter=0, device=DEV, quiet=True, eval_every=0, log_every=1)
    tr.sess.close()
    return model_dir


def test_evaluate_cli_end_to_end(tmp_path):
    model_dir = _train_checkpoint(tmp_path, dna=True)
    rng = np.random.default_rng(31)
    frames = rng.uniform(-1, 1, (10, 5, 64, 64, 3)).astype(np.float32)
    acts = rng.standard_normal((10, 5, 10)).astype(np.float32)
    f, a, out = str(tmp_path / 'frames.npy'), str(tmp_path / 'actions.npy'), tmp_path / 'eval'
    np.save(f, frames)
    np.save(a, acts)
    res = E.main([model_dir, f, str(out), '--actions', a, '--dna', '--batch_size', '4', '--dump', '--gif', '--samples', '3'])
    got = json.load(open(out / 'metrics.json'))
    assert got == json.loads(json.dumps(res))
    assert got['sequences'] == 10 and got['steps'] == 4 and got['checkpoint'].endswith('model2')
    assert 'Gaussian' in got['ssim_definition'] and got['frames_per_s'] > 0
    pred = np.load(out / 'predictions.npy')
    assert pred.shape == (10, 4, 64, 64, 3) and np.isfinite(pred).all()
    truth = frames[:, 1:]
    ident = np.broadcast_to(frames[:, :1], truth.shape)
    for key, src in (('', pred), ('identity_', ident)):
        want_ssim = R.ssim(src, truth).mean(axis=0)
        want_psnr = 10 * np.log10(1.0 / (R.sqerr(src, truth).sum(axis=0) / (10 * 64 * 64 * 3)))
        assert np.abs(np.array(got[key + 'ssim']) - want_ssim).max() <= 1e-5, key
        assert np.abs(np.array(got[key + 'psnr']) - want_psnr).max() <= 1e-4, key
    for i in range(3):
        for name in ('generated.gif', 'ground_truth.gif'):
            assert (out / 'sample0' / ('vid%d' % i) / name).is_file()
    assert not (out / 'sample0' / 'vid3').exists()
    # the same checkpoint through its prefix, with PNG samples (BatchNorm runs on batch statistics, as in the reference: another
    # batch size gives other predictions, so only the run itself is checked)
    res2 = E.evaluate(os.path.join(model_dir, 'model2'), f, str(tmp_path / 'eval2'), actions_path=a, dna=True, batch_size=5, samples=1)
    assert res2['sequences'] == 10 and np.isfinite(res2['ssim']).all()
    assert (tmp_path / 'eval2' / 'sample0' / 'vid0' / 'generated3.png').is_file()


def test_evaluate_refuses_the_other_generator(tmp_path):
    model_dir = _train_checkpoint(tmp_path, dna=False, iters=1)
    E.evaluate(model_dir, 'synthetic', str(tmp_path / 'ok'), dna=False, batch_size=4, seq_len=3, num_sequences=4, samples=0)
    with pytest.raises(ValueError, match='checkpoint'):
        E.main([model_dir, 'synthetic', str(tmp_path / 'bad'), '--dna', '--batch_size', '4', '--seq_len', '3', '--num_sequences', '4'])


# ---- train()'s eval block ----------------------------------------------------------------------------------------------
def test_train_eval_block_logs_rollout_ssim(tmp_path):
    log_dir = str(tmp_path / 'logs')
    os.makedirs(log_dir)
    tr = T.train('synthetic', None, None, log_dir, None, False, 'bce', 'adam', True, batch_size=4, seq_len=6, train_iter=5,
                 pretrain_iter=1, device=DEV, quiet=True, eval_every=2, log_every=2)
    tr.sess.close()
    recs = [json.loads(line) for line in open(os.path.join(log_dir, 'test.jsonl'))]
    assert [r['iteration'] for r in recs] == [2, 4]
    for r in recs:
        assert len(r['rollout_ssim']) == 5 and len(r['rollout_psnr']) == 5
        assert all(np.isfinite(v) and -1.0 < v <= 1.0 for v in r['rollout_ssim'])
        assert all(np.isfinite(v) for v in r['rollout_psnr'])
