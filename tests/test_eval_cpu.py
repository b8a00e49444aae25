"""Checkpoint evaluation without a GPU: the float64 SSIM restatement's known answers, util.save_samples, the evaluate CLI's
argument handling, the set-level PSNR and the one-pass PushDataset."""
import os
import shutil

import numpy as np
import pytest

import ssim_ref as R

from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import metrics as M
from action_conditioned_gans_amd import push_data as P
from action_conditioned_gans_amd import util

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the float64 restatement --------------------------------------------------------------------------------------
def test_window_sums_to_one():
    assert abs(R.window_1d().sum() - 1.0) < 1e-15
    assert abs(R.window_2d().sum() - 1.0) < 1e-15
    assert R.window_1d().argmax() == 5 and np.allclose(R.window_1d(), R.window_1d()[::-1])


def test_identical_frames_give_one():
    x = np.random.default_rng(0).uniform(-1, 1, (3, 16, 20, 3))
    assert np.array_equal(R.ssim(x, x), np.ones(3))


@pytest.mark.parametrize('a,b', [(0.3, -0.5), (1.0, -1.0), (0.0, 0.7), (-0.2, -0.2)])
def test_constant_frames(a, b):
    c1 = (0.01 * 2.0) ** 2
    x, y = np.full((12, 13, 3), a), np.full((12, 13, 3), b)
    assert abs(R.ssim(x, y) - (2 * a * b + c1) / (a * a + b * b + c1)) < 1e-12


def test_symmetric_and_valid_only():
    rng = np.random.default_rng(1)
    x, y = rng.uniform(-1, 1, (2, 15, 17, 3)), rng.uniform(-1, 1, (2, 15, 17, 3))
    assert np.allclose(R.ssim(x, y), R.ssim(y, x), rtol=0, atol=1e-14)
    assert R.ssim_map(x, y).shape == (2, 5, 7, 3)
    with pytest.raises(ValueError):
        R.ssim(x[:, :10], y[:, :10])


def test_psnr_formula_and_set_level_psnr_skips_padding():
    assert M.psnr_from_sqerr(4.0, 4) == 0.0
    assert abs(M.psnr_from_sqerr(1.0, 100) - 20.0) < 1e-12
    rng = np.random.default_rng(2)
    sq = rng.uniform(1, 50, (10, 3))
    valid = np.arange(10) < 7
    sq_pad = sq.copy()
    sq_pad[7:] = 1e9                                   # padded rows: whatever they hold must not count
    want = 10 * np.log10(1.0 / (sq[:7].sum(axis=0) / (7 * 64 * 64 * 3)))
    assert np.allclose(E.set_psnr(sq_pad, valid, 64 * 64 * 3), want, rtol=0, atol=1e-12)


def test_frame_metrics_refuses_a_library_without_the_entry():
    """The C oracle implements the training ABI only: there is no host SSIM to fall back to."""
    import torch
    from action_conditioned_gans_amd import _lib
    from oracle import cbind
    x = torch.zeros(1, 11, 11, 3)
    with pytest.raises(_lib.AcgError, match='acg_frame_metrics'):
        M.frame_metrics(x, x, lib=cbind.load())


# ---- save_samples -------------------------------------------------------------------------------------------------
def _video(rng, v, t, s=16):
    return rng.uniform(-1, 1, (v, t, s, s, 3)).astype(np.float32)


def test_save_samples_png_layout_reads_back(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    inp, gen, gt = _video(rng, 2, 4), _video(rng, 2, 3), _video(rng, 2, 3)
    gen[0, 0, 0, 0] = [1.5, -1.5, 1.0]                 # out of range: clipped, not wrapped
    util.save_samples(str(tmp_path), inp, gen, gt, 5)
    for i in range(2):
        d = tmp_path / 'sample5' / ('vid%d' % i)
        assert sorted(os.listdir(d)) == sorted(['frame%d.png' % j for j in range(4)] + ['generated%d.png' % j for j in range(3)]
                                               + ['ground_truth%d.png' % j for j in range(3)])
        for name, src, n in (('frame', inp, 4), ('generated', gen, 3), ('ground_truth', gt, 3)):
            for j in range(n):
                got = np.asarray(Image.open(d / ('%s%d.png' % (name, j))))
                assert got.dtype == np.uint8 and np.array_equal(got, util.to_uint8(src[i, j])), (name, i, j)
    assert np.array_equal(util.to_uint8(np.array([1.5, -1.5, 1.0, -1.0, 0.0])), np.array([255, 0, 255, 0, 127], np.uint8))


def test_save_samples_gif(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(4)
    inp, gen = _video(rng, 3, 7, 24), _video(rng, 3, 6, 24)
    util.save_samples(str(tmp_path), inp, gen, np.array([0]), 0, gif=True)
    for i in range(3):
        d = tmp_path / 'sample0' / ('vid%d' % i)
        assert sorted(os.listdir(d)) == ['generated.gif', 'ground_truth.gif']
        for name, t in (('ground_truth.gif', 7), ('generated.gif', 6)):
            im = Image.open(d / name)
            assert im.n_frames == t and im.size == (24, 24)
            for k in range(t):
                im.seek(k)
                assert im.info['duration'] == 250


# ---- CLI argument handling (no device is touched) --------------------------------------------------------------------
def _npy(tmp_path, n=5, t=4, na=None, ta=None):
    f, a = str(tmp_path / 'frames.npy'), str(tmp_path / 'actions.npy')
    np.save(f, np.zeros((n, t, 64, 64, 3), np.uint8))
    np.save(a, np.zeros((na or n, ta or t, 10), np.float32))
    return f, a


def test_cli_npy_needs_actions(tmp_path, monkeypatch):
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: pytest.fail('evaluate() reached'))
    f, _ = _npy(tmp_path)
    with pytest.raises(SystemExit):
        E.main(['ckpt', f, str(tmp_path / 'out')])


@pytest.mark.parametrize('na,ta', [(6, None), (None, 5)])
def test_cli_frames_and_actions_must_agree(tmp_path, monkeypatch, na, ta):
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: pytest.fail('evaluate() reached'))
    f, a = _npy(tmp_path, na=na, ta=ta)
    with pytest.raises(SystemExit):
        E.main(['ckpt', f, str(tmp_path / 'out'), '--actions', a])


def test_cli_reaches_evaluate(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: seen.update(kw, positional=a))
    f, a = _npy(tmp_path)
    E.main(['models', f, str(tmp_path / 'out'), '--actions', a, '--dna', '--ksize', '11', '--img_size', '64', '--dtype', 'bf16',
            '--batch_size', '4', '--num_sequences', '3', '--samples', '2', '--gif', '--dump'])
    assert seen['positional'] == ('models', f, str(tmp_path / 'out'))
    assert seen['actions_path'] == a and seen['dna'] is True and seen['ksize'] == 11 and seen['dtype'] == 'bf16'
    assert seen['batch_size'] == 4 and seen['num_sequences'] == 3 and seen['samples'] == 2 and seen['gif'] and seen['dump']
    E.main(['models', 'synthetic', str(tmp_path / 'o2'), '--num_sequences', '7'])
    assert seen['positional'][1] == 'synthetic' and seen['dna'] is False and seen['samples'] == 16 and not seen['gif']
    with pytest.raises(SystemExit):
        E.main(['models', 'synthetic', str(tmp_path / 'o3')])          # synthetic needs a count


def test_npy_batches_pad_nothing_and_scale_uint8(tmp_path):
    f, a = _npy(tmp_path, n=10)
    got = list(E._batches(f, a, 4, 64, 8, None))
    assert [b[0].shape[0] for b in got] == [4, 4, 2]
    assert got[0][0].dtype == np.float32 and np.all(got[0][0] == -1.0)
    assert [b[0].shape[0] for b in E._batches(f, a, 4, 64, 8, 5)] == [4, 1]
    padded = E._pad(got[-1][0], 4)
    assert padded.shape[0] == 4 and np.array_equal(padded[3], got[-1][0][1])


# ---- one-pass PushDataset -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('threads', [0, 2])
def test_push_dataset_one_pass(tmp_path, threads):
    src = os.path.join(HERE, 'golden', 'push_tiny.tfrecord')
    for k in range(3):
        shutil.copy(src, str(tmp_path / ('val_%d.tfrecord' % k)))
    img, act, state = P.decode_example(next(iter(P.read_records(src))))
    ds = P.PushDataset(str(tmp_path), 2, train_val_split=0.0, training=False, one_pass=True, num_threads=threads)
    with ds:
        sizes = []
        for frames, _, acts, _ in ds:
            sizes.append(frames.shape[0])
            assert np.array_equal(acts[..., :5], np.broadcast_to(act, acts[..., :5].shape))
            assert np.abs(np.asarray(frames) - img).max() == 0
        assert sizes == [2, 1]                         # each record once, the last batch partial
        with pytest.raises(StopIteration):
            ds.get_batch()
    # the default stream is unchanged: shuffled, endless
    with P.PushDataset(str(tmp_path), 2, train_val_split=0.0, training=False, num_threads=0) as ds2:
        for _ in range(3):
            assert ds2.get_batch()[0].shape[0] == 2
        with pytest.raises(TypeError):
            iter(ds2).__next__()
