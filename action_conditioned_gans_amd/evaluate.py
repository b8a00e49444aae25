"""Checkpoint evaluation: ``python -m action_conditioned_gans_amd.evaluate MODEL_PATH INPUT OUTPUT [options]``.

The reference's test.py (restore the latest checkpoint, recursive rollout on ``.npy`` frames and actions, GIF samples through
util.save_samples), made to run (defect D5), plus the numbers its report publishes: SSIM and PSNR per rollout step for the
model and for the identity baseline (Fig. 4), scored on the GPU (metrics.frame_metrics).

INPUT: a ``.npy`` of frames [N, T, H, W, 3] (float in [-1, 1], or uint8 read as x / 127.5 - 1) with ``--actions`` [N, T, 10];
a push TFRecord directory (its validation split, read once in sorted file order); or ``synthetic`` (seeded random sequences).
``--num_sequences`` caps any of them.  The rollout runs ``--batch_size`` sequences at a time; the last batch is padded by
repeating its last sequence and the padded rows enter no sum.

OUTPUT/metrics.json: the checkpoint, sequences, steps, the SSIM definition, per step the mean SSIM over sequences and the PSNR
of the whole set by the reference's formula (10 log10(1 / MSE), MSE over all sequences' frames of that step - for a single
batch the train loop's ``rollout_psnr``), the same two curves for the identity baseline, and the rollout rate in frames/s.

``--weights ema``: predict with the moving average of the generator weights that a run trained with ``--g_ema`` keeps in its
checkpoints (``state:g/ema/shadow``): after the restore the average is COPIED into the variables (with ``--bn_stats calibrate``
before calibrating, so that OUTPUT/calibrated.npz restores to the same weights again); metrics.json then also holds ``weights``
and ``ema_updates``.  ``raw`` (default): the weights as trained.

``--noise_dim Z``: the checkpoint is of a run trained with ``--noise_dim Z`` (it must match: the generator's bottleneck layers
are Z channels wider).  ``--noise zero`` (default) predicts with z = 0; ``--noise sample`` rolls every sequence out
``--noise_samples`` N times, every step of every rollout with a fresh z from the stream (``--noise_seed``, 0): ``ssim`` and
``psnr`` are then the mean over the N samples (of N curves, each computed as above), and ``best_ssim`` / ``best_psnr`` the
best-of-N protocol of stochastic video prediction - for each sequence and each metric separately the sample whose mean over
the steps is best, then the same reductions over sequences.  metrics.json also holds ``noise_dim``, ``noise`` and
``noise_samples``.  Not with ``--bn_stats stored`` / ``calibrate``.

``--posterior`` (with ``--noise_dim Z``, float32): the checkpoint is of a run trained with ``--posterior``; the encoder
``g/posterior`` is built and restored, and ``--noise posterior`` / ``posterior_mean`` draw z from q(z | x_t, x_{t+1}) - every step
of the rollout encodes its current input frame (the prediction, from the second step on) and the TRUE next frame, so these two
modes score a reconstruction that has seen the target, the VAE's upper bound, not a prediction.  ``--noise_samples`` applies to
``posterior`` as to ``sample``; metrics.json then also holds ``posterior: true``.  Without the flag such a checkpoint predicts
from the prior like any ``--noise_dim`` run: its extra ``g/posterior/*`` keys are ignored, and so are the G optimizers' flat slots,
which are laid out with the encoder and which predicting does not read (``--weights ema`` reads such a buffer: it needs ``--posterior``).
"""
import argparse
import json
import os
import time

import numpy as np

ACTION_DIM = 10
EMA_BUILD_DECAY = 0.999      # evaluation only reads the average: the decay its graph is built with is never applied


def load_frames(path):
    """A frames ``.npy`` [N, T, H, W, 3] -> float32 in [-1, 1] (uint8 is read as x / 127.5 - 1)."""
    arr = np.load(path, mmap_mode='r')
    if arr.ndim != 5 or arr.shape[-1] != 3:
        raise ValueError('%s: expected frames [N, T, H, W, 3], got %s' % (path, arr.shape))
    return arr


def _as_float(frames):
    frames = np.asarray(frames)
    if frames.dtype == np.uint8:
        return frames.astype(np.float32) / 127.5 - 1.0
    return np.array(frames, dtype=np.float32)          # (a writable copy: the .npy is memory-mapped read-only)


def _batches(input_path, actions_path, batch_size, img_size, seq_len, num_sequences):
    """-> generator of (frames [b, T, S, S, 3] float32, actions [b, T, 10] float32), b <= batch_size, at most num_sequences rows."""
    left = num_sequences if num_sequences is not None else float('inf')
    if input_path == 'synthetic':
        from .train import SyntheticPush
        data = SyntheticPush(batch_size, seq_len, img_size, seed=1007)
        if num_sequences is None:
            raise ValueError('the synthetic source needs --num_sequences')
        while left > 0:
            img, _, acts, _ = data.get_batch()
            b = int(min(left, batch_size))
            yield img[:b], acts[:b]
            left -= b
    elif os.path.isdir(input_path):
        from .push_data import PushDataset
        with PushDataset(input_path, batch_size, training=False, img_size=img_size, one_pass=True) as data:
            for img, _, acts, _ in data:
                if left <= 0:
                    break
                b = int(min(left, img.shape[0]))
                yield np.asarray(img[:b], np.float32), np.asarray(acts[:b], np.float32)
                left -= b
    else:
        frames, actions = load_frames(input_path), np.load(actions_path, mmap_mode='r')
        n = int(min(left, frames.shape[0]))
        for s in range(0, n, batch_size):
            e = min(s + batch_size, n)
            yield _as_float(frames[s:e]), np.array(actions[s:e], dtype=np.float32)


def _pad(x, batch_size):
    if x.shape[0] == batch_size:
        return x
    return np.concatenate([x, np.repeat(x[-1:], batch_size - x.shape[0], axis=0)], axis=0)


def _calibration_pairs(input_path, actions_path, pair_batch, img_size, seq_len, num_batches):
    """-> generator of at most ``num_batches`` full batches (frames [pair_batch, S, S, 3], actions [pair_batch, 10]) of one-step
    pairs (frame t, action t), t = 0 .. T-2 of every sequence, in the order of the source."""
    frames_q, acts_q, have, done = [], [], 0, 0
    # (the synthetic source has no end: it is asked for exactly the sequences the batches need)
    n_seq = -(-num_batches * pair_batch // max(seq_len - 1, 1)) if input_path == 'synthetic' else None
    for frames, acts in _batches(input_path, actions_path, pair_batch, img_size, seq_len, n_seq):
        if frames.shape[2:4] != (img_size, img_size):
            raise ValueError('frames of %s x %s, the model is built for --img_size %d' % (frames.shape[2], frames.shape[3], img_size))
        t = frames.shape[1] - 1
        frames_q.append(frames[:, :t].reshape((-1,) + frames.shape[2:]))
        acts_q.append(acts[:, :t].reshape(-1, acts.shape[2]))
        have += frames_q[-1].shape[0]
        while have >= pair_batch and done < num_batches:
            f, a = np.concatenate(frames_q), np.concatenate(acts_q)
            yield np.ascontiguousarray(f[:pair_batch]), np.ascontiguousarray(a[:pair_batch])
            frames_q, acts_q, have, done = [f[pair_batch:]], [a[pair_batch:]], have - pair_batch, done + 1
        if done >= num_batches:
            return


def _use_ema_weights(trainer, ckpt):
    """--weights ema, after the restore: the averaged weights into the variables; -> the average's update count."""
    updates = trainer.ema_updates()
    if updates < 1:
        raise ValueError('--weights ema: checkpoint %s holds no generator weight average (no state:g/ema/shadow, or 0 updates): '
                         'train with --g_ema' % os.path.abspath(ckpt))
    trainer.load_ema_weights()
    return updates


def _slots_to_skip(path, posterior, weights):
    """A checkpoint of a run trained with --posterior, read into a graph without the encoder (prior predictions from a plain
    --noise_dim graph): its ``g/posterior/*`` variables are extra keys the Saver ignores, but the flat buffers laid out over scope
    ``g`` - the G optimizers' slots - hold the encoder too and fit no buffer of this graph.  A session that predicts reads none of
    them: -> the Saver.restore ``skip_state`` that leaves them out (None for every other checkpoint).  The weight average is such
    a buffer as well and IS read by ``--weights ema``: that needs --posterior."""
    with np.load(path if path.endswith('.npz') else path + '.npz') as data:
        extra = any(k.startswith('var:g/posterior/') for k in data.files)
    if posterior or not extra:
        return None
    if weights == 'ema':
        raise ValueError('--weights ema: checkpoint %s is of a run trained with --posterior, whose weight average is laid out with the '
                         'encoder: add --posterior' % os.path.abspath(path))
    return lambda name: name.startswith(('g_opt/', 'g_pretrain_opt/', 'g/ema/'))


def predicting_trainer(ckpt, transform, batch_size, ksize, img_size, dtype, device, num_masks, bn_stats='batch', weights='raw',
                       noise_dim=None, noise_seed=0, restore_from=None, calibrate_with='--bn_stats calibrate', pixel_maps=0, canvas=False,
                       posterior=False):
    """A checkpoint as a Trainer that predicts: a fresh graph and session, the generator ``transform`` / ``ksize`` / ``num_masks`` at
    ``batch_size`` with what the modes need and nothing else - ``bn_stats`` 'stored' or 'calibrate': the stored-statistics instances;
    ``weights='ema'``: the average (then copied into the variables, _use_ema_weights); ``noise_dim`` > 0: the noise input, its stream
    restarted at ``noise_seed`` - initialised and restored from ``restore_from`` (default: ``ckpt``, which the messages name).  An int
    ``noise_dim`` also makes the Saver's shape refusal ask about --noise_dim.  'stored' needs calibrated rows in the checkpoint (the
    error names ``calibrate_with``).  ``pixel_maps`` > 0: the map path of plan.Planner's designated-pixel cost (DNA generator).
    ``canvas``: the CDNA / affine generator with its painted candidate (Trainer ``canvas``).  ``posterior``: the encoder of the
    latent posterior (Trainer ``posterior``; the KL weight plays no part in predicting).
    -> (trainer, updates of the average or None, calibrated rows or None); the caller closes
    ``trainer.sess``."""
    from . import graph as G
    from .saver import Saver
    from .train import Trainer
    extra = {'bn_inference': True} if bn_stats != 'batch' else {}      # ('batch' builds exactly the graph it always built)
    if weights == 'ema':
        extra['ema_decay'] = EMA_BUILD_DECAY
    if noise_dim:
        extra.update(noise_dim=noise_dim, noise_seed=noise_seed)
    if pixel_maps:
        extra['pixel_maps'] = pixel_maps
    if canvas:
        extra['canvas'] = True
    if posterior:
        extra['posterior'] = True
    G.reset_default_graph()
    sess = G.Session(device=device, dtype=dtype)
    try:
        trainer = Trainer(sess, False, 'bce', 'adam', transform, batch_size=batch_size, img_size=img_size, ksize=ksize, lookahead=False,
                          num_masks=num_masks, **extra)
        sess.run(G.global_variables_initializer())
        try:
            Saver().restore(sess, restore_from or ckpt, skip_state=_slots_to_skip(restore_from or ckpt, posterior, weights))
        except ValueError as e:
            if noise_dim is not None and 'has shape' in str(e):        # the Saver's shape refusal: the bottleneck layers are noise_dim channels wider
                raise ValueError('%s - the generator is built with --noise_dim %d: does that match the run that wrote the checkpoint?'
                                 % (e, noise_dim)) from None
            raise
        if noise_dim:
            trainer.set_noise_state(noise_seed)        # the stream of this evaluation, not the training run's
        ema_updates = _use_ema_weights(trainer, ckpt) if weights == 'ema' else None      # (copied into the variables: 'raw' from here on)
        calibration_rows = trainer.bn_calibration_rows() if bn_stats == 'stored' else None
        if bn_stats == 'stored' and calibration_rows < 1:
            raise ValueError('--bn_stats stored: checkpoint %s holds no calibrated BatchNorm statistics (run %s first)'
                             % (os.path.abspath(ckpt), calibrate_with))
        return trainer, ema_updates, calibration_rows
    except BaseException:
        sess.close()
        raise


def calibrate(ckpt, save_prefix, input_path, actions_path, transform, ksize, img_size, dtype, pair_batch, num_batches, seq_len, device,
              num_masks, weights='raw', canvas=False):
    """Restore ``ckpt`` into a generator built at batch ``pair_batch``, pool its BatchNorm statistics over ``num_batches`` batches
    of one-step pairs of ``input_path`` (Trainer.calibrate_bn) and save everything as ``save_prefix``.npz.  -> pairs pooled.
    ``weights='ema'``: calibrate (and save) the averaged weights (_use_ema_weights)."""
    from .saver import Saver
    trainer, _, _ = predicting_trainer(ckpt, transform, pair_batch, ksize, img_size, dtype, device, num_masks, 'calibrate', weights,
                                       canvas=canvas)
    sess = trainer.sess
    try:
        trainer.reset_bn_statistics()
        rows = 0
        for frames, acts in _calibration_pairs(input_path, actions_path, pair_batch, img_size, seq_len, num_batches):
            rows = trainer.calibrate_bn(frames, acts)
        if rows == 0:
            raise ValueError('%s holds fewer than one batch of %d one-step pairs to calibrate on' % (input_path, pair_batch))
        Saver().save(sess, save_prefix)
        return rows
    finally:
        sess.close()


def set_psnr(sqerr, valid, count_per_frame):
    """PSNR of a set by the reference's formula: ``sqerr`` [N, steps] sums of squared errors per frame, ``valid`` [N] bool (False:
    a padding row) -> [steps] 10 log10(1 / (sum over valid rows / (rows * count_per_frame)))."""
    from .metrics import psnr_from_sqerr
    sqerr = np.asarray(sqerr, np.float64)[np.asarray(valid, bool)]
    return psnr_from_sqerr(sqerr.sum(axis=0), sqerr.shape[0] * count_per_frame)


def evaluate(model_path, input_path, output_path, actions_path=None, dna=False, ksize=5, img_size=64, dtype='f32', batch_size=32,
             seq_len=8, num_sequences=None, samples=16, gif=False, dump=False, device='cuda:0', cdna=False, num_masks=10, bn_stats='batch',
             calibrate_batch_size=32, calibrate_batches=16, calibrate_input=None, calibrate_actions=None, weights='raw', noise_dim=0,
             noise='zero', noise_samples=1, noise_seed=0, affine=False, canvas=False, posterior=False):
    """Restore ``model_path`` (a checkpoint directory - its latest checkpoint - or a checkpoint prefix) into the generator
    ``dna`` / ``cdna`` / ``affine`` (with ``num_masks``) / ``ksize`` / ``img_size`` / ``dtype`` describe, roll it out over the sequences of
    ``input_path`` and write ``output_path``/metrics.json (module docstring), ``samples`` sample videos (util.save_samples, GIFs
    with ``gif``) and with ``dump`` the predictions as ``predictions.npy`` [N, steps, H, W, 3].  ``bn_stats`` 'batch', 'stored' or 'calibrate' and the
    ``calibrate_*`` arguments: the module docstring (``calibrate_actions``: the actions of a ``calibrate_input`` .npy).
    ``weights``: 'raw' or 'ema' (module docstring); 'ema' on a checkpoint without an average is a ValueError.
    ``noise_dim`` / ``noise`` ('zero', 'sample', and with ``posterior`` 'posterior' or 'posterior_mean') / ``noise_samples`` /
    ``noise_seed`` / ``posterior``: the module docstring.
    ``canvas``: the checkpoint is of a ``cdna`` / ``affine`` generator trained with its painted candidate (Trainer ``canvas``);
    metrics.json then holds ``canvas: true``.
    -> the metrics dict."""
    from . import models as M
    transform = M.transform_argument(dict(dna=dna, cdna=cdna, affine=affine))
    if bn_stats not in ('batch', 'stored', 'calibrate'):
        raise ValueError("bn_stats must be 'batch', 'stored' or 'calibrate', got %r" % (bn_stats,))
    if weights not in ('raw', 'ema'):
        raise ValueError("weights must be 'raw' or 'ema', got %r" % (weights,))
    if bn_stats == 'calibrate' and (calibrate_batch_size < 1 or calibrate_batches < 1):
        raise ValueError('calibrate_batch_size and calibrate_batches must be >= 1')
    from .train import NOISE_MODES, check_canvas, check_noise, check_posterior
    canvas = check_canvas(canvas, M.model_kind(transform), ksize, num_masks)
    noise_dim = check_noise(noise_dim, noise_seed, 1, bn_stats != 'batch', batch_size)
    posterior, _ = check_posterior(posterior, 1.0, noise_dim, bf16=dtype != 'f32')
    if noise not in NOISE_MODES:
        raise ValueError("noise must be 'zero', 'sample', 'posterior' or 'posterior_mean', got %r" % (noise,))
    if noise == 'sample' and not noise_dim:
        raise ValueError("noise 'sample' needs noise_dim > 0")
    if NOISE_MODES[noise][1] and not posterior:
        raise ValueError('noise %r needs posterior (the encoder it draws from)' % (noise,))
    drawn = noise in ('sample', 'posterior')         # the modes that draw: several rollouts per sequence differ
    if int(noise_samples) < 1 or (not drawn and int(noise_samples) != 1):
        raise ValueError("noise_samples must be >= 1, and 1 unless noise is 'sample' or 'posterior' (got %r)" % (noise_samples,))
    n_draws = int(noise_samples)
    from .metrics import SSIM_DEFINITION
    from .saver import latest_checkpoint
    from .util import save_samples

    ckpt = latest_checkpoint(model_path) if os.path.isdir(model_path) else model_path
    if ckpt is None:
        raise FileNotFoundError('no checkpoint under %s' % model_path)
    os.makedirs(output_path, exist_ok=True)
    restore_from = ckpt
    if bn_stats == 'calibrate':
        if calibrate_input is None:
            calibrate_input, calibrate_actions = input_path, actions_path
        restore_from = os.path.join(output_path, 'calibrated')
        calibrate(ckpt, restore_from, calibrate_input, calibrate_actions, transform, ksize, img_size, dtype, calibrate_batch_size,
                  calibrate_batches, seq_len, device, num_masks, **({'weights': weights} if weights == 'ema' else {}),
                  **({'canvas': True} if canvas else {}))
    stored = bn_stats != 'batch'
    bn = 'stored' if stored else 'batch'
    trainer, ema_updates, calibration_rows = predicting_trainer(ckpt, transform, batch_size, ksize, img_size, dtype, device, num_masks, bn,
                                                                weights, noise_dim, noise_seed, restore_from=restore_from,
                                                                **({'canvas': True} if canvas else {}),
                                                                **({'posterior': True} if posterior else {}))
    sess = trainer.sess
    try:
        keys =('ssim', 'sqerr', 'identity_ssim', 'identity_sqerr')
        acc = {k: [] for k in keys}
        draws = {'ssim': [], 'sqerr': []}        # noise 'sample': [n_draws, batch, steps] per batch
        valid, kept_frames, kept_pred, dumped = [], [], [], []
        rollout_s, n_seq, steps, hw = 0.0, 0, None, None
        for frames, acts in _batches(input_path, actions_path, batch_size, img_size, seq_len, num_sequences):
            b = frames.shape[0]
            if frames.shape[2:4] != (img_size, img_size):
                raise ValueError('frames of %s x %s, the model is built for --img_size %d' % (frames.shape[2], frames.shape[3], img_size))
            steps, hw = frames.shape[1] - 1, frames.shape[2:]
            want = dump or len(kept_pred) < samples
            t0 = time.perf_counter()
            m = trainer.rollout_metrics(_pad(frames, batch_size), _pad(acts, batch_size), return_frames=want, **({'bn': bn} if stored else {}),
                                        **({'noise': noise} if noise_dim else {}))
            if drawn:        # the first draw is the one that is kept as a sample video; the others are scored only
                more = [trainer.rollout_metrics(_pad(frames, batch_size), _pad(acts, batch_size), identity=False, noise=noise)
                        for _ in range(n_draws - 1)]
                for k in draws:
                    draws[k].append(np.stack([m[k]] + [d[k] for d in more]))
            rollout_s += time.perf_counter() - t0
            for k in keys:
                acc[k].append(m[k])
            valid.append(np.arange(batch_size) < b)
            if want:
                pred = m['frames'][:b]
                if dump:
                    dumped.append(pred)
                take = min(samples - len(kept_pred), b)
                kept_pred.extend(pred[:take])
                kept_frames.extend(frames[:take])
            n_seq += b
        if n_seq == 0:
            raise ValueError('%s holds no sequences' % input_path)
        valid = np.concatenate(valid)
        acc = {k: np.concatenate(v) for k, v in acc.items()}
        count = int(np.prod(hw))        # H * W * 3 values per frame
        result = {
            'checkpoint': os.path.abspath(ckpt),
            'model': trainer.model,
            **M.KINDS[trainer.model].result_fields(ksize, num_masks, trainer.canvas),
            'sequences': n_seq,
            'steps': int(steps),
            'ssim_definition': SSIM_DEFINITION + ' (data_range 2 for frames in [-1, 1])',
            'psnr_definition': '10 log10(1 / MSE) on [-1, 1] frames (reference build_psnr): 6.02 dB below a [0, 1]-range PSNR; '
                               'MSE over all sequences of the step',
            'ssim': [float(v) for v in acc['ssim'][valid].mean(axis=0, dtype=np.float64)],
            'psnr': [float(v) for v in set_psnr(acc['sqerr'], valid, count)],
            'identity_ssim': [float(v) for v in acc['identity_ssim'][valid].mean(axis=0, dtype=np.float64)],
            'identity_psnr': [float(v) for v in set_psnr(acc['identity_sqerr'], valid, count)],
            'frames_per_s': float(valid.size * steps * n_draws / rollout_s),
        }
        if noise_dim:
            result.update(noise_dim=noise_dim, noise=noise, noise_samples=n_draws, **({'posterior': True} if posterior else {}))
        if drawn:
            result.update(best_of_n(np.concatenate(draws['ssim'], axis=1)[:, valid], np.concatenate(draws['sqerr'], axis=1)[:, valid], count))
        if stored:
            result['bn_statistics'] = bn_stats
            result['calibration_rows'] = int(calibration_rows)
        if weights == 'ema':
            result['weights'] = weights
            result['ema_updates'] = int(ema_updates)
        with open(os.path.join(output_path, 'metrics.json'), 'w') as f:
            json.dump(result, f, indent=1)
        if dump:
            np.save(os.path.join(output_path, 'predictions.npy'), np.concatenate(dumped))
        if kept_pred:
            seqs = np.stack(kept_frames)
            save_samples(output_path, seqs, np.stack(kept_pred), seqs[:, 1:], 0, gif=gif)
        return result
    finally:
        sess.close()


def best_of_n(ssim, sqerr, count_per_frame):
    """``ssim`` / ``sqerr`` [N draws, sequences, steps] -> the curves of a sampled evaluation.  ``ssim`` / ``psnr``: the mean over
    the N draws of the curve of each draw (mean SSIM over sequences; set_psnr).  ``best_ssim`` / ``best_psnr``: for each sequence
    the draw whose mean over the steps is best - SSIM, and the PSNR of the sequence's own frames, chosen separately - then the
    same reductions over sequences."""
    from .metrics import psnr_from_sqerr
    ssim, sqerr = np.asarray(ssim, np.float64), np.asarray(sqerr, np.float64)
    every = np.ones(ssim.shape[1], bool)
    seq = np.arange(ssim.shape[1])
    frame_psnr = 10.0 * np.log10(count_per_frame / np.maximum(sqerr, 1e-30))
    pick_s, pick_p = ssim.mean(axis=2).argmax(axis=0), frame_psnr.mean(axis=2).argmax(axis=0)
    return {'ssim': [float(v) for v in ssim.mean(axis=(0, 1))],
            'psnr': [float(v) for v in np.mean([psnr_from_sqerr(d.sum(axis=0), d.shape[0] * count_per_frame) for d in sqerr], axis=0)],
            'best_ssim': [float(v) for v in ssim[pick_s, seq].mean(axis=0)],
            'best_psnr': [float(v) for v in set_psnr(sqerr[pick_p, seq], every, count_per_frame)]}


def check_bn_args(parser, args):
    """parser.error for --bn_stats / --calibrate_* flags that do not go together (before anything is created); fills the defaults."""
    given = [n for n in ('calibrate_batch_size', 'calibrate_batches', 'calibrate_input', 'calibrate_actions') if getattr(args, n) is not None]
    if given and args.bn_stats != 'calibrate':
        parser.error('--%s goes with --bn_stats calibrate (got --bn_stats %s)' % (given[0], args.bn_stats))
    if args.calibrate_batch_size is None:
        args.calibrate_batch_size = 32
    if args.calibrate_batches is None:
        args.calibrate_batches = 16
    if args.calibrate_batch_size < 1 or args.calibrate_batches < 1:
        parser.error('--calibrate_batch_size and --calibrate_batches must be >= 1')
    if args.calibrate_actions is not None and args.calibrate_input is None:
        parser.error('--calibrate_actions goes with --calibrate_input')
    ci = args.calibrate_input
    if ci is not None and ci != 'synthetic' and not os.path.isdir(ci):
        if args.calibrate_actions is None:
            parser.error('a --calibrate_input frames .npy needs --calibrate_actions ACTIONS.npy')
        if not os.path.exists(ci) or not os.path.exists(args.calibrate_actions):
            parser.error('--calibrate_input / --calibrate_actions: no such file')


def main(argv=None):
    parser = argparse.ArgumentParser(description='evaluate a checkpoint: rollout SSIM / PSNR per step, model and identity baseline')
    parser.add_argument('model_path', type=str, help='checkpoint directory (its latest checkpoint) or checkpoint prefix')
    parser.add_argument('input', type=str, help="frames .npy [N,T,H,W,3], push TFRecord directory, or 'synthetic'")
    parser.add_argument('output', type=str)
    parser.add_argument('--actions', type=str, default=None, help='actions .npy [N,T,10] (with a frames .npy)')
    from . import models as M
    from .train import add_model_args, check_model_args
    add_model_args(parser)
    parser.add_argument('--ksize', type=int, default=5)
    parser.add_argument('--img_size', type=int, default=64)
    parser.add_argument('--dtype', type=str, default='f32', choices=['f32', 'bf16'])
    parser.add_argument('--batch_size', type=int, default=32)
    parser.add_argument('--seq_len', type=int, default=8, help='sequence length of the synthetic source')
    parser.add_argument('--num_sequences', type=int, default=None)
    parser.add_argument('--samples', type=int, default=16, help='sample videos written (train.py:300-305 writes 16)')
    parser.add_argument('--gif', action='store_true')
    parser.add_argument('--dump', action='store_true', help='save the predictions as predictions.npy')
    parser.add_argument('--device', type=str, default='cuda:0')
    parser.add_argument('--bn_stats', type=str, default='batch', choices=['batch', 'stored', 'calibrate'],
                        help="BatchNorm statistics of the generator: of each batch (as in training), stored in the checkpoint, or "
                             "calibrated first (writes OUTPUT/calibrated.npz) and then stored")
    parser.add_argument('--calibrate_batch_size', type=int, default=None, help='pairs per calibration batch (default 32)')
    parser.add_argument('--calibrate_batches', type=int, default=None, help='calibration batches (default 16)')
    parser.add_argument('--calibrate_input', type=str, default=None, help='source of the calibration pairs (default: INPUT)')
    parser.add_argument('--calibrate_actions', type=str, default=None, help='actions .npy of a --calibrate_input frames .npy')
    parser.add_argument('--weights', type=str, default='raw', choices=['raw', 'ema'],
                        help="the generator weights as trained, or their moving average (a checkpoint of a run trained with --g_ema)")
    from .train import add_noise_args, add_posterior_args, check_noise_args, check_posterior_args
    add_noise_args(parser)
    add_posterior_args(parser, training=False)
    parser.add_argument('--noise', type=str, default='zero', choices=['zero', 'sample', 'posterior', 'posterior_mean'],
                        help="predict with z = 0, or roll every sequence out --noise_samples times with fresh noise (needs --noise_dim); "
                             "with --posterior also: z drawn from the encoder's q(z | x_t, x_t+1), or its mean")
    parser.add_argument('--noise_samples', type=int, default=None, metavar='N',
                        help="rollouts per sequence with --noise sample or posterior (default 1)")
    args = parser.parse_args(argv)
    check_model_args(parser, args)
    check_bn_args(parser, args)
    check_noise_args(parser, args)
    check_posterior_args(parser, args)
    if args.noise.startswith('posterior') and not args.posterior:
        parser.error('--noise %s needs --posterior' % args.noise)
    if args.noise_dim > 0 and args.bn_stats != 'batch':
        parser.error('--noise_dim > 0 predicts with batch statistics (--bn_stats %s)' % args.bn_stats)
    if args.noise == 'sample' and args.noise_dim < 1:
        parser.error('--noise sample needs --noise_dim > 0')
    if args.noise_samples is not None and (args.noise not in ('sample', 'posterior') or args.noise_samples < 1):
        parser.error('--noise_samples N >= 1 goes with --noise sample' + (' or posterior' if args.posterior else ''))
    if args.noise_samples is None:
        args.noise_samples = 1
    if args.batch_size < 1:
        parser.error('--batch_size must be >= 1')
    if args.num_sequences is not None and args.num_sequences < 1:
        parser.error('--num_sequences must be >= 1')
    if args.input == 'synthetic':
        if args.num_sequences is None:
            parser.error('the synthetic source needs --num_sequences')
    elif not os.path.isdir(args.input):
        if args.actions is None:
            parser.error('a frames .npy needs --actions ACTIONS.npy')
        try:
            frames, actions = load_frames(args.input), np.load(args.actions, mmap_mode='r')
        except (OSError, ValueError) as e:
            parser.error(str(e))
        if actions.ndim != 3 or actions.shape[2] != ACTION_DIM:
            parser.error('%s: expected actions [N, T, %d], got %s' % (args.actions, ACTION_DIM, actions.shape))
        if actions.shape[:2] != frames.shape[:2]:
            parser.error('frames %s and actions %s disagree in N or T' % (frames.shape[:2], actions.shape[:2]))
    return evaluate(args.model_path, args.input, args.output, actions_path=args.actions, ksize=args.ksize,
                    img_size=args.img_size, dtype=args.dtype, batch_size=args.batch_size, seq_len=args.seq_len,
                    num_sequences=args.num_sequences, samples=args.samples, gif=args.gif, dump=args.dump, device=args.device,
                    num_masks=args.num_masks, bn_stats=args.bn_stats, calibrate_batch_size=args.calibrate_batch_size,
                    calibrate_batches=args.calibrate_batches, calibrate_input=args.calibrate_input, calibrate_actions=args.calibrate_actions,
                    **({'weights': args.weights} if args.weights != 'raw' else {}), **{flag: getattr(args, flag) for flag in M.flags()},
                    **({'canvas': True} if args.canvas else {}),
                    **({'noise_dim': args.noise_dim, 'noise': args.noise, 'noise_samples': args.noise_samples, 'noise_seed': args.noise_seed}
                       if args.noise_dim else {}), **({'posterior': True} if args.posterior else {}))


if __name__ == '__main__':
    main()
