"""Host-side helpers of the training loop (util.py:10-58 of the reference)."""
import os

import numpy as np


def build_all_mask(num_frame):
    """One-hot boolean rows selecting frame t for t in [0, num_frame-2]; ``np.roll(mask, 1, axis=1)``
    then selects frame t+1 (train.py:231-232)."""
    masks = np.zeros((num_frame - 1, num_frame), dtype=bool)
    for t in range(num_frame - 1):
        masks[t, t] = True
    return masks


def to_uint8(frames):
    """[-1, 1] -> uint8 as the reference, ``(x + 1) * 127.5`` truncated - but clipped to [0, 255] first: the reference's
    ``astype(np.uint8)`` wraps a value past the range around (1.01 -> 1, -0.01 -> 254)."""
    return np.clip((255. / 2) * (np.asarray(frames, dtype=np.float32) + 1.), 0., 255.).astype(np.uint8)


def _save_gif(path, vid):
    from PIL import Image
    frames = [Image.fromarray(f) for f in vid]
    frames[0].save(path, save_all=True, append_images=frames[1:], duration=250, loop=0)


def _save_png(path, frame):
    from PIL import Image
    Image.fromarray(frame).save(path)


def save_samples(output_path, input_sample, generated_sample, ground_truth, sample_number, gif=False):
    """util.save_samples of the reference (util.py:18-58), same signature and layout: ``output_path/sample{n}/vid{i}/``
    per video i of ``input_sample`` [V, T, H, W, 3];
      * ``gif=True``: ``ground_truth.gif`` from ``input_sample`` (as the reference does) and ``generated.gif`` from
        ``generated_sample``, 250 ms per frame; ``ground_truth`` is not read;
      * otherwise ``frame{j}.png`` (``input_sample``), ``generated{j}.png`` and ``ground_truth{j}.png``.
    Pixels are ``(x + 1) * 127.5`` as uint8 (``to_uint8``: clipped where the reference wraps).  Written with PIL (the
    reference's imageio / matplotlib are not used; its ``plt.imsave`` PNGs are RGBA, these are RGB)."""
    input_sample = to_uint8(input_sample)
    generated_sample = to_uint8(generated_sample)
    if not gif:
        ground_truth = to_uint8(ground_truth)
    save_folder = os.path.join(output_path, 'sample{:d}'.format(sample_number))
    os.makedirs(save_folder, exist_ok=True)
    for i in range(input_sample.shape[0]):
        vid_folder = os.path.join(save_folder, 'vid{:d}'.format(i))
        os.makedirs(vid_folder, exist_ok=True)
        if gif:
            _save_gif(os.path.join(vid_folder, 'ground_truth.gif'), input_sample[i])
            _save_gif(os.path.join(vid_folder, 'generated.gif'), generated_sample[i])
            continue
        for j in range(input_sample.shape[1]):
            _save_png(os.path.join(vid_folder, 'frame{:d}.png'.format(j)), input_sample[i, j])
        for j in range(generated_sample.shape[1]):
            _save_png(os.path.join(vid_folder, 'generated{:d}.png'.format(j)), generated_sample[i, j])
        for j in range(ground_truth.shape[1]):
            _save_png(os.path.join(vid_folder, 'ground_truth{:d}.png'.format(j)), ground_truth[i, j])
