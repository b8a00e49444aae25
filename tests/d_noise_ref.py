"""float64 restatement of the instance noise on the discriminator's inputs (include/acgan_rollout.h: acg_inst_noise_prepare /
acg_inst_noise_add) and of acg_logit_stats in numpy - the schedule, the key protocol and z(p, l), on tests/noise_ref.py's Philox -
and an OracleTrainer whose discriminator judges frame + a given noise.  Test infrastructure."""
import numpy as np
import torch

import noise_ref as NR
from oracle import models as OM        # noqa: F401  (the oracle step below runs oracle.models through OracleTrainer)
from oracle.trainer import OracleTrainer

STREAM_TAG = 0x444E4F49          # ACG_DN_STREAM_TAG
SLOTS = 64                       # stream id = rank * 64 + the D instance's slot
SLOT = {'gen': 0, 'real': 1, 'both': 2}


def sigma(k, start, final, offset, decay_steps):
    """sigma at schedule position k: float64 with every operation rounded on its own, from the float32 levels the kernel is
    handed; -> the float32 the kernel stores."""
    s, f = np.float64(np.float32(start)), np.float64(np.float32(final))
    if decay_steps == 0:
        return np.float32(s)
    j = np.float64(max(int(k) - int(offset), 0))
    t = min(j / np.float64(decay_steps), np.float64(1.0))
    return np.float32(s + (f - s) * t)


def prepare(state, updates, start, final, offset, decay_steps, advance_schedule):
    """acg_inst_noise_prepare on host values: state (seed, counter), updates k -> (key, sigma float32, new state, new updates)."""
    seed, counter = int(state[0]) % 2 ** 64, int(state[1]) % 2 ** 64
    k = int(updates) % 2 ** 64
    return ((seed, counter), sigma(k, start, final, offset, decay_steps), (seed, (counter + 1) % 2 ** 64),
            (k + 1) % 2 ** 64 if advance_schedule else k)


def z(key, stream_id, pixels, cn=4):
    """z(p, l) for p < pixels, l < cn, float64 [pixels, cn]: lane l of Philox block p of the draw (key[0], key[1], stream_id ^ tag)."""
    return NR.normals(key[0], key[1], (int(stream_id) ^ STREAM_TAG) & NR.MASK, 4 * pixels).reshape(pixels, 4)[:, :cn]


def add(x, key, sig, c0, cn, stream_id):
    """acg_inst_noise_add in float64: x [pixels, pitch] (the stored values) -> x with sigma * z on the channels [c0, c0 + cn)."""
    out = np.array(x, dtype=np.float64)
    if float(sig) != 0.0:
        out[:, c0:c0 + cn] += np.float64(np.float32(sig)) * z(key, stream_id, out.shape[0], cn)
    return out


def round_bf16(v):
    """float64 -> the nearest bfloat16 value (8 significant bits, ties to even), as float64; for normal values."""
    m, e = np.frexp(np.asarray(v, np.float64))
    return np.ldexp(np.rint(m * 256.0), e - 8)


def logit_stats(fake, real):
    """acg_logit_stats in float64 -> [mean fake, mean real, share of fake < 0, share of real > 0]."""
    fake, real = np.asarray(fake, np.float64).reshape(-1), np.asarray(real, np.float64).reshape(-1)
    return np.array([fake.mean(), real.mean(), (fake < 0).mean(), (real > 0).mean()])


class DNoiseOracleTrainer(OracleTrainer):
    """OracleTrainer whose discriminator judges frame + noise: ``d_add`` holds one [B, H, W, 3] array (sigma * z, float64) per
    discriminator call of the step that follows, in call order - train_d: D(fake), then D(real); train_g: D(fake) - set before
    every step.  The noise is a constant: the gradient of the frame is the gradient of D's noisy input."""
    d_add = ()

    def _d(self, p, img, frame, actions):
        add_now, self.d_add = self.d_add[0], self.d_add[1:]
        return super()._d(p, img, frame + torch.as_tensor(np.asarray(add_now), dtype=frame.dtype), actions)
