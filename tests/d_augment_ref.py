"""float64 restatement of the differentiable augmentation of the discriminator's inputs (include/acgan_rollout.h:
acg_d_augment_draw / _fwd / _bwd): the draw in numpy on tests/noise_ref.py's Philox, the transform in torch so that autograd gives
its gradient, the adjoint as the header states it, and an OracleTrainer whose discriminator judges transformed pairs.  Test
infrastructure."""
import numpy as np
import torch

import noise_ref as NR
from oracle import models as OM        # noqa: F401  (the oracle step below runs oracle.models through OracleTrainer)
from oracle.trainer import OracleTrainer

STREAM_TAG = 0x44415547          # ACG_DA_STREAM_TAG
SLOTS = 64                       # stream id = rank * 64 + the D instance's slot
SLOT = {'gen': 0, 'real': 1, 'both': 2}
COLOR, TRANSLATION, CUTOUT = 1, 2, 4
IDENTITY = (0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def draw(seed, counter, stream_id, rows, h, w, policy):
    """acg_d_augment_draw -> params float64 [rows, 8] (every value is a float32 value), integer arithmetic throughout."""
    seed, counter = int(seed) % 2 ** 64, int(counter) % 2 ** 64
    ctr = np.empty((2 * rows, 4), np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2] = counter & NR.MASK, counter >> 32, np.arange(2 * rows, dtype=np.uint32)
    ctr[:, 3] = (int(stream_id) ^ STREAM_TAG) & NR.MASK
    x = NR.philox4x32_10(ctr, np.array([seed & NR.MASK, seed >> 32], np.uint32)).reshape(rows, 8)
    ry, rx, n = (h + 4) // 8, (w + 4) // 8, (min(h, w) + 1) // 2
    out = np.empty((rows, 8), np.float64)
    for r in range(rows):
        m = [int(v) >> 9 for v in x[r]]
        b, s, c = (m[0] - 2 ** 22) * 2.0 ** -23, m[1] * 2.0 ** -22, 0.5 + m[2] * 2.0 ** -23
        ty, tx = ((m[3] * (2 * ry + 1)) >> 23) - ry, ((m[4] * (2 * rx + 1)) >> 23) - rx
        cy0, cx0 = ((m[5] * (h + 1)) >> 23) - n // 2, ((m[6] * (w + 1)) >> 23) - n // 2
        out[r] = ((b, s, c) if policy & COLOR else (0.0, 1.0, 1.0)) + ((ty, tx) if policy & TRANSLATION else (0, 0)) \
            + ((cy0, cx0, n) if policy & CUTOUT else (0, 0, 0))
    return out


def _frames(x, frames, cf):
    return [x[..., f * cf:(f + 1) * cf] for f in range(frames)]


def _live(p, h, w):
    """bool [h, w]: output pixel (y, x) is written from a source - (y - ty, x - tx) inside and (y, x) not in the cut rectangle."""
    ty, tx, cy0, cx0, n = (int(v) for v in p[3:8])
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    inside = (yy - ty >= 0) & (yy - ty < h) & (xx - tx >= 0) & (xx - tx < w)
    cut = (yy >= cy0) & (yy < cy0 + n) & (xx >= cx0) & (xx < cx0 + n)
    return inside & ~cut


def _move(col, p):
    """[h, w, c] -> out[y, x] = col[y - ty, x - tx] where live, 0 elsewhere."""
    h, w = col.shape[:2]
    ty, tx = int(p[3]), int(p[4])
    live = _live(p, h, w)
    yy, xx = (torch.as_tensor(v) for v in np.nonzero(live))
    out = torch.zeros_like(col)
    out[yy, xx] = col[yy - ty, xx - tx]
    return out


def _move_back(g, p):
    """The adjoint of _move: g'[q] = g[q + t] where q + t is live, 0 elsewhere."""
    h, w = g.shape[:2]
    ty, tx = int(p[3]), int(p[4])
    yy, xx = (torch.as_tensor(v) for v in np.nonzero(_live(p, h, w)))
    out = torch.zeros_like(g)
    out[yy - ty, xx - tx] = g[yy, xx]
    return out


def apply(x, params, frames, cf, offset=True):
    """acg_d_augment_fwd in closed form: x [rows, h, w, >= frames * cf] (torch float64) -> the valid channels [rows, h, w,
    frames * cf].  ``offset=False`` leaves + b out: the linear part of the map."""
    x = torch.as_tensor(x, dtype=torch.float64)
    rows = []
    for r in range(x.shape[0]):
        b, s, c = (float(v) for v in params[r][:3])
        outs = []
        for X in _frames(x[r], frames, cf):
            col = c * s * X + c * (1 - s) * X.mean(dim=2, keepdim=True) + (1 - c) * X.mean() + (b if offset else 0.0)
            outs.append(_move(col, params[r]))
        rows.append(torch.cat(outs, dim=2))
    return torch.stack(rows)


def stepwise(x, params, frames, cf):
    """The same, written out step by step: brightness -> saturation -> contrast -> shift -> cut."""
    x = torch.as_tensor(x, dtype=torch.float64)
    rows = []
    for r in range(x.shape[0]):
        b, s, c, ty, tx, cy0, cx0, n = (float(v) for v in params[r])
        ty, tx, cy0, cx0, n = int(ty), int(tx), int(cy0), int(cx0), int(n)
        outs = []
        for X in _frames(x[r], frames, cf):
            h, w = X.shape[:2]
            y = X + b
            m = y.mean(dim=2, keepdim=True)
            y = (y - m) * s + m
            mu = y.mean()
            y = (y - mu) * c + mu
            shifted = torch.zeros_like(y)
            for yy in range(h):
                for xx in range(w):
                    if 0 <= yy - ty < h and 0 <= xx - tx < w:
                        shifted[yy, xx] = y[yy - ty, xx - tx]
            for yy in range(max(cy0, 0), min(cy0 + n, h)):
                for xx in range(max(cx0, 0), min(cx0 + n, w)):
                    shifted[yy, xx] = 0.0
            outs.append(shifted)
        rows.append(torch.cat(outs, dim=2))
    return torch.stack(rows)


def adjoint(dout, params, frames, cf):
    """acg_d_augment_bwd as the header states it: dout [rows, h, w, >= frames * cf] -> din [rows, h, w, frames * cf]."""
    dout = torch.as_tensor(dout, dtype=torch.float64)
    rows = []
    for r in range(dout.shape[0]):
        s, c = float(params[r][1]), float(params[r][2])
        outs = []
        for g in _frames(dout[r], frames, cf):
            gp = _move_back(g, params[r])
            outs.append(c * s * gp + c * (1 - s) * gp.mean(dim=2, keepdim=True) + (1 - c) * gp.mean())
        rows.append(torch.cat(outs, dim=2))
    return torch.stack(rows)


class DAugOracleTrainer(OracleTrainer):
    """OracleTrainer whose discriminator judges augmented pairs: ``d_params`` holds one [B, 8] array per discriminator call of the
    step that follows, in call order - train_d: D(fake), then D(real); train_g: D(fake) - set before every step.  The per-frame map
    applied to ``img`` and ``frame`` under the same parameters is the 6-channel op.  ``d_add`` (optional, same protocol): noise
    added to the augmented judged frame (d_noise behind the augmentation)."""
    d_params = ()
    d_add = None

    def _d(self, p, img, frame, actions):
        now, self.d_params = self.d_params[0], self.d_params[1:]
        pair = apply(torch.cat([img, frame], dim=3), np.asarray(now, np.float64), 2, 3).to(frame.dtype)
        img, frame = pair[..., :3], pair[..., 3:]
        if self.d_add is not None:
            add_now, self.d_add = self.d_add[0], self.d_add[1:]
            frame = frame + torch.as_tensor(np.asarray(add_now), dtype=frame.dtype)
        return super()._d(p, img, frame, actions)
