"""Restatements of the SSIM training loss (include/acgan_ssim_loss.h) for the tests.

value       sum_n (1 - SSIM_n), float64, from tests/ssim_ref.py's definition.
gradient    of that value with respect to the first argument:
  grad_autograd(x, y, torch.float64)   the reference: torch autograd through the direct definition;
  grad_closed64(x, y)                  the closed form of the header in float64 (checked against the reference on the CPU);
  grad_autograd(x, y, torch.float32)   float32 floor (a): autograd of the direct definition in float32;
  grad_closed32(x, y)                  float32 floor (b): the closed form in float32 with one shift per (frame, channel) and
                                       2 sxy = sxx + syy - Var(x - y).
The two float32 evaluations bracket the reasonable float32 designs; neither is the kernel.  Their errors against the float64
reference on a case are the rounding floor the kernel's error on that case is held to (tests/test_gpu_ssim_loss.py).

SsimOracleTrainer / SsimRolloutOracle: the oracle's one-step and K-step generator updates with the term
W / B * sum_b (1 - SSIM(frame_b, next_frame_b)) added to the l2 part of every step's loss (train.Trainer ssim_weight)."""
import numpy as np
import torch

import rollout_train_ref as RR
import ssim_ref as SR
from oracle.trainer import OracleTrainer

DATA_RANGE, K1, K2 = 2.0, 0.01, 0.03
C1, C2 = (K1 * DATA_RANGE) ** 2, (K2 * DATA_RANGE) ** 2
HALO = SR.TAPS - 1


def value64(x, y):
    """sum_n (1 - SSIM_n) of [n, h, w, c] frames, float64."""
    return float((1.0 - SR.ssim(x, y, DATA_RANGE, K1, K2)).sum())


# ---- torch: the direct definition, differentiable ------------------------------------------------------------------------
def _filter_t(a, g):
    h, w = a.shape[-3], a.shape[-2]
    rows = sum(g[k] * a[..., k:h - HALO + k, :, :] for k in range(SR.TAPS))
    return sum(g[k] * rows[..., :, k:w - HALO + k, :] for k in range(SR.TAPS))


def ssim_t(x, y):
    """Per-frame SSIM of torch tensors [..., h, w, c] in their own dtype (the direct definition: no shift, no rewrite)."""
    g = torch.as_tensor(SR.window_1d(), dtype=x.dtype)
    c1, c2 = torch.tensor(C1, dtype=x.dtype), torch.tensor(C2, dtype=x.dtype)
    mx, my = _filter_t(x, g), _filter_t(y, g)
    vx = _filter_t(x * x, g) - mx * mx
    vy = _filter_t(y * y, g) - my * my
    cxy = _filter_t(x * y, g) - mx * my
    s = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return s.mean(dim=(-3, -2, -1))


def loss_t(x, y):
    """sum over the frames of (1 - SSIM), torch, differentiable."""
    return (1.0 - ssim_t(x, y)).sum()


def grad_autograd(x, y, dtype=torch.float64):
    """d sum_n (1 - SSIM_n) / d x by autograd in ``dtype`` -> float64 numpy array."""
    xt = torch.as_tensor(np.asarray(x)).to(dtype).clone().requires_grad_(True)
    yt = torch.as_tensor(np.asarray(y)).to(dtype)
    g, = torch.autograd.grad(loss_t(xt, yt), [xt])
    return g.detach().numpy().astype(np.float64)


# ---- numpy: the closed form ------------------------------------------------------------------------------------------------
def _filter_np(a, g):
    h, w = a.shape[-3], a.shape[-2]
    rows = sum(g[k] * a[..., k:h - HALO + k, :, :] for k in range(SR.TAPS))
    return sum(g[k] * rows[..., :, k:w - HALO + k, :] for k in range(SR.TAPS))


def _adjoint_np(m, g):
    """G^T: the full (zero-padded) correlation of a [..., h - 10, w - 10, c] map back to [..., h, w, c], in m's dtype."""
    oh, ow = m.shape[-3], m.shape[-2]
    cols = np.zeros(m.shape[:-2] + (ow + HALO, m.shape[-1]), m.dtype)
    for k in range(SR.TAPS):
        cols[..., :, k:k + ow, :] += g[k] * m
    out = np.zeros(m.shape[:-3] + (oh + HALO, ow + HALO, m.shape[-1]), m.dtype)
    for k in range(SR.TAPS):
        out[..., k:k + oh, :, :] += g[k] * cols
    return out


def _closed(x, y, dtype, shift, rewrite):
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    g = SR.window_1d().astype(dtype)
    c1, c2, two = dtype(C1), dtype(C2), dtype(2)
    sx = x[..., :1, :1, :] if shift else np.zeros((), dtype)       # one constant per (frame, channel): the first value
    sy = y[..., :1, :1, :] if shift else np.zeros((), dtype)
    xs, ys = x - sx, y - sy
    a_, m_ = _filter_np(xs, g), _filter_np(ys, g)                   # means of the shifted frames
    sxx = _filter_np(xs * xs, g) - a_ * a_
    syy = _filter_np(ys * ys, g) - m_ * m_
    if rewrite:
        d = xs - ys
        two_sxy = sxx + syy - (_filter_np(d * d, g) - (a_ - m_) * (a_ - m_))
    else:
        two_sxy = two * (_filter_np(xs * ys, g) - a_ * m_)
    a, m = a_ + sx, m_ + sy
    A1, A2 = two * a * m + c1, two_sxy + c2
    B1, B2 = a * a + m * m + c1, sxx + syy + c2
    S = A1 * A2 / (B1 * B2)
    Pq, Pr = -S / B2, two * A1 / (B1 * B2)
    U = two * m * A2 / (B1 * B2) - two * a * S / B1
    ds = _adjoint_np(U - two * a_ * Pq - m_ * Pr, g) + xs * _adjoint_np(two * Pq, g) + ys * _adjoint_np(Pr, g)
    positions = (x.shape[-3] - HALO) * (x.shape[-2] - HALO) * x.shape[-1]
    return (ds * dtype(-1.0 / positions)).astype(np.float64)


def grad_closed64(x, y):
    return _closed(x, y, np.float64, shift=False, rewrite=False)


def grad_closed32(x, y):
    return _closed(x, y, np.float32, shift=True, rewrite=True)


# ---- the input classes of the kernel tests -----------------------------------------------------------------------------------
CLASSES = ('uniform', 'smooth', 'saturated', 'near_identical', 'constant')


def case(kind, shape, seed=0):
    """-> (pred, truth) float32 [n, h, w, c]."""
    rng = np.random.default_rng(seed)
    n, h, w, c = shape
    if kind == 'uniform':
        return rng.uniform(-1, 1, shape).astype(np.float32), rng.uniform(-1, 1, shape).astype(np.float32)
    if kind == 'smooth':
        i, j = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        base = 0.6 * np.sin(2 * np.pi * (i / 23.0 + j / 31.0))[None, :, :, None] + 0.2 * np.cos(i * j / 97.0)[None, :, :, None]
        base = base + 0.1 * np.arange(c)[None, None, None, :] - 0.05 * np.arange(n)[:, None, None, None]
        return ((base + 0.05 * rng.standard_normal(shape)).astype(np.float32), (base + 0.05 * rng.standard_normal(shape)).astype(np.float32))
    if kind == 'saturated':
        return np.sign(rng.standard_normal(shape)).astype(np.float32), np.sign(rng.standard_normal(shape)).astype(np.float32)
    if kind == 'near_identical':
        y = rng.uniform(-1, 1, shape).astype(np.float32)
        return (y + 1e-3 * rng.standard_normal(shape)).astype(np.float32), y
    if kind == 'constant':
        return np.full(shape, 0.30, np.float32), np.full(shape, 0.31, np.float32)
    raise ValueError(kind)


# ---- the oracle's steps with the term ------------------------------------------------------------------------------------------
def ssim_term(frame, next_frame):
    """sum_b (1 - SSIM_b) / B, torch in the frames' dtype (unweighted: the summary g_ssim_loss)."""
    return loss_t(frame, next_frame) / frame.shape[0]


class SsimOracleTrainer(OracleTrainer):
    def __init__(self, params, arg_adv, arg_loss, arg_opt, arg_transform, ksize=5, ssim_weight=0.0):
        super().__init__(params, arg_adv, arg_loss, arg_opt, arg_transform, ksize=ksize)
        self.ssim_weight = float(ssim_weight)

    def _g_losses(self, p, img, next_frame, actions, state):
        out = super()._g_losses(p, img, next_frame, actions, state)
        out['g_ssim_loss'] = ssim_term(out['frame'], next_frame)
        out['g_l2_loss'] = out['g_l2_loss'] + self.ssim_weight * out['g_ssim_loss']
        out['g_loss'] = out['g_loss'] + self.ssim_weight * out['g_ssim_loss']
        return out


def rollout(p, dna, adv, loss, ksize, frames, actions, states, ssim_weight):
    """rollout_train_ref.rollout with W * ssim_term added to every step's l2 part (and so to its loss)."""
    out = RR.rollout(p, dna, adv, loss, ksize, frames, actions, states)
    K = actions.shape[1]
    out['step_ssim'] = [ssim_term(out['frames'][j], frames[:, j + 1]) for j in range(K)]
    out['step_l2'] = [out['step_l2'][j] + ssim_weight * out['step_ssim'][j] for j in range(K)]
    out['step_loss'] = [out['step_loss'][j] + ssim_weight * out['step_ssim'][j] for j in range(K)]
    out['g_loss'] = sum(out['step_loss']) / K
    out['l2_loss'] = sum(out['step_l2']) / K
    return out


class SsimRolloutOracle(RR.RolloutOracle):
    def __init__(self, params, adv, loss, opt, dna, ksize=5, ssim_weight=0.0):
        super().__init__(params, adv, loss, opt, dna, ksize=ksize)
        self.ssim_weight = float(ssim_weight)

    def _step(self, opt, key, frames, actions, states):
        p = dict(self.p)
        for n in self.g_names:
            p[n] = self.p[n].detach().clone().requires_grad_(True)
        out = rollout(p, self.dna, self.adv, self.loss, self.ksize, frames, actions, states, self.ssim_weight)
        grads = torch.autograd.grad(out[key], [p[n] for n in self.g_names], allow_unused=True)
        self.last_grads = {n: g for n, g in zip(self.g_names, grads) if g is not None}
        opt.apply(self.p, self.last_grads)
        return {k: ([t.detach() if t is not None else None for t in v] if isinstance(v, list) else v.detach()) for k, v in out.items()}
