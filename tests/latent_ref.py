"""float64 restatement of the latent posterior's two entries (include/acgan_rollout.h, acg_latent_fwd / acg_latent_bwd) in numpy,
on the draw of noise_ref, and an OracleTrainer with the encoder, the reparameterised z and the KL term.  Test infrastructure."""
import numpy as np
import torch

import noise_ref as NR
from oracle import models as OM
from oracle.trainer import OracleTrainer

Q_WIDTHS = (32, 64, 128, 256)


def kl_sum(stats):
    """0.5 * sum (mu^2 + exp(logvar) - logvar - 1) over a [B, 2 Z] array, float64."""
    s = np.asarray(stats, np.float64)
    z = s.shape[1] // 2
    mu, lv = s[:, :z], s[:, z:]
    return 0.5 * float(np.sum(mu * mu + np.exp(lv) - lv - 1.0))


def latent_fwd(actions, stats, seed, counter, stream_id=0, scale=1.0, posterior=True):
    """acg_latent_fwd: -> (out [B, A + Z] float64, kl float64, eps [B, Z] float64).  ``stats`` [B, 2 Z] = [mu, logvar]."""
    a, s = np.asarray(actions, np.float64), np.asarray(stats, np.float64)
    b, z = a.shape[0], s.shape[1] // 2
    eps = NR.normals(seed, counter, stream_id, b * z).reshape(b, z)
    if posterior:
        mu, lv = s[:, :z], s[:, z:]
        lat = mu.copy() if scale == 0 else mu + scale * np.exp(0.5 * lv) * eps
    else:
        lat = np.zeros_like(eps) if scale == 0 else scale * eps
    return np.concatenate([a, lat], axis=1), kl_sum(s), eps


def latent_bwd(dout, out, stats, posterior, kl_weight):
    """acg_latent_bwd: -> (dstats [B, 2 Z], dactions [B, A], magnitudes [B, 2 Z]) float64; ``dout`` None counts as zeros.
    ``magnitudes`` is the sum of the magnitudes of the two terms of every entry (what a rounding bound scales with)."""
    o, s = np.asarray(out, np.float64), np.asarray(stats, np.float64)
    z = s.shape[1] // 2
    a = o.shape[1] - z
    d = np.zeros_like(o) if dout is None else np.asarray(dout, np.float64)
    mu, lv, dz, lat = s[:, :z], s[:, z:], d[:, a:], o[:, a:]
    p = 1.0 if posterior else 0.0
    t_mu = (p * dz, kl_weight * mu)
    t_lv = (p * 0.5 * (lat - mu) * dz, kl_weight * 0.5 * np.expm1(lv))
    dstats = np.concatenate([t_mu[0] + t_mu[1], t_lv[0] + t_lv[1]], axis=1)
    mags = np.concatenate([np.abs(t_mu[0]) + np.abs(t_mu[1]), np.abs(t_lv[0]) + np.abs(t_lv[1])], axis=1)
    return dstats, d[:, :a].copy(), mags


def posterior_layers(z, head_k):
    """models.build_posterior as oracle/models.py layer rows: four conv 5x5/2 + BatchNorm + lrelu, a VALID head with bias."""
    rows = [('conv%d' % (i + 1), 'c', w, 5, 2, 'SAME', True, 'lrelu') for i, w in enumerate(Q_WIDTHS)]
    return rows + [('head', 'c', 2 * z, head_k, 1, 'VALID', False, None)]


def posterior(params, frame, next_frame, z, create=None):
    """The encoder: (x_t, x_{t+1}) [B, H, W, 3] each -> stats [B, 2 z]."""
    out = torch.cat([frame, next_frame], dim=3)
    for spec in posterior_layers(z, frame.shape[1] // 16):
        out = OM._layer(params, 'g/posterior', spec, out, create)
    return out.reshape(out.shape[0], -1)


def init_params(arg_transform, z, batch=2, img=64, ksize=5, seed=0, dtype=torch.float32):
    """The variables of a Trainer with ``noise_dim`` = z and ``posterior``: noise_ref.init_params plus g/posterior/*."""
    params = NR.init_params(arg_transform, z, batch=batch, img=img, ksize=ksize, seed=seed, dtype=dtype)
    x = torch.zeros(batch, img, img, 3, dtype=dtype)
    with torch.no_grad():
        posterior(params, x, x, z, create=(torch.Generator().manual_seed(seed + 1000), dtype))
    return params


class LatentOracleTrainer(OracleTrainer):
    """OracleTrainer whose generator reads [actions, z] with z = mu + exp(logvar / 2) * eps, (mu, logvar) the encoder's view of
    (x_t, x_{t+1}) and eps the restatement's draw at ``draw`` = (seed, counter), set before every step - the Trainer's
    noise_state() before its step.  kl_weight / B * KL joins g_l2_loss (the pretraining loss) and g_loss; the discriminator
    keeps the 10-dim action.  The next frame is stashed for _g by the steps."""
    draw = None
    stream_id = 0

    def __init__(self, params, arg_adv, arg_loss, arg_opt, arg_transform, ksize=5, latent_dim=4, kl_weight=1.0):
        super().__init__(params, arg_adv, arg_loss, arg_opt, arg_transform, ksize)
        self.latent_dim, self.kl_weight = latent_dim, float(kl_weight)
        self._next = self._kl = None

    def _g(self, p, img, actions):
        z = self.latent_dim
        stats = posterior(p, img, self._next, z)
        mu, lv = stats[:, :z], stats[:, z:]
        eps = torch.as_tensor(NR.normals(self.draw[0], self.draw[1], self.stream_id, img.shape[0] * z).reshape(img.shape[0], z), dtype=img.dtype)
        self.last_stats, self.last_z = stats.detach(), (mu + torch.exp(0.5 * lv) * eps).detach()
        self._kl = 0.5 * torch.sum(mu * mu + torch.exp(lv) - lv - 1.0)
        return super()._g(p, img, torch.cat([actions, mu + torch.exp(0.5 * lv) * eps], dim=1))

    def _g_losses(self, p, img, next_frame, actions, state):
        self._next = next_frame
        out = super()._g_losses(p, img, next_frame, actions, state)
        term = self._kl * (self.kl_weight / img.shape[0])
        out['g_kl'] = self._kl / img.shape[0]
        out['g_l2_loss'] = out['g_l2_loss'] + term
        out['g_loss'] = out['g_loss'] + term
        return out

    def train_d(self, img, next_frame, actions, return_all=False):
        self._next = next_frame
        return super().train_d(img, next_frame, actions, return_all=return_all)

    def test(self, img, next_frame, actions):
        self._next = next_frame
        return super().test(img, next_frame, actions)
