"""float64 restatement of the generator's noise draw (include/acgan_rollout.h, acg_noise_concat) in numpy, and an OracleTrainer
whose generator reads [action, z] with z given.  Test infrastructure."""
import numpy as np
import torch

from oracle import models as OM
from oracle.trainer import OracleTrainer

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 on uint32 arrays: ctr [..., 4], key [..., 2] (broadcast) -> [..., 4]."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]             # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(MASK), p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + np.uint64(W0)) & np.uint64(MASK), (k[1] + np.uint64(W1)) & np.uint64(MASK)]
    return np.stack(c, axis=-1).astype(np.uint32)


def normals(seed, counter, stream_id, n):
    """The first ``n`` values z[e] of the draw (seed, counter, stream_id), float64: block e // 4, lane e % 4."""
    seed, counter = int(seed) % 2 ** 64, int(counter) % 2 ** 64
    nb = -(-n // 4)
    ctr = np.empty((nb, 4), np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = counter & MASK, counter >> 32, np.arange(nb, dtype=np.uint32), int(stream_id) & MASK
    x = philox4x32_10(ctr, np.array([seed & MASK, seed >> 32], np.uint32))
    u = ((x >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r = np.sqrt(-2.0 * np.log(u[:, 0::2]))
    t = 2.0 * np.pi * u[:, 1::2]
    z = np.stack([r * np.cos(t), r * np.sin(t)], axis=-1)               # [nb, pair, (cos, sin)] -> lanes 0..3
    return z.reshape(-1)[:n]


def noise_concat(actions, noise_dim, seed, counter, stream_id=0, scale=1.0):
    """acg_noise_concat: [B, A] -> [B, A + Z] float64."""
    b = actions.shape[0]
    z = normals(seed, counter, stream_id, b * noise_dim).reshape(b, noise_dim)
    return np.concatenate([np.asarray(actions, np.float64), scale * z if scale != 0 else np.zeros_like(z)], axis=1)


def init_params(arg_transform, noise_dim, batch=2, img=64, ksize=5, seed=0, dtype=torch.float32):
    """The variables of a Trainer with ``noise_dim``: g/ built on 10 + Z action channels, d/ on the 10-dim action."""
    wide = OM.init_params(arg_transform, batch=batch, img=img, ksize=ksize, seed=seed, dtype=dtype, act_dim=10 + noise_dim)
    narrow = OM.init_params(arg_transform, batch=batch, img=img, ksize=ksize, seed=seed, dtype=dtype, act_dim=10)
    return {k: (wide[k] if k.startswith('g/') else narrow[k]) for k in wide}


class NoiseOracleTrainer(OracleTrainer):
    """OracleTrainer whose generator reads [actions, z]: ``z`` ([B, Z], set before every step - the Trainer's last_noise()) is
    appended inside _g, so the discriminator keeps the 10-dim action."""
    z = None

    def _g(self, p, img, actions):
        return super()._g(p, img, torch.cat([actions, torch.as_tensor(self.z, dtype=actions.dtype)], dim=1))
