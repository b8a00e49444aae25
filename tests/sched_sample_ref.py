"""float64 restatement of scheduled sampling for the K-step rollout (include/acgan_rollout.h, acg_sched_sample_*; train.Trainer
sched_sampling): the schedule, the coins (noise_ref's Philox4x32-10) and the K-step rollout with a given mask, composed from the
oracle's models as rollout_train_ref.rollout is.  Test infrastructure."""
import numpy as np
import torch

import noise_ref as NR
import rollout_train_ref as RR
from oracle import models as OM
from oracle import tf_ops as OT
from oracle.trainer import L2_WEIGHT

KINDS = ('constant', 'linear', 'inverse_sigmoid')
STREAM_TAG = 0x5353414D                       # acgan_rollout.h ACG_SS_STREAM_TAG
MASK32 = 0xFFFFFFFF


def probability(kind, k, start=1.0, final=0.0, decay_steps=0, offset=0):
    """The probability of truth at update ``k`` in float64, every operation rounded on its own (numpy scalars).  ``start`` / ``final``
    are taken as the float32 the C struct holds."""
    s, f = np.float64(np.float32(start)), np.float64(np.float32(final))
    if kind == 'constant':
        return s
    j, d = np.float64(max(int(k) - int(offset), 0)), np.float64(decay_steps)
    if kind == 'linear':
        return s + (f - s) * min(j / d, np.float64(1.0))
    if kind == 'inverse_sigmoid':
        with np.errstate(over='ignore'):
            e = np.exp(j / d)
        return f + (s - f) * (d / (d + e))
    raise ValueError(kind)


def probability32(*a, **kw):
    """(float)p: what prob_out holds."""
    return np.float32(probability(*a, **kw))


def uniforms(seed, counter, stream_id, steps, batch):
    """u [steps, batch] float64 in (0, 1), each exactly the float32 the kernel compares: element e = s * batch + b is lane e % 4 of
    Philox block e // 4 with the counter words (lo32(counter), hi32(counter), block, stream_id ^ STREAM_TAG)."""
    seed, counter = int(seed) % 2 ** 64, int(counter) % 2 ** 64
    n = steps * batch
    nb = -(-n // 4)
    ctr = np.empty((nb, 4), np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2] = counter & MASK32, counter >> 32, np.arange(nb, dtype=np.uint32)
    ctr[:, 3] = (int(stream_id) ^ STREAM_TAG) & MASK32
    x = NR.philox4x32_10(ctr, np.array([seed & MASK32, seed >> 32], np.uint32))
    u = ((x >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    return u.reshape(-1)[:n].reshape(steps, batch)


def coins(seed, counter, stream_id, steps, batch, prob32):
    """mask [steps, batch] bool (True: read the truth) given the float32 probability the device compared with."""
    return uniforms(seed, counter, stream_id, steps, batch) < np.float64(np.float32(prob32))


def select(mask_row, pred, truth):
    """Rows of ``truth`` where mask_row is set, of ``pred`` elsewhere (numpy arrays, any dtype: a copy of bits)."""
    m = np.asarray(mask_row) != 0
    return np.where(m.reshape((-1,) + (1,) * (pred.ndim - 1)), truth, pred)


def select_adjoint(mask_row, dout):
    m = np.asarray(mask_row) != 0
    return np.where(m.reshape((-1,) + (1,) * (dout.ndim - 1)), np.zeros_like(dout), dout)


def rollout(p, dna, adv, loss, ksize, frames, actions, states, mask):
    """rollout_train_ref.rollout with the inputs of step j >= 1 replaced per row where ``mask[j - 1]`` ([K-1, B] bool) is set: the
    frame by frames[:, j], the state half of the action vector (DNA generator) by states[:, j - 1].  Same dict."""
    K, B = actions.shape[1], frames.shape[0]
    mask = torch.as_tensor(np.asarray(mask), dtype=torch.bool).reshape(max(K - 1, 0), B)
    img, act = frames[:, 0], actions[:, 0]
    out = {'frames': [], 'states': [], 'step_loss': [], 'step_l2': []}
    for j in range(K):
        if dna:
            frame, st = OM.generator_transform(p, img, act, ksize)
        else:
            frame, st = OM.generator(p, img, act), None
        nxt = frames[:, j + 1]
        l2 = OT.l1_over_batch(frame, nxt, B)
        if dna:
            l2 = l2 * L2_WEIGHT + OT.l2norm_over_batch(st, states[:, j], B)
        g = l2
        if adv:
            g = l2 + OT.g_adv_loss(OM.discriminator(p, torch.cat([img, frame], dim=3), act), loss) + OT.gdl(nxt, frame)
        out['frames'].append(frame)
        out['states'].append(st)
        out['step_loss'].append(g)
        out['step_l2'].append(l2)
        if j + 1 < K:
            m = mask[j]
            img = torch.where(m[:, None, None, None], nxt, frame)
            if dna:
                act = torch.cat([actions[:, j + 1, :5], torch.where(m[:, None], states[:, j], st)], dim=1)
            else:
                act = actions[:, j + 1]
    out['g_loss'] = sum(out['step_loss']) / K
    out['l2_loss'] = sum(out['step_l2']) / K
    return out


class SchedOracle(RR.RolloutOracle):
    """RolloutOracle whose steps take the mask of the update ([K-1, B] bool, set before every step)."""
    mask = None

    def _step(self, opt, key, frames, actions, states):
        p = dict(self.p)
        for n in self.g_names:
            p[n] = self.p[n].detach().clone().requires_grad_(True)
        out = rollout(p, self.dna, self.adv, self.loss, self.ksize, frames, actions, states, self.mask)
        grads = torch.autograd.grad(out[key], [p[n] for n in self.g_names], allow_unused=True)
        self.last_grads = {n: g for n, g in zip(self.g_names, grads) if g is not None}
        opt.apply(self.p, self.last_grads)
        return {k: ([t.detach() if t is not None else None for t in v] if isinstance(v, list) else v.detach()) for k, v in out.items()}
