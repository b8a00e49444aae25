"""float64 restatement of the K-step rollout G loss and its gradient (train.Trainer rollout_steps), composed from the oracle's
models, losses and optimizers (torch autograd does the backward pass).

Step j = 0..K-1: frame_{j+1}, state_{j+1} = G(in_j, act_j); in_0 = frames[:, 0], in_j = frame_j; act_0 = actions[:, 0],
act_j = [actions[:, j, :5], state_j] (the plain generator: actions[:, j], as test_sequence feeds it).  Step loss = the one-step G
loss of that step: L1 (x L2_WEIGHT + the state norm against states[:, j] for the DNA generator), plus the adversarial term on
D(concat(in_j, frame_{j+1}), act_j) and the GDL against frames[:, j+1] with --adv.  G loss = the mean of the K step losses."""
import torch

from oracle import models as OM
from oracle import tf_ops as OT
from oracle.trainer import L2_WEIGHT, TFAdam, TFRMSProp


def rollout(p, dna, adv, loss, ksize, frames, actions, states):
    """-> dict: 'frames' / 'states' (lists of K tensors; states None for the plain generator), 'step_loss', 'step_l2' (lists of K
    scalars), 'g_loss' and 'l2_loss' (their means)."""
    K, B = actions.shape[1], frames.shape[0]
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
        img = frame
        if j + 1 < K:
            act = torch.cat([actions[:, j + 1, :5], st], dim=1) if dna else actions[:, j + 1]
    out['g_loss'] = sum(out['step_loss']) / K
    out['l2_loss'] = sum(out['step_l2']) / K
    return out


class RolloutOracle:
    """The generator's K-step G step and pretraining step in float64: parameters, one optimizer state per update kind (as the
    one-step trainer's g_opt / g_pretrain_opt, which the rollout updates continue)."""

    def __init__(self, params, adv, loss, opt, dna, ksize=5):
        self.p = {k: v.clone() for k, v in params.items()}
        self.adv, self.loss, self.dna, self.ksize = adv, loss, dna, ksize
        self.g_names = [k for k in self.p if k.startswith('g/')]
        mk = (lambda: TFRMSProp(self.g_names, self.p)) if opt == 'rmsprop' else (lambda: TFAdam(self.g_names, self.p))
        self.g_opt, self.g_pretrain_opt = mk(), mk()

    def _step(self, opt, key, frames, actions, states):
        p = dict(self.p)
        for n in self.g_names:
            p[n] = self.p[n].detach().clone().requires_grad_(True)
        out = rollout(p, self.dna, self.adv, self.loss, self.ksize, frames, actions, states)
        grads = torch.autograd.grad(out[key], [p[n] for n in self.g_names], allow_unused=True)
        self.last_grads = {n: g for n, g in zip(self.g_names, grads) if g is not None}
        opt.apply(self.p, self.last_grads)
        return {k: ([t.detach() if t is not None else None for t in v] if isinstance(v, list) else v.detach()) for k, v in out.items()}

    def train_g(self, frames, actions, states):
        return self._step(self.g_opt, 'g_loss', frames, actions, states)

    def pretrain_g(self, frames, actions, states):
        return self._step(self.g_pretrain_opt, 'l2_loss', frames, actions, states)
