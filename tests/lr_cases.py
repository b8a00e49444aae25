"""What the CPU and the GPU tests of the learning-rate keywords share: the float64 oracle trainer stepped with chosen constants, and
the comparison of a Trainer's weights with it at the project's bars for one optimizer step (tests/train_cases.py)."""
import functools

import numpy as np
import torch

import train_cases as TC
from oracle import models as OM
from oracle.trainer import OracleTrainer

from action_conditioned_gans_amd import graph as G


def t64(x):
    return torch.from_numpy(np.asarray(x)).double()


def inputs():
    return TC.MG.inputs(2)


def params():
    return OM.init_params(True, batch=2, ksize=5, seed=TC.MG.PARAM_SEED, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def oracle_steps(opt, calls, g_lr, d_lr, beta1=None, pretrain_lr=None):
    """The DNA / bce oracle trainer at B = 2 run through ``calls`` (a tuple of 'pretrain_g' / 'train_d' / 'train_g') with its three
    optimizers' rates (and Adam's beta1) set -> per call a dict in the form train_cases.check_adam_params reads: 'grad/<name>' the
    float64 gradient of the call, 'param/<name>' the scope's weights after it.  Computed once per argument set and shared; callers
    must not modify it."""
    x, y, a, s = inputs()
    feed = (t64(x), t64(y), t64(a), t64(s))
    ref = OracleTrainer({k: v.double() for k, v in params().items()}, True, 'bce', opt, True, 5)
    f32 = lambda v: float(np.float32(v))                                       # noqa: E731
    ref.g_opt.lr, ref.d_opt.lr, ref.g_pretrain_opt.lr = f32(g_lr), f32(d_lr), f32(g_lr if pretrain_lr is None else pretrain_lr)
    if beta1 is not None:
        for o in (ref.g_opt, ref.d_opt, ref.g_pretrain_opt):
            o.b1 = f32(beta1)
    out = []
    for call in calls:
        if call == 'train_d':
            ref.train_d(*feed[:3])
        else:
            getattr(ref, call)(*feed)
        names = ref.d_names if call == 'train_d' else ref.g_names
        gold = {'grad/' + n: g.numpy().copy() for n, g in ref.last_grads.items()}
        gold.update(('param/' + n, ref.p[n].detach().numpy().copy()) for n in names)
        out.append(gold)
    return out


def set_params(sess):
    p = params()
    for n, v in G.get_default_graph().variables.items():
        sess.set_value(v, p[n])


def weights(sess, variables):
    return {v.name: sess.get_value(v).double().numpy() for v in variables}


def check_step(got, gold, opt, lr, what):
    """One optimizer step at rate ``lr`` against the oracle's: Adam at check_adam_params' bar for that rate; RMSProp at the bar of
    train_cases.case_pretrain_golden with that rate in place of the constant (1e-3 of the rate, and 1e-7 for float32 storage)."""
    if opt == 'adam':
        TC.check_adam_params(got, gold, 'grad/', 'param/', what, lr=lr)
        return
    for n, v in got.items():
        err = np.abs(v - gold['param/' + n]).max()
        assert err <= 1e-3 * lr + 1e-7, '%s %s: weight off by %.3g after one RMSProp step (lr %g)' % (what, n, err, lr)
