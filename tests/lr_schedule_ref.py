"""The learning-rate schedule of acg_adam_step_lr / acg_rmsprop_step_lr (include/acgan_rollout.h) restated in numpy float64, with
the one rounding to float32 at the end.  Shared by the CPU and the GPU tests of the schedule; nothing here imports the package."""
import numpy as np

KINDS = ('constant', 'linear', 'cosine', 'exponential')


def rate(lr, kind, k, warmup=0, decay_steps=0, final=0.0):
    """lr_k as a numpy float32: the rate of the update that finds the counter at ``k``.  ``lr`` and ``final`` are taken as the
    float32 values the entry receives."""
    lr, F, k = np.float64(np.float32(lr)), np.float64(np.float32(final)), int(k)
    w = np.float64(k + 1) / np.float64(warmup) if warmup > 0 and k < warmup else np.float64(1.0)
    j = np.float64(max(k - warmup, 0))
    if kind == 'constant':
        f = np.float64(1.0)
    else:
        t = min(j / np.float64(decay_steps), np.float64(1.0))
        if kind == 'linear':
            f = 1.0 - (1.0 - F) * t
        elif kind == 'cosine':
            f = F + (1.0 - F) * 0.5 * (1.0 + np.cos(np.pi * t))
        elif kind == 'exponential':
            with np.errstate(under='ignore'):                        # (far behind the decay the factor underflows to 0, as pow's does)
                f = np.power(F, j / np.float64(decay_steps))
        else:
            raise ValueError(kind)
    return np.float32(lr * w * f)


def ulps(a, b):
    """Distance of two positive float32 values in units of the last place."""
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))
