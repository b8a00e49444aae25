"""Float64 restatement of the planner's designated-pixel cost (include/acgan_rollout.h: acg_plan_pixel_cost) and of the map rollout
it scores: the DNA gather of the oracle (oracle.tf_ops.dna_gather) applied to probability maps instead of a frame."""
import numpy as np
import torch

from oracle import tf_ops

EPS32 = 2.0 ** -24


def sum_bound(h, w):
    """Worst-case relative error of a float32 sum of h * w non-negative terms in ANY order, each term a few roundings of its own,
    carried through one division: 2 (h w + 4) 2^-24.  Derived, not measured: a sum of n non-negative float32 terms is off by at
    most (n - 1) 2^-24 relatively whatever the order, a term and the division add a handful of roundings, and a quotient of two
    such sums doubles it."""
    return 2.0 * (h * w + 4) * EPS32


def pixel_cost(maps, goals, pixel_weight=1.0, old=None):
    """maps [N, h, w, d], goals [d, 2] (y, x) -> {'cost' [N], 'maps' (every map divided by its mass), 'expected' [N, d, 2],
    'mass' [N, d]} in float64.  A map whose mass is not finite or not > 0 makes the row's cost +inf, stays as it is and has NaN
    expectations.  ``old`` [N]: the cost to accumulate on (None: nothing is read)."""
    maps = np.asarray(maps, np.float64)
    goals = np.asarray(goals, np.float64)
    n, h, w, d = maps.shape
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    cost = np.zeros(n) if old is None else np.asarray(old, np.float64).copy()
    out = maps.copy()
    expected, mass = np.full((n, d, 2), np.nan), np.zeros((n, d))
    for i in range(n):
        total, bad = 0.0, False
        for j in range(d):
            P = maps[i, :, :, j]
            m0 = P.sum()
            mass[i, j] = m0
            if not (np.isfinite(m0) and m0 > 0):
                bad = True
                continue
            dist = np.sqrt((y - goals[j, 0]) ** 2 + (x - goals[j, 1]) ** 2)
            total += (P * dist).sum() / m0
            expected[i, j] = (P * y).sum() / m0, (P * x).sum() / m0
            out[i, :, :, j] = P / m0
        cost[i] += np.inf if bad else pixel_weight * total
    return {'cost': cost, 'maps': out, 'expected': expected, 'mass': mass}


def gather(logits, maps, ksize, bias=None):
    """One step of the map path: softmax(logits + bias) over the k * k taps, the k x k gather of ``maps`` [B, h, w, d] (float64)."""
    lg = torch.as_tensor(np.asarray(logits, np.float64))
    if bias is not None:
        lg = lg + torch.as_tensor(np.asarray(bias, np.float64))
    return tf_ops.dna_gather(lg, torch.as_tensor(np.asarray(maps, np.float64)), ksize).numpy()


def one_hot(n, h, w, pixels):
    """[n, h, w, d]: map j is 1 at pixels[j] = (y, x) and 0 elsewhere, in every row."""
    maps = np.zeros((n, h, w, len(pixels)))
    for j, (y, x) in enumerate(pixels):
        maps[:, y, x, j] = 1.0
    return maps


def tap_logits(n, h, w, ksize, tap, value=40.0):
    """Logits [n, h, w, k * k] with ``value`` on tap (i, j) and 0 elsewhere: the softmax is 1 on that tap to within exp(-value)."""
    lg = np.zeros((n, h, w, ksize * ksize))
    lg[..., tap[0] * ksize + tap[1]] = value
    return lg


def rollout(logits_per_step, maps, ksize, goals, pixel_weight=1.0, cost_steps='all', bias=None):
    """The planner's map rollout restated: gather, then (at the scored steps) cost and renormalisation.
    -> (cost [N], maps after every step [N, H, h, w, d], the last step's expected positions [N, d, 2])."""
    cost, kept, res = None, [], None
    steps = len(logits_per_step)
    for t, lg in enumerate(logits_per_step):
        maps = gather(lg, maps, ksize, bias)
        if cost_steps == 'all' or t == steps - 1:
            res = pixel_cost(maps, goals, pixel_weight, old=cost)
            cost, maps = res['cost'], res['maps']
        kept.append(maps)
    return cost, np.stack(kept, axis=1), res['expected']
