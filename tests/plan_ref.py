"""float64 restatement of the planner's three launches (include/acgan_rollout.h: acg_plan_sample / acg_plan_cost /
acg_plan_refit) in numpy, and the cross-entropy-method loop built from them.  Test infrastructure."""
import numpy as np

import noise_ref

PLAN_STREAM_TAG = 0x504C414E          # ACG_PLAN_STREAM_TAG
SS_STREAM_TAG = 0x5353414D            # ACG_SS_STREAM_TAG: the two must differ


def normals(seed, counter, stream_id, n):
    """z[e] of the draw: the noise input's generator with the stream word stream_id ^ ACG_PLAN_STREAM_TAG."""
    return noise_ref.normals(seed, counter, (int(stream_id) ^ PLAN_STREAM_TAG) & 0xFFFFFFFF, n)


def unclamped(mean, std, seed, counter, shape, stream_id=0, keep_mean=True):
    """mean + std * z [N, H, A] before the clamp (row 0 the mean itself with ``keep_mean``); -> (values, std * z)."""
    n, h, a = shape
    mean, std = np.asarray(mean, np.float64).reshape(h, a), np.asarray(std, np.float64).reshape(h, a)
    z = normals(seed, counter, stream_id, n * h * a).reshape(n, h, a)
    noise = std[None] * z
    if keep_mean:
        noise[0] = 0.0
    return mean[None] + noise, noise


def sample(mean, std, lo, hi, seed, counter, shape, stream_id=0, keep_mean=True):
    """acg_plan_sample: clamp(mean + std * z, lo, hi) [N, H, A] float64."""
    v, _ = unclamped(mean, std, seed, counter, shape, stream_id, keep_mean)
    return np.minimum(np.maximum(v, np.asarray(lo, np.float64)), np.asarray(hi, np.float64))


def cost(frames, goal, states=None, goal_state=None, frame_weight=1.0, state_weight=0.0, old=None, channels=None):
    """acg_plan_cost: frames [N, h, w, pitch] (channels < ``channels`` scored), goal [h, w, C]; ``old`` [N]: accumulate onto it."""
    frames, goal = np.asarray(frames, np.float64), np.asarray(goal, np.float64)
    c = goal.shape[-1] if channels is None else channels
    out = frame_weight * ((frames[..., :c] - goal[None]) ** 2).sum(axis=(1, 2, 3))
    if states is not None:
        out = out + state_weight * ((np.asarray(states, np.float64) - np.asarray(goal_state, np.float64)[None]) ** 2).sum(axis=1)
    return out if old is None else np.asarray(old, np.float64) + out


def keys(costs):
    k = np.array(costs, np.float64)
    k[np.isnan(k)] = np.inf
    return k


def ranks(costs):
    """rank[n] = #{m: key(m) < key(n), or key(m) == key(n) and m < n}: counted, as the kernel counts."""
    k = keys(costs)
    idx = np.arange(k.size)
    before = (k[None, :] < k[:, None]) | ((k[None, :] == k[:, None]) & (idx[None, :] < idx[:, None]))
    return before.sum(axis=1)


def refit(costs, actions, mean, std, elites, alpha, min_std, best_cost=np.inf, best_actions=None):
    """acg_plan_refit -> dict(elite_idx [E], mean, std [H, A], best_cost, best_actions [H, A], history)."""
    actions = np.asarray(actions, np.float64)
    n, h, a = actions.shape
    r = ranks(costs)
    elite_idx = np.empty(elites, np.int64)
    for cand in range(n):
        if r[cand] < elites:
            elite_idx[r[cand]] = cand
    chosen = actions[elite_idx]
    mean_e = chosen.sum(axis=0) / elites
    std_e = np.sqrt(((chosen - mean_e[None]) ** 2).sum(axis=0) / elites)
    mean, std = np.asarray(mean, np.float64).reshape(h, a), np.asarray(std, np.float64).reshape(h, a)
    new_mean = alpha * mean + (1.0 - alpha) * mean_e
    new_std = np.maximum(alpha * std + (1.0 - alpha) * std_e, min_std)
    first = keys(costs)[elite_idx[0]]
    best_actions = np.zeros((h, a)) if best_actions is None else np.asarray(best_actions, np.float64).reshape(h, a)
    if first < best_cost:                  # strictly: an equal cost keeps the earlier plan
        best_cost, best_actions = float(first), actions[elite_idx[0]].copy()
    return {'elite_idx': elite_idx, 'mean': new_mean, 'std': new_std, 'best_cost': best_cost, 'best_actions': best_actions,
            'history': best_cost}


def cem(cost_fn, shape, elites, iterations, init_std, min_std, alpha, lo, hi, seed=0, counter=0, stream_id=0):
    """The planner's loop on a cost function of the candidates [N, H, A] -> [N]; -> dict as Planner.plan's, plus 'costs'."""
    n, h, a = shape
    mean = np.zeros((h, a))
    std = np.full((h, a), float(init_std))
    best_cost, best_actions, history, all_costs = np.inf, None, [], []
    for i in range(iterations):
        cand = sample(mean, std, lo, hi, seed, counter + i, shape, stream_id)
        costs = np.asarray(cost_fn(cand), np.float64)
        res = refit(costs, cand, mean, std, elites, alpha, min_std, best_cost, best_actions)
        mean, std, best_cost, best_actions = res['mean'], res['std'], res['best_cost'], res['best_actions']
        history.append(best_cost)
        all_costs.append(costs)
    return {'actions': best_actions, 'cost': best_cost, 'history': np.array(history), 'mean': mean, 'std': std,
            'costs': np.array(all_costs), 'counter': counter + iterations}
