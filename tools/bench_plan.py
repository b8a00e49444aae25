#!/usr/bin/env python
"""What planning costs on one MI355X beside the generator forwards it is made of (profiles/plan/).

  python tools/bench_plan.py [--reps 9] [--out profiles/plan/bench_plan.txt]

(a) Planner.plan() - config 2's DNA generator (64^2, k = 5, float32) at batch N = 256, horizon 5, 3 iterations, 32 elites, warm -
    against the rollout it is built around: 3 x one 5-step Trainer._rollout_on_device at the same batch, the code path that
    existed before the planner (host frames in, the first step through Trainer.test).  The two take turns inside every round;
    wall time of a call that ends in a device synchronisation, median over --reps rounds, and the spread of each.
    EXPECTATION: plan() <= 1.10 x the three rollouts.  Also timed, as the stricter figure: the 15 device-fed predict steps alone
    (the program plan() runs, no cost, no sampling, no refit) - what the three launches, the concatenation and the host loop add.
    And plan() with the designated-pixel cost instead of the frame cost (pixel_weight 1, frame_weight 0, one pixel, no goal frame):
    one more DNA launch on the map and acg_plan_pixel_cost per step, plus the one more rollout that reads the plan's expected
    position back - reported as a ratio to the frame-cost plan(), no expectation attached (profiles/plan_pixel/).  One
    evaluate_actions() of either kind - a single 5-step rollout with its cost - separates what a step costs more from that rollout.
(b) the four kernels at that shape (N = 256, H = 5, A = 5, E = 32, 64 x 64 x 3 frames) and at the largest one (N = 1024, H = 16,
    A = 8, E = 100): each a HIP graph of 40 calls replayed between events, the graphs taking turns; the cost kernel also as a
    share of the 8 TB/s HBM peak on the bytes it must read (the frames; they live in the caches at these sizes); the pixel cost on
    one map and on four (N x 64 x 64 x D, read and rewritten)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from action_conditioned_gans_amd import graph as G, optim, plan as P, train as T   # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s (MI355X)
LINES = []
N, H, I, E, S = 256, 5, 3, 32, 64


def say(line=''):
    print(line, flush=True)
    LINES.append(line)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def plan_times(reps):
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cuda:0')
    tr = T.Trainer(sess, True, 'bce', 'adam', True, batch_size=N, img_size=S, ksize=5, lookahead=False, pixel_maps=1)
    sess.run(G.global_variables_initializer())
    rng = np.random.default_rng(0)
    frames = rng.uniform(-1, 1, (N, H + 1, S, S, 3)).astype(np.float32)
    acts = rng.standard_normal((N, H + 1, 10)).astype(np.float32)
    frame, state, goal = frames[0, 0], acts[0, 0, 5:], frames[0, H]
    planner = P.Planner(tr, H, E, I, seed=1)
    pixel_planner = P.Planner(tr, H, E, I, seed=1, frame_weight=0.0, pixel_weight=1.0)
    pixels, goal_pixels = np.array([[20, 30]]), np.array([[24.0, 30.0]])
    dev = sess.rt.device
    f0 = torch.from_numpy(frames[:, 0]).to(dev)
    a_dev = torch.from_numpy(acts).to(dev)
    fetches = [tr.g_next_frame, tr.g_state_out]

    def forwards():
        f, s = f0, a_dev[:, 0, 5:]
        for k in range(I * H):
            t = k % H
            if t == 0:
                f, s = f0, a_dev[:, 0, 5:]
            tr._announced = None
            res = sess.run(fetches, tr._feed(f, f, torch.cat([a_dev[:, t, :5], s], dim=1)), device_fetch=True)
            f, s = res[0], res[1]

    calls = {
        'plan()': lambda: planner.plan(frame, state, goal),
        'plan() pixel cost': lambda: pixel_planner.plan(frame, state, None, pixels=pixels, goal_pixels=goal_pixels),
        'evaluate_actions()': lambda: planner.evaluate_actions(frame, state, acts[:, :H, :5], goal),
        'evaluate_actions() pixel': lambda: pixel_planner.evaluate_actions(frame, state, acts[:, :H, :5], None, pixels=pixels,
                                                                          goal_pixels=goal_pixels),
        '%d x 5-step rollout' % I: lambda: [tr._rollout_on_device(frames, frames, acts, H) for _ in range(I)],
        '%d predict steps' % (I * H): forwards,
    }
    for fn in calls.values():            # warm: eager pass, capture, replay
        for _ in range(3):
            fn()
    out = {k: [] for k in calls}
    for _ in range(reps):
        for label, fn in calls.items():
            out[label].append(wall(fn))
    sess.close()
    return out


def graph_of(fn, n_graph):
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(n_graph):
            fn()
    gr.replay()
    torch.cuda.synchronize()
    return gr


def kernel_times(n, h, a, e, reps, n_graph=40):
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    frames = torch.rand(n, S, S, 3, device=dev, generator=g) * 2 - 1
    goal = torch.rand(S, S, 3, device=dev, generator=g) * 2 - 1
    states, goal_state = torch.randn(n, 5, device=dev, generator=g), torch.randn(5, device=dev, generator=g)
    mean, std = torch.zeros(h, a, device=dev), torch.full((h, a), 0.5, device=dev)
    lo, hi = torch.full((a,), -1.0, device=dev), torch.full((a,), 1.0, device=dev)
    state = torch.tensor([1, 0], dtype=torch.int64, device=dev)
    actions, cost = torch.empty(n, h, a, device=dev), torch.empty(n, device=dev)
    best_cost, best_actions = torch.full((1,), float('inf'), device=dev), torch.zeros(h, a, device=dev)
    elite, history = torch.empty(e, dtype=torch.int32, device=dev), torch.empty(1, device=dev)
    P.sample_actions(mean, std, lo, hi, state, actions)
    P.accumulate_cost(frames, goal, cost, states=states, goal_state=goal_state, state_weight=0.5)
    maps = {d: torch.rand(n, S, S, d, device=dev, generator=g) + 0.1 for d in (1, 4)}       # (rescaled by every call: mass 1 from the second on)
    goals = torch.rand(4, 2, device=dev, generator=g) * (S - 1)
    calls = {
        'acg_plan_sample': lambda: P.sample_actions(mean, std, lo, hi, state, actions),
        'acg_plan_cost': lambda: P.accumulate_cost(frames, goal, cost, states=states, goal_state=goal_state, state_weight=0.5),
        'acg_plan_refit': lambda: P.refit(cost, actions, mean, std, best_cost, best_actions, elite, 1.0, 0.05, history=history),
        'acg_plan_pixel_cost d=1': lambda: P.accumulate_pixel_cost(maps[1], goals[:1], cost),
        'acg_plan_pixel_cost d=4': lambda: P.accumulate_pixel_cost(maps[4], goals, cost),
    }
    graphs = {k: graph_of(fn, n_graph) for k, fn in calls.items()}
    out = {k: [] for k in graphs}
    for _ in range(reps):
        for label, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            out[label].append(e0.elapsed_time(e1) * 1e3 / n_graph)
    say('# N = %d, H = %d, A = %d, E = %d, frames %d x %d x 3; us per call (HIP graph of %d calls), one column per round' % (n, h, a, e, S, S, n_graph))
    for label, v in out.items():
        say('%-24s %s   median %.2f' % (label, ' '.join('%.2f' % t for t in v), float(np.median(v))))
    nbytes = frames.numel() * 4.0
    med = float(np.median(out['acg_plan_cost']))
    say('acg_plan_cost: %.1f MB of frames = %.2f TB/s = %.1f %% of the 8 TB/s peak (bandwidth is the bound; cache-resident at this size)'
        % (nbytes / 1e6, nbytes / med / 1e6, 100 * nbytes / (med * 1e-6) / HBM_PEAK))
    for d in (1, 4):
        nbytes, med = maps[d].numel() * 8.0, float(np.median(out['acg_plan_pixel_cost d=%d' % d]))
        say('acg_plan_pixel_cost d=%d: %.1f MB of maps read and rewritten = %.2f TB/s = %.1f %% of the 8 TB/s peak (cache-resident at this size)'
            % (d, nbytes / 1e6, nbytes / med / 1e6, 100 * nbytes / (med * 1e-6) / HBM_PEAK))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'plan', 'bench_plan.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_plan.py measures on a GPU: none is visible')
    say('device: %s; %d rounds' % (torch.cuda.get_device_name(0), args.reps))
    times = plan_times(args.reps)
    say('# DNA generator (64^2, k=5, float32), N = %d candidates, horizon %d, %d iterations, %d elites; ms per call, one column per round'
        % (N, H, I, E))
    med = {}
    for label, v in times.items():
        med[label] = float(np.median(v))
        say('%-22s %s   median %.2f  (min %.2f, max %.2f)' % (label, ' '.join('%.2f' % t for t in v), med[label], min(v), max(v)))
    base = med['%d x 5-step rollout' % I]
    ratio = med['plan()'] / base
    say('EXPECTATION plan() <= 1.10 x %d rollouts: %.2f / %.2f = %.3f x: %s' % (I, med['plan()'], base, ratio, 'met' if ratio <= 1.10 else 'MISSED'))
    fwd = med['%d predict steps' % (I * H)]
    say('beside the %d device-fed predict steps alone: %.2f / %.2f = %.3f x (%.1f us per step for the three launches, the concatenation, '
        'the uploads and the one copy back)' % (I * H, med['plan()'], fwd, med['plan()'] / fwd, (med['plan()'] - fwd) * 1e3 / (I * H)))
    say('plan() with the pixel cost instead of the frame cost (one pixel, no goal frame): %.2f / %.2f = %.3f x'
        % (med['plan() pixel cost'], med['plan()'], med['plan() pixel cost'] / med['plan()']))
    ea, eap = med['evaluate_actions()'], med['evaluate_actions() pixel']
    say('one 5-step rollout with its cost, evaluate_actions(): pixel %.2f / frame %.2f = %.3f x (%.1f us per step more); the pixel plan() is '
        '%d such rounds and one more rollout for the plan\'s expected position' % (eap, ea, eap / ea, (eap - ea) * 1e3 / H, I))
    kernel_times(N, H, 5, E, args.reps)
    kernel_times(1024, 16, 8, 100, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
