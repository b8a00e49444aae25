#!/usr/bin/env python
"""What clipping by global norm costs on one MI355X (profiles/clip_norm/).

  python tools/bench_clip_norm.py [--steps 200] [--reps 7] [--stream-probe build/stream_probe] [--out profiles/clip_norm/bench.txt]

(a) acg_grad_clip_norm alone on the real layouts of G and D at config 2's shape (batch 32, 64^2, DNA k = 5): N launches captured
    into a HIP graph and replayed between two events, in three modes - measure only (max_norm = +inf: two launches, one read of
    the buffer), not clipping (a bound above the norm: three launches, one read) and clipping (launch k of the graph gets the
    bound norm0 / 2^(k+1), so every launch scales by about a half; the buffer is refilled before every replay: three launches,
    two reads and one write).  Each mode also COLD: the graph holds (refill, call) pairs - another kernel rewrites the whole
    buffer in front of every call, as backward does in a step - and the time of a graph of the refills alone is taken off; the
    hot figure re-reads what the previous call left in the caches and is a lower bound no step can see.  Reported as a fraction
    of the 8 TB/s HBM peak, with no threshold - the buffers live in the caches
    - beside tools/micro/stream_probe.hip on a buffer of the same size when the binary is there (`ew`: one read and one write,
    `tri`: two reads and one write; the probe has no read-only pass):
      hipcc -O3 --offload-arch=gfx950 -o build/stream_probe tools/micro/stream_probe.hip
(b) the G step and the D step (Trainer.train_g / train_d on the plain call path, device-resident inputs, replayed HIP graphs,
    bce, Adam, float32) with the feature off, measuring only, and clipping (bounds far below the norms: every step scales).  All
    sessions live in ONE process and take turns: --reps rounds, each timing --steps steps of every variant; microseconds per
    step, medians, and the run-to-run spread (max - min) of the variant without it.
Requirement written out with the numbers, against both stand-alone figures: on <= off + the entry's own stand-alone time of (a)
+ the spread of off."""
import argparse
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from action_conditioned_gans_amd import _lib, graph as G, optim, train as T   # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s (MI355X)
N_GRAPH = 40
LINES = []


def say(line=''):
    print(line, flush=True)
    LINES.append(line)


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def make(**kw):
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cuda:0')
    tr = T.Trainer(sess, True, 'bce', 'adam', True, batch_size=32, img_size=64, ksize=5, lookahead=False, **kw)
    sess.run(G.global_variables_initializer())
    return sess, tr


VARIANTS = [('off', {}), ('measure only', dict(grad_norms=True)), ('clipping', dict(g_clip_norm=1e-2, d_clip_norm=1e-5))]


def step_times(kind, steps, reps):
    """kind 'g' | 'd' -> ({label: [us per step of each round]}, {label: last stats or None}); the sessions take turns."""
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(32, 64, 64, 3, device=dev, generator=gen) * 2 - 1
    y = torch.rand(32, 64, 64, 3, device=dev, generator=gen) * 2 - 1
    a = torch.randn(32, 10, device=dev, generator=gen)
    s = a[:, 5:].contiguous()
    live = []
    for label, kw in VARIANTS:
        sess, tr = make(**kw)
        run = (lambda tr=tr: tr.train_g(x, y, a, s, device_fetch=True)) if kind == 'g' else (lambda tr=tr: tr.train_d(x, y, a))
        for _ in range(5):                                   # eager, capture, replays - while this session's graph is the default one
            run()
        live.append((label, sess, tr, run))
    torch.cuda.synchronize()
    out = {label: [] for label, _, _, _ in live}
    for _ in range(reps):
        for label, sess, tr, run in live:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                run()
            torch.cuda.synchronize()
            out[label].append((time.perf_counter() - t0) * 1e6 / steps)
    stats = {}
    for label, sess, tr, run in live:
        stats[label] = tr.grad_norm_stats(kind) if tr.grad_norm[kind] is not None else None
        sess.close()
    return out, stats


def layouts():
    """-> {scope: (total, [(offset, numel)])} of config 2's DNA generator and discriminator."""
    sess, tr = make()
    out = {}
    for scope in ('g', 'd'):
        _, windows = optim.GradNorm(1.0, scope).segments()
        out[scope] = (G.get_default_graph().layout(scope)[1], windows)
    sess.close()
    return out


def entry_times(total, windows, reps, lib=None):
    """-> ({mode: [us per call of each replay]}, {mode: [the same, cold]}, last scales, norm) for the three modes on one layout."""
    lib, dev = lib or _lib.get(), torch.device('cuda:0')
    segs = _lib.NormSegments()
    segs.count = len(windows)
    for i, (o, n) in enumerate(windows):
        segs.offset[i], segs.length[i] = o, n
    nbytes = lib.grad_clip_norm_workspace_bytes(total, ctypes.byref(segs))
    ws = torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=dev)
    stats = torch.zeros(2 + len(windows), device=dev)
    src = torch.randn(total, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    grad = src.clone()
    lib.grad_clip_norm(p(grad), total, ctypes.byref(segs), 1.0, float('inf'), p(stats), p(ws), nbytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    norm0 = float(stats[0].item())
    bounds = {'measure only': [float('inf')] * N_GRAPH, 'not clipping': [2.0 * norm0] * N_GRAPH,
              'clipping': [norm0 / 2.0 ** (k + 1) for k in range(N_GRAPH)]}

    def replays(bs, refill):
        """us per graph node pair of reps replays; bs None: the refills alone."""
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            for b in bs if bs is not None else [None] * N_GRAPH:
                if refill:
                    grad.copy_(src)
                if b is not None:
                    lib.grad_clip_norm(p(grad), total, ctypes.byref(segs), 1.0, b, p(stats), p(ws), nbytes, sp)
        got = []
        for _ in range(reps + 1):
            grad.copy_(src)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            got.append(e0.elapsed_time(e1) * 1e3 / N_GRAPH)
        return got[1:]                                                   # (the first replay warms up)
    out, cold, scales = {}, {}, {}
    refills = float(np.median(replays(None, True)))
    for mode, bs in bounds.items():
        out[mode], scales[mode] = replays(bs, False), float(stats[1].item())
        cold_bs = bs if mode != 'clipping' else [norm0 / 2.0] * N_GRAPH  # (refilled in front of every call: one bound does)
        cold[mode] = [t - refills for t in replays(cold_bs, True)]
        if mode == 'clipping' and not float(stats[1].item()) < 1.0:
            scales[mode] = float(stats[1].item())
    return out, cold, scales, norm0


def stream_probe(path, n):
    """-> (us of one read + one write, us of two reads + one write) over n floats, or None."""
    if not path or not os.path.exists(path):
        return None
    n4 = n // 4 * 4
    res = {}
    for args, key in ((['ew', str(n4 // 4), '4'], 'ew'), (['tri', str(n4)], 'tri')):
        text = subprocess.run([path] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, check=True).stdout.decode()
        for line in text.splitlines():
            f = line.split()
            if f and f[0] == key and 'stream_us' in f:
                res[key] = float(f[f.index('stream_us') + 1])
    return (res['ew'], res['tri']) if len(res) == 2 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--stream-probe', default=os.path.join(ROOT, 'build', 'stream_probe'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clip_norm', 'bench.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_clip_norm.py measures on a GPU: none is visible')
    say('device: %s' % torch.cuda.get_device_name(0))

    # (a) the entry alone
    alone, alone_cold = {}, {}
    for scope, (total, windows) in layouts().items():
        times, cold, scales, norm0 = entry_times(total, windows, args.reps)
        say('# acg_grad_clip_norm alone on the %s layout: %d floats (%.1f MB) in %d segments, %d partials; us per call (HIP graph of %d calls), '
            'one column per replay' % (scope.upper(), total, total * 4 / 1e6, len(windows), sum(-(-n // 8192) for _, n in windows), N_GRAPH))
        for mode, passes in (('measure only', 1), ('not clipping', 1), ('clipping', 3)):
            t = float(np.median(times[mode]))
            moved = passes * 4.0 * sum(n for _, n in windows)
            say('%-14s %s   median %.2f; %d pass(es), %.1f MB = %.2f TB/s = %.1f %% of the 8 TB/s peak; last scale %.4g'
                % (mode, ' '.join('%.2f' % v for v in times[mode]), t, passes, moved / 1e6, moved / t / 1e6, 100 * moved / (t * 1e-6) / HBM_PEAK, scales[mode]))
            say('%-14s %s   median %.2f (buffer rewritten by a copy kernel in front of every call; the copies alone taken off)'
                % ('  cold', ' '.join('%.2f' % v for v in cold[mode]), float(np.median(cold[mode]))))
        if not (scales['clipping'] < 1.0 and scales['not clipping'] == 1.0 and scales['measure only'] == 1.0):
            raise SystemExit('the modes did not do what they are named for: %r' % (scales,))
        pr = stream_probe(args.stream_probe, total)
        if pr:
            say('%-14s one read + one write %.2f us (%.2f TB/s), two reads + one write %.2f us (%.2f TB/s) over %d floats (tools/micro/stream_probe.hip)'
                % ('stream probe', pr[0], 8.0 * total / pr[0] / 1e6, pr[1], 12.0 * total / pr[1] / 1e6, total // 4 * 4))
        else:
            say('%-14s probe binary not built' % 'stream probe')
        alone[scope] = {m: float(np.median(v)) for m, v in times.items()}
        alone_cold[scope] = {m: float(np.median(v)) for m, v in cold.items()}

    # (b) the steps
    say('# %d rounds of %d steps per variant; config 2 (batch 32, 64^2, DNA k=5, bce, Adam, float32), plain call path' % (args.reps, args.steps))
    verdicts = []
    for kind in ('g', 'd'):
        times, stats = step_times(kind, args.steps, args.reps)
        say('# %s step; us per step, one column per round' % kind.upper())
        for label, v in times.items():
            st = stats[label]
            say('%-14s %s   median %.1f%s' % (label, ' '.join('%.1f' % t for t in v), float(np.median(v)),
                                             '' if st is None else '   (last norm %.4g, scale %.4g)' % (st['norm'], st['scale'])))
        spread = max(times['off']) - min(times['off'])
        say('run-to-run spread of off (max - min): %.1f us' % spread)
        if not stats['clipping']['scale'] < 1.0:
            raise SystemExit('%s: the clipping variant did not clip (scale %r)' % (kind, stats['clipping']['scale']))
        med = {k: float(np.median(v)) for k, v in times.items()}
        for label in ('measure only', 'clipping'):
            for what, budget in (('hot', alone[kind][label]), ('cold', alone_cold[kind][label])):
                ok = med[label] <= med['off'] + budget + spread
                verdicts.append('%s step, %s (%.1f) <= off (%.1f) + the entry alone, %s (%.2f) + spread (%.1f) = %.1f: %s'
                                % (kind.upper(), label, med[label], med['off'], what, budget, spread, med['off'] + budget + spread,
                                   'met' if ok else 'NOT met'))
    say('# requirement: on is not slower than off by more than the entry\'s own stand-alone time plus the off run\'s spread')
    for v in verdicts:
        say(v)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
