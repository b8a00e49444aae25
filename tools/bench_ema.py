#!/usr/bin/env python
"""What the generator's weight average costs on one MI355X (profiles/ema/).

  python tools/bench_ema.py [--steps 200] [--reps 7] [--stream-probe build/stream_probe] [--out profiles/ema/bench_ema.txt]

(a) the G step (Trainer.train_g on the plain call path, device-resident inputs, replayed HIP graph) at config 2's shape (batch 32,
    64^2, DNA k = 5, bce, Adam, float32) with the average off, carried by the optimizer launch (acg_adam_step_ema) and as a launch
    of its own behind it (Session(fuse_ema=False)); and at config 3's size (the same in bf16) with the average off and on (there
    it is always the stand-alone launch).  All sessions live in ONE process and take turns: --reps rounds, each timing --steps
    steps of every variant; microseconds per step, medians, and the run-to-run spread (max - min) of the variant without it.
(b) acg_ema_update alone over a buffer of the generator's size (N launches captured into a HIP graph, replayed between two
    events), as a fraction of the 8 TB/s HBM peak (three passes: shadow in, parameters in, shadow out; no threshold - 11.5 MB
    live in the caches), beside a three-pass stream of the same bytes when the probe binary is there:
      hipcc -O3 --offload-arch=gfx950 -o build/stream_probe tools/micro/stream_probe.hip
Expectations written out with the numbers: carried <= stand-alone, and on <= off + the stand-alone launch of (b), each within the
spread of the off variant."""
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
DECAY = 0.999
LINES = []


def say(line=''):
    print(line, flush=True)
    LINES.append(line)


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def make(dtype, ema, fuse=True):
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cuda:0', dtype=dtype, fuse_ema=fuse)
    tr = T.Trainer(sess, True, 'bce', 'adam', True, batch_size=32, img_size=64, ksize=5, lookahead=False, **({'ema_decay': DECAY} if ema else {}))
    sess.run(G.global_variables_initializer())
    return sess, tr


def g_step_times(variants, steps, reps):
    """variants: [(label, dtype, ema, fuse)] -> {label: [us per step of each round]}; the sessions take turns inside every round."""
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(32, 64, 64, 3, device=dev, generator=g) * 2 - 1
    y = torch.rand(32, 64, 64, 3, device=dev, generator=g) * 2 - 1
    a = torch.randn(32, 10, device=dev, generator=g)
    s = a[:, 5:].contiguous()
    live = []
    for label, dtype, ema, fuse in variants:
        sess, tr = make(dtype, ema, fuse)
        for _ in range(5):                                   # eager, capture, replays - while this session's graph is the default one
            tr.train_g(x, y, a, s, device_fetch=True)
        live.append((label, (sess, tr)))
    torch.cuda.synchronize()
    out = {label: [] for label, _ in live}
    for _ in range(reps):
        for label, (sess, tr) in live:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.train_g(x, y, a, s, device_fetch=True)
            torch.cuda.synchronize()
            out[label].append((time.perf_counter() - t0) * 1e6 / steps)
    total = live[0][1][0].graph.layout('g')[1]
    for label, (sess, tr) in live:
        if tr.ema is not None and tr.ema_updates() != 5 + reps * steps:
            raise SystemExit('%s: %d updates counted, %d run' % (label, tr.ema_updates(), 5 + reps * steps))
        sess.close()
    return out, total


def timed(fn, n_graph=40, reps=7):
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for _ in range(n_graph):
            fn(sp)
    gr.replay()
    torch.cuda.synchronize()
    got = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gr.replay()
        e1.record()
        torch.cuda.synchronize()
        got.append(e0.elapsed_time(e1) * 1e3 / n_graph)
    return got


def stream_probe(path, n):
    if not path or not os.path.exists(path):
        return None
    out = subprocess.run([path, 'tri', str(n)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, check=True).stdout.decode()
    for line in out.splitlines():
        f = line.split()
        if len(f) == 4 and f[0] == 'tri' and f[2] == 'stream_us':
            return float(f[3])
    return None


def report(title, times, off):
    say('# %s; us per G step, one column per round' % title)
    for label, v in times.items():
        say('%-22s %s   median %.1f' % (label, ' '.join('%.1f' % t for t in v), float(np.median(v))))
    spread = max(times[off]) - min(times[off])
    say('run-to-run spread of %r (max - min): %.1f us' % (off, spread))
    return {k: float(np.median(v)) for k, v in times.items()}, spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--stream-probe', default=os.path.join(ROOT, 'build', 'stream_probe'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ema', 'bench_ema.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ema.py measures on a GPU: none is visible')
    say('device: %s; %d rounds of %d steps per variant' % (torch.cuda.get_device_name(0), args.reps, args.steps))
    f32, total = g_step_times([('f32 off', 'f32', False, True), ('f32 ema carried', 'f32', True, True), ('f32 ema stand-alone', 'f32', True, False)],
                              args.steps, args.reps)
    m32, spread32 = report('config 2 (batch 32, 64^2, DNA k=5, bce, Adam, float32)', f32, 'f32 off')
    bf, _ = g_step_times([('bf16 off', 'bf16', False, True), ('bf16 ema', 'bf16', True, True)], args.steps, args.reps)
    mbf, spreadbf = report('config 3 size (the same in bf16)', bf, 'bf16 off')

    # (b) the stand-alone launch over a buffer of the generator's size
    lib, dev = _lib.get(), torch.device('cuda:0')
    shadow, param = torch.randn(total, device=dev), torch.randn(total, device=dev)
    count, word = torch.ones(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    t = timed(lambda s: lib.ema_update(p(shadow), p(param), total, DECAY, p(count), p(word), s))
    t_med, nbytes = float(np.median(t)), 3.0 * total * 4
    say('# acg_ema_update alone, %d floats (%.1f MB per buffer, %.1f MB moved); us per launch (HIP graph of 40 launches), one column per replay'
        % (total, total * 4 / 1e6, nbytes / 1e6))
    say('%-22s %s   median %.2f = %.2f TB/s = %.1f %% of the 8 TB/s peak' % ('acg_ema_update', ' '.join('%.2f' % v for v in t), t_med,
                                                                            nbytes / t_med / 1e6, 100 * nbytes / (t_med * 1e-6) / HBM_PEAK))
    pr = stream_probe(args.stream_probe, total)
    say('%-22s %s' % ('three-pass stream', ('%.2f us (tools/micro/stream_probe.hip tri %d)' % (pr, total)) if pr else 'probe binary not built'))

    say('# expectations')
    ok1 = m32['f32 ema carried'] <= m32['f32 ema stand-alone'] + spread32
    say('carried (%.1f) is not slower than stand-alone (%.1f) by more than the spread (%.1f): %s'
        % (m32['f32 ema carried'], m32['f32 ema stand-alone'], spread32, 'met' if ok1 else 'NOT met'))
    ok2 = m32['f32 ema carried'] <= m32['f32 off'] + t_med + spread32
    say('float32: on (%.1f) <= off (%.1f) + the stand-alone launch (%.2f) + spread (%.1f): %s'
        % (m32['f32 ema carried'], m32['f32 off'], t_med, spread32, 'met' if ok2 else 'NOT met'))
    ok3 = mbf['bf16 ema'] <= mbf['bf16 off'] + t_med + spreadbf
    say('bf16: on (%.1f) <= off (%.1f) + the stand-alone launch (%.2f) + spread (%.1f): %s'
        % (mbf['bf16 ema'], mbf['bf16 off'], t_med, spreadbf, 'met' if ok3 else 'NOT met'))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
