#!/usr/bin/env python
"""What the SSIM training loss costs on one MI355X (profiles/ssim_loss/).

  python tools/bench_ssim_loss.py [--steps 200] [--reps 7] [--out profiles/ssim_loss/bench.txt]
  python tools/bench_ssim_loss.py --parity profiles/ssim_loss/parity.txt

(a) acg_ssim_loss, gradient only (what a training program launches), at (32, 64^2, 3) and (32, 128^2, 3), beside
    acg_frame_metrics on the same frames: each is N launches captured into a HIP graph, and the two graphs are replayed in turn
    between events in ONE process.  Also the value-only and the combined call, and the gradient-only call as a fraction of the
    8 TB/s HBM peak on its algorithmic bytes (pred and truth in, dpred out; reported, no threshold - the frames live in the
    caches).  REQUIREMENT: the gradient-only call takes no longer than 3 x acg_frame_metrics on the same frames in this run.
(b) the G step (Trainer.train_g on the plain call path, device-resident inputs, replayed HIP graph) at config 2's shape (batch 32,
    64^2, DNA k = 5, bce, Adam, float32) with ssim_weight 0 and 50: two sessions in one process taking turns, --reps rounds of
    --steps steps; microseconds per step, medians, and the run-to-run spread of the variant without the term.
--parity: every kernel case of tests/test_gpu_ssim_loss.py - its error against float64, the two float32 CPU floors, the bar and
the ratio of the error to the bar - as a table."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from action_conditioned_gans_amd import _lib, graph as G, optim, train as T   # noqa: E402
from action_conditioned_gans_amd.ops import SSIM_DATA_RANGE, SSIM_K1, SSIM_K2   # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s (MI355X)
LINES = []


def say(line=''):
    print(line, flush=True)
    LINES.append(line)


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def graph_of(fn, n_graph):
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for _ in range(n_graph):
            fn(sp)
    gr.replay()
    torch.cuda.synchronize()
    return gr


def alternate(graphs, n_graph, reps):
    """{label: graph} -> {label: [us per call of each round]}; the graphs take turns inside every round."""
    out = {k: [] for k in graphs}
    for _ in range(reps):
        for label, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            out[label].append(e0.elapsed_time(e1) * 1e3 / n_graph)
    return out


def kernel_times(shape, reps, n_graph=40):
    n, h, w, c = shape
    lib, dev = _lib.get(), torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(*shape, device=dev, generator=g) * 2 - 1
    y = (x + 0.1 * torch.randn(*shape, device=dev, generator=g)).clamp(-1, 1)
    nb = lib.ssim_loss_workspace_bytes(n, h, w, c)
    ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
    dp, val = torch.empty_like(x), torch.empty(1, device=dev)
    mb = lib.frame_metrics_workspace_bytes(n, h, w)
    mws = torch.zeros(mb, dtype=torch.uint8, device=dev)
    ssim, sq = torch.empty(n, device=dev), torch.empty(n, device=dev)
    tail = (n, h, w, c, SSIM_DATA_RANGE, SSIM_K1, SSIM_K2, p(ws), nb)
    calls = {
        'acg_ssim_loss grad': lambda s: lib.ssim_loss(p(x), p(y), None, p(dp), 1.0, *tail, s),
        'acg_frame_metrics': lambda s: lib.frame_metrics(p(x), p(y), p(ssim), p(sq), n, h, w, c, 0, _lib.ACG_F32, SSIM_DATA_RANGE, SSIM_K1,
                                                         SSIM_K2, p(mws), mb, s),
        'acg_ssim_loss value': lambda s: lib.ssim_loss(p(x), p(y), p(val), None, 1.0, *tail, s),
        'acg_ssim_loss both': lambda s: lib.ssim_loss(p(x), p(y), p(val), p(dp), 1.0, *tail, s),
    }
    times = alternate({k: graph_of(fn, n_graph) for k, fn in calls.items()}, n_graph, reps)
    say('# %s; us per call (HIP graph of %d calls), one column per round' % (shape, n_graph))
    med = {}
    for label, v in times.items():
        med[label] = float(np.median(v))
        say('%-22s %s   median %.2f' % (label, ' '.join('%.2f' % t for t in v), med[label]))
    nbytes = 3.0 * x.numel() * 4
    say('gradient only: %.1f MB algorithmic (pred, truth in; dpred out) = %.2f TB/s = %.1f %% of the 8 TB/s peak; workspace %.2f MB'
        % (nbytes / 1e6, nbytes / med['acg_ssim_loss grad'] / 1e6, 100 * nbytes / (med['acg_ssim_loss grad'] * 1e-6) / HBM_PEAK, nb / 1e6))
    ratio = med['acg_ssim_loss grad'] / med['acg_frame_metrics']
    say('REQUIREMENT gradient only <= 3 x acg_frame_metrics: %.2f / %.2f = %.2f x: %s' % (med['acg_ssim_loss grad'], med['acg_frame_metrics'],
                                                                                          ratio, 'met' if ratio <= 3.0 else 'NOT met'))
    return ratio


def g_step_times(weights, steps, reps):
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(32, 64, 64, 3, device=dev, generator=g) * 2 - 1
    y = torch.rand(32, 64, 64, 3, device=dev, generator=g) * 2 - 1
    a = torch.randn(32, 10, device=dev, generator=g)
    s = a[:, 5:].contiguous()
    live = []
    for w in weights:
        G.reset_default_graph()
        optim.set_data_parallel(1)
        sess = G.Session(device='cuda:0')
        tr = T.Trainer(sess, True, 'bce', 'adam', True, batch_size=32, img_size=64, ksize=5, lookahead=False, ssim_weight=w)
        sess.run(G.global_variables_initializer())
        for _ in range(5):                                   # eager, capture, replays - while this session's graph is the default one
            tr.train_g(x, y, a, s, device_fetch=True)
        live.append(('ssim_weight %g' % w, sess, tr))
    torch.cuda.synchronize()
    out = {label: [] for label, _, _ in live}
    for _ in range(reps):
        for label, sess, tr in live:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.train_g(x, y, a, s, device_fetch=True)
            torch.cuda.synchronize()
            out[label].append((time.perf_counter() - t0) * 1e6 / steps)
    for _, sess, _ in live:
        sess.close()
    return out


def parity(path):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import ssim_loss_ref as R
    import test_gpu_ssim_loss as K
    say('# acg_ssim_loss on %s against float64 autograd (tests/ssim_loss_ref.py); bar = %g x max(e_a, e_b), the errors of the two' %
        (torch.cuda.get_device_name(0), K.FACTOR))
    say('# float32 CPU evaluations of the same case; value bar = n x %g' % K.VALUE_BAR)
    say('%-18s %-15s %10s %10s %10s %10s %8s %10s %10s' % ('shape', 'class', 'max|g|', 'e_a', 'e_b', 'err', 'err/bar', 'value err', 'value bar'))
    worst = 0.0
    for shape in K.SHAPES:
        for kind in R.CLASSES:
            m = K.measure(kind, shape)
            worst = max(worst, m['ratio'])
            say('%-18s %-15s %10.3e %10.3e %10.3e %10.3e %8.3f %10.2e %10.2e' % (str(shape), kind, m['scale'], m['e_a'], m['e_b'], m['err'], m['ratio'],
                                                                               m['value_err'], shape[0] * K.VALUE_BAR))
    say('largest err/bar: %.3f' % worst)
    write(path)


def write(path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        f.write('\n'.join(LINES) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ssim_loss', 'bench.txt'))
    ap.add_argument('--parity', default=None, metavar='PATH', help='write the parity table of the kernel cases there and stop')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ssim_loss.py measures on a GPU: none is visible')
    if args.parity:
        return parity(args.parity)
    say('device: %s; %d rounds' % (torch.cuda.get_device_name(0), args.reps))
    for shape in [(32, 64, 64, 3), (32, 128, 128, 3)]:
        kernel_times(shape, args.reps)
    times = g_step_times([0.0, 50.0], args.steps, args.reps)
    say('# config 2 G step (batch 32, 64^2, DNA k=5, bce, Adam, float32); us per step over %d steps, one column per round' % args.steps)
    for label, v in times.items():
        say('%-22s %s   median %.1f' % (label, ' '.join('%.1f' % t for t in v), float(np.median(v))))
    off = times['ssim_weight 0']
    say('run-to-run spread of the step without the term (max - min): %.1f us; the term adds %.1f us per step (medians)'
        % (max(off) - min(off), float(np.median(times['ssim_weight 50'])) - float(np.median(off))))
    write(args.out)


if __name__ == '__main__':
    main()
