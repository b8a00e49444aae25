"""GPU: the generator's weight average (include/acgan_ema.h).  Everything is compared BITWISE: the kernels round explicitly and
use no FMA, so tests/ema_ref.py restates them in numpy float32 bit for bit; the optimizer entries that carry the update are
compared with the two launches they replace; a Trainer with the average is compared with the same Trainer without it.

Kernel cases use values of magnitude in [2^-10, 2^7] (ema_ref.kernel_values), for which no intermediate of the update is a
subnormal float32 (tests/test_ema_cpu.py checks exactly these inputs).  A training trajectory offers no such promise: there,
elements for which the restatement reports a subnormal intermediate are compared to 2^-126 absolute instead, and at most 0.01 %
of the elements may be so excused (tests/test_ema_cpu.py confirms the share on a float32 trajectory of the same steps)."""
import ctypes
import json

import numpy as np
import pytest
import torch

import ema_ref as R
from action_conditioned_gans_amd import _lib
from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T
from action_conditioned_gans_amd.saver import Saver

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
DECAY = float(np.float32(0.999))
# the launch grid is min(4096, ceil((n / 4 + 1) / 256)) blocks of 256 threads: only past 4 * 4096 * 256 elements does the grid-stride
# loop of a float4 path run (here for the first blocks, and n % 4 == 3); N_TAIL is for views one float off the 16-byte grid
N_STRIDE = 4 * 4096 * 256 + 2051
N_TAIL = 4096 * 256 + 5


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _ema_state(start):
    return torch.full((1,), start, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)


# ---- kernels ------------------------------------------------------------------------------------------------------------------
def _ema_inputs(n, start):
    """(initial shadow, the parameters of four successive updates) of a kernel case."""
    rng = np.random.default_rng(n + start)
    return R.kernel_values(rng, n), [R.kernel_values(rng, n) for _ in range(4)]


def _ema_sequence(lib, n, start, inputs, offset=0):
    """Four successive acg_ema_update launches -> [shadow after each]; counter, state word and untouched memory are asserted."""
    host, params = inputs
    buf = torch.zeros(n + offset, device=DEV)
    shadow = buf[offset:]
    shadow.copy_(_dev(host))
    count, word = _ema_state(start)
    out = []
    for j, p_host in enumerate(params):
        pbuf = torch.zeros(n + offset, device=DEV)
        pbuf[offset:].copy_(_dev(p_host))
        lib.ema_update(_p(shadow), _p(pbuf[offset:]), n, DECAY, _p(count), _p(word), _stream())
        out.append(shadow.cpu().numpy())
        assert int(count.item()) == start + j + 1 and int(word.item()) == 0
        assert torch.equal(pbuf[offset:], _dev(p_host)), 'the parameters were written'
    assert bool((buf[:offset] == 0).all())
    return out


def _check_against_restatement(n, start, inputs, got):
    host, params = inputs
    for j, p_host in enumerate(params):
        host = R.update(host, p_host, start + j, DECAY)
        diff = int((got[j].view(np.uint32) != host.view(np.uint32)).sum())
        assert diff == 0, 'n %d, counter %d: %d elements differ from the restatement' % (n, start + j, diff)


@pytest.mark.parametrize('n', [1, 3, 4, 5, 255, 257, 4097, 1048579, N_STRIDE])
def test_ema_update_is_the_restatement_bit_for_bit(n):
    lib = _lib.get()
    for start in (0, 1, 2, 8, 8989, 8991, 10 ** 7) if n < N_STRIDE else (0, 8989):          # (the coefficient does not depend on n)
        inputs = _ema_inputs(n, start)
        first = _ema_sequence(lib, n, start, inputs)
        _check_against_restatement(n, start, inputs, first)
        again = _ema_sequence(lib, n, start, inputs)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(first, again)), 'a second sequence gives other bits'


@pytest.mark.parametrize('n', [1, 6, 4097, N_TAIL])
def test_ema_update_on_buffers_off_the_16_byte_grid(n):
    inputs = _ema_inputs(n, 3)
    _check_against_restatement(n, 3, inputs, _ema_sequence(_lib.get(), n, 3, inputs, offset=1))


def test_ema_update_replays_in_a_captured_graph():
    """No memset between replays: the retired-block word resets itself and the counter advances once per launch."""
    lib, n = _lib.get(), 300001
    rng = np.random.default_rng(5)
    host, p_host = R.kernel_values(rng, n), R.kernel_values(rng, n)
    shadow, p = _dev(host), _dev(p_host)
    count, word = _ema_state(0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        lib.ema_update(_p(shadow), _p(p), n, DECAY, _p(count), _p(word), _stream())            # eager: counter 0 -> the copy
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.ema_update(_p(shadow), _p(p), n, DECAY, _p(count), _p(word), _stream())
        lib.ema_update(_p(shadow), _p(p), n, DECAY, _p(count), _p(word), _stream())
    host = R.update(host, p_host, 0, DECAY)
    k = 1
    for _ in range(3):
        p_host = R.kernel_values(rng, n)
        p.copy_(_dev(p_host))
        graph.replay()
        for _ in range(2):
            host = R.update(host, p_host, k, DECAY)
            k += 1
    torch.cuda.synchronize()
    assert int(count.item()) == k == 7 and int(word.item()) == 0
    assert np.array_equal(shadow.cpu().numpy().view(np.uint32), host.view(np.uint32))


def _opt_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    param = (torch.randn(n, generator=g) * 0.02).to(DEV)
    grads = [(torch.randn(n, generator=g) * 0.3).to(DEV) for _ in range(3)]
    return param, grads


def _shifted(t, offset):
    """``t`` as a view ``offset`` floats into an allocation of its own (offset 1: off the 16-byte grid)."""
    buf = torch.zeros(t.numel() + offset, dtype=t.dtype, device=DEV)
    buf[offset:].copy_(t)
    return buf[offset:]


@pytest.mark.parametrize('start', [0, 8989])
@pytest.mark.parametrize('n,offset', [(5, 0), (4097, 0), (1048579, 0), (4097, 1), (N_STRIDE, 0), (N_TAIL, 1)],
                         ids=['5', '4097', '1048579', '4097_off1', str(N_STRIDE), '%d_off1' % N_TAIL])
@pytest.mark.parametrize('clip', [False, True])
@pytest.mark.parametrize('kind', ['adam', 'rmsprop'])
def test_fused_steps_equal_the_two_launches(kind, clip, n, offset, start):
    lib = _lib.get()
    lr, b1, b2, eps, gs = (float(np.float32(v)) for v in (1e-3, 0.9, 0.999, 1e-8, 0.5))
    rlr, rdecay, reps = (float(np.float32(v)) for v in (5e-5, 0.9, 1e-10))
    tail = (gs, 1 if clip else 0, float(np.float32(-0.01)), float(np.float32(0.01)))
    results = []
    for fused in (False, True):
        param, grads = _opt_inputs(n, n + start)
        param, grads = _shifted(param, offset), [_shifted(g, offset) for g in grads]
        s1 = _shifted(torch.zeros(n, device=DEV) if kind == 'adam' else torch.ones(n, device=DEV), offset)
        s2 = _shifted(torch.zeros(n, device=DEV), offset)
        step = torch.zeros(1, dtype=torch.int32, device=DEV)
        shadow = _shifted(_dev(R.kernel_values(np.random.default_rng(n), n)), offset)
        count, word = _ema_state(start)
        for t, g in enumerate(grads):
            step.fill_(t + 1)
            ema = (_p(shadow), DECAY, _p(count), _p(word))
            if kind == 'adam':
                args = (_p(param), _p(g), _p(s1), _p(s2), _p(step), n, lr, b1, b2, eps) + tail
                if fused:
                    lib.adam_step_ema(*args, *ema, _stream())
                else:
                    lib.adam_step(*args, _stream())
            else:
                args = (_p(param), _p(g), _p(s1), n, rlr, rdecay, reps) + tail
                if fused:
                    lib.rmsprop_step_ema(*args, *ema, _stream())
                else:
                    lib.rmsprop_step(*args, _stream())
            if not fused:
                lib.ema_update(_p(shadow), _p(param), n, DECAY, _p(count), _p(word), _stream())
            results.append([x.clone() for x in (param, s1, s2, shadow, count, word)])
    torch.cuda.synchronize()
    half = len(results) // 2
    for t, (two, one) in enumerate(zip(results[:half], results[half:])):
        for name, a, b in zip(('param', 'slot 1', 'slot 2', 'shadow', 'counter', 'state word'), two, one):
            assert torch.equal(a, b) and np.array_equal(_bits(a), _bits(b)), '%s differs after step %d' % (name, t + 1)
    assert int(results[-1][4].item()) == start + 3 and int(results[-1][5].item()) == 0
    if clip:
        assert float(results[-1][0].abs().max()) <= float(np.float32(0.01))
    if start == 0:          # the first update copied the parameter it found, whatever the shadow held
        assert torch.equal(results[0][3], results[0][0])


@pytest.mark.parametrize('n', [1, 3, 5, 255, 257, 4097, 1048579, N_STRIDE])
def test_swap_exchanges_and_two_swaps_restore(n):
    lib = _lib.get()
    rng = np.random.default_rng(n)
    a_host, b_host = R.kernel_values(rng, n), R.kernel_values(rng, n)
    a_host[0], b_host[-1] = np.float32(np.nan), np.float32(-0.0)          # bits move, whatever they mean
    buf = torch.zeros(2 * n + 9, device=DEV)
    off = -(-n // 4) * 4 + 4                      # (both on the 16-byte grid)
    a, b = buf[:n], buf[off:off + n]
    a.copy_(_dev(a_host))
    b.copy_(_dev(b_host))
    lib.swap_f32(_p(a), _p(b), n, _stream())
    assert np.array_equal(_bits(a), b_host.view(np.uint32)) and np.array_equal(_bits(b), a_host.view(np.uint32))
    lib.swap_f32(_p(a), _p(b), n, _stream())
    assert np.array_equal(_bits(a), a_host.view(np.uint32)) and np.array_equal(_bits(b), b_host.view(np.uint32))
    if n > 2:               # off the 16-byte grid
        lib.swap_f32(_p(a[1:]), _p(b[1:]), n - 1, _stream())
        assert np.array_equal(_bits(a)[1:], b_host.view(np.uint32)[1:]) and _bits(a)[0] == a_host.view(np.uint32)[0]


def test_arguments_are_checked():
    lib = _lib.get()
    x, y = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    count, word = _ema_state(0)
    for decay in (0.0, 1.0, -0.5, 2.0):
        with pytest.raises(_lib.AcgError, match='decay'):
            lib.ema_update(_p(x), _p(y), 8, decay, _p(count), _p(word), _stream())
    with pytest.raises(_lib.AcgError, match='ema_update'):
        lib.ema_update(_p(x), _p(y), 0, DECAY, _p(count), _p(word), _stream())
    with pytest.raises(_lib.AcgError, match='ema_update'):
        lib.ema_update(_p(x), _p(y), 8, DECAY, None, _p(word), _stream())
    with pytest.raises(_lib.AcgError, match='overlap'):
        lib.swap_f32(_p(x), _p(x[4:]), 8, _stream())
    with pytest.raises(_lib.AcgError, match='decay'):
        lib.rmsprop_step_ema(_p(x), _p(y), _p(torch.ones(8, device=DEV)), 8, 1e-3, 0.9, 1e-10, 1.0, 0, 0.0, 0.0, _p(y), 1.0, _p(count), _p(word),
                             _stream())
    torch.cuda.synchronize()
    assert int(count.item()) == 0


def test_library_exports_the_ema_table():
    lib = _lib.get()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    assert set(_lib.EXTENSIONS['ema'].signatures) == {'acg_ema_update', 'acg_adam_step_ema', 'acg_rmsprop_step_ema', 'acg_swap_f32'}
    for name in _lib.EXTENSIONS['ema'].signatures:
        assert hasattr(cdll, name) and callable(getattr(lib, name[4:]))
    assert lib.version() == _lib.ABI_VERSION == 8


# ---- the Trainer ----------------------------------------------------------------------------------------------------------------
def _inputs(b=2, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (b, 64, 64, 3)).astype(np.float32)
    y = rng.uniform(-1, 1, (b, 64, 64, 3)).astype(np.float32)
    a = rng.standard_normal((b, 10)).astype(np.float32)
    return x, y, a, a[:, 5:].copy()


def _window(k, b=2, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (b, k + 1, 64, 64, 3)).astype(np.float32), rng.standard_normal((b, k, 10)).astype(np.float32),
            rng.standard_normal((b, k, 5)).astype(np.float32))


def _trainer(dtype='f32', loss='bce', opt='adam', **kw):
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess_kw = {k: kw.pop(k) for k in ('fuse_ema',) if k in kw}
    sess = G.Session(device=DEV, dtype=dtype, **sess_kw)
    tr = T.Trainer(sess, True, loss, opt, True, batch_size=2, **kw)
    sess.run(G.global_variables_initializer())
    return sess, tr


def _flat(sess, tr):
    return sess._materialize(tr.g_vars[0].graph.layout('g')[2])


def _snapshot(sess):
    """Every variable and every named piece of state but the average's own."""
    return {k: sess._materialize(t).detach().clone() for k, t in Saver(sess.graph)._tensors().items() if '/ema/' not in k}


def _warm_up(tr, steps=2):
    x, y, a, s = _inputs()
    frames = [tr.pretrain_g(x, y, a, s)]
    for i in range(steps):
        x, y, a, s = _inputs(seed=i + 1)
        if i % 2:
            tr.train_d(x, y, a, next_g=(x, a))          # the look-ahead call path
        else:
            tr.train_d(x, y, a)
        frames.append(tr.train_g(x, y, a, s))
    return frames


def test_training_with_the_average_is_training_without_it():
    sess, tr = _trainer()
    want_frames, want = _warm_up(tr), _snapshot(sess)
    sess.close()
    sess, tr = _trainer(ema_decay=DECAY)
    got_frames, got = _warm_up(tr), _snapshot(sess)
    assert tr.ema_updates() == 3
    assert set(got) == set(want) and len(want) > 40
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got_frames, want_frames))
    # the stand-alone launch behind the plain step leaves the same average as the fused entry
    fused = sess._materialize(tr.ema.shadow).clone()
    sess.close()
    sess, tr = _trainer(ema_decay=DECAY, fuse_ema=False)
    _warm_up(tr)
    assert torch.equal(sess._materialize(tr.ema.shadow), fused) and tr.ema_updates() == 3
    assert all(torch.equal(v, want[k]) for k, v in _snapshot(sess).items())
    sess.close()


TRAJECTORIES = {
    'bce_adam': dict(),
    'wass_rmsprop': dict(loss='wass', opt='rmsprop'),
    'rollout2': dict(rollout_steps=2, lookahead=False),
    'bf16': dict(dtype='bf16'),
}


@pytest.mark.parametrize('name', list(TRAJECTORIES))
def test_shadow_follows_the_trajectory(name):
    kw = dict(TRAJECTORIES[name])
    sess, tr = _trainer(ema_decay=DECAY, **kw)
    flat = _flat(sess, tr)
    assert flat.dtype == torch.float32 and sess._materialize(tr.ema.shadow).dtype == torch.float32
    trajectory = []
    for _ in range(5):                                   # the eager run, the capture run and three replays of one program
        if kw.get('rollout_steps', 1) > 1:
            tr.train_g_rollout(*_window(2))
        else:
            tr.train_g(*_inputs())
        trajectory.append(flat.detach().cpu().numpy().copy())
    assert not np.array_equal(trajectory[0], trajectory[4])
    want, excused, k = R.fold(trajectory, DECAY)
    got = sess._materialize(tr.ema.shadow).cpu().numpy()
    share = float(excused.mean())
    print('%s: %d of %d elements excused for a subnormal intermediate (%.5f %%)' % (name, int(excused.sum()), excused.size, 100 * share))
    assert tr.ema_updates() == k == 5
    assert share <= 1e-4
    exact = ~excused
    assert np.array_equal(got[exact].view(np.uint32), want[exact].view(np.uint32)), \
        '%d elements differ from the restatement' % int((got[exact].view(np.uint32) != want[exact].view(np.uint32)).sum())
    assert np.all(np.abs(got[excused].astype(np.float64) - want[excused].astype(np.float64)) <= 2.0 ** -126)
    stats = tr.ema_statistics()
    offsets = sess.graph.layout('g')[0]
    assert all(np.array_equal(stats[v.name].reshape(-1), got[offsets[v.name]:offsets[v.name] + v.numel]) for v in tr.g_vars)
    tr.reset_ema()
    tr.train_g_rollout(*_window(2)) if kw.get('rollout_steps', 1) > 1 else tr.train_g(*_inputs())
    assert tr.ema_updates() == 1 and torch.equal(sess._materialize(tr.ema.shadow), flat)          # a counter of 0 seeds
    sess.close()


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_ema_weights_context(dtype):
    x, y, a, s = _inputs(seed=9)
    sess, tr = _trainer(dtype=dtype, ema_decay=0.9)
    with pytest.raises(RuntimeError, match='0 updates'):
        with tr.ema_weights():
            pass
    _warm_up(tr)
    flat, shadow = _flat(sess, tr), sess._materialize(tr.ema.shadow)
    p0, s0 = flat.clone(), shadow.clone()
    assert not torch.equal(p0, s0)
    raw = tr.test(x, y, a)[0]
    with tr.ema_weights():
        assert torch.equal(flat, s0) and torch.equal(shadow, p0)
        inside = tr.test(x, y, a)
        with pytest.raises(RuntimeError, match='already entered'):
            tr.test(x, y, a, weights='ema')
    assert torch.equal(flat, p0) and torch.equal(shadow, s0) and tr.ema_updates() == 3
    assert not np.array_equal(inside[0], raw)
    by_argument = tr.test(x, y, a, weights='ema')
    assert np.array_equal(by_argument[0], inside[0]) and np.array_equal(by_argument[1], inside[1])
    assert np.array_equal(tr.test(x, y, a)[0], raw)                     # and the raw weights (and their bf16 copies) are back
    tr.train_d(x, y, a)
    after = tr.train_g(x, y, a, s)
    after_flat, after_shadow = flat.clone(), shadow.clone()
    sess.close()
    # a fresh session whose variables were set to that average predicts the same frames
    sess, tr = _trainer(dtype=dtype)
    _flat(sess, tr).copy_(s0)
    sess._weights_dirty = True
    fresh = tr.test(x, y, a)
    assert np.array_equal(fresh[0], inside[0]) and np.array_equal(fresh[1], inside[1])
    sess.close()
    # a run that never entered the context takes the same next step
    sess, tr = _trainer(dtype=dtype, ema_decay=0.9)
    _warm_up(tr)
    tr.test(x, y, a)
    tr.train_d(x, y, a)
    assert np.array_equal(tr.train_g(x, y, a, s), after)
    assert torch.equal(_flat(sess, tr), after_flat) and torch.equal(sess._materialize(tr.ema.shadow), after_shadow)
    sess.close()


def test_checkpoints(tmp_path):
    def iterate(tr, first, n):
        for i in range(first, first + n):
            x, y, a, s = _inputs(seed=20 + i)
            tr.train_d(x, y, a)
            tr.train_g(x, y, a, s)
    sess, tr = _trainer(ema_decay=DECAY)
    iterate(tr, 0, 3)
    Saver().save(sess, str(tmp_path / 'three'))
    iterate(tr, 3, 2)
    want, want_flat = sess._materialize(tr.ema.shadow).clone(), _flat(sess, tr).clone()
    assert tr.ema_updates() == 5
    sess.close()
    sess, tr = _trainer(ema_decay=DECAY)
    Saver().restore(sess, str(tmp_path / 'three'))
    assert tr.ema_updates() == 3
    iterate(tr, 3, 2)
    assert tr.ema_updates() == 5
    assert torch.equal(_flat(sess, tr), want_flat) and torch.equal(sess._materialize(tr.ema.shadow), want)
    sess.close()
    # an EMA checkpoint restores into a plain graph, which trains on as the EMA run did
    sess, tr = _trainer()
    Saver().restore(sess, str(tmp_path / 'three'))
    iterate(tr, 3, 2)
    assert torch.equal(_flat(sess, tr), want_flat)
    Saver().save(sess, str(tmp_path / 'plain'))
    assert not any('/ema/' in k for k in np.load(str(tmp_path / 'plain.npz')).files)
    sess.close()
    # a checkpoint from before the average restores into a graph with it: count 0, and the first update seeds the shadow
    sess, tr = _trainer(ema_decay=DECAY)
    Saver().restore(sess, str(tmp_path / 'plain'))
    assert tr.ema_updates() == 0 and torch.equal(_flat(sess, tr), want_flat)
    iterate(tr, 5, 1)
    assert tr.ema_updates() == 1 and torch.equal(sess._materialize(tr.ema.shadow), _flat(sess, tr))
    sess.close()


# ---- the CLIs ----------------------------------------------------------------------------------------------------------------
def test_cli_train_then_evaluate_with_the_average(tmp_path):
    out = tmp_path / 'run'
    # (checkpoints are written every 100 iterations: model100 holds an average of 101 updates, which is no longer the weights)
    T.main(['synthetic', str(out), '--adv', 'True', '--dna', '--g_ema', '0.99', '--batch_size', '4', '--pretrain_iter', '0', '--train_iter', '101'])
    rec = [json.loads(line) for line in open(out / 'logs' / 'train.jsonl')]
    assert rec and all(r['g_ema'] == 0.99 for r in rec)
    ev = [json.loads(line) for line in open(out / 'logs' / 'test.jsonl')]
    assert ev and all(len(r['rollout_psnr_ema']) == len(r['rollout_psnr']) and np.isfinite(r['rollout_ssim_ema']).all() for r in ev)
    saved = np.load(str(out / 'models' / 'model100.npz'))
    assert int(saved['state:g/ema/num_updates'][0]) == 101 and saved['state:g/ema/shadow'].dtype == np.float32
    common = [str(out / 'models'), 'synthetic', None, '--dna', '--num_sequences', '8', '--batch_size', '4', '--samples', '0']
    res = {}
    for weights in ('raw', 'ema'):
        common[2] = str(tmp_path / ('ev_' + weights))
        E.main(common + ['--weights', weights])
        res[weights] = json.load(open(tmp_path / ('ev_' + weights) / 'metrics.json'))
    assert res['ema']['weights'] == 'ema' and res['ema']['ema_updates'] == 101
    assert 'weights' not in res['raw'] and 'ema_updates' not in res['raw']
    assert np.isfinite(res['ema']['ssim']).all() and np.isfinite(res['ema']['psnr']).all()
    assert res['ema']['psnr'] != res['raw']['psnr'] and res['ema']['ssim'] != res['raw']['ssim']
    assert res['ema']['identity_psnr'] == res['raw']['identity_psnr']
    # calibrated statistics of the averaged weights; the checkpoint it writes restores to the same weights again
    common[2] = str(tmp_path / 'ev_cal')
    cal = E.main(common + ['--weights', 'ema', '--bn_stats', 'calibrate', '--calibrate_batch_size', '8', '--calibrate_batches', '2'])
    assert cal['weights'] == 'ema' and cal['bn_statistics'] == 'calibrate' and np.isfinite(cal['psnr']).all()
    written = np.load(str(tmp_path / 'ev_cal' / 'calibrated.npz'))
    shadow = written['state:g/ema/shadow']
    assert int(written['state:g/ema/num_updates'][0]) == 101 and np.array_equal(shadow, saved['state:g/ema/shadow'])
    w = written['var:g/conv1/weights']
    assert np.array_equal(w.reshape(-1), shadow[:w.size])                      # the first variable of the layout
    common[0], common[2] = str(tmp_path / 'ev_cal' / 'calibrated'), str(tmp_path / 'ev_again')
    again = E.main(common + ['--weights', 'ema', '--bn_stats', 'stored'])
    assert again['psnr'] == cal['psnr'] and again['ssim'] == cal['ssim']


def test_cli_evaluate_rejects_a_checkpoint_without_the_average(tmp_path):
    out = tmp_path / 'run'
    T.main(['synthetic', str(out), '--adv', 'True', '--dna', '--batch_size', '4', '--pretrain_iter', '0', '--train_iter', '1'])
    assert 'g_ema' not in json.loads(open(out / 'logs' / 'train.jsonl').readline())
    with pytest.raises(ValueError, match='model0'):
        E.main([str(out / 'models'), 'synthetic', str(tmp_path / 'ev'), '--dna', '--num_sequences', '4', '--batch_size', '4', '--weights', 'ema'])
    assert not (tmp_path / 'ev' / 'metrics.json').exists()
