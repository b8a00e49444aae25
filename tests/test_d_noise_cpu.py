"""Instance noise on the discriminator's inputs and the D statistics without a GPU: the restatement's known answers
(tests/d_noise_ref.py), the binding and the header, the graph with the arguments off and on, every refusal of the Trainer, train()
and the CLI, and the clear error on the C oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import d_noise_ref as R
import noise_ref as NR
from action_conditioned_gans_amd import _lib
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import ops as O
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import train as T
from action_conditioned_gans_amd.saver import Saver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('acg_inst_noise_prepare', 'acg_inst_noise_add', 'acg_logit_stats')
STATS = ['d_fake_acc', 'd_fake_logit', 'd_real_acc', 'd_real_logit']


# ---- the restatement
def test_sigma_known_answers():
    # 1.0 -> 0.25 over 4 positions behind an offset of 2
    got = [float(R.sigma(k, 1.0, 0.25, 2, 4)) for k in range(9)]
    assert got == [1.0, 1.0, 1.0, 0.8125, 0.625, 0.4375, 0.25, 0.25, 0.25]
    assert R.sigma(2, 1.0, 0.25, 2, 4) == np.float32(1.0)                       # at the offset
    assert R.sigma(4, 1.0, 0.25, 2, 4) == np.float32(0.625)                     # mid-decay
    assert R.sigma(10 ** 12, 1.0, 0.25, 2, 4) == np.float32(0.25)               # past the end
    assert R.sigma(10 ** 12, 0.3, 0.9, 5, 0) == np.float32(0.3)                 # decay_steps = 0: constant, the float32 level
    assert R.sigma(3, 0.1, 0.5, 0, 2) == np.float32(0.5)                        # a rising schedule clamps too
    assert R.sigma(1, 0.1, 0.0, 0, 3).dtype == np.float32
    # float64 from the float32 levels: 0.1f + (0 - 0.1f) / 3, rounded to float32 once
    s = np.float64(np.float32(0.1))
    assert R.sigma(1, 0.1, 0.0, 0, 3) == np.float32(s + (0.0 - s) * (np.float64(1.0) / np.float64(3.0)))


def test_prepare_protocol():
    key, sig, state, updates = R.prepare((7, 2 ** 64 - 1), 3, 1.0, 0.0, 1, 4, 1)
    assert key == (7, 2 ** 64 - 1) and sig == np.float32(0.5) and state == (7, 0) and updates == 4
    key, sig, state, updates = R.prepare((7, 5), 3, 1.0, 0.0, 1, 4, 0)
    assert key == (7, 5) and state == (7, 6) and updates == 3


def test_lane_and_block_mapping():
    """z(p, l) is lane l of Philox block p under the tagged stream word: written out against the generator itself."""
    key, sid = (0x123456789abcdef, 2 ** 32 + 5), 66
    ctr = np.array([[5, 1, p, sid ^ R.STREAM_TAG] for p in range(6)], np.uint32)
    x = NR.philox4x32_10(ctr, np.array([key[0] & NR.MASK, key[0] >> 32], np.uint32))
    u = ((x >> 9).astype(np.float64) + 0.5) * 2.0 ** -23
    r0, r1 = np.sqrt(-2 * np.log(u[:, 0])), np.sqrt(-2 * np.log(u[:, 2]))
    want = np.stack([r0 * np.cos(2 * np.pi * u[:, 1]), r0 * np.sin(2 * np.pi * u[:, 1]), r1 * np.cos(2 * np.pi * u[:, 3]),
                     r1 * np.sin(2 * np.pi * u[:, 3])], axis=1)
    assert np.array_equal(R.z(key, sid, 6), want)
    assert np.array_equal(R.z(key, sid, 6, 3), want[:, :3]) and np.array_equal(R.z(key, sid, 4, 2), want[:4, :2])     # prefixes
    # apart from the generator's noise stream of the same seed, counter and stream id, from another stream id and another counter
    assert not np.array_equal(R.z(key, sid, 6).reshape(-1), NR.normals(key[0], key[1], sid, 24))
    assert not np.isclose(R.z(key, sid, 6), R.z(key, sid + 1, 6)).any()
    assert not np.isclose(R.z(key, sid, 6), R.z((key[0], key[1] + 1), sid, 6)).any()


def test_add_and_rounding_of_the_restatement():
    x = np.arange(40, dtype=np.float64).reshape(5, 8)
    out = R.add(x, (1, 2), 0.5, 3, 3, 0)
    keep = [0, 1, 2, 6, 7]
    assert np.array_equal(out[:, keep], x[:, keep]) and np.array_equal(out[:, 3:6], x[:, 3:6] + np.float64(0.5) * R.z((1, 2), 0, 5, 3))
    assert np.array_equal(R.add(x, (1, 2), 0.0, 3, 3, 0), x)
    v = np.array([1.0, 1.00390625, 1.01171875, -3.0e38, 1e-3])         # 1 + 2^-8 is a tie (to even: 1), 1 + 3 * 2^-8 a tie (to 1 + 2^-6)
    got = R.round_bf16(v)
    assert np.array_equal(got[:3], [1.0, 1.0, 1.015625])
    assert np.array_equal(got, torch.tensor(v, dtype=torch.float64).to(torch.float32).to(torch.bfloat16).double().numpy())
    assert np.allclose(R.logit_stats([-1.0, 0.0, 2.0, -0.5], [1.0, 0.0, -2.0, 3.0]), [0.125, 0.5, 0.5, 0.5])


# ---- the binding
def test_binding_header_and_abi():
    sigs = _lib.EXTENSIONS['rollout'].signatures
    header = open(os.path.join(ROOT, 'include', 'acgan_rollout.h')).read()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in sigs and sigs[name][0] is _lib.STATUS, name             # a status, not a value
        assert re.search(r'int32_t %s\(' % name, code), name
        assert hasattr(cdll, name), name
        assert not any(name in ext.signatures for key, ext in _lib.EXTENSIONS.items() if key != 'rollout') and name not in _lib.SIGNATURES
    assert len(sigs['acg_inst_noise_prepare'][1]) == 10 and len(sigs['acg_inst_noise_add'][1]) == 12 and len(sigs['acg_logit_stats'][1]) == 5
    assert re.search(r'#define ACG_DN_STREAM_TAG 0x%08Xu' % R.STREAM_TAG, code)
    assert _lib.ABI_VERSION == 8 and re.search(r'#define ACG_ABI_VERSION 8\b', open(os.path.join(ROOT, 'include', 'acgan_hip.h')).read())
    assert list(_lib.EXTENSIONS) == ['metrics', 'cdna', 'rollout', 'bn_infer', 'ema', 'ssim_loss', 'conv_plan']         # no new key
    assert set(os.listdir(os.path.join(ROOT, 'include'))) == {os.path.basename(e.header) for e in _lib.EXTENSIONS.values()} | {'acgan_hip.h'}    # no new header
    lib = _lib.get()
    assert all(callable(getattr(lib, n[4:])) for n in ENTRIES)
    assert O.INST_NOISE_SLOTS == R.SLOTS


# ---- Trainer
def _trainer(transform=True, adv=True, dtype='f32', **kw):
    from oracle import cbind
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cpu', lib=cbind.load(), dtype=dtype) if dtype == 'f32' else None
    if sess is None:                                   # a bf16 graph is built, never run, without a GPU
        G.get_default_graph().act_dtype = torch.bfloat16
    tr = T.Trainer(sess, adv, 'bce', 'adam', transform, batch_size=2, **kw)
    return sess, tr, G.get_default_graph()


def _describe(g, tr):
    return ([(type(o).__name__, o.name, o.index, [t.shape for t in o.outputs]) for o in g.ops],
            [(n, v.shape) for n, v in g.variables.items()], [(s.name, s.shape, s.dtype, s.init) for s in g.state],
            sorted(Saver()._tensors()), list(tr._summary_names), sorted(g.collections))


OFF = dict(d_noise=0.0, d_noise_final=0.7, d_noise_decay_steps=9, d_noise_offset=2, d_noise_seed=5, d_stats=False)


@pytest.mark.parametrize('transform,batched', [(False, True), (True, True), (True, False), ('cdna', True)], ids=str)
def test_off_builds_the_graph_it_always_built(transform, batched):
    _, tr, g = _trainer(transform, batched_d=batched)
    a = _describe(g, tr)
    _, tr, g = _trainer(transform, batched_d=batched, **OFF)
    assert _describe(g, tr) == a
    assert tr.d_noise is None and tr.lookahead == batched and 'inst_noise' not in g.collections
    assert not any(isinstance(o, (O.InstNoisePrepareOp, O.InstNoiseOp, O.LogitStatsOp)) for o in g.ops)
    for call in (tr.d_noise_last, tr.d_noise_state):
        with pytest.raises(RuntimeError, match='d_noise'):
            call()


def _program(fetches):
    seen, stack = {}, [f if isinstance(f, G.Op) else (f.tensor() if hasattr(f, 'tensor') else f).op for f in fetches]
    while stack:
        op = stack.pop()
        if op is None or id(op) in seen:
            continue
        seen[id(op)] = op
        stack.extend(t.op for t in op.inputs)
        stack.extend(op.control_inputs)
    return seen


@pytest.mark.parametrize('transform,batched,dtype', [(True, True, 'f32'), (False, True, 'f32'), (True, False, 'f32'), ('cdna', True, 'f32'),
                                                     (True, True, 'bf16')], ids=str)
def test_on_adds_two_checkpoint_keys_and_no_variable_or_slot(transform, batched, dtype):
    _, tr0, g0 = _trainer(transform, batched_d=batched, dtype=dtype, lookahead=False)
    base = _describe(g0, tr0)
    _, tr, g = _trainer(transform, batched_d=batched, dtype=dtype, d_noise=0.5, d_noise_final=0.125, d_noise_decay_steps=10, d_noise_offset=3,
                        d_noise_seed=2 ** 64 - 2)
    got = _describe(g, tr)
    assert got[1] == base[1] and got[4] == base[4]                            # variables and summaries
    assert sorted(set(got[3]) - set(base[3])) == ['state:d/inst_noise/state', 'state:d/inst_noise/updates'] and set(base[3]) <= set(got[3])
    new = [s for s in got[2] if s not in base[2]]
    assert new == [('d/inst_noise/state', (2,), torch.int64, (-2, 0)), ('d/inst_noise/updates', (1,), torch.int64, 0)]     # the seed keeps its bits
    assert not tr.lookahead and tr.d_noise == {'start': 0.5, 'final': 0.125, 'decay_steps': 10, 'offset': 3, 'seed': 2 ** 64 - 2}
    preps = [o for o in g.ops if isinstance(o, O.InstNoisePrepareOp)]
    adds = [o for o in g.ops if isinstance(o, O.InstNoiseOp)]
    assert len(preps) == 1 and preps[0].sched == (0.5, 0.125, 3, 10) and preps[0].advance_schedule is tr.d_opt_op
    assert [t.dtype for t in preps[0].outputs] == [torch.int64, torch.float32] and all(t not in g.state for t in preps[0].outputs)
    assert sorted(o.slot for o in adds) == ([0, 2] if batched else [0, 1]) and all((o.c0, o.cn) == (3, 3) for o in adds)
    for o in adds:
        x, y = o.inputs[0], o.outputs[0]
        assert (y.shape, y.dtype, y.valid_c) == (x.shape, x.dtype, 6) and x.shape[-1] == 8 and y is not x
        assert y.dtype == (torch.bfloat16 if dtype == 'bf16' else torch.float32)
        assert o.inputs[1] is preps[0].key and o.inputs[2] is preps[0].sigma
    # every program that runs D holds the one prepare and its own instances' adds; pretraining holds none
    by_slot = {o.slot: o for o in adds}
    for fetches, slots in (([tr.d_opt_op], [2] if batched else [0, 1]), ([tr.g_opt_op], [0]), ([tr.g_pretrain_opt_op], []),
                           (tr.merged_summaries, sorted(by_slot))):
        prog = _program(fetches)
        assert sorted(s for s, o in by_slot.items() if id(o) in prog) == slots
        assert (id(preps[0]) in prog) == bool(slots)
    # the schedule advances with D's optimizer step and with nothing else (decided when a program is bound)
    rt = G.Runtime(type('Lib', (), {'inst_noise_prepare': staticmethod(lambda *a: seen.append(a))})(), 'cpu')
    for t in preps[0].outputs + preps[0].extras:
        t.buf = torch.zeros(t.shape, dtype=t.dtype)
    for fetches, advance in (([tr.d_opt_op], 1), ([tr.g_opt_op], 0), (tr.merged_summaries, 0), ([tr.d_opt_op] + tr.merged_summaries, 1)):
        seen = []
        rt.program_ops = frozenset(_program(fetches))
        preps[0].bind(rt)(None)
        assert seen[0][4:9] == (0.5, 0.125, 3, 10, advance), (fetches, seen)


def test_the_gradient_is_the_incoming_tensor():
    G.reset_default_graph()
    x = G.placeholder((2, 4, 4, 6), name='x', channel_pitch=8)
    prep = O.InstNoisePrepareOp(1.0, 0.0, 4, 0, 1, 'prep')
    op = O.InstNoiseOp(x, prep.key, prep.sigma, 3, 3, 5, 'noisy')
    y = op.outputs[0]
    assert y.shape == (2, 4, 4, 8) and y.valid_c == 6 and y.op is op
    gy = G.placeholder((2, 4, 4, 8), name='gy')
    got = op.grad([gy], [True, False, False], None)
    assert got[0] is gy and got[1:] == [None, None]
    assert op.grad([gy], [False, False, False], None) == [None, None, None]
    n_ops = len(G.get_default_graph().ops)
    for bad in (dict(c0=4, cn=3), dict(c0=0, cn=5), dict(c0=-1, cn=2), dict(c0=0, cn=0), dict(c0=3, cn=3, stream_id=64), dict(c0=3, cn=3, stream_id=-1)):
        kw = dict(dict(c0=3, cn=3, stream_id=0), **bad)
        with pytest.raises(ValueError, match='inst_noise'):
            O.InstNoiseOp(x, prep.key, prep.sigma, kw['c0'], kw['cn'], kw['stream_id'], 'bad')
    with pytest.raises(ValueError, match='inst_noise'):
        O.InstNoiseOp(G.placeholder((2, 3), name='i', dtype=torch.int32), prep.key, prep.sigma, 0, 1, 0, 'bad')
    for bad in ((-1.0, 0.0, 0, 0), (1.0, float('inf'), 0, 0), (float('nan'), 0.0, 0, 0), (1.0, 0.0, -1, 0), (1.0, 0.0, 0, -1)):
        with pytest.raises(ValueError, match='inst_noise_prepare'):
            O.InstNoisePrepareOp(bad[0], bad[1], bad[2], bad[3], 1, 'bad')
    assert len(G.get_default_graph().ops) == n_ops


@pytest.mark.parametrize('batched', [True, False], ids=['batched', 'two_instances'])
def test_d_stats_adds_four_summaries_and_sigma_with_noise(batched):
    _, tr0, g0 = _trainer(batched_d=batched)
    _, tr, g = _trainer(batched_d=batched, d_stats=True)
    assert sorted(set(tr._summary_names) - set(tr0._summary_names)) == STATS and set(tr0._summary_names) <= set(tr._summary_names)
    assert sorted(Saver()._tensors()) == sorted(Saver(g0)._tensors())          # no state
    assert tr.lookahead == batched
    stats = [o for o in g.ops if isinstance(o, O.LogitStatsOp)]
    assert len(stats) == 1 and stats[0].inputs[1] is tr.d_out_real and stats[0].inputs[0].numel == tr.d_out_real.numel == 2 * 2 * 2
    assert stats[0].inputs[0].root() is (tr.d_out_both if batched else tr.d_out_gen).root()
    # the statistics never reach a training program unless asked for
    assert id(stats[0]) not in _program([tr.d_opt_op]) and id(stats[0]) in _program(tr.merged_summaries)
    _, tr, g = _trainer(batched_d=batched, d_stats=True, d_noise=0.25)
    assert sorted(set(tr._summary_names) - set(tr0._summary_names)) == sorted(STATS + ['d_noise_sigma'])
    assert tr.summaries['d_noise_sigma'] is tr._d_noise_prep.sigma
    _, tr, g = _trainer(batched_d=batched, d_noise=0.25)
    assert tr._summary_names == tr0._summary_names


REFUSED = [dict(d_noise=0.5, rollout_steps=2), dict(d_noise=-0.5), dict(d_noise=float('nan')), dict(d_noise=float('inf')), dict(d_noise=1e39),
           dict(d_noise=1e-50), dict(d_noise=True), dict(d_noise='x'), dict(d_noise=None),
           dict(d_noise=0.5, d_noise_final=-1e-3), dict(d_noise=0.5, d_noise_final=float('nan')), dict(d_noise=0.5, d_noise_final=float('inf')),
           dict(d_noise_final=-1.0), dict(d_noise=0.5, d_noise_decay_steps=-1), dict(d_noise=0.5, d_noise_decay_steps=2.5),
           dict(d_noise=0.5, d_noise_offset=-1), dict(d_noise=0.5, d_noise_offset=True), dict(d_noise=0.5, d_noise_seed=-1),
           dict(d_noise=0.5, d_noise_seed=2 ** 64), dict(d_noise_seed=1.5)]


@pytest.mark.parametrize('kw', REFUSED + [dict(d_noise=0.5, arg_adv=False)], ids=str)
def test_trainer_refusals_leave_the_graph_alone(kw):
    G.reset_default_graph()
    optim.set_data_parallel(1)
    g = G.get_default_graph()
    kw = dict(kw)
    adv = kw.pop('arg_adv', True)
    with pytest.raises(ValueError, match='d_noise'):
        T.Trainer(None, adv, 'bce', 'adam', True, batch_size=2, **kw)
    assert not g.ops and not g.variables and not g.state and 'inst_noise' not in g.collections


def test_state_accessors_on_the_host_and_a_checkpoint_without_the_keys(tmp_path):
    sess, tr0, g0 = _trainer()
    sess.run(G.global_variables_initializer())
    old = Saver().save(sess, str(tmp_path / 'old'))                            # a checkpoint of a run without the arguments
    sess, tr, g = _trainer(d_noise=0.5, d_noise_seed=2 ** 63 + 5)
    sess.run(G.global_variables_initializer())
    assert tr.d_noise_state() == (2 ** 63 + 5, 0, 0)
    assert tr.d_noise_last() == {'sigma': 0.0, 'key': (0, 0)}
    state, updates = O.inst_noise_state()
    O.write_draw_state(sess._materialize(state), 2 ** 64 - 1, 17)
    sess._materialize(updates).fill_(9)
    path = Saver().save(sess, str(tmp_path / 'new'))
    saved = np.load(path)
    assert [int(v) % 2 ** 64 for v in saved['state:d/inst_noise/state']] == [2 ** 64 - 1, 17] and saved['state:d/inst_noise/updates'].tolist() == [9]
    sess.run(G.global_variables_initializer())
    assert tr.d_noise_state() == (2 ** 63 + 5, 0, 0)
    Saver().restore(sess, path)
    assert tr.d_noise_state() == (2 ** 64 - 1, 17, 9)
    sess.run(G.global_variables_initializer())
    Saver().restore(sess, old)                                                 # starts at 0
    assert tr.d_noise_state() == (2 ** 63 + 5, 0, 0)


@pytest.mark.parametrize('batched', [True, False], ids=['batched', 'two_instances'])
def test_the_c_oracle_raises_a_clear_error(batched):
    sess, tr, _ = _trainer(batched_d=batched, d_noise=0.5)
    sess.run(G.global_variables_initializer())
    x, a = np.zeros((2, 64, 64, 3), np.float32), np.zeros((2, 10), np.float32)
    for step in (lambda: tr.train_d(x, x, a), lambda: tr.train_g(x, x, a, np.zeros((2, 5), np.float32))):
        with pytest.raises(_lib.AcgError, match=r'acg_inst_noise_prepare \(include/acgan_rollout\.h\)'):
            step()
    sess.run(tr.g_pretrain_opt_op, tr._feed(x, x, a, np.zeros((2, 5), np.float32)))       # runs no D: nothing of the noise is asked for
    sess, tr, _ = _trainer(batched_d=batched, d_stats=True)
    sess.run(G.global_variables_initializer())
    tr.train_d(x, x, a)                                                        # the statistics are summaries: not in this program
    with pytest.raises(_lib.AcgError, match=r'acg_logit_stats \(include/acgan_rollout\.h\)'):
        tr.train_d(x, x, a, summarize=True)


# ---- train() and the CLI
def test_cli_passes_the_flags_on(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(T, 'train', lambda *a, **kw: seen.update(kw))
    T.main(['synthetic', str(tmp_path / 'out'), '--adv', 'True', '--dna', '--d_noise', '0.5', '--d_noise_final', '0.05', '--d_noise_decay_iters', '500',
            '--d_noise_seed', '12345678901234567890', '--log_d_stats'])
    assert (seen['d_noise'], seen['d_noise_final'], seen['d_noise_decay_steps'], seen['d_noise_seed'], seen['d_stats']) == \
        (0.5, 0.05, 500, 12345678901234567890, True)
    assert 'd_noise_decay_iters' not in seen and 'log_d_stats' not in seen
    T.main(['synthetic', str(tmp_path / 'out2')])
    assert (seen['d_noise'], seen['d_noise_final'], seen['d_noise_decay_steps'], seen['d_noise_seed'], seen['d_stats']) == (0.0, 0.0, 0, 0, False)
    T.main(['synthetic', str(tmp_path / 'out3'), '--log_d_stats', 'True'])     # the statistics alone need no --adv
    assert seen['d_stats'] is True and seen['d_noise'] == 0.0


@pytest.mark.parametrize('extra', [['--d_noise', '0.5'],                                                          # no --adv
                                   ['--adv', 'True', '--d_noise', '0.5', '--rollout_steps', '2'],
                                   ['--adv', 'True', '--d_noise', '-0.5'],
                                   ['--adv', 'True', '--d_noise', 'nan'],
                                   ['--adv', 'True', '--d_noise', 'inf'],
                                   ['--adv', 'True', '--d_noise', '0.5', '--d_noise_final', '-1'],
                                   ['--adv', 'True', '--d_noise', '0.5', '--d_noise_final', 'inf'],
                                   ['--adv', 'True', '--d_noise', '0.5', '--d_noise_decay_iters', '-2'],
                                   ['--adv', 'True', '--d_noise', '0.5', '--d_noise_decay_iters', '2.5'],
                                   ['--adv', 'True', '--d_noise', '0.5', '--d_noise_seed', '-1'],
                                   ['--adv', 'True', '--d_noise', '0.5', '--d_noise_seed', str(2 ** 64)],
                                   ['--adv', 'True', '--d_noise_final', 'nan']], ids=str)
def test_cli_rejections_create_nothing(tmp_path, monkeypatch, capsys, extra):
    monkeypatch.setattr(T, 'train', lambda *a, **kw: pytest.fail('train() reached'))
    with pytest.raises(SystemExit):
        T.main(['synthetic', str(tmp_path / 'out'), '--dna'] + extra)
    assert 'd_noise' in capsys.readouterr().err
    assert not (tmp_path / 'out').exists()


def test_train_converts_iterations_to_d_updates_and_passes_nothing_when_off(monkeypatch):
    G.reset_default_graph()
    g = G.get_default_graph()
    for kw in (dict(d_noise=0.5, rollout_steps=2), dict(d_noise=-1.0), dict(d_noise=0.5, d_noise_decay_steps=-1), dict(d_noise=0.5, arg_adv=False)):
        kw = dict(kw)
        adv = kw.pop('arg_adv', True)
        with pytest.raises(ValueError, match='d_noise'):
            T.train('synthetic', None, None, None, None, adv, 'bce', 'adam', True, batch_size=2, train_iter=1, seq_len=4, **kw)
    assert G.get_default_graph() is g and not g.ops
    seen = {}

    class NoSession:                             # train() up to its loop: what the loop is handed is the point
        def __init__(self, **kw):
            self.rt = self

        def check_exchange_flags(self):
            pass

    monkeypatch.setattr(G, 'Session', NoSession)
    monkeypatch.setattr(T, '_train_loop', lambda *a, **kw: seen.update(kw))
    noise = lambda: {k: v for k, v in seen['options'].items() if k.startswith('d_noise') or k == 'd_stats'}     # noqa: E731
    T.train('synthetic', None, None, None, None, True, 'wass', 'rmsprop', True, batch_size=2, train_iter=9, pretrain_iter=7, d_noise=0.5,
            d_noise_final=0.1, d_noise_decay_steps=40, d_noise_seed=5, d_stats=True)
    assert noise() == {'d_noise': 0.5, 'd_noise_final': 0.1, 'd_noise_decay_steps': 200, 'd_noise_seed': 5, 'd_stats': True}      # wass: 5 D steps
    T.train('synthetic', None, None, None, None, True, 'bce', 'adam', True, batch_size=2, train_iter=9, n_critic=3, d_noise=0.5, d_noise_decay_steps=40)
    assert noise() == {'d_noise': 0.5, 'd_noise_final': 0.0, 'd_noise_decay_steps': 120, 'd_noise_seed': 0}
    T.train('synthetic', None, None, None, None, True, 'bce', 'adam', True, batch_size=2, train_iter=9, d_noise_final=0.3, d_noise_decay_steps=4)
    assert noise() == {}                         # nothing at all with the noise and the statistics off
