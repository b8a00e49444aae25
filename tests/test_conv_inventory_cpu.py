"""CPU half of tests/test_gpu_conv_inventory.py: the inventory helper (tests/conv_inventory.py) on a C-oracle session yields the
descriptors the model's layers must have at per-GPU size - generator layers at batch B and at 2 B (the look-ahead pair
instance, train.py Trainer(lookahead=True)), discriminator layers at 2 B (D on [fake ; real]) and B (D(fake) in the G step),
the 16-byte gather pitches and the dgrad_c / adj_dgrad_c limits of the action-concatenated maps.  The descriptors do not depend
on the library; the paths do (those are checked on the GPU)."""
import ctypes

import pytest

import conv_inventory as CI
from oracle import cbind

from action_conditioned_gans_amd import _lib as L
from action_conditioned_gans_amd import graph as G


def _expected(cfg):
    """name -> (transposed, in_h as a divisor of the image size, in_c, out_c, k, stride): acg_conv_desc (the adjoint for a
    transposed layer) of every conv / deconv layer (models.py), the state head aside."""
    c = CI.CONFIGS[cfg]
    kk = c['ksize'] ** 2
    if c['dna']:
        g = {'g/conv1': (False, 1, 3, 32, 5, 2), 'g/conv2': (False, 2, 32, 64, 5, 2), 'g/conv3': (False, 4, 64, 128, 5, 2),
             'g/conv4': (False, 8, 128, 256, 5, 2), 'g/tconv1': (True, 8, 128, 266, 5, 2), 'g/tconv2': (True, 4, 128, 128, 5, 2),
             'g/tconv3': (True, 2, 128, 128, 5, 2), 'g/tconv4': (True, 1, kk, 128, 5, 2)}
    else:
        g = {'g/conv1': (False, 1, 3, 64, 5, 2), 'g/conv2': (False, 2, 64, 128, 5, 2), 'g/conv3': (False, 4, 128, 256, 5, 2),
             'g/conv4': (False, 8, 256, 512, 5, 2), 'g/tconv1': (True, 8, 256, 522, 5, 2), 'g/tconv2': (True, 4, 128, 256, 5, 2),
             'g/tconv3': (True, 2, 64, 128, 5, 2), 'g/tconv4': (True, 1, 3, 64, 5, 2)}
    d = {'d/conv1': (False, 1, 6, 64, 5, 2), 'd/conv2': (False, 2, 64, 128, 5, 2), 'd/conv3': (False, 4, 138, 128, 5, 2),
         'd/conv4': (False, 8, 128, 256, 5, 2), 'd/conv5': (False, 16, 256, 512, 5, 2), 'd/conv6': (False, 32, 512, 1, 2, 1)}
    return dict(g, **d)


def _layer(opname):
    return '/'.join(opname.split('/')[:2])


@pytest.mark.parametrize('cfg', list(CI.CONFIGS))
def test_inventory_descriptors_on_the_oracle(cfg, monkeypatch):
    inv, sess, tr = CI.record(monkeypatch, lambda **kw: G.Session(device='cpu', lib=cbind.load(), **kw), cfg)
    c = CI.CONFIGS[cfg]
    B, S, half = c['batch'], c['img'], c['dtype'] == 'bf16'
    want = _expected(cfg)
    lib = cbind.load()
    seen = {}
    assert inv.entries and inv.reduces
    for e in inv.entries.values():
        d = L.ConvDesc(*e['desc'])
        for op in e['ops']:
            name = _layer(op)
            seen.setdefault((name, e['role']), set()).add(d.batch)
            if name not in want:
                assert name.startswith('g/sconv'), op
                continue
            transposed, div, cin, cout, k, s = want[name]
            tag = '%s %s %s' % (cfg, op, CI.describe(e))
            assert e['transposed'] == transposed, tag
            # the rest of the descriptor is what acg_conv_desc_init makes of the layer's arguments (SAME padding)
            ref = L.ConvDesc()
            lib.conv_desc_init(ctypes.byref(ref), d.batch, S // div, S // div, cin, k, k, cout, s, 1)
            assert d.key()[:13] == ref.key()[:13], tag
            pitch_in, pitch_out = {'g/conv1': ((8 if half else 4), 0), 'd/conv1': (8, 0), 'd/conv3': ((0 if half else 140), 0)}.get(name, (0, 0))
            if name == 'g/tconv1':
                pitch_out = 0 if half else (268 if c['dna'] else 524)
            assert (d.in_pitch, d.out_pitch) == (pitch_in, pitch_out) or (half and (d.in_pitch, d.out_pitch) == (0, 0)), tag
            # only the first 128 / 256 channels of the action-concatenated maps have a reader (ConcatActionsOp.grad)
            assert d.dgrad_c == (128 if name == 'd/conv3' else 0), tag
            if e['role'] == 'dgrad' and name == 'g/tconv1' and c['dna'] and d.batch == B:
                assert d.adj_dgrad_c == 256, tag
            elif e['role'] == 'dgrad' or d.batch != B:
                assert d.adj_dgrad_c == 0 or name == 'g/tconv1', tag
    for name in want:
        # look-ahead pair generator at 2 B next to the batch-B instance; D on [fake ; real] at 2 B and D(fake) at B
        assert seen.get((name, 'fwd')) == {B, 2 * B}, (cfg, name, seen.get((name, 'fwd')))
        if name != 'g/conv1':              # (the frames need no gradient)
            assert B in seen.get((name, 'dgrad'), ()), (cfg, name)
    # a reduce list holds the layers that left weight-gradient slabs: deferred wgrads and paired launches with flag 1
    for program, items in inv.reduces:
        for key, splits, _ in items:
            e = inv.entries[key]
            assert splits > 1 and (e['path'] == 'deferred' or (e['path'] == 'pair' and e['flags'] & 1)), (program, CI.describe(e))
