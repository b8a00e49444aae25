"""The painted canvas of the CDNA and affine generators without a GPU: the float64 restatement (tests/canvas_ref.py) against
autograd of its own forward, the graph the option builds, and the refusals of the Trainer and of the three CLIs."""
import json

import pytest
import torch

import canvas_ref as R
from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import models as M
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import plan as P
from action_conditioned_gans_amd import train as T


def _restatement_case(kind):
    if kind == 'cdna':
        shape = (2, 20, 36, 3, 4, 3)
        params, z, bias, img, canvas, dout = R.cdna_case(shape, seed=2)
        return shape[4], shape[5], params, z, bias, img, canvas, dout
    shape = (2, 20, 36, 3, 4)
    params, z, bias, img, canvas, dout = R.affine_case(shape, seed=2)
    return shape[4], None, params, z, bias, img, canvas, dout


@pytest.mark.parametrize('kind', ['cdna', 'affine'])
def test_the_restated_gradients_equal_autograd_of_the_restated_forward(kind):
    """dz, dparams, dbias and dcanvas by the formulas of include/acgan_cdna.h against float64 autograd, to 1e-10."""
    m, k, params, z, bias, img, canvas, dout = [t.double() if torch.is_tensor(t) else t for t in _restatement_case(kind)]
    pd, zd, bd, cd = (t.clone().requires_grad_(True) for t in (params, z, bias, canvas))
    if kind == 'cdna':
        out = R.cdna_composite(zd + bd, img, pd, cd, m, k)
    else:
        out = R.affine_composite(zd + bd, img, pd, cd, m)
    out.backward(dout)
    dz, dparams, dbias, dcanvas = R.composite_grads(kind, z, bias, img, params, canvas, dout, m, k)
    for name, got, want in (('dz', dz, zd.grad), ('dparams', dparams, pd.grad), ('dbias', dbias, bd.grad), ('dcanvas', dcanvas, cd.grad)):
        assert float(want.abs().max()) > 0, name
        assert float((got - want).abs().max()) <= 1e-10 * max(float(want.abs().max()), 1.0), name
    # the canvas alone under a logit of +30, and no trace of it under -30
    with torch.no_grad():
        assert float((out[:, 1] - canvas[:, 1]).abs().max()) <= 1e-9 and float(cd.grad[:, 2].abs().max()) <= 1e-9 * float(dout.abs().max())


def _variables(transform, **kw):
    from oracle import cbind
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cpu', lib=cbind.load())
    tr = T.Trainer(sess, True, 'bce', 'adam', transform, batch_size=2, **kw)
    graph = G.get_default_graph()
    return tr, {n: v.shape for n, v in graph.variables.items()}, [op.name for op in graph.ops], [t.name for t in graph.state]


@pytest.mark.parametrize('kind', ['cdna', 'affine'])
def test_the_canvas_widens_tconv4_and_adds_one_layer(kind):
    tr, variables, ops, _ = _variables(kind, ksize=3, num_masks=6, canvas=True)
    assert tr.canvas is True
    assert variables['g/tconv4/weights'] == (5, 5, 8, 128) and variables['g/tconv4/biases'] == (8,)
    assert variables['g/tconv4_canvas/weights'] == (5, 5, 3, 128) and variables['g/tconv4_canvas/biases'] == (3,)
    assert not any('tconv4_canvas/BatchNorm' in n for n in variables)
    _, plain, plain_ops, _ = _variables(kind, ksize=3, num_masks=6)
    assert plain['g/tconv4/weights'] == (5, 5, 7, 128)
    assert set(variables) - set(plain) == {'g/tconv4_canvas/weights', 'g/tconv4_canvas/biases'} and set(plain) <= set(variables)
    assert {n for n in ops if 'tconv4_canvas' in n} and not {n for n in plain_ops if 'canvas' in n}


@pytest.mark.parametrize('kind', ['cdna', 'affine'])
def test_canvas_false_builds_the_graph_built_without_the_argument(kind):
    tr0, variables0, ops0, state0 = _variables(kind, ksize=3, num_masks=6)
    tr1, variables1, ops1, state1 = _variables(kind, ksize=3, num_masks=6, canvas=False)
    assert tr0.canvas is False and tr1.canvas is False
    assert variables1 == variables0 and list(variables1) == list(variables0) and ops1 == ops0 and state1 == state0


def test_the_builders_take_the_canvas_and_the_kind_passes_it_only_when_set():
    assert M.KINDS['cdna'].no_canvas is None and M.KINDS['affine'].no_canvas is None
    assert M.KINDS['plain'].no_canvas and M.KINDS['dna'].no_canvas and 'no mask' in M.KINDS['dna'].no_canvas
    seen = []
    six = M.KINDS['dna']._replace(build=lambda images, actions, batch, reuse, ksize, num_masks: seen.append(1) or ('frame', None))
    assert six.build_with(1, 2, 3, 4, 5, 6) == ('frame', None) and six.build_with(1, 2, 3, 4, 5, 6, False) == ('frame', None)
    assert M.KINDS['cdna'].result_fields(5, 4) == {'num_masks': 4, 'ksize': 5}
    assert M.KINDS['cdna'].result_fields(5, 4, True) == {'num_masks': 4, 'ksize': 5, 'canvas': True}


def test_a_kind_registered_without_the_field_refuses_the_canvas(monkeypatch):
    cdna = M.KINDS['cdna']
    bare = M.Kind('bare', 'bare', cdna.build, ksizes=cdna.ksizes, ksize_text=cdna.ksize_text, num_masks=True, float32_only=True,
                  flag='bare')
    monkeypatch.setitem(M.KINDS, 'bare', bare)
    assert bare.no_canvas
    bare.check_args(3, 6)
    with pytest.raises(ValueError, match='canvas'):
        bare.check_args(3, 6, True)
    with pytest.raises(ValueError, match='canvas'):
        T.check_canvas(True, 'bare', 3, 6)
    with pytest.raises(ValueError, match='canvas'):
        _variables('bare', ksize=3, num_masks=6, canvas=True)
    assert T.check_canvas(False, 'bare', 3, 6) is False


REFUSED = [([], 'plain'), (['--dna'], 'DNA'), (['--cdna', '--num_masks', '32'], '31'), (['--affine', '--num_masks', '32'], '31')]


@pytest.mark.parametrize('flags,word', REFUSED, ids=lambda v: ' '.join(v) if isinstance(v, list) else v)
def test_the_trainer_and_the_clis_refuse_a_canvas_that_cannot_be(tmp_path, monkeypatch, capsys, flags, word):
    transform = M.transform_argument({f[2:]: True for f in flags if f[2:] in M.flags()})
    num_masks = 32 if '32' in flags else 10
    G.reset_default_graph()
    with pytest.raises(ValueError, match=word):
        T.Trainer(None, True, 'bce', 'adam', transform, batch_size=2, num_masks=num_masks, canvas=True)
    assert not G.get_default_graph().ops and not G.get_default_graph().variables, 'refused before anything is created'
    with pytest.raises(ValueError, match=word):
        T.train('synthetic', None, None, None, None, True, 'bce', 'adam', transform, batch_size=2, num_masks=num_masks, canvas=True)
    for what, fn in (('train', lambda *a, **kw: pytest.fail('train() reached')), ):
        monkeypatch.setattr(T, what, fn)
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: pytest.fail('evaluate() reached'))
    monkeypatch.setattr(P, 'plan_sequences', lambda *a, **kw: pytest.fail('plan_sequences() reached'))
    for main, out in ((lambda o: T.main(['synthetic', o, '--canvas'] + flags), tmp_path / 'run'),
                      (lambda o: E.main(['models', 'synthetic', o, '--num_sequences', '4', '--canvas'] + flags), tmp_path / 'eval'),
                      (lambda o: P.main(['models', 'synthetic', o, '--num_sequences', '4', '--canvas'] + flags), tmp_path / 'plan')):
        with pytest.raises(SystemExit):
            main(str(out))
        assert word in capsys.readouterr().err
        assert not out.exists()
    # the functions behind the CLIs refuse it themselves, before they create their output directory
    monkeypatch.undo()
    kw = {f[2:]: True for f in flags if f[2:] in M.flags()}
    with pytest.raises(ValueError, match=word):
        E.evaluate('models', 'synthetic', str(tmp_path / 'eval'), num_masks=num_masks, canvas=True, **kw)
    with pytest.raises(ValueError, match=word):
        P.plan_sequences('models', 'synthetic', str(tmp_path / 'plan'), num_masks=num_masks, canvas=True, **kw)
    assert not (tmp_path / 'eval').exists() and not (tmp_path / 'plan').exists()


@pytest.mark.parametrize('flag', ['--cdna', '--affine'])
def test_the_clis_hand_the_canvas_on(tmp_path, monkeypatch, flag):
    seen = {}
    monkeypatch.setattr(T, 'train', lambda *a, **kw: seen.update(kw))
    T.main(['synthetic', str(tmp_path / 'a'), flag, '--canvas', '--num_masks', '31'])
    assert seen['canvas'] is True and seen['num_masks'] == 31
    T.main(['synthetic', str(tmp_path / 'b'), flag])
    assert seen['canvas'] is False
    for mod, name, extra in ((E, 'evaluate', []), (P, 'plan_sequences', [])):
        seen.clear()
        monkeypatch.setattr(mod, name, lambda *a, **kw: seen.update(kw))
        mod.main(['models', 'synthetic', str(tmp_path / 'o'), '--num_sequences', '4', flag, '--canvas'] + extra)
        assert seen['canvas'] is True and seen[flag[2:]] is True
        seen.clear()
        mod.main(['models', 'synthetic', str(tmp_path / 'o'), '--num_sequences', '4', flag])
        assert 'canvas' not in seen, 'without the flag the call is the one it was'


def test_what_the_kinds_refuse_stays_refused_with_a_canvas(tmp_path):
    for extra, word in ((['--rollout_steps', '2'], 'rollout_steps'), (['--dtype', 'bf16'], 'float32 only')):
        with pytest.raises(SystemExit):
            T.main(['synthetic', str(tmp_path / 'run'), '--cdna', '--canvas'] + extra)
        assert not (tmp_path / 'run').exists()
    with pytest.raises(ValueError, match='pixel_maps'):
        T.Trainer(None, True, 'bce', 'adam', 'affine', batch_size=2, canvas=True, pixel_maps=1)
    with pytest.raises(ValueError, match='image gradient'):
        T.Trainer(None, True, 'bce', 'adam', 'cdna', batch_size=2, canvas=True, rollout_steps=2)


def test_the_train_record_names_the_canvas_only_when_it_is_on():
    assert 'canvas' not in T.train_record({'g_loss': 1.0}, 3, 0.5, 1)
    rec = T.train_record({'g_loss': 1.0}, 3, 0.5, 1, canvas=True)
    assert rec['canvas'] is True and json.loads(json.dumps(rec))['canvas'] is True


def test_the_composite_ops_check_the_canvas():
    from action_conditioned_gans_amd import ops as O
    from oracle import cbind
    G.reset_default_graph()
    optim.set_data_parallel(1)
    G.Session(device='cpu', lib=cbind.load())
    img = G.placeholder((2, 16, 16, 3), name='img')
    canvas = G.placeholder((2, 16, 16, 3), name='canvas')
    z7, z8 = G.placeholder((2, 16, 16, 7), name='z7'), G.placeholder((2, 16, 16, 8), name='z8')
    par = G.placeholder((2, 36), name='par')
    frame = O.affine_composite(z8, img, par, 6, canvas=canvas)
    assert frame.op.has_canvas and frame.op.prefix() == 'affine_composite_canvas' and frame.op.inputs[-1] is canvas
    plain = O.affine_composite(z7, img, par, 6)
    assert not plain.op.has_canvas and plain.op.prefix() == 'affine_composite' and len(plain.op.inputs) == 3
    with pytest.raises(ValueError, match='mask logits'):
        O.affine_composite(z7, img, par, 6, canvas=canvas)
    with pytest.raises(ValueError, match='canvas'):
        O.affine_composite(z8, img, par, 6, canvas=G.placeholder((2, 16, 16, 4), name='c4'))
    with pytest.raises(ValueError, match='31'):
        O.cdna_composite(G.placeholder((2, 16, 16, 34), name='z34'), img, G.placeholder((2, 9 * 32), name='p32'), 32, 3, canvas=canvas)
