"""The table of generator kinds (models.KINDS): what a record declares is what the Trainer's checks, the planner's, the CLIs and
the result files do - and a kind that exists in the table alone is accepted by all of them."""
import argparse

import pytest

from action_conditioned_gans_amd import evaluate as E
from action_conditioned_gans_amd import graph as G
from action_conditioned_gans_amd import models as M
from action_conditioned_gans_amd import optim
from action_conditioned_gans_amd import plan as P
from action_conditioned_gans_amd import train as T

KINDS = ['plain', 'dna', 'cdna', 'affine']


def _raises_iff(refused, exc, call):
    if refused:
        with pytest.raises(exc):
            call()
    else:
        call()


def test_the_table_holds_the_four_generators():
    assert list(M.KINDS) == KINDS and [k.name for k in M.KINDS.values()] == KINDS
    assert [k.label for k in M.KINDS.values()] == ['plain', 'DNA', 'CDNA', 'affine']
    assert M.flags() == ['dna', 'cdna', 'affine']
    assert [T.model_kind(v) for v in (False, True) + tuple(KINDS)] == ['plain', 'dna'] + KINDS
    with pytest.raises(ValueError, match="'cdna'"):          # (the message lists what is accepted)
        T.model_kind('stp')


@pytest.mark.parametrize('name', KINDS)
def test_rollout_training_is_refused_as_the_record_says(name):
    kind = M.KINDS[name]
    assert (kind.no_rollout is not None) == (name in ('cdna', 'affine'))
    _raises_iff(kind.no_rollout, ValueError, lambda: T.check_rollout(2, name))
    assert T.check_rollout(1, name) == 1
    if kind.no_rollout:
        with pytest.raises(ValueError) as e:
            T.check_rollout(2, name)
        assert kind.no_rollout in str(e.value) and kind.label in str(e.value)


@pytest.mark.parametrize('name', KINDS)
def test_pixel_maps_are_refused_as_the_record_says(name):
    kind = M.KINDS[name]
    assert (kind.no_maps is not None) == (name != 'dna')
    _raises_iff(kind.no_maps, ValueError, lambda: T.check_pixel_maps(1, name))
    _raises_iff(kind.no_maps, ValueError, lambda: P.check_pixel_args([[1, 2]], [[3.0, 4.0]], None, name, 64))
    assert T.check_pixel_maps(0, name) == 0
    if kind.no_maps:
        with pytest.raises(ValueError) as e:
            T.check_pixel_maps(1, name)
        assert kind.no_maps in str(e.value)


@pytest.mark.parametrize('name', KINDS)
def test_bf16_is_a_cli_error_exactly_for_the_float32_kinds(tmp_path, monkeypatch, name):
    kind = M.KINDS[name]
    assert kind.float32_only == (name in ('cdna', 'affine'))
    flag = ['--' + kind.flag] if kind.flag else []
    seen = {}
    monkeypatch.setattr(T, 'train', lambda *a, **kw: seen.update(kw, positional=a))
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: seen.update(kw))
    monkeypatch.setattr(P, 'plan_sequences', lambda *a, **kw: seen.update(kw))
    for k, main in enumerate((lambda extra: T.main(['synthetic', str(tmp_path / 'out')] + extra),
                              lambda extra: E.main(['models', 'synthetic', str(tmp_path / 'eval'), '--num_sequences', '4'] + extra),
                              lambda extra: P.main(['models', 'synthetic', str(tmp_path / 'plan'), '--num_sequences', '4'] + extra))):
        seen.clear()
        _raises_iff(kind.float32_only, SystemExit, lambda: main(flag + ['--dtype', 'bf16']))
        assert bool(seen) == (not kind.float32_only)
        if seen and k == 0:
            assert T.model_kind(seen['positional'][8]) == name


@pytest.mark.parametrize('name', KINDS)
def test_result_fields_are_none_for_what_the_kind_does_not_read(name):
    kind = M.KINDS[name]
    assert (kind.ksizes is not None) == (name in ('dna', 'cdna')) and kind.num_masks == (name in ('cdna', 'affine'))
    assert kind.result_fields(7, 4) == {'num_masks': 4 if kind.num_masks else None, 'ksize': 7 if kind.ksizes is not None else None}
    assert list(kind.result_fields(7, 4)) == ['num_masks', 'ksize']          # (the order of the keys in metrics.json / plan.json)
    # ... and what it reads it checks, at the CLI as in its builder
    _raises_iff(kind.ksizes is not None, ValueError, lambda: kind.check_args(12, 4))
    _raises_iff(kind.num_masks, ValueError, lambda: kind.check_args(5, 33))
    kind.check_args(5, 4)


def _variables(transform, **kw):
    from oracle import cbind
    G.reset_default_graph()
    optim.set_data_parallel(1)
    sess = G.Session(device='cpu', lib=cbind.load())
    tr = T.Trainer(sess, True, 'bce', 'adam', transform, batch_size=2, **kw)
    return tr, {n: v.shape for n, v in G.get_default_graph().variables.items()}, [op.name for op in G.get_default_graph().ops]


def test_a_fifth_kind_is_one_record(tmp_path, monkeypatch):
    """A kind that is registered in the table and named nowhere else: its builder is the DNA generator's."""
    dna = M.KINDS['dna']
    monkeypatch.setitem(M.KINDS, 'dummy', dna._replace(name='dummy', label='dummy', flag='dummy', help='a stand-in',
                                                       build=lambda *args: dna.build(*args), no_rollout='it is a stand-in'))
    assert T.model_kind('dummy') == 'dummy'
    # the flag resolver
    assert M.flags() == ['dna', 'cdna', 'affine', 'dummy']
    assert M.transform_argument({'dummy': True}) == 'dummy' and M.transform_argument({'dummy': False}) is False
    with pytest.raises(ValueError, match='--cdna and --dummy name two different generators'):
        M.transform_argument({'dummy': True, 'cdna': True}, '--%s')
    # the CLI's flags and their checks
    parser = argparse.ArgumentParser()
    T.add_model_args(parser)
    parser.add_argument('--ksize', type=int, default=5)
    parser.add_argument('--dtype', type=str, default='f32')
    assert T.check_model_args(parser, parser.parse_args(['--dummy', '--ksize', '3'])) == 'dummy'
    assert T.check_model_args(parser, parser.parse_args(['--dummy', 'false', '--dna'])) is True
    for extra in (['--dummy', '--affine'], ['--dummy', '--ksize', '12'], ['--dummy', '--rollout_steps', '2']):
        monkeypatch.setattr(T, 'train', lambda *a, **kw: pytest.fail('train() reached'))
        with pytest.raises(SystemExit):
            T.main(['synthetic', str(tmp_path / 'declined')] + extra)
        assert not (tmp_path / 'declined').exists()
    seen = {}
    monkeypatch.setattr(T, 'train', lambda *a, **kw: seen.update(kw, positional=a))
    T.main(['synthetic', str(tmp_path / 'out'), '--dummy', '--ksize', '3'])
    assert seen['positional'][8] == 'dummy' and seen['ksize'] == 3 and 'dummy' not in seen
    monkeypatch.setattr(E, 'evaluate', lambda *a, **kw: seen.update(kw))
    E.main(['models', 'synthetic', str(tmp_path / 'eval'), '--dummy', '--num_sequences', '4'])
    assert seen['dummy'] is True and seen['dna'] is False
    # the Trainer: the DNA generator's graph under the new name, and the record's refusal
    tr, variables, ops = _variables('dummy', ksize=3)
    assert tr.model == 'dummy' and tr.g_state_out is not None
    with pytest.raises(ValueError, match='it is a stand-in'):
        T.Trainer(tr.sess, True, 'bce', 'adam', 'dummy', batch_size=2, rollout_steps=2)
    _, dna_variables, dna_ops = _variables('dna', ksize=3)
    assert variables == dna_variables and ops == dna_ops and variables['g/tconv4/weights'] == (5, 5, 9, 128)
