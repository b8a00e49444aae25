"""float64 restatement of BatchNorm with stored statistics, from read-only oracle pieces.  Test infrastructure.

``oracle.models._layer`` reaches BatchNorm through the attribute ``oracle.tf_ops.batch_norm_train``; it is substituted for the
duration of one generator call.  Recording mode: the batch-statistics result, keeping every layer's input rows (for pooled
moments).  Stored mode: the given statistics are applied.  Plain and DNA generators through ``oracle.models``, the CDNA generator
through ``cdna_ref.generator_cdna``.  Layers are named as slim names them (``g/conv1/BatchNorm``): a layer is recognised by the
identity of the ``beta`` tensor it is handed."""
import contextlib

import torch

import cdna_ref
from oracle import models as OM
from oracle import tf_ops as OT

EPS = 1e-3


@contextlib.contextmanager
def _substituted(fn):
    prev = OT.batch_norm_train
    OT.batch_norm_train = fn
    try:
        yield prev
    finally:
        OT.batch_norm_train = prev


def _scope(params, beta):
    for k, v in params.items():
        if v is beta:
            assert k.endswith('/beta'), k
            return k[:-len('/beta')]
    raise KeyError('batch_norm_train was handed a beta that is not in params')


def _generator(model, params, images, actions, ksize=5, num_masks=10):
    if model == 'plain':
        return OM.generator(params, images, actions), None
    if model == 'dna':
        return OM.generator_transform(params, images, actions, ksize)
    if model == 'cdna':
        return cdna_ref.generator_cdna(params, images, actions, num_masks, ksize)
    raise ValueError(model)


def run_recording(model, params, images, actions, record, **kw):
    """The generator on batch statistics; ``record`` (scope -> list of [rows, C] tensors) gains every layer's input rows."""
    def bn(x, beta, eps=EPS):
        record.setdefault(_scope(params, beta), []).append(x.detach().reshape(-1, x.shape[-1]).clone())
        return prev[0](x, beta, eps)
    prev = []
    with torch.no_grad(), _substituted(bn) as orig:
        prev.append(orig)
        return _generator(model, params, images, actions, **kw)


def pooled_moments(record):
    """scope -> (mean [C], biased variance [C], rows) of the concatenation of everything recorded for the layer."""
    out = {}
    for scope, chunks in record.items():
        rows = torch.cat(chunks).double()
        mean = rows.mean(dim=0)
        out[scope] = (mean, ((rows - mean) ** 2).mean(dim=0), rows.shape[0])
    return out


def merge_moments(state, rows):
    """The parallel-variance (Chan) update of (count, mean, variance) with the rows [n, C] of one batch, as acg_bn_collect defines
    it: a count of 0 takes the batch's moments and ignores whatever mean / variance held."""
    count, mean, var = state
    rows = rows.double()
    n_b, m_b = rows.shape[0], rows.mean(dim=0)
    m2_b = ((rows - m_b) ** 2).sum(dim=0)
    if count == 0:
        return n_b, m_b, m2_b / n_b
    n = count + n_b
    d = m_b - mean
    return n, mean + d * (n_b / n), (var * count + m2_b + d * d * (count * n_b / n)) / n


def run_stored(model, params, images, actions, stats, **kw):
    """The generator with every BatchNorm layer applying ``stats`` (scope -> (mean, variance, ...))."""
    def bn(x, beta, eps=EPS):
        mean, var = stats[_scope(params, beta)][:2]
        return (x - mean.to(x.dtype)) * torch.rsqrt(var.to(x.dtype) + eps) + beta
    with torch.no_grad(), _substituted(bn):
        return _generator(model, params, images, actions, **kw)


def rollout_stored(model, params, stats, frames, actions, steps, **kw):
    """Trainer.test_sequence's default rollout on stored statistics: step j commanded by actions[:, j, :5] and the state the
    generator predicted (the plain generator: the given one).  -> predicted [B, steps, H, W, 3]."""
    frame, state, out = frames[:, 0], actions[:, 0, 5:], []
    for j in range(steps):
        frame, st = run_stored(model, params, frame, torch.cat([actions[:, j, :5], state], dim=1), stats, **kw)
        state = st if st is not None else actions[:, j + 1, 5:]
        out.append(frame)
    return torch.stack(out, dim=1)
