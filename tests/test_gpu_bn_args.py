"""The argument checks of the BatchNorm and bias entries of bn.hip, one spoiled argument at a time: the error code of
include/acgan_hip.h and an acg_last_error() that starts with the entry's name.  Every call returns from the host checks, so no
BatchNorm kernel runs (acg_bn_act_fwd_moments converts its 8-channel moments before it looks at `dtype`: that one launch is the
exception).  One argument - or the few that make up one class, e.g. rows and groups for `too many groups` - changes per call and
everything else stays valid, also the workspace size for the spoiled shape, so the ORDER of the checks inside an entry is free."""
import os
import re

import pytest
import torch

from abi_call import _p
from action_conditioned_gans_amd import _lib as L

pytestmark = pytest.mark.gpu

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'acgan_hip.h')
with open(HEADER) as fh:
    ERR = {k: int(v) for k, v in re.findall(r'(ACG_ERR_\w+) = (\d+)', fh.read())}
INVALID, WORKSPACE, UNSUPPORTED = ERR['ACG_ERR_INVALID_ARG'], ERR['ACG_ERR_WORKSPACE'], ERR['ACG_ERR_UNSUPPORTED']

ROWS, CH = 8, 8
F32 = L.ACG_F32
BAD_DTYPE = 7
NG = L.BN_NO_GRID_EXCHANGE


def ws_bytes(rows, c, groups):
    """acgan_hip.h: 16 state bytes + the larger of the partial sums and the exchange area of the one-launch kernels."""
    return 16 + max(groups * (512 * 2 + 2) * c * 4, 512 * 512)


class Pool:
    """Device buffers every baseline shares; nothing writes them."""

    def __init__(self, dev):
        z = lambda *s: torch.zeros(*s, device=dev)
        self.t = {n: z(ROWS, CH) for n in ('x', 'y', 'dy', 'dx')}
        self.t.update({n: z(CH) for n in ('beta', 'bias', 'mean', 'rstd', 'dbeta')})
        self.t.update({n: z(2 * CH) for n in ('moments', 'sums', 'local_sums')})
        self.t['slabs'] = z(2, ROWS, CH)
        self.t['partials'] = z(2 * 2 * CH)
        self.t['ws'] = torch.zeros(ws_bytes(ROWS, CH, 1), dtype=torch.uint8, device=dev)
        self.t['bias_ws'] = torch.zeros(512 * CH * 4, dtype=torch.uint8, device=dev)

    def __getitem__(self, name):
        return self.t[name]


# Argument lists in the order of acgan_hip.h: (name, baseline).  A string names a Pool buffer.
SHAPE = [('rows', ROWS), ('C', CH), ('x_pitch', 0), ('y_pitch', 0), ('groups', 1)]
ACT = [('act', L.ACT_RELU), ('leak', 0.2)]
WS = [('ws', 'ws'), ('wsb', ws_bytes(ROWS, CH, 1))]
ENTRIES = {
    'bn_act_fwd': [('x', 'x'), ('beta', 'beta'), ('y', 'y'), ('save_mean', 'mean'), ('save_rstd', 'rstd')] + SHAPE + [('eps', 1e-3)] + ACT
                  + [('dtype', F32), ('flags', 0)] + WS,
    'bn_act_fwd_partials': [('x', 'x'), ('beta', 'beta'), ('partials', 'partials'), ('nblk', 2), ('block_rows', 4), ('run_rows', 8), ('y', 'y'),
                            ('save_mean', 'mean'), ('save_rstd', 'rstd')] + SHAPE + [('eps', 1e-3)] + ACT + [('dtype', F32)],
    'bn_act_bwd': [('x', 'x'), ('dy', 'dy'), ('beta', 'beta'), ('save_mean', 'mean'), ('save_rstd', 'rstd'), ('dx', 'dx'), ('dbeta', 'dbeta'),
                   ('dbeta_acc', 0.0)] + SHAPE + ACT + [('dtype', F32), ('flags', 0)] + WS,
    'bn_act_fwd_slabs': [('slabs', 'slabs'), ('splits', 2), ('x', 'x'), ('beta', 'beta'), ('y', 'y'), ('save_mean', 'mean'), ('save_rstd', 'rstd')]
                        + SHAPE + [('eps', 1e-3)] + ACT + [('dtype', F32), ('layout', L.SLABS_ROWS), ('flags', 0)] + WS,
    'bn_act_bwd_slabs': [('x', 'x'), ('dy_slabs', 'slabs'), ('splits', 2), ('beta', 'beta'), ('save_mean', 'mean'), ('save_rstd', 'rstd'), ('dx', 'dx'),
                         ('dbeta', 'dbeta'), ('dbeta_acc', 0.0)] + SHAPE + ACT + [('dtype', F32), ('layout', L.SLABS_ROWS), ('flags', 0)] + WS,
    'bn_moments': [('x', 'x'), ('moments', 'moments'), ('rows', ROWS), ('C', CH), ('x_pitch', 0), ('groups', 1), ('dtype', F32)] + WS,
    'bn_act_fwd_moments': [('x', 'x'), ('beta', 'beta'), ('moments', 'moments'), ('y', 'y'), ('save_mean', 'mean'), ('save_rstd', 'rstd')] + SHAPE
                          + [('eps', 1e-3)] + ACT + [('dtype', F32)],
    'bn_bwd_sums': [('x', 'x'), ('dy', 'dy'), ('beta', 'beta'), ('save_mean', 'mean'), ('save_rstd', 'rstd'), ('sums', 'sums')] + SHAPE + ACT
                   + [('dtype', F32)] + WS,
    'bn_act_bwd_sums': [('x', 'x'), ('dy', 'dy'), ('beta', 'beta'), ('save_mean', 'mean'), ('save_rstd', 'rstd'), ('sums', 'sums'),
                        ('local_sums', 'local_sums'), ('total_rows', 2 * ROWS), ('dx', 'dx'), ('dbeta', 'dbeta'), ('dbeta_acc', 0.0)] + SHAPE + ACT
                       + [('dtype', F32)],
    'bias_act_fwd': [('x', 'x'), ('bias', 'bias'), ('y', 'y'), ('rows', ROWS), ('C', CH), ('x_pitch', 0), ('y_pitch', 0)] + ACT + [('dtype', F32)],
    'bias_act_bwd': [('y', 'y'), ('dy', 'dy'), ('dx', 'dx'), ('dbias', 'dbeta'), ('dbias_acc', 0.0), ('rows', ROWS), ('C', CH), ('x_pitch', 0),
                     ('y_pitch', 0)] + ACT + [('dtype', F32), ('ws', 'bias_ws'), ('wsb', 512 * CH * 4)],
}
# pointers an entry requires (acg_bias_act_fwd takes a NULL bias; acg_bias_act_bwd needs one of dx / dbias: below)
REQUIRED = {
    'bn_act_fwd': ('x', 'beta', 'y', 'save_mean', 'save_rstd'),
    'bn_act_fwd_partials': ('x', 'beta', 'partials', 'y', 'save_mean', 'save_rstd'),
    'bn_act_bwd': ('x', 'dy', 'beta', 'save_mean', 'save_rstd', 'dx', 'dbeta'),
    'bn_act_fwd_slabs': ('slabs', 'x', 'beta', 'y', 'save_mean', 'save_rstd'),
    'bn_act_bwd_slabs': ('x', 'dy_slabs', 'beta', 'save_mean', 'save_rstd', 'dx', 'dbeta'),
    'bn_moments': ('x', 'moments'),
    'bn_act_fwd_moments': ('x', 'beta', 'moments', 'y', 'save_mean', 'save_rstd'),
    'bn_bwd_sums': ('x', 'dy', 'beta', 'save_mean', 'save_rstd', 'sums'),
    'bn_act_bwd_sums': ('x', 'dy', 'beta', 'save_mean', 'save_rstd', 'sums', 'local_sums', 'dx', 'dbeta'),
    'bias_act_fwd': ('x', 'y'),
    'bias_act_bwd': ('y', 'dy'),
}
CHECKS_ACT = ('bn_act_fwd', 'bn_act_fwd_partials', 'bn_act_bwd', 'bn_act_fwd_slabs', 'bn_act_bwd_slabs', 'bn_act_fwd_moments')
CHECKS_WS = ('bn_act_fwd', 'bn_act_bwd', 'bn_act_fwd_slabs', 'bn_moments', 'bn_bwd_sums')


def spoils(name):
    """[(what, {argument: value}, error code)] for one entry."""
    names = [n for n, _ in ENTRIES[name]]
    bn = name.startswith('bn_')
    has_ws = name in CHECKS_WS
    out = [('x_pitch < C', {'x_pitch': CH - 1}, INVALID), ('rows 0', {'rows': 0}, INVALID), ('rows < 0', {'rows': -8}, INVALID), ('C 0', {'C': 0}, INVALID)]
    if 'y_pitch' in names:
        out.append(('y_pitch < C', {'y_pitch': CH - 1}, INVALID))
    if bn:
        # the tile geometry / total_rows / workspace size follow the spoiled shape: only the class under test is wrong
        g_many = {'rows': 65536, 'groups': 65536, 'nblk': 1, 'block_rows': 1, 'run_rows': 1}
        many = {k: v for k, v in g_many.items() if k in names}
        out += [('groups 0', {'groups': 0}, INVALID), ('rows % groups', {'groups': 3}, INVALID),
                ('C > 1024', dict({'C': 1025}, **({'wsb': ws_bytes(ROWS, 1025, 1)} if has_ws else {})), UNSUPPORTED),
                ('groups > 65535', dict(many, **({'wsb': ws_bytes(65536, CH, 65536)} if has_ws else {})), UNSUPPORTED)]
    out += [('%s NULL' % p, {p: None}, INVALID) for p in REQUIRED[name]]
    if name in CHECKS_ACT:
        out += [('tanh', {'act': L.ACT_TANH}, UNSUPPORTED), ('act 9', {'act': 9}, UNSUPPORTED), ('act -1', {'act': -1}, UNSUPPORTED)]
    if not bn:
        out += [('act 4', {'act': 4}, INVALID), ('act -1', {'act': -1}, INVALID)]
    if 'flags' in names:
        out += [('unknown flag bit', {'flags': 2}, INVALID), ('unknown flag bit beside a known one', {'flags': NG | 4}, INVALID)]
    if has_ws:
        out += [('ws NULL', {'ws': None}, WORKSPACE), ('workspace one byte short', {'wsb': ws_bytes(ROWS, CH, 1) - 1}, WORKSPACE)]
    out.append(('dtype', {'dtype': BAD_DTYPE}, UNSUPPORTED))
    if name in ('bn_act_fwd', 'bn_act_fwd_partials', 'bn_act_fwd_slabs', 'bn_act_bwd_slabs', 'bn_act_fwd_moments', 'bias_act_fwd', 'bias_act_bwd'):
        out.append(('dtype (f32, bf16)', {'dtype': L.dtype2(L.ACG_F32, L.ACG_BF16)}, UNSUPPORTED))      # the backward entries alone take it
    if name == 'bn_moments':
        out.append(('dtype pair', {'dtype': L.dtype2(L.ACG_BF16, L.ACG_F32)}, UNSUPPORTED))
    if 'layout' in names:
        # 8 x 8 runs the one-launch grid kernel: acg_bn_slabs_layout answers ROWS (asserted below), QUADS is refused
        out += [('QUADS where acg_bn_slabs_layout answers ROWS', {'layout': L.SLABS_QUADS}, UNSUPPORTED), ('layout 2', {'layout': 2}, UNSUPPORTED),
                ('splits 0', {'splits': 0}, INVALID),
                ('quad slabs, x not 16-byte aligned', {'layout': L.SLABS_QUADS, 'flags': NG, 'x': ('x', 4)}, INVALID)]
    if name == 'bn_act_bwd_slabs':
        out.append(('too many rows for a one-launch kernel', {'rows': 4096, 'flags': NG}, UNSUPPORTED))
    if name == 'bn_act_fwd_partials':
        out += [('nblk 0', {'nblk': 0}, INVALID), ('block_rows 0', {'block_rows': 0}, INVALID), ('run_rows 0', {'run_rows': 0}, INVALID),
                ('nblk no multiple of the blocks per run', {'nblk': 3}, INVALID), ('nblk covers 2 R', {'nblk': 4}, INVALID),
                ('block_rows covers 2 R', {'block_rows': 16}, INVALID), ('run_rows covers 6 of 8', {'run_rows': 6}, INVALID)]
    if name == 'bn_act_bwd_sums':
        out += [('total_rows < R', {'total_rows': ROWS - 1}, INVALID), ('total_rows 0', {'total_rows': 0}, INVALID)]
    if name == 'bias_act_bwd':
        out += [('dx and dbias NULL', {'dx': None, 'dbias': None}, INVALID), ('dx NULL with an activation', {'dx': None}, INVALID),
                ('ws NULL', {'ws': None}, WORKSPACE), ('workspace one byte short', {'wsb': 512 * CH * 4 - 1}, WORKSPACE)]
    return out


CASES = [(name, what) for name in ENTRIES for what, _, _ in spoils(name)]


@pytest.fixture(scope='module')
def pool(hip_abi):
    return Pool(hip_abi.device)


def _arg(pool, v):
    if isinstance(v, tuple):                                 # (buffer, byte offset)
        return _p(pool[v[0]].view(-1)[v[1] // 4:])
    return _p(pool[v]) if isinstance(v, str) else v


@pytest.mark.parametrize('name,what', CASES, ids=lambda v: str(v).replace(' ', '_'))
def test_spoiled_argument(hip_abi, pool, name, what):
    change, code = next((c, e) for w, c, e in spoils(name) if w == what)
    assert set(change) <= {n for n, _ in ENTRIES[name]}, 'test premise: %s has no argument %s' % (name, sorted(change))
    args = [_arg(pool, change.get(n, v)) for n, v in ENTRIES[name]]
    with pytest.raises(L.AcgError) as err:
        getattr(hip_abi.lib, name)(*(args + [hip_abi.stream()]))
    m = re.match(r'acg_(\w+) failed \(code (\d+)\): (.*)', str(err.value), re.S)
    assert m and m.group(1) == name
    assert int(m.group(2)) == code, '%s, %s: code %s where %d is documented: %s' % (name, what, m.group(2), code, m.group(3))
    assert m.group(3).startswith(name + ':'), '%s, %s: acg_last_error() does not name the entry: %r' % (name, what, m.group(3))


def test_baseline_premises(hip_abi):
    """What the table above assumes about its 8 x 8 baseline: the slab layout, and the workspace sizes of acgan_hip.h."""
    lib = hip_abi.lib
    for backward in (0, 1):
        assert lib.bn_slabs_layout(ROWS, CH, 0, 0, 1, F32, backward, 0) == L.SLABS_ROWS
        assert lib.bn_slabs_layout(ROWS, CH, 0, 0, 1, F32, backward, NG) == L.SLABS_QUADS
    assert lib.bn_slabs_layout(4096, CH, 0, 0, 1, F32, 1, NG) == -1
    for rows, c, groups in ((ROWS, CH, 1), (ROWS, CH, 3), (1024, 64, 1), (ROWS, 128, 2), (ROWS, 1024, 1), (65536, CH, 65536)):
        assert lib.bn_workspace_bytes(rows, c, groups) == ws_bytes(rows, c, groups), (rows, c, groups)
    assert ws_bytes(ROWS, CH, 1) == 16 + 512 * 512 and ws_bytes(ROWS, 128, 2) == 16 + 2 * 1026 * 128 * 4
    assert lib.bias_workspace_bytes(ROWS, CH) == 512 * CH * 4
