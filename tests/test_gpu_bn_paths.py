"""GPU parity: BatchNorm at every kernel path of bn.hip, storage type and accumulate mode against float64, with the kernel family
that ran asserted from the workspace (tests/bn_cases.py), also behind the slabs and the tile partials of a producer; accumulate on
acg_bn_act_bwd_slabs, acg_bias_act_bwd and acg_dna_bwd."""
import pytest

import bn_cases as B
from action_conditioned_gans_amd import _lib as L

pytestmark = pytest.mark.gpu

TOL = 2e-5


@pytest.fixture(scope='module')
def ncu():
    """fused_shape sizes its grids by the device's CU count: so do the rows of the table that sit on a grid limit."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope='module')
def hip_abi_bf16(hip_abi):
    from abi_call import Abi
    return Abi(hip_abi.lib, 'cuda:0', conv_dtype=L.ACG_BF16)


def test_path_classifier_on_known_launches(hip_abi, ncu):
    """bn_path itself, on launches whose kernel is not in doubt: the exchange self-test (a grid of n blocks: epoch 1, n slots) and
    a tensor of 64 rows (register-resident: the workspace stays zero)."""
    import torch
    from abi_call import bn_path, _p
    for blocks, threads in ((7, 256), (min(ncu, 512), 1024)):
        ws, n = hip_abi.ws(16 + 512 * 512)
        out = torch.zeros(blocks, device='cuda')
        hip_abi.lib.bn_exchange_selftest(_p(ws), n, _p(out), blocks, threads, -1, 1 << 22, hip_abi.stream())
        torch.cuda.synchronize()
        assert bn_path(ws) == ('grid', blocks)
    x = B.randn((64, 8), 6000).to('cuda')
    *_, ws = hip_abi.bn_act_fwd(x, torch.zeros(8, device='cuda'), None, want_ws=True)
    torch.cuda.synchronize()
    assert bn_path(ws) == ('resident', None)


@pytest.mark.parametrize('name,storage', B.PATH_CASES, ids=lambda v: str(v))
def test_bn_path(hip_abi, ncu, name, storage):
    B.case_bn_path(hip_abi, name, storage, ncu=ncu)


@pytest.mark.parametrize('name,storage', B.SLAB_CASES, ids=lambda v: str(v))
def test_bn_slabs(hip_abi, ncu, name, storage):
    B.case_bn_slabs(hip_abi, name, storage, ncu)


@pytest.mark.parametrize('name', B.PARTIAL_CASES)
def test_bn_tile_partials(hip_abi, name):
    B.case_bn_partials(hip_abi, name)


@pytest.mark.parametrize('name,storage', B.PAD_CASES, ids=lambda v: str(v))
def test_bn_pad_channels_are_neither_read_nor_written(hip_abi, name, storage):
    B.case_bn_pads(hip_abi, name, storage)


@pytest.mark.parametrize('quads', [False, True], ids=['rows_grid', 'quads_resident'])
def test_bn_slabs_accumulate(hip_abi, quads):
    B.case_slab_accumulate(hip_abi, TOL, quads)


@pytest.mark.parametrize('quads', [False, True], ids=['rows_grid', 'quads_resident'])
def test_bn_slabs_accumulate_bf16(hip_abi_bf16, quads):
    B.case_slab_accumulate(hip_abi_bf16, TOL, quads)


def test_bias_accumulate(hip_abi):
    B.case_bias_accumulate(hip_abi, TOL)


@pytest.mark.parametrize('half', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', B.DNA_ACC_SHAPES, ids=str)
def test_dna_dbias_accumulate(hip_abi, shape, half):
    B.case_dna_accumulate(hip_abi, shape, TOL, half)
