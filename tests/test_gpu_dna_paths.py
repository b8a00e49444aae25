"""GPU parity: the DNA tail (dna_kernel, dna_rows_kernel, dna_dimage_kernel) at every kernel size 1..11, float32 and bf16 logits,
C = 1..4 and every staging path, against float64 (tests/dna_cases.py): outputs prefilled with NaN between guards, saturated
softmaxes, the second home at any C, and forward against the image gradient as adjoints."""
import pytest

import dna_cases as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', D.PATH_NAMES, ids=str)
def test_dna_path(hip_abi, name):
    D.case_dna_path(hip_abi, name)


@pytest.mark.parametrize('k,half,mode', D.ONE_HOT_CASES, ids=str)
def test_dna_one_hot(hip_abi, k, half, mode):
    D.case_dna_one_hot(hip_abi, k, half, D.family_shape(k), mode)


@pytest.mark.parametrize('c,k,dt', D.SECOND_CASES, ids=str)
def test_dna_second_any_c(hip_abi, c, k, dt):
    D.case_dna_second_any_c(hip_abi, c, k, dt)


@pytest.mark.parametrize('shape', D.ADJOINT_SHAPES, ids=str)
def test_dna_forward_and_image_gradient_are_adjoint(hip_abi, shape):
    D.case_dna_adjoint(hip_abi, shape)
