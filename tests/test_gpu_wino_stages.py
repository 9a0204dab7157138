"""The Winograd data, plane-GEMM and output stages on the MI355X (nirgan_wino6_input / _input_norm / _input_dy / nirgan_wino6_dy,
nirgan_wino6_gemm on every plane-GEMM route, nirgan_wino6_output plain and fused), each stage alone against float64: bitwise on integer
data, under the derived bounds on random data, every output guarded by sentinels (cases, inputs, references, bounds and bodies are in
tests/wino_stage_cases.py)."""
import pytest

import wino_stage_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("case", S.IN_CASES, ids=lambda c: "-".join(map(str, c)).replace(" ", ""))
def test_input_transform(case):
    S.input_against_float64(DEV, case)


@pytest.mark.parametrize("case", S.GEMM_CASES, ids=lambda c: "-".join(map(str, c)).replace(" ", ""))
def test_plane_gemm(case):
    S.gemm_against_float64(DEV, case)


@pytest.mark.parametrize("case", S.OUT_CASES, ids=lambda c: "-".join(map(str, c)).replace(" ", ""))
def test_output_transform(case):
    S.output_against_float64(DEV, case)


@pytest.mark.parametrize("case", S.FUSE_CASES, ids=lambda c: "-".join(map(str, c)).replace(" ", ""))
def test_fused_output_transform(case):
    S.fused_output_against_float64(DEV, case)


def test_input_guards():
    S.input_guards(DEV)


def test_gemm_guards():
    S.gemm_guards(DEV)


def test_output_guards():
    S.output_guards(DEV)


@pytest.mark.parametrize("case", S.DYNORM_CASES, ids=lambda c: "-".join(map(str, c)).replace(" ", ""))
def test_input_transform_of_the_instance_norm_backward(case):
    S.dynorm_against_float64(DEV, case)


@pytest.mark.parametrize("case", S.PAIR_CASES, ids=lambda c: "-".join(map(str, c)).replace(" ", ""))
def test_plane_gemm_with_the_weight_gradient(case):
    S.pair_against_float64(DEV, case)
