"""The flat fp32 streaming kernels on the MI355X (nirgan_inject_fwd / _bwd, nirgan_bilinear_fwd / _bwd, nirgan_colsum,
nirgan_param_scale_fwd / _bwd, nirgan_fill, nirgan_axpy, nirgan_adam, nirgan_lsgan, nirgan_pix_loss, nirgan_tap_scatter), each raw entry
against float64 under the derived bounds of tests/streaming_cases.py (cases, inputs, references, bounds and bodies are there), and the
generator with the unscaled multiply injection against the float64 oracle."""
import pytest

import streaming_cases as Sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("shape,pad,variant", Sc.INJECT_CASES, ids=str)
def test_inject_forward_and_backward(shape, pad, variant):
    Sc.inject_against_float64(DEV, shape, pad, variant)


@pytest.mark.parametrize("src,dst", Sc.BILINEAR_CASES, ids=str)
def test_bilinear_forward_backward_and_adjoint_identity(src, dst):
    Sc.bilinear_against_float64(DEV, src, dst)


@pytest.mark.parametrize("rows", Sc.COLSUM_ROWS + ("net",), ids=str)
def test_colsum(rows):
    Sc.colsum_against_float64(DEV, rows)


@pytest.mark.parametrize("n", Sc.PARAM_SCALE_N)
def test_param_scale(n):
    Sc.param_scale_against_float64(DEV, n)


@pytest.mark.parametrize("n", Sc.FLAT_N)
def test_fill_and_axpy(n):
    Sc.fill_axpy_against_torch(DEV, n)


@pytest.mark.parametrize("n", Sc.ADAM_N)
def test_adam_three_steps(n):
    Sc.adam_against_float64(DEV, n)


@pytest.mark.parametrize("n", Sc.LSGAN_N)
def test_lsgan(n):
    Sc.lsgan_against_float64(DEV, n)


@pytest.mark.parametrize("shape", Sc.PIX_SHAPES, ids=str)
def test_pix_loss_sums_and_gradient(shape):
    Sc.pix_loss_against_float64(DEV, shape)


def test_pix_loss_guards():
    Sc.pix_loss_guards(DEV)


@pytest.mark.parametrize("case", Sc.TAP_CASES, ids=str)
def test_tap_scatter(case):
    Sc.tap_scatter_against_float64(DEV, case)


@pytest.mark.parametrize("shape", Sc.OPPOSITE_HALVES, ids=str)
def test_tap_scatter_opposite_halves_leave_the_bias_gradient_at_zero(shape):
    Sc.tap_scatter_opposite_halves(DEV, shape)


def test_generator_with_the_unscaled_multiply_injection():
    Sc.unscaled_multiply_generator(DEV)
