"""nirgan_image_metrics, nirgan_ssim_loss, nirgan_emd_loss and nirgan_hist_match on the MI355X, each raw entry against float64 under the
derived bounds of tests/metric_loss_cases.py (cases, inputs, references, bounds and bodies are there), their argument guards, and the
Python surfaces in front of them."""
import pytest

import metric_loss_cases as Mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("shape,kind", Mc.SSIM_CASES, ids=str)
def test_image_metrics(shape, kind):
    Mc.metrics_against_float64(DEV, shape, kind)
    if (shape, kind) == Mc.SSIM_VARIED:
        Mc.metrics_against_float64(DEV, shape, kind, max_val=2.0)


@pytest.mark.parametrize("shape,kind", Mc.SSIM_CASES, ids=str)
def test_ssim_loss_value_and_gradient(shape, kind):
    Mc.ssim_loss_against_float64(DEV, shape, kind)


@pytest.mark.parametrize("shape,kind", Mc.EMD_CASES, ids=str)
def test_emd_loss_value_and_gradient(shape, kind):
    Mc.emd_loss_against_float64(DEV, shape, kind)


@pytest.mark.parametrize("shape", Mc.HIST_SHAPES, ids=str)
def test_hist_match(shape):
    Mc.hist_match_against_float64(DEV, shape)


def test_guards():
    Mc.metric_loss_guards(DEV)


def test_python_surfaces():
    Mc.python_surfaces(DEV)
