"""The vanilla and wgangp GAN objectives ON THE MI355X: nirgan_gan_loss against stock torch in float64 (bodies in
tests/gan_loss_cases.py, shared with the CPU suite; every case prints e32 and the entry's error), GANLoss through autograd, and one fused
train_batch per objective on full-width networks."""
import pytest

import gan_loss_cases as Gc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("n", Gc.SIZES)
@pytest.mark.parametrize("mode", Gc.MODES)
def test_entry(mode, n):
    Gc.kernel_case(DEV, mode, n)


@pytest.mark.parametrize("mode", Gc.MODES)
def test_entry_at_an_odd_float_offset(mode):
    Gc.odd_offset_case(DEV, mode)


@pytest.mark.parametrize("mode", Gc.MODES)
def test_autograd_route(mode):
    Gc.autograd_route(DEV, mode)


@pytest.mark.parametrize("mode", Gc.MODES)
def test_fused_step_runs_and_repeats(mode):
    Gc.fused_step_runs_and_repeats(DEV, mode)
