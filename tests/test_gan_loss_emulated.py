"""The vanilla and wgangp GAN objectives without a GPU: the bodies of tests/gan_loss_cases.py with the C ABI served by the numpy statement
of tests/emu_gan_loss.py -- the entry's contract, GANLoss / GanLossFn, and the fused trainer's ``gan_mode`` against the autograd route
and against stock torch in float64.  The argument errors are checked on the library itself (they come before any launch)."""
import pytest
import torch

import gan_loss_cases as Gc
from emu_gan_loss import EmuGanLoss
from nirgan_hip import lib as L

DEV = "cpu"


@pytest.fixture()
def emu():
    be = EmuGanLoss()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.mark.parametrize("n", Gc.SIZES)
@pytest.mark.parametrize("mode", Gc.MODES)
def test_entry(emu, mode, n):
    Gc.kernel_case(DEV, mode, n)


@pytest.mark.parametrize("mode", Gc.MODES)
def test_entry_at_an_odd_float_offset(emu, mode):
    Gc.odd_offset_case(DEV, mode)


def test_argument_errors_on_the_library():
    assert not L.is_emulated()
    Gc.argument_errors(L.backend())


def test_argument_errors_on_the_emulator(emu):
    Gc.argument_errors(emu)
    assert emu.calls == ["gan_loss"] * 5


def test_construction():
    Gc.construction()


@pytest.mark.parametrize("mode", Gc.MODES)
def test_autograd_route(emu, mode):
    Gc.autograd_route(DEV, mode)
    assert emu.calls == ["gan_loss"] * 3


def test_no_cpu_fallback():
    from model import networks
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        networks.GANLoss("vanilla")(torch.zeros(1, 1, 4, 4), True)


@pytest.mark.parametrize("mode", Gc.MODES)
def test_fused_step_against_the_autograd_route(emu, golden_dir, mode):
    Gc.fused_against_autograd(DEV, golden_dir, mode)


@pytest.mark.parametrize("mode", Gc.MODES)
def test_fused_step_against_stock_torch_float64(emu, golden_dir, mode):
    Gc.fused_against_float64(DEV, golden_dir, mode)
    assert emu.calls.count("gan_loss") == 3 and emu.calls.count("lsgan") == 0


def test_lsgan_launches_what_it_launched(emu, golden_dir):
    m = Gc.make_model(DEV, "lsgan", golden_dir=golden_dir)
    m.train_batch(Gc.batch64(DEV))
    assert emu.calls.count("lsgan") == 3 and emu.calls.count("gan_loss") == 0
    assert m.fused_trainer().gan_mode == "lsgan"


def test_trainer_refuses_unknown_modes(golden_dir):
    from model import networks
    from nirgan_hip.trainer import Pix2PixTrainer
    netG = networks.define_G(3, 1, 8, "resnet_6blocks", "instance", False, "normal", 0.02)
    netD = networks.define_D(4, 8, "basic", 3, "instance", "normal", 0.02)
    with pytest.raises(NotImplementedError):
        Pix2PixTrainer(netG, netD, n_blocks=6, gan_mode="hinge")
    assert Pix2PixTrainer(netG, netD, n_blocks=6).gan_mode == "lsgan"
