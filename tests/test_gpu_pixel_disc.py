"""The pixel discriminator (netD 'pixel') ON THE MI355X through csrc/pixdisc.hip: against stock torch.nn in float64 with bounds of ten
times the stock-fp32 error on the same inputs (tests/pixel_disc_cases.py states them), guard values around every output, bitwise
repeatability, and the fused trainer with ``netD: pixel``.  Bodies shared with tests/test_pixel_disc_emulated.py."""
import os

import numpy as np
import pytest
import torch

import pixel_disc_cases as Pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("wset", [1, 2])
@pytest.mark.parametrize("shape", Pc.SHAPES, ids=str)
def test_engine_forward_params_input_pred_against_float64(shape, wset):
    Pc.engine_level(shape, wset, DEV)


@pytest.mark.parametrize("shape", Pc.LARGE_MEAN_SHAPES, ids=str)
def test_large_mean_forward(shape):
    Pc.large_mean_forward(shape, DEV)


def test_eight_256_tiles_against_float64_and_two_runs_bitwise():
    c = Pc.case(Pc.BIG, 2)
    res = Pc.two_runs_bitwise(Pc.BIG, DEV, c)
    m = Pc.ours(2, "cpu")
    Pc.raw_compare(f"{Pc.BIG} w2", Pc.BIG, c, res, m._flat())


@pytest.mark.parametrize("shape", Pc.GUARD_SHAPES, ids=str)
def test_guard_values_stay_and_the_workspace_is_not_read_before_written(shape):
    Pc.guarded(shape, DEV)


def test_two_runs_are_bitwise_equal():
    Pc.two_runs_bitwise((3, 67, 93), DEV)


@pytest.mark.parametrize("shape", [(2, 7, 9), (3, 67, 93)], ids=str)
def test_zero_dout_gives_exact_zeros(shape):
    Pc.zero_dout(shape, DEV)


@pytest.mark.parametrize("shape", [(2, 7, 9), (3, 67, 93)], ids=str)
def test_fake_real_batch_equals_two_forwards_bitwise(shape):
    Pc.doubled_batch(shape, DEV)


def test_module_autograd_route_against_float64():
    Pc.autograd_route((2, 7, 9), 2, DEV)


def test_golden_forward():
    Pc.golden_forward(np.load(os.path.join(HERE, "golden", "f11_pixel_d.npz")), DEV)


def test_thirty_fused_steps_twice_are_bitwise_equal():
    Pc.thirty_steps_twice(DEV)


def test_lightning_sequence_and_train_batch_agree_over_five_steps():
    Pc.routes_agree(DEV)


@pytest.mark.parametrize("mode", ["lsgan", "vanilla", "wgangp"])
def test_fused_step_losses_against_float64(mode):
    Pc.fused_losses_against_float64(DEV, mode)


def test_fit_history_checkpoint_resume(tmp_path):
    Pc.fit_checkpoint_resume(DEV, tmp_path)
