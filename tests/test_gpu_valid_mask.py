"""Valid-pixel masks on the MI355X: nirgan_scene_valid bitwise against the numpy restatement and the raw scenes (guarded outputs, an
exactly allocated pool, every view, partial 64-blocks, rows the kernel has to bound itself), nirgan_valid_count, nirgan_pix_loss_masked
against nirgan_pix_loss (bitwise under a mask of ones) and float64, and the masked step (tests/emu_valid_mask.py; bodies:
tests/valid_mask_cases.py)."""
import pytest
import torch

import api_cases as A
import valid_mask_cases as Vc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("B,augment,scales", Vc.SAMPLED, ids=str)
def test_sampled_masks(B, augment, scales):
    Vc.sampled_masks(DEV, "u16", B, augment, scales)


@pytest.mark.parametrize("T,f,origin", Vc.PLACED, ids=str)
def test_placed_masks(T, f, origin):
    Vc.placed_masks(DEV, T, f, origin)


def test_float_pool_masks():
    Vc.float_pool_masks(DEV)


def test_pool_without_nodata_is_all_ones():
    Vc.pool_without_nodata_is_all_ones(DEV)


def test_scene_without_a_table():
    Vc.scene_without_a_table(DEV)


def test_rows_outside_their_scene():
    Vc.rows_outside_their_scene(DEV)


def test_loader_carries_valid():
    Vc.loader_carries_valid(DEV)


@pytest.mark.parametrize("n", Vc.COUNT_N)
def test_count_is_exact(n):
    Vc.count_is_exact(DEV, n)


@pytest.mark.parametrize("shape", Vc.LOSS_SHAPES, ids=str)
def test_ones_equal_the_unmasked_entry(shape):
    Vc.ones_equal_the_unmasked_entry(DEV, shape)


@pytest.mark.parametrize("shape", Vc.LOSS_SHAPES, ids=str)
def test_half_mask_against_float64(shape):
    Vc.half_mask_against_float64(DEV, shape)


@pytest.mark.parametrize("shape", Vc.LOSS_SHAPES, ids=str)
def test_garbage_at_dropped_pixels(shape):
    Vc.garbage_at_dropped_pixels(DEV, shape)


@pytest.mark.parametrize("shape", Vc.LOSS_SHAPES, ids=str)
def test_count_zero(shape):
    Vc.count_zero(DEV, shape)


def test_python_masked_loss():
    Vc.python_masked_loss(DEV, Vc.LOSS_SHAPES[1])


def test_null_valid_or_count_is_refused():
    Vc.null_valid_or_count_is_refused(DEV)


def test_device_entries_reject_bad_arguments_before_any_launch():
    from nirgan_hip import lib as L
    Vc.valid_refusals(L.backend())
    torch.cuda.synchronize()


def test_ones_step_equals_the_unmasked_step(golden_dir):
    Vc.ones_step_equals_the_unmasked_step(DEV, golden_dir)


def test_half_mask_step_means(golden_dir):
    Vc.half_mask_step_means(DEV, golden_dir)


def test_lightning_and_train_batch_agree(golden_dir):
    Vc.lightning_and_train_batch_agree(DEV, golden_dir, A.GPU_TOL)


def test_micro_batches_share_one_count(golden_dir):
    Vc.micro_batches_share_one_count(DEV, golden_dir)


def test_valid_with_ssim_raises(golden_dir):
    Vc.valid_with_ssim_raises(DEV, golden_dir)


def test_fit_with_masks_resumes_bitwise(tmp_path):
    Vc.fit_with_masks_resumes_bitwise(DEV, tmp_path)
