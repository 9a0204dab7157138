"""Valid-pixel masks without a GPU: ``return_valid`` of the scene pool, the masked losses and the masked step on the numpy / torch
statement of nirgan_scene_valid / nirgan_valid_count / nirgan_pix_loss_masked (tests/emu_valid_mask.py), plus the argument checks and
the struct layouts of the real library.  Bodies shared with tests/test_gpu_valid_mask.py (tests/valid_mask_cases.py)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import api_cases as A
import valid_mask_cases as Vc
from emu_valid_mask import EmuValidMask
from nirgan_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(4)


@pytest.fixture()
def emu():
    be = EmuValidMask()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.mark.parametrize("B,augment,scales", Vc.SAMPLED, ids=str)
def test_sampled_masks(emu, B, augment, scales):
    Vc.sampled_masks("cpu", "u16", B, augment, scales)
    assert emu.calls.count("scene_valid") == 2                                   # the sample's and the gather's; the plain sample has none


@pytest.mark.parametrize("T,f,origin", Vc.PLACED, ids=str)
def test_placed_masks(emu, T, f, origin):
    Vc.placed_masks("cpu", T, f, origin)


def test_float_pool_masks(emu):
    Vc.float_pool_masks("cpu")


def test_pool_without_nodata_is_all_ones(emu):
    Vc.pool_without_nodata_is_all_ones("cpu")


def test_scene_without_a_table(emu):
    Vc.scene_without_a_table("cpu")


def test_rows_outside_their_scene(emu):
    Vc.rows_outside_their_scene("cpu")


def test_loader_carries_valid(emu):
    Vc.loader_carries_valid("cpu")


@pytest.mark.parametrize("n", Vc.COUNT_N)
def test_count_is_exact(emu, n):
    Vc.count_is_exact("cpu", n)


@pytest.mark.parametrize("shape", Vc.LOSS_SHAPES, ids=str)
def test_ones_equal_the_unmasked_entry(emu, shape):
    Vc.ones_equal_the_unmasked_entry("cpu", shape)


@pytest.mark.parametrize("shape", Vc.LOSS_SHAPES, ids=str)
def test_half_mask_against_float64(emu, shape):
    Vc.half_mask_against_float64("cpu", shape)


@pytest.mark.parametrize("shape", Vc.LOSS_SHAPES, ids=str)
def test_garbage_at_dropped_pixels(emu, shape):
    Vc.garbage_at_dropped_pixels("cpu", shape)


@pytest.mark.parametrize("shape", Vc.LOSS_SHAPES, ids=str)
def test_count_zero(emu, shape):
    Vc.count_zero("cpu", shape)


def test_python_masked_loss(emu):
    Vc.python_masked_loss("cpu", Vc.LOSS_SHAPES[1])


def test_null_valid_or_count_is_refused(emu):
    Vc.null_valid_or_count_is_refused("cpu")


def test_ones_step_equals_the_unmasked_step(emu, golden_dir):
    Vc.ones_step_equals_the_unmasked_step("cpu", golden_dir)
    assert "pix_loss_masked" in emu.calls and "valid_count" in emu.calls


def test_half_mask_step_means(emu, golden_dir):
    Vc.half_mask_step_means("cpu", golden_dir)


def test_lightning_and_train_batch_agree(emu, golden_dir):
    Vc.lightning_and_train_batch_agree("cpu", golden_dir, A.CPU_TOL)


def test_valid_with_ssim_raises(emu, golden_dir):
    Vc.valid_with_ssim_raises("cpu", golden_dir)


def test_fit_with_masks_resumes_bitwise(emu, tmp_path):
    Vc.fit_with_masks_resumes_bitwise("cpu", tmp_path)


def test_emulator_rejects_bad_arguments(emu):
    Vc.valid_refusals(emu)


def test_real_library_rejects_bad_arguments_before_any_launch():
    assert not L.is_emulated()
    Vc.valid_refusals(L.backend())


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof and every field offset of the two new descriptors, computed by gcc"""
    pairs = [("nirgan_scene_valid_desc", L.SceneValidDesc), ("nirgan_pix_loss_masked_desc", L.PixLossMaskedDesc)]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
    for cname, ct in pairs:
        src += f'printf("%zu", sizeof({cname}));\n'
        for name, _ in ct._fields_:
            src += f'printf(" %zu", offsetof({cname}, {name}));\n'
        src += 'printf("\\n");\n'
    src += "return 0;}\n"
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    for (cname, ct), line in zip(pairs, lines):
        nums = [int(x) for x in line.split()]
        assert nums[0] == C.sizeof(ct), cname
        assert nums[1:] == [getattr(ct, name).offset for name, _ in ct._fields_], cname
