"""nirgan_tile_metrics_masked on the MI355X: every column against float64 per tile over the valid / support-clean pixels (bodies and
bounds: tests/tile_metrics_masked_cases.py), a mask of ones against nirgan_tile_metrics bitwise, poison at dropped pixels, the edge
rows, bitwise repeatability and batch independence, the untouched-column and guard contracts, calculate_metrics(valid=), and
validation_utils.evaluate_tiles(masked=True) from a ScenePool and on a small-width Px2Px_PL."""
import pytest
import torch

import tile_metric_cases as Tc
import tile_metrics_masked_cases as Mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

COLUMNS = [(shape, crop, kind, w) for shape, crop, kind, windows in Mc.COLUMN_CASES for w in windows]


@pytest.mark.parametrize("shape,crop,kind,window", COLUMNS, ids=lambda v: getattr(v, "__name__", str(v)))
def test_columns_against_float64(shape, crop, kind, window):
    Mc.columns_against_float64(DEV, shape, crop, kind, window)


@pytest.mark.parametrize("window", [11, 5])
def test_raw_window_with_nan_everywhere_outside_it(window):
    Mc.raw_window_with_nan_outside(DEV, window)


@pytest.mark.parametrize("shape,crop", [((3, 67, 93), 41), ((1, 12, 12), None), ((16, 256, 256), 240)], ids=str)
def test_mask_of_ones_equals_the_unmasked_entry(shape, crop):
    Mc.ones_equal_the_unmasked_entry(DEV, shape, crop)


def test_poison_at_dropped_pixels_reaches_no_output():
    Mc.poison_at_dropped_pixels(DEV)


def test_all_invalid_tile_between_two_ordinary_ones():
    Mc.all_invalid_tile_between_two(DEV)


def test_no_clean_support_gives_nan_ssim_and_finite_rest():
    Mc.no_clean_support_but_valid_pixels(DEV)


def test_patch_without_a_valid_pixel_gives_nan_patch_means():
    Mc.patch_without_a_valid_pixel(DEV)


def test_identical_images():
    Mc.identical_images(DEV)


def test_negative_zero_is_invalid_and_any_other_value_valid():
    Mc.values_of_valid(DEV)


def test_repeatable_and_a_tile_alone_equals_its_row_in_the_batch():
    Mc.repeatable_and_batch_independent(DEV)


def test_null_rgb_and_patch_zero_leave_their_columns_and_guards_stay_intact():
    Mc.null_rgb_and_no_patch_leave_their_columns(DEV)


def test_calculate_metrics_over_valid():
    Mc.calculate_metrics_over_valid(DEV)


def test_evaluate_tiles_masked_from_the_pool(tmp_path):
    Mc.table_from_the_pool(DEV, tmp_path)


def test_evaluate_tiles_masked_on_a_small_px2px_pl_equals_single_tile_metrics(tmp_path):
    import api_cases as A
    from model.pix2pix import Px2Px_PL
    from validation_utils import evaluate_tiles
    torch.manual_seed(0)
    m = Px2Px_PL(A.px_config(6, 8)).to(DEV)
    # an untrained generator's output crosses -rgb, where the indices are singular: lift the output layer's bias so that the
    # prediction stays positive (tanh(~1.5) ~ 0.9) and fp32 against float64 is a fair comparison for every column
    sd = m.state_dict()
    last = [k for k in sd if k.startswith("netG.") and k.endswith(".bias") and sd[k].numel() == 1][-1]
    sd[last] = torch.full_like(sd[last], 1.5)
    m.load_state_dict(sd)
    data = Tc.samples([(64, 64)] * 5)
    valid = Mc.mask_planes(5, 64, 64, Mc.centre(64, 64, 40))
    for i, s in enumerate(data):
        s["valid"] = valid[i]
    m.train()
    table = evaluate_tiles(m, data, crop=40, batch_size=4, device=DEV, csv_path=str(tmp_path / "t.csv"), patch=16, masked=True)
    assert m.training and (tmp_path / "t.csv").exists()
    m.with_coords = False                       # Px2Px_PL without SatCLIP: predict_step(rgb) on each tile alone
    tiles = [(s["rgb"], s["nir"], s["valid"][0], None) for s in data]
    ref = Mc.masked_table_rows_equal_single_tile_metrics(DEV, m, tiles, table, 40, 16)
    Mc.cap(ref, (0, 0, 40, 40), "px2px table")
    assert table["x"] == [float(s["coords"][0]) for s in data]
