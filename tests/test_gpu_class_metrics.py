"""nirgan_class_metrics on the MI355X: every (tile, class) row against float64 (bodies, masks and bounds: tests/class_metric_cases.py),
agreement with the per-tile entry, the window contract under NaN poison, bitwise repeatability and batch independence, the
overwrite / untouched-column / guard contracts of the raw entry, and validation_utils.evaluate_land_cover / summarize_land_cover."""
import pytest

import class_metric_cases as Cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("shape,crop", Cc.CASES, ids=str)
def test_rows_against_float64(shape, crop):
    Cc.rows_against_float64(DEV, shape, crop)


def test_one_class_equals_the_per_tile_entry():
    Cc.one_class_equals_tile_metrics(DEV)
    Cc.one_class_equals_tile_metrics(DEV, (2, 256, 256), 240)


def test_count_weighted_classes_reproduce_the_per_tile_entry():
    Cc.weighted_classes_reproduce_tile_metrics(DEV)
    Cc.weighted_classes_reproduce_tile_metrics(DEV, (2, 256, 256), 240)


def test_nan_outside_the_window_changes_nothing():
    Cc.poison_outside_the_window_changes_nothing(DEV)


def test_no_rgb_gives_nan_index_columns():
    Cc.no_rgb_gives_nan_index_columns(DEV)


def test_bitwise_repeatable_and_a_tile_alone_equals_its_rows_in_a_batch_of_64():
    Cc.bitwise_repeatable_and_batch_independent(DEV)


def test_raw_entry_overwrites_and_keeps_its_guards():
    Cc.raw_entry_overwrites_and_keeps_its_guards(DEV)


def test_land_cover_table_csv_and_summary(tmp_path):
    Cc.land_cover_table_and_summary(DEV, tmp_path)
