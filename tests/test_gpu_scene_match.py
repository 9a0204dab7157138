"""Scene histogram matching on the MI355X: nirgan_scene_hist / nirgan_scene_match_lut / nirgan_scene_lut_apply alone (guarded tables
and planes, planes two bytes off a 16-byte line, exact allocations, grids that wrap, the most contended count) and under
``histogram_match_scene`` / ``predict_scene(match=...)`` / ``ScenePool``, bitwise against the numpy restatement
(tests/emu_scene_match.py; bodies: tests/scene_match_cases.py), and the cross-check against the per-tile float entry."""
import pytest
import torch

import scene_match_cases as Mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", Mc.COUNT_SIZES)
def test_count_sizes(n, shift):
    Mc.count_sizes(DEV, n, shift)


def test_count_every_code_once():
    Mc.count_every_code_once(DEV)


def test_count_one_code():
    Mc.count_one_code(DEV)


def test_count_pools():
    Mc.count_pools(DEV)


def test_count_and_apply_wrap():
    Mc.count_and_apply_wrap(DEV)


@pytest.mark.parametrize("shift_in,shift_out", [(0, 0), (1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("n", Mc.COUNT_SIZES)
def test_apply_sizes(n, shift_in, shift_out):
    Mc.apply_sizes(DEV, n, shift_in, shift_out)


def test_tables():
    Mc.tables(DEV)


def test_ties_on_the_device():
    Mc.ties_on_the_device(DEV)


def test_main_route():
    Mc.main_route(DEV)


def test_properties():
    Mc.properties(DEV)


def test_nodata_codes():
    Mc.nodata_codes(DEV)


def test_predict_scene_matches():
    Mc.predict_scene_matches(DEV)


def test_predict_scene_without_nodata_reserves_nothing():
    Mc.predict_scene_without_nodata_reserves_nothing(DEV)


def test_python_refusals():
    Mc.python_refusals(DEV)


def test_band_histogram():
    Mc.band_histogram(DEV)


def test_pool_predict():
    Mc.pool_predict(DEV)


def test_close_to_the_float_entry():
    Mc.close_to_the_float_entry(DEV)


def test_device_entries_reject_bad_arguments_before_any_launch():
    from nirgan_hip import lib as L
    Mc.entries_reject_bad_arguments(L.backend())
    torch.cuda.synchronize()
