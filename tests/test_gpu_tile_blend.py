"""Blended tiled inference on the MI355X: nirgan_tile_gather_ov / nirgan_tile_blend under predict_tiled(blend="blend") against the
float64 restatement of the geometry (bodies and bounds: tests/tile_blend_cases.py) -- partition of unity, the recorded tiles and
their float64 blend, bitwise independence of the launch split, NaN-filled scenes and guard bands through the raw entries (aligned
and unaligned addresses), overlap = 0 against the existing gather / scatter path, the embeds index and the seam bound."""
import pytest

import tile_blend_cases as Bc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(s, t) for s in Bc.SCENES for t in Bc.TILINGS]
OLD_PATH_CASES = [(s, t) for s in Bc.SCENES[1:2] + Bc.SCENES[3:] for t in (Bc.TILINGS[0], Bc.TILINGS[3], Bc.TILINGS[4])]


@pytest.mark.parametrize("shape,tiling", CASES, ids=str)
def test_partition_of_unity(shape, tiling):
    Bc.partition_of_unity(DEV, shape, tiling)


@pytest.mark.parametrize("shape,tiling", CASES, ids=str)
def test_against_float64(shape, tiling):
    Bc.against_float64(DEV, shape, tiling)


@pytest.mark.parametrize("shape,tiling", [(s, t) for s in Bc.SCENES[2:4] for t in Bc.TILINGS], ids=str)
def test_result_is_bitwise_independent_of_the_launch_split(shape, tiling):
    Bc.split_independence(DEV, shape, tiling)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("shape,tiling", CASES, ids=str)
def test_raw_entries_need_no_initialisation_and_keep_their_guards(shape, tiling, shift):
    Bc.raw_entries_need_no_initialisation(DEV, shape, tiling, shift)


@pytest.mark.parametrize("shape,tiling", OLD_PATH_CASES, ids=str)
def test_overlap_zero_equals_todays_path(shape, tiling):
    Bc.overlap_zero_is_todays_path(DEV, shape, tiling)


def test_embeds_follow_the_scene():
    Bc.embeds_follow_the_scene(DEV)


@pytest.mark.parametrize("tiling", Bc.TILINGS, ids=str)
def test_seam_moves_as_designed(tiling):
    Bc.seam_moves_as_designed(DEV, tiling)
