"""Dihedral test-time augmentation on the MI355X: nirgan_tile_views_expand / nirgan_tile_views_merge raw (guard bands, aligned and
shifted addresses, extents around the staged block) and under predict_tiled(tta=...) / predict_tta, bitwise against the np.flip /
np.swapaxes restatement (bodies and the one derived bound: tests/tile_views_cases.py), plus a small real generator."""
import pytest
import torch

import tile_blend_cases as Bc
import tile_views_cases as Vc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILED = [(s, t, b) for s in Vc.SCENES for t in Vc.TILINGS for b in Vc.BLENDS]


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("hw,k", Vc.SHAPE_VIEWS, ids=str)
def test_expand_is_bitwise_the_restated_views(hw, k, shift):
    Vc.expand_is_bitwise(DEV, hw, k, shift)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("hw,k", Vc.SHAPE_VIEWS, ids=str)
def test_merge_is_bitwise_the_restated_tree(hw, k, shift):
    Vc.merge_is_bitwise(DEV, hw, k, shift)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("hw,k", Vc.SHAPE_VIEWS, ids=str)
def test_merge_of_expand_is_the_input(hw, k, shift):
    Vc.round_trip_is_bitwise(DEV, hw, k, shift)


@pytest.mark.parametrize("shape,tiling,blend", TILED, ids=str)
def test_model_sees_the_right_views(shape, tiling, blend):
    Vc.model_sees_the_right_views(DEV, shape, tiling, blend)


@pytest.mark.parametrize("shape,tiling,blend", TILED, ids=str)
def test_equivariant_model_is_unchanged(shape, tiling, blend):
    Vc.equivariant_model_is_unchanged(DEV, shape, tiling, blend)


@pytest.mark.parametrize("shape,tiling,blend", TILED, ids=str)
def test_split_does_not_matter(shape, tiling, blend):
    Vc.split_does_not_matter(DEV, shape, tiling, blend)


def test_output_commutes_with_a_mirror():
    Vc.output_commutes_with_a_mirror(DEV)


def test_embeds_follow_the_scene():
    Vc.embeds_follow_the_scene(DEV)


@pytest.mark.parametrize("shape,tta", [((2, 3, 5, 7), "flip"), ((1, 3, 64, 23), "flips"), ((2, 3, 12, 12), "d4"), ((1, 3, 65, 65), "d4")], ids=str)
def test_predict_tta_on_whole_tiles(shape, tta):
    Vc.whole_tiles(DEV, shape, tta)


def test_predict_tta_with_embeds():
    Vc.whole_tiles_with_embeds(DEV)


@pytest.mark.parametrize("shape,tiling,blend", TILED[:2] + TILED[-2:], ids=str)
def test_tta_none_is_todays_path(shape, tiling, blend):
    Vc.tta_none_is_todays_path(DEV, shape, tiling, blend)


def test_device_entries_reject_bad_arguments_before_any_launch():
    from nirgan_hip import lib as L
    Vc.entries_reject_bad_arguments(L.backend())
    torch.cuda.synchronize()


def test_real_generator_with_d4():
    """case 10: a small 6-block generator on a (1, 3, 40, 52) scene, tile 32, margin 4.  What the model was given are the views of
    the plain run's tiles, and the scene is the restated merge + scatter of what it answered -- bitwise, so the bound is the new
    code's alone; nothing is asserted against a separately batched model run (an engine's plan may depend on the batch size)."""
    from model import networks
    from nirgan_hip.inference import predict_tiled
    torch.manual_seed(0)
    net = networks.define_G(3, 1, 8, "resnet_6blocks", "instance", False, "normal", 0.02).to(DEV).eval()
    shape, tiling = (1, 3, 40, 52), (32, 4, 0)
    scene = Bc.scene_of(shape).to(DEV)
    plain = Bc.Recorder(net)
    predict_tiled(plain, scene, tile=32, margin=4, batch=8)
    seen_plain, _ = plain.tiles()
    rec = Bc.Recorder(net)
    got = predict_tiled(rec, scene, tile=32, margin=4, batch=16, tta="d4")
    assert bool(torch.isfinite(got).all())
    Vc.check_against_recorded(DEV, got, rec, seen_plain, shape, tiling, "none", 8)
