"""Dihedral test-time augmentation without a GPU: predict_tiled(tta=...) and predict_tta on the numpy statement of the view entries
(tests/emu_tile_views.py) against the np.flip / np.swapaxes restatement, and the argument checks and struct layout of the real
library.  Bodies shared with tests/test_gpu_tile_views.py (tests/tile_views_cases.py)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import tile_blend_cases as Bc
import tile_views_cases as Vc
from emu_tile_views import EmuTileViews
from nirgan_hip import lib as L
from nirgan_hip.inference import predict_tiled, predict_tta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILED = [(s, t, b) for s in Vc.SCENES for t in Vc.TILINGS for b in Vc.BLENDS]


@pytest.fixture()
def emu():
    be = EmuTileViews()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("hw,k", Vc.SHAPE_VIEWS, ids=str)
def test_expand_is_bitwise_the_restated_views(emu, hw, k, shift):
    Vc.expand_is_bitwise("cpu", hw, k, shift)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("hw,k", Vc.SHAPE_VIEWS, ids=str)
def test_merge_is_bitwise_the_restated_tree(emu, hw, k, shift):
    Vc.merge_is_bitwise("cpu", hw, k, shift)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("hw,k", Vc.SHAPE_VIEWS, ids=str)
def test_merge_of_expand_is_the_input(emu, hw, k, shift):
    Vc.round_trip_is_bitwise("cpu", hw, k, shift)


@pytest.mark.parametrize("shape,tiling,blend", TILED, ids=str)
def test_model_sees_the_right_views(emu, shape, tiling, blend):
    Vc.model_sees_the_right_views("cpu", shape, tiling, blend)


@pytest.mark.parametrize("shape,tiling,blend", TILED, ids=str)
def test_equivariant_model_is_unchanged(emu, shape, tiling, blend):
    Vc.equivariant_model_is_unchanged("cpu", shape, tiling, blend)


@pytest.mark.parametrize("shape,tiling,blend", TILED, ids=str)
def test_split_does_not_matter(emu, shape, tiling, blend):
    Vc.split_does_not_matter("cpu", shape, tiling, blend)


def test_output_commutes_with_a_mirror(emu):
    Vc.output_commutes_with_a_mirror("cpu")


def test_embeds_follow_the_scene(emu):
    Vc.embeds_follow_the_scene("cpu")


@pytest.mark.parametrize("shape,tta", [((2, 3, 5, 7), "flip"), ((2, 3, 5, 7), "flips"), ((1, 3, 64, 23), "flips"), ((2, 3, 12, 12), "d4"),
                                       ((1, 3, 65, 65), "d4"), ((2, 3, 5, 7), "none")], ids=str)
def test_predict_tta_on_whole_tiles(emu, shape, tta):
    Vc.whole_tiles("cpu", shape, tta)
    assert emu.calls == ([] if tta == "none" else ["tile_views_expand", "tile_views_merge"])


def test_predict_tta_with_embeds(emu):
    Vc.whole_tiles_with_embeds("cpu")


@pytest.mark.parametrize("shape,tiling,blend", TILED, ids=str)
def test_tta_none_is_todays_path(emu, shape, tiling, blend):
    Vc.tta_none_is_todays_path("cpu", shape, tiling, blend)


def test_launches_per_step_and_tta_none_issues_todays_launches(emu):
    scene = Bc.scene_of((1, 3, 37, 50))
    predict_tiled(Bc.take0, scene, tile=16, margin=2, batch=8)
    plain = list(emu.calls)
    emu.calls.clear()
    predict_tiled(Bc.take0, scene, tile=16, margin=2, batch=8, tta="none")
    assert emu.calls == plain and set(plain) == {"tile_gather", "tile_scatter"}
    total = Bc.count(1, 37, 50, 16, 2, 0)
    for tta, k in (("flip", 2), ("flips", 4), ("d4", 8)):
        for batch in (8, 3):
            emu.calls.clear()
            predict_tiled(Bc.take0, scene, tile=16, margin=2, batch=batch, tta=tta)
            steps = -(-total // max(1, batch // k))
            assert emu.calls == ["tile_gather", "tile_views_expand", "tile_views_merge", "tile_scatter"] * steps, (tta, batch)
    emu.calls.clear()
    predict_tiled(Bc.take0, scene, tile=16, margin=2, batch=8, blend="blend", overlap=3, tta="flips")
    steps = -(-Bc.count(1, 37, 50, 16, 2, 3) // 2)
    assert emu.calls == ["tile_gather_ov", "tile_views_expand", "tile_views_merge", "tile_blend"] * steps
    half = predict_tiled(Bc.take0, scene.half(), tile=16, margin=2, tta="d4")
    assert half.dtype == torch.float16                                            # the output dtype follows rgb


def test_bad_arguments_raise_before_any_call(emu):
    scene = Bc.scene_of((1, 3, 37, 50))
    for bad in ("rot90", "D4", "", None, 8):
        with pytest.raises(ValueError, match="tta"):
            predict_tiled(Bc.take0, scene, tile=16, margin=2, tta=bad)
        with pytest.raises(ValueError, match="tta"):
            predict_tta(Bc.take0, scene[..., :37], tta=bad)
    with pytest.raises(ValueError, match="square"):
        predict_tta(Bc.take0, scene, tta="d4")
    with pytest.raises(ValueError, match="square"):
        predict_tta(Bc.take0, scene)                                              # "d4" is the default
    with pytest.raises(ValueError, match="blend"):
        predict_tiled(Bc.take0, scene, tile=16, margin=2, blend="feather", tta="d4")
    with pytest.raises(ValueError, match="window"):
        predict_tiled(Bc.take0, scene, tile=16, margin=2, blend="blend", window="hann", tta="d4")
    with pytest.raises(ValueError, match="overlap"):
        predict_tiled(Bc.take0, scene, tile=16, margin=2, blend="blend", overlap=7, tta="d4")
    assert emu.calls == []
    predict_tta(Bc.take0, scene, tta="flips")                                     # the flips take any extent
    L.set_backend(None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        predict_tiled(Bc.take0, scene, tile=16, margin=2, tta="d4")
    with pytest.raises(RuntimeError, match="no CPU path"):
        predict_tta(Bc.take0, scene, tta="flip")


def test_emulator_rejects_bad_arguments(emu):
    Vc.entries_reject_bad_arguments(emu)


def test_real_library_rejects_bad_arguments_before_any_launch():
    be = L.backend()
    assert not L.is_emulated()
    for entry in ("nirgan_tile_views_expand", "nirgan_tile_views_merge"):
        fn = getattr(be, entry)
        assert fn(None, None) == -1 and entry[7:].encode() in be.nirgan_last_error()
        assert fn(L.TileViewsDesc(), None) == -1 and b"null" in be.nirgan_last_error()
    Vc.entries_reject_bad_arguments(be)


def test_struct_layout_matches_the_header(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
           'printf("%zu", sizeof(nirgan_tile_views_desc));\n')
    for name, _ in L.TileViewsDesc._fields_:
        src += f'printf(" %zu", offsetof(nirgan_tile_views_desc, {name}));\n'
    src += "return 0;}\n"
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert nums[0] == C.sizeof(L.TileViewsDesc)
    assert nums[1:] == [getattr(L.TileViewsDesc, name).offset for name, _ in L.TileViewsDesc._fields_]
    assert L.TTA_VIEWS == Vc.TTA
