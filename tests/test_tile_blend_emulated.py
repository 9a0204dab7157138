"""Blended tiled inference without a GPU: predict_tiled(blend="blend") on the numpy statement of the overlapping-tile entries
(tests/emu_tile_blend.py) against the float64 restatement of the geometry, and the argument checks, tile counts and struct layout of
the real library.  Bodies shared with tests/test_gpu_tile_blend.py (tests/tile_blend_cases.py)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import tile_blend_cases as Bc
from emu_tile_blend import EmuTileBlend
from nirgan_hip import lib as L
from nirgan_hip.inference import predict_tiled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(s, t) for s in Bc.SCENES for t in Bc.TILINGS]
OLD_PATH_CASES = [(s, t) for s in Bc.SCENES[1:2] + Bc.SCENES[3:] for t in (Bc.TILINGS[0], Bc.TILINGS[3], Bc.TILINGS[4])]


@pytest.fixture()
def emu():
    be = EmuTileBlend()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.mark.parametrize("shape,tiling", CASES, ids=str)
def test_partition_of_unity(emu, shape, tiling):
    Bc.partition_of_unity("cpu", shape, tiling)
    assert set(emu.calls) == {"tile_gather_ov", "tile_blend"}


@pytest.mark.parametrize("shape,tiling", CASES, ids=str)
def test_against_float64(emu, shape, tiling):
    Bc.against_float64("cpu", shape, tiling)


@pytest.mark.parametrize("shape,tiling", [(s, t) for s in Bc.SCENES[2:4] for t in Bc.TILINGS], ids=str)
def test_result_is_bitwise_independent_of_the_launch_split(emu, shape, tiling):
    Bc.split_independence("cpu", shape, tiling)


@pytest.mark.parametrize("shape,tiling", CASES, ids=str)
def test_raw_entries_need_no_initialisation_and_keep_their_guards(emu, shape, tiling):
    Bc.raw_entries_need_no_initialisation("cpu", shape, tiling)


@pytest.mark.parametrize("shape,tiling", OLD_PATH_CASES, ids=str)
def test_overlap_zero_equals_todays_path(emu, shape, tiling):
    Bc.overlap_zero_is_todays_path("cpu", shape, tiling)
    assert "tile_scatter" in emu.calls and "tile_blend" in emu.calls


def test_embeds_follow_the_scene(emu):
    Bc.embeds_follow_the_scene("cpu")


@pytest.mark.parametrize("tiling", Bc.TILINGS, ids=str)
def test_seam_moves_as_designed(emu, tiling):
    Bc.seam_moves_as_designed("cpu", tiling)


def test_blend_none_runs_todays_calls_and_bad_arguments_raise(emu):
    scene = Bc.scene_of((1, 3, 37, 50))
    predict_tiled(Bc.take0, scene, tile=16, margin=2, batch=8)
    plain = list(emu.calls)
    emu.calls.clear()
    predict_tiled(Bc.take0, scene, tile=16, margin=2, batch=8, blend="none", overlap=5, window="cosine")
    assert emu.calls == plain and set(plain) == {"tile_gather", "tile_scatter"}
    # overlap defaults to core // 4
    emu.calls.clear()
    a = predict_tiled(Bc.tile_ramp, scene, tile=16, margin=2, blend="blend")
    assert emu.calls.count("tile_blend") == -(-Bc.count(1, 37, 50, 16, 2, 3) // 8)
    assert torch.equal(a, predict_tiled(Bc.tile_ramp, scene, tile=16, margin=2, blend="blend", overlap=3))
    half = predict_tiled(Bc.take0, scene.half(), tile=16, margin=2, blend="blend")
    assert half.dtype == torch.float16                                            # the output dtype follows rgb
    for bad in (-1, 7, 12):
        with pytest.raises(ValueError, match="overlap"):
            predict_tiled(Bc.take0, scene, tile=16, margin=2, blend="blend", overlap=bad)
    with pytest.raises(ValueError, match="window"):
        predict_tiled(Bc.take0, scene, tile=16, margin=2, blend="blend", window="hann")
    with pytest.raises(ValueError, match="blend"):
        predict_tiled(Bc.take0, scene, tile=16, margin=2, blend="feather")
    L.set_backend(None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        predict_tiled(Bc.take0, scene, tile=16, margin=2, blend="blend")


def _bad_fields():
    return [("scene", None, b"null"), ("tiles", None, b"null"), ("overlap", -1, b"overlap"), ("overlap", 7, b"overlap"),
            ("margin", 8, b"margin"), ("margin", -1, b"margin"), ("first", -1, b"tiles"), ("first", 20, b"tiles"), ("n", 0, b"tiles"),
            ("n", 21, b"tiles"), ("window", 2, b"window"), ("window", -1, b"window"), ("B", 0, b"shape"), ("C", 0, b"shape"),
            ("H", 1 << 27, b"2^31"), ("C", 1 << 23, b"2^31"), ("B", 1 << 28, b"2^31")]


def _valid_desc(buf):
    d = L.TileBlendDesc()
    d.B, d.C, d.H, d.W, d.tile, d.margin, d.overlap, d.window, d.first, d.n = 1, 3, 37, 29, 16, 2, 4, 0, 0, 20      # 5 x 4 tiles
    d.scene = d.tiles = buf.data_ptr()
    return d


def test_emulator_rejects_bad_arguments(emu):
    buf = torch.zeros(64)
    d = _valid_desc(buf)
    for entry in ("nirgan_tile_gather_ov", "nirgan_tile_blend"):
        for field, value, _ in _bad_fields():
            keep = getattr(d, field)
            setattr(d, field, value)
            assert getattr(emu, entry)(C.byref(d)) == -1 and entry[7:].encode() in emu.nirgan_last_error(), (entry, field)
            setattr(d, field, keep)
    assert (buf == 0).all()


def test_real_library_rejects_bad_arguments_before_any_launch_and_counts_agree():
    be = L.backend()
    assert not L.is_emulated()
    for entry in ("nirgan_tile_gather_ov", "nirgan_tile_blend"):
        fn = getattr(be, entry)
        assert fn(None, None) == -1 and entry[7:].encode() in be.nirgan_last_error()
        assert fn(L.TileBlendDesc(), None) == -1 and b"null" in be.nirgan_last_error()
        buf = torch.zeros(64)
        d = _valid_desc(buf)
        for field, value, word in _bad_fields():
            keep = getattr(d, field)
            setattr(d, field, value)
            assert fn(d, None) == -1, (entry, field)
            msg = be.nirgan_last_error()
            assert entry[7:].encode() in msg and word in msg, (entry, field, msg)
            setattr(d, field, keep)
    emu = EmuTileBlend()
    for (B, _, H, W) in Bc.SCENES + [(1, 3, 4096, 4096), (3, 3, 481, 960)]:
        for tiling in Bc.TILINGS + [(512, 16, 120), (512, 16, 0), (512, 16, 240)]:
            n = be.nirgan_tile_count_ov(B, H, W, *tiling)
            assert n == emu.nirgan_tile_count_ov(B, H, W, *tiling) == Bc.count(B, H, W, *tiling), (B, H, W, tiling)
            assert be.nirgan_tile_count_ov(B, H, W, tiling[0], tiling[1], 0) == be.nirgan_tile_count(B, H, W, tiling[0], tiling[1])
    assert be.nirgan_tile_count_ov(1, 4096, 4096, 512, 16, 120) == 12 * 12                  # ceil((4096 - 480) / 360) + 1 per axis
    for args in [(0, 8, 8, 16, 2, 4), (1, 0, 8, 16, 2, 4), (1, 8, 8, 16, 8, 0), (1, 8, 8, 16, 2, 7), (1, 8, 8, 16, 2, -1), (1, 8, 8, 0, 0, 0)]:
        assert be.nirgan_tile_count_ov(*args) == 0 and emu.nirgan_tile_count_ov(*args) == 0, args


def test_struct_layout_matches_the_header(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
           'printf("%zu %d %d", sizeof(nirgan_tile_blend_desc), NIRGAN_BLEND_LINEAR, NIRGAN_BLEND_COSINE);\n')
    for name, _ in L.TileBlendDesc._fields_:
        src += f'printf(" %zu", offsetof(nirgan_tile_blend_desc, {name}));\n'
    src += "return 0;}\n"
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert nums[:3] == [C.sizeof(L.TileBlendDesc), L.BLEND_LINEAR, L.BLEND_COSINE]
    assert nums[3:] == [getattr(L.TileBlendDesc, name).offset for name, _ in L.TileBlendDesc._fields_]
