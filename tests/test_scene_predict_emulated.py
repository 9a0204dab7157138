"""In-place scene prediction without a GPU: ``predict_scene`` / ``ScenePool.predict`` on the numpy statement of
nirgan_scene_tile_invalid / nirgan_scene_tile_gather / nirgan_scene_finish (tests/emu_scene_predict.py), bitwise against
``predict_tiled(blend="blend")`` on the host-converted scene, plus the argument checks and the struct layout of the real library.
Bodies shared with tests/test_gpu_scene_predict.py (tests/scene_predict_cases.py)."""
import ctypes as C
import os
import subprocess

import pytest

import scene_predict_cases as Sc
from emu_scene_predict import EmuScenePredict
from nirgan_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def emu():
    be = EmuScenePredict()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.mark.parametrize("batch", Sc.BATCHES)
@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("shape", Sc.SCENES, ids=str)
def test_equals_the_float_path(emu, shape, kind, batch):
    Sc.equals_the_float_path("cpu", shape, kind, batch)
    assert "scene_tile_invalid" not in emu.calls


def test_flips_equal_the_float_path(emu):
    Sc.flips_equal_the_float_path("cpu")
    assert "tile_views_merge" in emu.calls


def test_numpy_scene_is_uploaded_as_it_is(emu):
    Sc.numpy_scene_is_uploaded_as_it_is("cpu")


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("shape,every", [(Sc.SCENES[0], 3), (Sc.SCENES[1], None), (Sc.SCENES[2], 2)], ids=str)
def test_gather_alone(emu, shape, every, kind):
    Sc.gather_alone("cpu", shape, kind, Sc.TILING, every)
    Sc.gather_alone("cpu", shape, kind, Sc.TILING, every, with_coords=False)


def test_gather_wide(emu):
    Sc.gather_wide("cpu")


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("shape", [Sc.SKIP_SHAPE, (5, 100, 140)], ids=str)
def test_counts(emu, shape, kind):
    Sc.counts_are_the_brute_force_count("cpu", shape, kind, Sc.TILING)
    Sc.counts_are_the_brute_force_count("cpu", shape, kind, (32, 4, 0))


def test_counts_wide(emu):
    Sc.counts_wide("cpu")


@pytest.mark.parametrize("out", ["uint16", "float16", "float32"])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_skipping(emu, kind, out):
    rec = Sc.skipping("cpu", kind, out)
    n_run = sum(len(x) for x in rec.inputs)
    assert emu.calls.count("scene_tile_invalid") == 1 and emu.calls.count("scene_finish") == 1
    assert emu.calls.count("scene_tile_gather") == -(-n_run // 3)              # the list is compact: ceil(n / batch) model calls
    assert sorted({len(x) for x in rec.inputs}) in ([3], [n_run % 3, 3])        # at most two batch sizes


@pytest.mark.parametrize("window,batch,tta", [("cosine", 8, "none"), ("linear", 1, "none"), ("linear", 8, "flips")])
def test_skipping_other_steps(emu, window, batch, tta):
    Sc.skipping("cpu", "u16", "uint16", window, batch, tta)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_without_nodata_nothing_is_skipped(emu, kind):
    Sc.without_nodata_nothing_is_skipped("cpu", kind)
    assert "scene_tile_invalid" not in emu.calls                                 # no count launch, so no copy to the host either
    # every step is one run of consecutive tiles: one blend per gather (and the float path of the comparison blends once per step too)
    assert emu.calls.count("tile_blend") == 2 * emu.calls.count("scene_tile_gather") == 2 * emu.calls.count("tile_gather_ov")


def test_all_nodata_scene(emu):
    Sc.all_nodata_scene("cpu")
    assert emu.calls == ["scene_tile_invalid", "scene_finish"]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("width", [24, 23])
@pytest.mark.parametrize("out,nodata_out", [("uint16", 0), ("uint16", 7), ("uint16", 65535), ("float16", -1.0), ("float16", float("nan")),
                                            ("float32", float("nan")), ("float32", 3.5)])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_finish_alone(emu, kind, out, nodata_out, width, shift):
    Sc.finish_alone("cpu", kind, out, nodata_out, width, shift)


def test_finish_wraps_its_grid(emu):
    Sc.finish_wraps_its_grid("cpu")


@pytest.mark.parametrize("tta", ["none", "flips"])
def test_coords_per_tile(emu, tta):
    Sc.coords_per_tile("cpu", tta)


def test_one_row_for_every_tile(emu):
    Sc.one_row_for_every_tile("cpu")


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_pool_predict(emu, kind):
    Sc.pool_predict("cpu", kind)
    assert L.backend() is emu


def test_python_refusals(emu):
    Sc.python_refusals("cpu")
    assert emu.calls == []


def test_emulator_rejects_bad_arguments(emu):
    Sc.entries_reject_bad_arguments(emu)


def test_real_library_rejects_bad_arguments_before_any_launch():
    assert not L.is_emulated()
    Sc.entries_reject_bad_arguments(L.backend())


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof and every field offset of nirgan_scene_predict_desc, and the three output kinds, computed by gcc"""
    cname, ct = "nirgan_scene_predict_desc", L.ScenePredictDesc
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
    src += f'printf("%zu %d %d %d", sizeof({cname}), NIRGAN_SCENE_OUT_U16, NIRGAN_SCENE_OUT_F16, NIRGAN_SCENE_OUT_F32);\n'
    for name, _ in ct._fields_:
        src += f'printf(" %zu", offsetof({cname}, {name}));\n'
    src += 'printf("\\n");\nreturn 0;}\n'
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert nums[0] == C.sizeof(ct)
    assert nums[1:4] == [L.SCENE_OUT_U16, L.SCENE_OUT_F16, L.SCENE_OUT_F32] == [L.SCENE_OUT_KINDS[k] for k in ("uint16", "float16", "float32")]
    assert nums[4:] == [getattr(ct, name).offset for name, _ in ct._fields_]
