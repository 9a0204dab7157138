"""In-place scene prediction on the MI355X: nirgan_scene_tile_invalid / nirgan_scene_tile_gather / nirgan_scene_finish alone (guarded
buffers, exactly allocated scenes, lists with gaps, grids that wrap) and under ``predict_scene`` / ``ScenePool.predict``, bitwise
against ``predict_tiled(blend="blend")`` on the host-converted scene and against the numpy restatement (tests/emu_scene_predict.py;
bodies: tests/scene_predict_cases.py), and one case with a real generator."""
import pytest
import torch

import scene_predict_cases as Sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("batch", Sc.BATCHES)
@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("shape", Sc.SCENES, ids=str)
def test_equals_the_float_path(shape, kind, batch):
    Sc.equals_the_float_path(DEV, shape, kind, batch)


def test_flips_equal_the_float_path():
    Sc.flips_equal_the_float_path(DEV)


def test_numpy_scene_is_uploaded_as_it_is():
    Sc.numpy_scene_is_uploaded_as_it_is(DEV)


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("shape,every", [(Sc.SCENES[0], 3), (Sc.SCENES[1], None), (Sc.SCENES[2], 2)], ids=str)
def test_gather_alone(shape, every, kind):
    Sc.gather_alone(DEV, shape, kind, Sc.TILING, every)
    Sc.gather_alone(DEV, shape, kind, Sc.TILING, every, with_coords=False)


def test_gather_wide():
    Sc.gather_wide(DEV)


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("shape", [Sc.SKIP_SHAPE, (5, 100, 140)], ids=str)
def test_counts(shape, kind):
    Sc.counts_are_the_brute_force_count(DEV, shape, kind, Sc.TILING)
    Sc.counts_are_the_brute_force_count(DEV, shape, kind, (32, 4, 0))


def test_counts_wide():
    Sc.counts_wide(DEV)


@pytest.mark.parametrize("out", ["uint16", "float16", "float32"])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_skipping(kind, out):
    Sc.skipping(DEV, kind, out)


@pytest.mark.parametrize("window,batch,tta", [("cosine", 8, "none"), ("linear", 1, "none"), ("linear", 8, "flips")])
def test_skipping_other_steps(window, batch, tta):
    Sc.skipping(DEV, "u16", "uint16", window, batch, tta)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_without_nodata_nothing_is_skipped(kind):
    Sc.without_nodata_nothing_is_skipped(DEV, kind)


def test_all_nodata_scene():
    Sc.all_nodata_scene(DEV)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("width", [24, 23])
@pytest.mark.parametrize("out,nodata_out", [("uint16", 0), ("uint16", 7), ("uint16", 65535), ("float16", -1.0), ("float16", float("nan")),
                                            ("float32", float("nan")), ("float32", 3.5)])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_finish_alone(kind, out, nodata_out, width, shift):
    Sc.finish_alone(DEV, kind, out, nodata_out, width, shift)


def test_finish_wraps_its_grid():
    Sc.finish_wraps_its_grid(DEV)


@pytest.mark.parametrize("tta", ["none", "flips"])
def test_coords_per_tile(tta):
    Sc.coords_per_tile(DEV, tta)


def test_one_row_for_every_tile():
    Sc.one_row_for_every_tile(DEV)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_pool_predict(kind):
    Sc.pool_predict(DEV, kind)


def test_python_refusals():
    Sc.python_refusals(DEV)


def test_device_entries_reject_bad_arguments_before_any_launch():
    from nirgan_hip import lib as L
    Sc.entries_reject_bad_arguments(L.backend())
    torch.cuda.synchronize()


def test_real_generator():
    Sc.real_generator(DEV)
