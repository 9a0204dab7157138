"""Hold-out inside a scene pool on the MI355X: nirgan_scene_sample_origins through ``split`` / ``split_blocks`` of
nirgan_hip.data.ScenePool, bitwise against nirgan_scene_sample_scaled / nirgan_scene_sample on whole-scene rows and against the numpy
restatement (tests/emu_scene_split.py; bodies: tests/scene_split_cases.py) -- guarded outputs, an exactly allocated pool, three
scales with a cum that restarts, a table of hundreds of rows, the workload's tile, the guarantee on 4096 samples of a mostly-nodata
scene, replay through nirgan_scene_gather, both loaders and ``fit``."""
import pytest
import torch

import baseline_cases as Bc
import scene_split_cases as Sp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EQUIVALENCE = [(kind, *case) for kind in ("u16", "f32") for case in Sp.EQUIVALENCE]


@pytest.mark.parametrize("kind,T,B,augment,scales", EQUIVALENCE, ids=str)
def test_whole_scene_rows_are_the_scaled_sampler(kind, T, B, augment, scales):
    Sp.whole_scene_rows_are_the_scaled_sampler(DEV, kind, T, B, augment, scales)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_factor_one_is_scene_sample(kind):
    Sp.factor_one_is_scene_sample(DEV, kind)


def test_workload_tile():
    Sp.workload_tile(DEV)


def test_tables_and_counts():
    Sp.tables_and_counts(DEV)


@pytest.mark.parametrize("guard", [0, 2])
@pytest.mark.parametrize("with_nodata", [False, True])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_restatement(kind, with_nodata, guard):
    Sp.restatement(DEV, kind, with_nodata, guard)


def test_a_table_of_hundreds_of_rows():
    Sp.a_table_of_hundreds_of_rows(DEV)


@pytest.mark.parametrize("guard", [0, 2])
def test_guarantee(guard):
    Sp.guarantee(DEV, guard)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_val_grid_is_the_double_loop(kind):
    Sp.val_grid_is_the_double_loop(DEV, kind)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_replay(kind):
    Sp.replay(DEV, kind)


def test_loader_epochs_and_ranks():
    Sp.loader_epochs_and_ranks(DEV)


def test_val_loader_is_fixed():
    Sp.val_loader_is_fixed(DEV)


def test_fit_resume_and_validate_mlp(tmp_path):
    Sp.fit_resume_and_validate(lambda seed: Bc.make("mlp", seed, DEV), DEV, tmp_path)


def test_split_blocks_examples():
    Sp.split_blocks_examples(DEV)


def test_python_refusals():
    Sp.python_refusals(DEV)


def test_device_entry_rejects_bad_arguments_before_any_launch():
    from nirgan_hip import lib as L
    Sp.entry_rejects_bad_arguments(L.backend())
    torch.cuda.synchronize()
