"""The device-resident scene pool on the MI355X: nirgan_scene_invalid_prefix / nirgan_scene_sample through nirgan_hip.data.ScenePool,
bitwise against the numpy / Python-int restatement (tests/emu_scene_pool.py; bodies: tests/scene_pool_cases.py) -- guarded outputs,
an exactly allocated pool, odd widths and offsets, scan boundaries of the prefix table, the rejection rule, sharding, and ``fit`` on
the pool's loader with a checkpoint in the middle."""
import pytest
import torch

import baseline_cases as Bc
import scene_pool_cases as Sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAMPLING = [(kind, T, B, aug) for kind in ("u16", "f32") for T in (5, 4) for B in (1, 3, 17) for aug in ("none", "flips", "d4")]


@pytest.mark.parametrize("kind,T,B,augment", SAMPLING, ids=str)
def test_sampling_is_bitwise_the_restatement(kind, T, B, augment):
    Sc.sampling_is_bitwise(DEV, kind, T, B, augment)


def test_workload_width_small():
    Sc.workload_width_small(DEV)


@pytest.mark.parametrize("T", Sc.PARTIAL_TILES)
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_partial_second_block(kind, T):
    Sc.partial_second_block(DEV, kind, T)


def test_small_scenes_are_never_chosen():
    Sc.small_scenes_are_never_chosen(DEV)


def test_views_follow_the_tile_views_rule():
    Sc.views_follow_the_tile_views_rule(DEV)


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("hw", Sc.PREFIX_SHAPES, ids=str)
def test_prefix_table_is_cumsum(hw, kind):
    Sc.prefix_is_cumsum(DEV, hw[0], hw[1], kind)


def test_rejection():
    Sc.rejection_cases(DEV)


def test_determinism_and_sharding():
    Sc.determinism_and_sharding(DEV)


def test_loader_epochs_and_buffers():
    Sc.loader_epochs_and_buffers(DEV)


def test_from_npz(tmp_path):
    Sc.from_npz_round_trip(DEV, tmp_path)


def test_fit_resume_mlp(tmp_path):
    Sc.fit_resume_equals_uninterrupted(lambda seed: Bc.make("mlp", seed, DEV), DEV, tmp_path)


def test_python_refusals():
    Sc.python_refusals(DEV)


def test_device_entries_reject_bad_arguments_before_any_launch():
    from nirgan_hip import lib as L
    Sc.entries_reject_bad_arguments(L.backend())
    torch.cuda.synchronize()
