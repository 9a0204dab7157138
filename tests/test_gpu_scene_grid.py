"""The explicit window gather and the validation grid on the MI355X: nirgan_scene_gather through ``gather`` / ``grid`` /
``grid_loader`` of nirgan_hip.data.ScenePool, bitwise against what the two samplers delivered for the same window rows and against
the numpy restatement (tests/emu_scene_grid.py; bodies: tests/scene_grid_cases.py) -- guarded outputs, an exactly allocated pool,
every factor and view, windows at the scenes' far corners, a tile past the 64-block, the workload's width, the grid's nodata filter on
the device's prefix tables, and ``fit`` / ``evaluate_tiles`` on a grid loader."""
import pytest
import torch

import baseline_cases as Bc
import scene_grid_cases as Sg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPLAY = [(kind, *case[1:], with_scales) for kind in ("u16", "f32") for case in Sg.REPLAY for with_scales in (False, True)]


@pytest.mark.parametrize("kind,shapes,T,scales,B,with_scales", REPLAY, ids=str)
def test_replay_of_a_sampled_batch(kind, shapes, T, scales, B, with_scales):
    Sg.replay(DEV, kind, shapes, T, scales if with_scales else None, B)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_replay_ignores_attempt_and_exhausted(kind):
    Sg.replay_exhausted(DEV, kind)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_explicit_windows(kind):
    Sg.explicit_windows(DEV, kind)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_explicit_parts(kind):
    Sg.explicit_parts(DEV, kind)


def test_workload_width():
    Sg.workload_width(DEV)


def test_grid_is_the_double_loop():
    Sg.grid_is_the_double_loop(DEV)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_grid_rejects_like_the_sampler(kind):
    Sg.grid_rejects_like_the_sampler(DEV, kind)


def test_grid_refusals():
    Sg.grid_refusals(DEV)


def test_loader_is_fixed():
    Sg.loader_is_fixed(DEV)


def test_loader_ranks_and_factors():
    Sg.loader_ranks_and_factors(DEV)


def test_fit_and_evaluate_mlp():
    Sg.fit_and_evaluate(lambda seed: Bc.make("mlp", seed, DEV), DEV)


def test_device_entry_rejects_bad_arguments_before_any_launch():
    from nirgan_hip import lib as L
    Sg.entry_rejects_bad_arguments(L.backend())
    torch.cuda.synchronize()
