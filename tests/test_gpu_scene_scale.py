"""The multi-scale sampler on the MI355X: nirgan_scene_sample_scaled through ``scales`` / ``scale_weights`` of
nirgan_hip.data.ScenePool, bitwise against the numpy / Python-int restatement (tests/emu_scene_scale.py; bodies:
tests/scene_scale_cases.py) and, independently of it, against float64 avg_pool2d -- guarded outputs, an exactly allocated pool, odd
widths and offsets, partial 64-blocks through both routes of the gather, the largest block sum, the rejection bound at every scale,
the mix of scales, sharding, and ``fit`` on a scaled loader with a checkpoint in the middle."""
import pytest
import torch

import baseline_cases as Bc
import scene_scale_cases as Ss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAMPLING = [(kind, T, B, aug, scales) for kind in ("u16", "f32") for T in (5, 4) for B in (1, 3, 17) for aug in ("none", "flips", "d4")
            for scales in ((1, 2, 3), (2,), (3,))]


@pytest.mark.parametrize("kind,T,B,augment,scales", SAMPLING, ids=str)
def test_sampling_is_bitwise_the_restatement(kind, T, B, augment, scales):
    Ss.sampling_is_bitwise(DEV, kind, T, B, augment, scales)


def test_small_scene_only_at_native_resolution():
    Ss.small_scene_only_at_native_resolution(DEV)


@pytest.mark.parametrize("augment", ["none", "flips", "d4"])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_factor_one_is_scene_sample(kind, augment):
    Ss.factor_one_is_scene_sample(DEV, kind, augment)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_block_boundaries(kind):
    Ss.block_boundaries(DEV, kind)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_every_factor(kind):
    Ss.every_factor(DEV, kind)


def test_top_of_the_factor_range():
    Ss.top_of_the_factor_range(DEV)


def test_workload_width_small():
    Ss.workload_width_small(DEV)


@pytest.mark.parametrize("max_invalid", [0, 1])
@pytest.mark.parametrize("f", [1, 2, 3])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_rejection_bound(kind, f, max_invalid):
    Ss.rejection_bound(DEV, kind, f, max_invalid)


def test_exhausted_keeps_the_scale():
    Ss.exhausted_keeps_the_scale(DEV)


def test_scale_mix():
    Ss.scale_mix(DEV)


def test_scale_does_not_depend_on_rejection():
    Ss.scale_does_not_depend_on_rejection(DEV)


def test_determinism_and_sharding():
    Ss.determinism_and_sharding(DEV)


def test_loader_epochs_and_buffers():
    Ss.loader_epochs_and_buffers(DEV)


def test_fit_resume_mlp(tmp_path):
    Ss.fit_resume_equals_uninterrupted(lambda seed: Bc.make("mlp", seed, DEV), DEV, tmp_path)


def test_python_refusals():
    Ss.python_refusals(DEV)


def test_device_entry_rejects_bad_arguments_before_any_launch():
    from nirgan_hip import lib as L
    Ss.entry_rejects_bad_arguments(L.backend())
    torch.cuda.synchronize()
