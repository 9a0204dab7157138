"""The multi-scale sampler without a GPU: ``scales`` / ``scale_weights`` of nirgan_hip.data.ScenePool and its loader on the numpy
statement of nirgan_scene_sample_scaled (tests/emu_scene_scale.py), the restated mix of scales, and the argument checks and struct
layout of the real library.  Bodies shared with tests/test_gpu_scene_scale.py (tests/scene_scale_cases.py)."""
import ctypes as C
import os
import subprocess

import pytest

import baseline_cases as Bc
import scene_scale_cases as Ss
from emu_scene_scale import EmuSceneScale
from nirgan_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLING = [(kind, T, B, aug, scales) for kind in ("u16", "f32") for T in (5, 4) for B in (1, 3, 17) for aug in ("none", "flips", "d4")
            for scales in ((1, 2, 3), (2,), (3,))]


@pytest.fixture()
def emu():
    be = EmuSceneScale()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.mark.parametrize("kind,T,B,augment,scales", SAMPLING, ids=str)
def test_sampling_is_bitwise_the_restatement(emu, kind, T, B, augment, scales):
    Ss.sampling_is_bitwise("cpu", kind, T, B, augment, scales)


def test_small_scene_only_at_native_resolution(emu):
    Ss.small_scene_only_at_native_resolution("cpu")


@pytest.mark.parametrize("augment", ["none", "flips", "d4"])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_factor_one_is_scene_sample(emu, kind, augment):
    Ss.factor_one_is_scene_sample("cpu", kind, augment)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_block_boundaries(emu, kind):
    Ss.block_boundaries("cpu", kind)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_every_factor(emu, kind):
    Ss.every_factor("cpu", kind)


def test_top_of_the_factor_range(emu):
    Ss.top_of_the_factor_range("cpu")


def test_workload_width_small(emu):
    Ss.workload_width_small("cpu")


@pytest.mark.parametrize("max_invalid", [0, 1])
@pytest.mark.parametrize("f", [1, 2, 3])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_rejection_bound(emu, kind, f, max_invalid):
    Ss.rejection_bound("cpu", kind, f, max_invalid)


def test_exhausted_keeps_the_scale(emu):
    Ss.exhausted_keeps_the_scale("cpu")


def test_scale_mix_of_the_restatement():
    Ss.scale_mix_of_the_restatement()


def test_scale_mix(emu):
    Ss.scale_mix("cpu")


def test_scale_does_not_depend_on_rejection(emu):
    Ss.scale_does_not_depend_on_rejection("cpu")


def test_determinism_and_sharding(emu):
    Ss.determinism_and_sharding("cpu")


def test_loader_epochs_and_buffers(emu):
    Ss.loader_epochs_and_buffers("cpu")


def test_one_sample_is_one_call_and_no_scales_is_the_old_entry(emu):
    _, pool = Ss.pool4("cpu")
    list(pool.loader(2, 4, 3, seed=1))
    pool.sample(2, 4, seed=1, draw=0)
    assert emu.calls == ["scene_sample"] * 4
    emu.calls.clear()
    list(pool.loader(2, 4, 3, seed=1, scales=(1, 2)))
    pool.sample(2, 4, seed=1, draw=0, scales=(1,))
    assert emu.calls == ["scene_sample_scaled"] * 4


def test_fit_resume_mlp(emu, tmp_path):
    Ss.fit_resume_equals_uninterrupted(lambda seed: Bc.make("mlp", seed, "cpu"), "cpu", tmp_path)


def test_python_refusals(emu):
    Ss.python_refusals("cpu")


def test_emulator_rejects_bad_arguments(emu):
    Ss.entry_rejects_bad_arguments(emu)
    assert set(emu.calls) == {"scene_sample_scaled"}


def test_real_library_rejects_bad_arguments_before_any_launch():
    assert not L.is_emulated()
    Ss.entry_rejects_bad_arguments(L.backend())


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof and every field offset of nirgan_scene_scaled_desc, and the two new constants, computed by gcc"""
    cname, ct = "nirgan_scene_scaled_desc", L.SceneScaledDesc
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
    src += f'printf("%zu", sizeof({cname}));\n'
    for name, _ in ct._fields_:
        src += f'printf(" %zu", offsetof({cname}, {name}));\n'
    src += 'printf("\\n%d %d\\n", NIRGAN_SCENE_MAX_SCALES, NIRGAN_SCENE_MAX_FACTOR);\nreturn 0;}\n'
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    nums = [int(x) for x in lines[0].split()]
    assert nums[0] == C.sizeof(ct)
    assert nums[1:] == [getattr(ct, name).offset for name, _ in ct._fields_]
    assert ct._fields_[-1][0] == "weight" and nums[-1] == ct.weight.offset
    assert [int(x) for x in lines[1].split()] == [L.SCENE_MAX_SCALES, L.SCENE_MAX_FACTOR]
    import emu_scene_scale as ES
    assert (ES.MAX_SCALES, ES.MAX_FACTOR) == (L.SCENE_MAX_SCALES, L.SCENE_MAX_FACTOR)
    assert [f for f, _ in ct._fields_[:len(L.SceneSampleDesc._fields_)]] == [f for f, _ in L.SceneSampleDesc._fields_]
