"""The explicit window gather and the validation grid without a GPU: ``grid`` / ``gather`` / ``grid_loader`` of
nirgan_hip.data.ScenePool on the numpy statement of nirgan_scene_gather (tests/emu_scene_grid.py), the grid against a plain double
loop, and the argument checks and struct layout of the real library.  Bodies shared with tests/test_gpu_scene_grid.py
(tests/scene_grid_cases.py)."""
import ctypes as C
import os
import subprocess

import pytest

import baseline_cases as Bc
import scene_grid_cases as Sg
from emu_scene_grid import EmuSceneGrid
from nirgan_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAY = [(kind, *case[1:], with_scales) for kind in ("u16", "f32") for case in Sg.REPLAY for with_scales in (False, True)]


@pytest.fixture()
def emu():
    be = EmuSceneGrid()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.mark.parametrize("kind,shapes,T,scales,B,with_scales", REPLAY, ids=str)
def test_replay_of_a_sampled_batch(emu, kind, shapes, T, scales, B, with_scales):
    Sg.replay("cpu", kind, shapes, T, scales if with_scales else None, B)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_replay_ignores_attempt_and_exhausted(emu, kind):
    Sg.replay_exhausted("cpu", kind)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_explicit_windows(emu, kind):
    Sg.explicit_windows("cpu", kind)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_explicit_parts(emu, kind):
    Sg.explicit_parts("cpu", kind)


def test_workload_width(emu):
    Sg.workload_width("cpu")


def test_grid_is_the_double_loop(emu):
    Sg.grid_is_the_double_loop("cpu")
    assert "scene_gather" not in emu.calls                                       # the grid is set-up: no entry is called for it


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_grid_rejects_like_the_sampler(emu, kind):
    Sg.grid_rejects_like_the_sampler("cpu", kind)


def test_grid_refusals(emu):
    Sg.grid_refusals("cpu")


def test_loader_is_fixed(emu):
    Sg.loader_is_fixed("cpu")


def test_loader_ranks_and_factors(emu):
    Sg.loader_ranks_and_factors("cpu")


def test_one_batch_is_one_call(emu):
    _, pool = Sg.loader_pool("cpu")
    ld = pool.grid_loader(4, Sg.GRID_T)
    assert emu.calls == []
    list(ld)
    assert emu.calls == ["scene_gather"] * len(ld)


def test_fit_and_evaluate_mlp(emu):
    Sg.fit_and_evaluate(lambda seed: Bc.make("mlp", seed, "cpu"), "cpu")


def test_cpu_pool_without_the_emulator_raises():
    assert not L.is_emulated()
    with pytest.raises(RuntimeError, match="cuda"):
        Sg.make_pool("cpu", Sg.make_scenes(Sg.GRID_SHAPES, "u16", 77), "u16")


def test_emulator_rejects_bad_arguments(emu):
    Sg.entry_rejects_bad_arguments(emu)
    Sg.emulator_accepts_what_is_valid(emu)
    assert set(emu.calls) == {"scene_gather"}


def test_real_library_rejects_bad_arguments_before_any_launch():
    assert not L.is_emulated()
    Sg.entry_rejects_bad_arguments(L.backend())


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof and every field offset of nirgan_scene_gather_desc, computed by gcc"""
    cname, ct = "nirgan_scene_gather_desc", L.SceneGatherDesc
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
    src += f'printf("%zu", sizeof({cname}));\n'
    for name, _ in ct._fields_:
        src += f'printf(" %zu", offsetof({cname}, {name}));\n'
    src += 'printf("\\n");\nreturn 0;}\n'
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert nums[0] == C.sizeof(ct)
    assert nums[1:] == [getattr(ct, name).offset for name, _ in ct._fields_]
    assert ct._fields_[-1][0] == "coords"
