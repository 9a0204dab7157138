"""Hold-out inside a scene pool without a GPU: ``split`` / ``split_blocks`` of nirgan_hip.data.ScenePool and the two halves of a
``PoolSplit`` on the numpy statement of nirgan_scene_sample_origins (tests/emu_scene_split.py), the slab sweep against a brute-force
mask, the uniformity of the draw, and the argument checks and struct layout of the real library.  Bodies shared with
tests/test_gpu_scene_split.py (tests/scene_split_cases.py)."""
import ctypes as C
import os
import subprocess

import pytest

import baseline_cases as Bc
import scene_split_cases as Sp
from emu_scene_split import EmuSceneSplit
from nirgan_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQUIVALENCE = [(kind, *case) for kind in ("u16", "f32") for case in Sp.EQUIVALENCE]


@pytest.fixture()
def emu():
    be = EmuSceneSplit()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.mark.parametrize("kind,T,B,augment,scales", EQUIVALENCE, ids=str)
def test_whole_scene_rows_are_the_scaled_sampler(emu, kind, T, B, augment, scales):
    Sp.whole_scene_rows_are_the_scaled_sampler("cpu", kind, T, B, augment, scales)
    assert set(emu.calls) >= {"scene_sample_scaled", "scene_sample_origins"}


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_factor_one_is_scene_sample(emu, kind):
    Sp.factor_one_is_scene_sample("cpu", kind)
    assert "scene_sample_scaled" not in emu.calls                               # scales=None goes through the new entry too


def test_workload_tile(emu):
    Sp.workload_tile("cpu")


def test_sweep_is_the_brute_force_mask():
    Sp.sweep_is_the_brute_force_mask()


def test_tables_and_counts(emu):
    Sp.tables_and_counts("cpu")
    assert "scene_sample_origins" not in emu.calls                              # the tables are set-up: no entry is called for them


@pytest.mark.parametrize("guard", [0, 2])
@pytest.mark.parametrize("with_nodata", [False, True])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_restatement(emu, kind, with_nodata, guard):
    Sp.restatement("cpu", kind, with_nodata, guard)


def test_a_table_of_hundreds_of_rows(emu):
    Sp.a_table_of_hundreds_of_rows("cpu")


@pytest.mark.parametrize("guard", [0, 2])
def test_guarantee(emu, guard):
    Sp.guarantee("cpu", guard)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_val_grid_is_the_double_loop(emu, kind):
    Sp.val_grid_is_the_double_loop("cpu", kind)


def test_uniformity_of_the_restatement():
    Sp.uniformity_of_the_restatement()


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_replay(emu, kind):
    Sp.replay("cpu", kind)


def test_loader_epochs_and_ranks(emu):
    Sp.loader_epochs_and_ranks("cpu")


def test_val_loader_is_fixed(emu):
    Sp.val_loader_is_fixed("cpu")


def test_one_step_is_one_call(emu):
    pool = Sp.pool_of("cpu", Sp.scenes_of(Sp.SHAPES, "u16", 41), "u16")
    ld = pool.split(Sp.VAL).train.loader(3, Sp.T3, 4, seed=1, scales=(1, 2))
    assert emu.calls == []
    list(ld)
    assert emu.calls == ["scene_sample_origins"] * 4


def test_fit_resume_and_validate_mlp(emu, tmp_path):
    Sp.fit_resume_and_validate(lambda seed: Bc.make("mlp", seed, "cpu"), "cpu", tmp_path)


def test_split_blocks_examples(emu):
    Sp.split_blocks_examples("cpu")


def test_python_refusals(emu):
    Sp.python_refusals("cpu")


def test_emulator_rejects_bad_arguments(emu):
    Sp.entry_rejects_bad_arguments(emu)
    Sp.emulator_accepts_what_is_valid(emu)
    assert set(emu.calls) == {"scene_sample_origins"}


def test_real_library_rejects_bad_arguments_before_any_launch():
    assert not L.is_emulated()
    Sp.entry_rejects_bad_arguments(L.backend())


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof and every field offset of nirgan_scene_origins_desc, computed by gcc; its head is nirgan_scene_scaled_desc's"""
    cname, ct = "nirgan_scene_origins_desc", L.SceneOriginsDesc
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
    src += f'printf("%zu %d", sizeof({cname}), NIRGAN_SCENE_ORIGIN_COLS);\n'
    for name, _ in ct._fields_:
        src += f'printf(" %zu", offsetof({cname}, {name}));\n'
    for name, _ in L.SceneScaledDesc._fields_:
        src += f'printf(" %zu", offsetof(nirgan_scene_scaled_desc, {name}));\n'
    src += 'printf("\\n");\nreturn 0;}\n'
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    n = len(ct._fields_)
    assert nums[0] == C.sizeof(ct) and nums[1] == L.SCENE_ORIGIN_COLS == 6
    assert nums[2:2 + n] == [getattr(ct, name).offset for name, _ in ct._fields_]
    assert nums[2 + n:] == nums[2:2 + len(L.SceneScaledDesc._fields_)]
    assert [name for name, _ in ct._fields_[-5:]] == ["origins", "origins_host", "R", "first", "count"]
