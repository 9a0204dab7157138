"""The device-resident scene pool without a GPU: nirgan_hip.data.ScenePool, its loader and the ``set_epoch`` hook of ``fit`` on the
numpy statement of the two entries (tests/emu_scene_pool.py), the uniformity of the restated draw, and the argument checks and
struct layouts of the real library.  Bodies shared with tests/test_gpu_scene_pool.py (tests/scene_pool_cases.py)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import api_cases as A
import baseline_cases as Bc
import scene_pool_cases as Sc
from emu_scene_pool import EmuScenePool
from nirgan_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLING = [(kind, T, B, aug) for kind in ("u16", "f32") for T in (5, 4) for B in (1, 3, 17) for aug in ("none", "flips", "d4")]


@pytest.fixture()
def emu():
    be = EmuScenePool()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.mark.parametrize("kind,T,B,augment", SAMPLING, ids=str)
def test_sampling_is_bitwise_the_restatement(emu, kind, T, B, augment):
    Sc.sampling_is_bitwise("cpu", kind, T, B, augment)


def test_workload_width_small(emu):
    Sc.workload_width_small("cpu")


@pytest.mark.parametrize("T", Sc.PARTIAL_TILES)
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_partial_second_block(emu, kind, T):
    Sc.partial_second_block("cpu", kind, T)


def test_small_scenes_are_never_chosen(emu):
    Sc.small_scenes_are_never_chosen("cpu")


def test_views_follow_the_tile_views_rule(emu):
    Sc.views_follow_the_tile_views_rule("cpu")


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("hw", Sc.PREFIX_SHAPES, ids=str)
def test_prefix_table_is_cumsum(emu, hw, kind):
    Sc.prefix_is_cumsum("cpu", hw[0], hw[1], kind)


def test_rejection(emu):
    Sc.rejection_cases("cpu")


def test_determinism_and_sharding(emu):
    Sc.determinism_and_sharding("cpu")


def test_loader_epochs_and_buffers(emu):
    Sc.loader_epochs_and_buffers("cpu")


def test_from_npz(emu, tmp_path):
    Sc.from_npz_round_trip("cpu", tmp_path)


def test_one_sample_is_one_call_and_the_prefix_is_built_once(emu):
    _, pool = Sc.pool3("cpu", nodata=0)
    assert emu.calls == ["scene_invalid_prefix"] * 3
    emu.calls.clear()
    list(pool.loader(2, 4, 3, seed=1))
    assert emu.calls == ["scene_sample"] * 3
    emu.calls.clear()
    Sc.pool3("cpu")
    assert emu.calls == []                                                        # no nodata: no table, 4 bytes per pixel saved


def test_uniformity_of_the_restated_draw():
    Sc.uniformity_of_the_restatement()


def test_fit_resume_mlp(emu, tmp_path):
    Sc.fit_resume_equals_uninterrupted(lambda seed: Bc.make("mlp", seed, "cpu"), "cpu", tmp_path)


def test_fit_resume_px2px(emu, tmp_path):
    """ngf = ndf = 8, tile 24: at tile 16 the PatchGAN's last convolution has no output left (16 -> 8 -> 4 -> 2 -> 1 -> 0) and the
    model refuses the batch wherever it comes from; 24 is the smallest multiple of 8 it takes (24 -> 12 -> 6 -> 3 -> 2 -> 1)"""
    from model.pix2pix import Px2Px_PL
    cfg = A.px_config(6, 8)

    def fresh(seed):
        torch.manual_seed(seed)
        return Px2Px_PL(cfg).to("cpu")
    Sc.fit_resume_equals_uninterrupted(fresh, "cpu", tmp_path, tile=24)


def test_python_refusals(emu):
    Sc.python_refusals("cpu")


def test_cpu_device_without_the_emulator_is_refused():
    assert not L.is_emulated()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Sc.pool3("cpu")


def test_emulator_rejects_bad_arguments(emu):
    Sc.entries_reject_bad_arguments(emu)
    assert set(emu.calls) == {"scene_sample", "scene_invalid_prefix"}


def test_real_library_rejects_bad_arguments_before_any_launch():
    assert not L.is_emulated()
    Sc.entries_reject_bad_arguments(L.backend())


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof and every field offset of the two new descriptors, and the header's constants, computed by gcc"""
    pairs = [("nirgan_scene_prefix_desc", L.ScenePrefixDesc), ("nirgan_scene_sample_desc", L.SceneSampleDesc)]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
    for cname, ct in pairs:
        src += f'printf("%zu", sizeof({cname}));\n'
        for name, _ in ct._fields_:
            src += f'printf(" %zu", offsetof({cname}, {name}));\n'
        src += 'printf("\\n");\n'
    src += 'printf("%d %d %d %d\\n", NIRGAN_SCENE_ATTEMPTS, NIRGAN_SCENE_TABLE_COLS, NIRGAN_SCENE_U16, NIRGAN_SCENE_F32);\nreturn 0;}\n'
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    for (cname, ct), line in zip(pairs, lines):
        nums = [int(x) for x in line.split()]
        assert nums[0] == C.sizeof(ct), cname
        assert nums[1:] == [getattr(ct, name).offset for name, _ in ct._fields_], cname
        assert nums[-1] == getattr(ct, ct._fields_[-1][0]).offset
    assert [int(x) for x in lines[2].split()] == [L.SCENE_ATTEMPTS, L.SCENE_TABLE_COLS, L.SCENE_U16, L.SCENE_F32]
    import emu_scene_pool as E
    assert (E.ATTEMPTS, E.COLS) == (L.SCENE_ATTEMPTS, L.SCENE_TABLE_COLS)
