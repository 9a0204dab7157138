"""Scene histogram matching without a GPU: ``scene_histogram`` / ``scene_match_lut`` / ``histogram_match_scene`` /
``predict_scene(match=...)`` / ``ScenePool.band_histogram`` on the numpy statement of nirgan_scene_hist / nirgan_scene_match_lut /
nirgan_scene_lut_apply (tests/emu_scene_match.py), that statement pinned to the oracle's ``match_histograms_plane``, plus the argument
checks and the struct layout of the real library.  Bodies shared with tests/test_gpu_scene_match.py (tests/scene_match_cases.py)."""
import ctypes as C
import os
import subprocess

import pytest

import scene_match_cases as Mc
from emu_scene_match import EmuSceneMatch
from nirgan_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def emu():
    be = EmuSceneMatch()
    L.set_backend(be)
    yield be
    L.set_backend(None)


def test_restatement_equals_the_oracle():
    Mc.restatement_equals_the_oracle()


def test_main_input_is_a_real_test():
    Mc.main_input_is_a_real_test()


def test_ties_by_hand():
    Mc.ties_by_hand()


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", Mc.COUNT_SIZES)
def test_count_sizes(emu, n, shift):
    Mc.count_sizes("cpu", n, shift)
    assert emu.calls == ["scene_hist"]


def test_count_every_code_once(emu):
    Mc.count_every_code_once("cpu")


def test_count_one_code(emu):
    Mc.count_one_code("cpu")


def test_count_pools(emu):
    Mc.count_pools("cpu")


def test_count_and_apply_wrap(emu):
    Mc.count_and_apply_wrap("cpu")


@pytest.mark.parametrize("shift_in,shift_out", [(0, 0), (1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("n", Mc.COUNT_SIZES)
def test_apply_sizes(emu, n, shift_in, shift_out):
    Mc.apply_sizes("cpu", n, shift_in, shift_out)


def test_tables(emu):
    Mc.tables("cpu")


def test_ties_on_the_entries(emu):
    Mc.ties_on_the_device("cpu")


def test_main_route(emu):
    Mc.main_route("cpu")


def test_properties(emu):
    Mc.properties("cpu")


def test_nodata_codes(emu):
    Mc.nodata_codes("cpu")


def test_predict_scene_matches(emu):
    Mc.predict_scene_matches("cpu")


def test_predict_scene_without_nodata_reserves_nothing(emu):
    Mc.predict_scene_without_nodata_reserves_nothing("cpu")


def test_python_refusals(emu):
    Mc.python_refusals("cpu")


def test_band_histogram(emu):
    Mc.band_histogram("cpu")
    assert emu.calls.count("scene_hist") == 3 * 2 + 2 + 3                        # one count per scene and call


def test_pool_predict(emu):
    Mc.pool_predict("cpu")
    assert L.backend() is emu


def test_emulator_rejects_bad_arguments(emu):
    Mc.entries_reject_bad_arguments(emu)


def test_real_library_rejects_bad_arguments_before_any_launch():
    assert not L.is_emulated()
    Mc.entries_reject_bad_arguments(L.backend())


def test_struct_layout_matches_the_header(tmp_path):
    """sizeof and every field offset of nirgan_scene_match_desc, and NIRGAN_SCENE_CODES, computed by gcc"""
    cname, ct = "nirgan_scene_match_desc", L.SceneMatchDesc
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
    src += f'printf("%zu %d", sizeof({cname}), NIRGAN_SCENE_CODES);\n'
    for name, _ in ct._fields_:
        src += f'printf(" %zu", offsetof({cname}, {name}));\n'
    src += 'printf("\\n");\nreturn 0;}\n'
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert nums[0] == C.sizeof(ct) and nums[1] == L.SCENE_CODES == 65536
    assert nums[2:] == [getattr(ct, name).offset for name, _ in ct._fields_]
