"""nirgan_location_encoder on the MI355X through its raw entry: the harmonics against numpy longdouble under the conditioning-aware
bound, the Siren layers teacher-forced under a running bound, guards, bits and refusals.  Cases, references, bounds and bodies are in
tests/locenc_cases.py; the same bodies run on the emulator in tests/test_locenc_emulated.py."""
import pytest

import locenc_cases as Lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("L_,variant", Lc.HARMONICS_CASES, ids=lambda v: str(v))
def test_harmonics_against_longdouble(L_, variant):
    Lc.harmonics_against_longdouble(DEV, L_, variant, report=print)


@pytest.mark.parametrize("name", [c[0] for c in Lc.SIREN_CASES])
def test_siren_layers_teacher_forced(name):
    Lc.siren_teacher_forced(DEV, name, report=print)


@pytest.mark.parametrize("name", Lc.BITWISE_CASES)
def test_placement_and_bits(name):
    Lc.placement_and_bits(DEV, name)


def test_module_end_to_end(tmp_path):
    Lc.module_end_to_end(DEV, tmp_path)


def test_refusals():
    from nirgan_hip import lib as L
    Lc.refusals(L.backend())
