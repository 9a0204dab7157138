"""nirgan_instnorm_fwd / nirgan_instnorm_bwd on the MI355X: both raw entries against float64 on every kernel route (fast and general
apply / pass 1 / pass 2, sliced and unsliced finalize, ragged chunks, a producer's partial sums, every output form, norm = 0), under
the derived bounds of tests/instnorm_cases.py (cases, inputs, references, bounds and bodies are there)."""
import pytest

import instnorm_cases as Ic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", list(Ic.FWD))
def test_forward(name):
    Ic.fwd_against_float64(DEV, name)


@pytest.mark.parametrize("name", list(Ic.BWD))
def test_backward(name):
    Ic.bwd_against_float64(DEV, name)


def test_argument_guards():
    Ic.guards(DEV)
