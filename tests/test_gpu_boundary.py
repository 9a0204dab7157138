"""The kernels at the two ends of both networks on the MI355X (nirgan_nchw_to_halo, nirgan_tap_gather, nirgan_conv_channel_dgrad,
nirgan_endconv_fwd / _dz / _dgrad / _wgrad), each raw entry on every launch route against float64 under the derived bounds of
tests/boundary_cases.py (cases, inputs, references, bounds and bodies are there)."""
import pytest

import boundary_cases as Bc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("writes", Bc.HALO_CASES, ids=str)
def test_nchw_to_halo_writes_its_window_and_nothing_else(writes):
    Bc.halo_against_float64(DEV, writes)


def test_nchw_to_halo_guards():
    Bc.halo_guards(DEV)


@pytest.mark.parametrize("case", Bc.GATHER_CASES, ids=Bc.gather_id)
def test_tap_gather(case):
    Bc.gather_against_float64(DEV, case)


def test_tap_gather_guards():
    Bc.gather_guards(DEV)


@pytest.mark.parametrize("case", Bc.DGRAD_CASES, ids=str)
def test_conv_channel_dgrad(case):
    Bc.dgrad_against_float64(DEV, case)


def test_conv_channel_dgrad_guards():
    Bc.dgrad_guards(DEV)


@pytest.mark.parametrize("case", Bc.END_CASES, ids=str)
def test_endconv(case):
    Bc.end_against_float64(DEV, case)
