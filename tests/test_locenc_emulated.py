"""The location encoder without a GPU: the bodies of tests/locenc_cases.py on the numpy emulator (tests/emu_backend.py), and the checks
that keep their bounds honest -- the constant K against exact factorial ratios, the measured arithmetic term reproduced, the float64
restatement inside every bound with k = 1 ulp (glibc's cos / sin), the refusals on the real library, and emulators with one deliberate,
subtle error each that must fail a body under the device's bound.  Bodies shared with tests/test_gpu_locenc.py."""
import math

import numpy as np
import pytest

import locenc_cases as Lc
from emu_backend import EmuBackend
from nirgan_hip import lib as L


@pytest.fixture()
def emu():
    be = EmuBackend()
    L.set_backend(be)
    yield be
    L.set_backend(None)


# ------------------------------------------------------------------------------------------------ the reference alone
def test_sh_normalisation_against_exact_factorial_ratios():
    Lc.norm_against_exact(45)


@pytest.mark.parametrize("L_,variant", Lc.HARMONICS_CASES, ids=lambda v: str(v))
def test_recorded_arithmetic_term_is_the_measured_one(L_, variant):
    """the float64 restatement against longdouble on the same float64 x and phi: at or below the record, and the record is not inflated"""
    err, S = Lc.measure_arithmetic(L_, variant)
    assert 0.5 * Lc.ARITH[L_] * S <= err <= Lc.ARITH[L_] * S, (err, S, err / S)


def test_exact_poles_give_exact_cosines():
    """what the bodies' exact-zero check at the poles rests on: theta = fl(pi) and 0 give x = -1 and 1 in float64 and in longdouble"""
    ll = Lc.coordinates()
    _, theta = Lc.angles(ll)
    for row, lat in Lc.POLES.items():
        assert ll[row, 1] == lat and math.cos(theta[row]) == (-1.0 if lat > 0 else 1.0) and np.cos(theta.astype(Lc.LD))[row] == (-1 if lat > 0 else 1)


# ------------------------------------------------------------------------------------------------ bodies on the emulator
@pytest.mark.parametrize("L_,variant", Lc.HARMONICS_CASES, ids=lambda v: str(v))
def test_harmonics_against_longdouble_with_one_ulp(emu, L_, variant):
    """the condition on the bound: with k = 1 the restatement alone passes every case (and so passes with the device's k)"""
    Lc.harmonics_against_longdouble("cpu", L_, variant, k=1)
    assert emu.calls == ["locenc", "locenc"]


@pytest.mark.parametrize("name", [c[0] for c in Lc.SIREN_CASES])
def test_siren_layers_teacher_forced(emu, name):
    Lc.siren_teacher_forced("cpu", name)


@pytest.mark.parametrize("name", Lc.BITWISE_CASES)
def test_placement_and_bits(emu, name):
    Lc.placement_and_bits("cpu", name)


def test_module_end_to_end(emu, tmp_path):
    Lc.module_end_to_end("cpu", tmp_path)


def test_refusals_of_the_emulator(emu):
    Lc.refusals(emu)
    assert emu.calls == ["locenc"] * (len(Lc.REFUSALS) + 1)


def test_refusals_of_the_real_library_before_any_launch():
    assert not L.is_emulated()
    Lc.refusals(L.backend())


# ------------------------------------------------------------------------------------------------ mutations
class RecurrenceTakesLlPlusM(EmuBackend):
    def _locenc_step(self, q, am, x, pmmp1, pmm):
        return ((2.0 * q - 1.0) * x * pmmp1 - (q + am) * pmm) / (q - am)


class SineAndCosineSwappedForNegativeM(EmuBackend):
    def _locenc_azimuth(self, m, phi):
        return super()._locenc_azimuth(-m, phi)


class DecodeOffByOneAtPerfectSquares(EmuBackend):
    """sqrt(f) a hair below l at f = l*l and no correction: (l - 1, l), whose recurrence never runs"""

    def _locenc_decode(self, f):
        l = math.isqrt(f)
        if f > 0 and l * l == f:
            l -= 1
        return l, f - l * l - l


class LastRowOfAnOddLayerNotWritten(EmuBackend):
    def _locenc_layer(self, h, W, b, w0, i):
        out = super()._locenc_layer(h, W, b, w0, i)
        if out.shape[1] % 2:
            out[:, -1] = 0.0
        return out


class LastRowOfAnOddLayerFromItsNeighbour(EmuBackend):
    def _locenc_layer(self, h, W, b, w0, i):
        out = super()._locenc_layer(h, W, b, w0, i)
        if out.shape[1] % 2 and out.shape[1] > 1:
            out[:, -1] = out[:, -2]
        return out


class BiasSkippedOnOddRows(EmuBackend):
    def _locenc_layer(self, h, W, b, w0, i):
        if b is not None:
            b = b.copy()
            b[1::2] = 0.0
        return super()._locenc_layer(h, W, b, w0, i)


class FrequencyOfTheNextLayer(EmuBackend):
    def _locenc_layer(self, h, W, b, w0, i):
        return super()._locenc_layer(h, W, b, list(w0[1:]) + [w0[-1]], i)


class FeaturesBeyond1023LeftAtZero(EmuBackend):
    def _locenc_harmonics(self, x, phi, K, L_):
        Y = super()._locenc_harmonics(x, phi, K, L_)
        Y[:, 1024:] = 0.0
        return Y


class CosThetaInFloat32(EmuBackend):
    def _locenc_cos_theta(self, theta):
        return np.cos(theta.astype(np.float32)).astype(np.float64)


class XMovedBy64Ulps(EmuBackend):
    """away from the poles only (|lat| < 84): there the envelope is 1e-14 and has to be tight, not a blanket"""

    def _locenc_cos_theta(self, theta):
        x = super()._locenc_cos_theta(theta)
        return np.where(np.abs(x) < 0.99, x - np.sign(x) * 64 * np.spacing(x), x)


def _harmonics(L_, variant="closed-form"):
    return lambda: Lc.harmonics_against_longdouble("cpu", L_, variant)


def _siren(name):
    return lambda: Lc.siren_teacher_forced("cpu", name)


MUTANTS = [
    (RecurrenceTakesLlPlusM, _harmonics(10)),
    (RecurrenceTakesLlPlusM, _harmonics(10, "analytic")),
    (SineAndCosineSwappedForNegativeM, _harmonics(2)),
    (SineAndCosineSwappedForNegativeM, _harmonics(10, "analytic-generator-text")),
    (DecodeOffByOneAtPerfectSquares, _harmonics(2)),
    (DecodeOffByOneAtPerfectSquares, _harmonics(16)),
    (LastRowOfAnOddLayerNotWritten, _siren("one-layer-4-1")),
    (LastRowOfAnOddLayerNotWritten, _siren("identity-inside-sine-last")),
    (LastRowOfAnOddLayerNotWritten, _siren("gates-2025-33-2048-5")),
    (LastRowOfAnOddLayerFromItsNeighbour, _siren("odd-widths-null-biases")),
    (LastRowOfAnOddLayerFromItsNeighbour, _siren("eight-layers-of-3")),
    (LastRowOfAnOddLayerFromItsNeighbour, _siren("identity-inside-sine-last")),
    (BiasSkippedOnOddRows, _siren("4-2")),
    (BiasSkippedOnOddRows, _siren("satclip-100-512-512-256")),
    (FrequencyOfTheNextLayer, _siren("odd-widths-null-biases")),
    (FrequencyOfTheNextLayer, _siren("identity-inside-sine-last")),
    (FeaturesBeyond1023LeftAtZero, _harmonics(33)),
    (FeaturesBeyond1023LeftAtZero, _harmonics(45)),
    (CosThetaInFloat32, _harmonics(10)),
    (XMovedBy64Ulps, _harmonics(10)),
    (XMovedBy64Ulps, _harmonics(2)),
]


@pytest.mark.parametrize("at", range(len(MUTANTS)), ids=lambda i: f"{MUTANTS[i][0].__name__}-{i}")
def test_an_emulator_with_one_planted_error_fails_the_body(at):
    mutant, body = MUTANTS[at]
    try:
        L.set_backend(EmuBackend())
        body()                                      # the plain emulator passes ...
        L.set_backend(mutant())
        with pytest.raises(AssertionError):         # ... and the mutant does not
            body()
    finally:
        L.set_backend(None)
