"""nirgan_image_metrics, nirgan_ssim_loss, nirgan_emd_loss and nirgan_hist_match without a GPU: the bodies of tests/metric_loss_cases.py on
the numpy emulator (tests/emu_backend.py), and the checks that keep their derived bounds honest -- the input conditions, the kernels'
formulas in eager fp32 torch inside every bound, and emulators with one deliberate error each that must fail a named body.  Bodies shared
with tests/test_gpu_metric_loss.py."""
import pytest
import torch

import metric_loss_cases as Mc
from emu_backend import EmuBackend, arr, obj
from nirgan_hip import lib as L


@pytest.fixture()
def emu():
    be = EmuBackend()
    L.set_backend(be)
    yield be
    L.set_backend(None)


# ------------------------------------------------------------------------------------------------ bodies on the emulator
@pytest.mark.parametrize("shape,kind", Mc.SSIM_CASES, ids=str)
def test_image_metrics(emu, shape, kind):
    Mc.ssim_conditions_hold(shape, kind)
    Mc.metrics_against_float64("cpu", shape, kind)
    if (shape, kind) == Mc.SSIM_VARIED:
        Mc.metrics_against_float64("cpu", shape, kind, max_val=2.0)
    assert set(emu.calls) == {"metrics"}


@pytest.mark.parametrize("shape,kind", Mc.SSIM_CASES, ids=str)
def test_ssim_loss_value_and_gradient(emu, shape, kind):
    Mc.ssim_loss_against_float64("cpu", shape, kind)
    assert set(emu.calls) == {"ssim_loss"}


@pytest.mark.parametrize("shape,kind", Mc.EMD_CASES, ids=str)
def test_emd_loss_value_and_gradient(emu, shape, kind):
    Mc.emd_conditions_hold(shape, kind)
    Mc.emd_loss_against_float64("cpu", shape, kind)
    assert set(emu.calls) == {"emd_loss"}


@pytest.mark.parametrize("shape", Mc.HIST_SHAPES, ids=str)
def test_hist_match(emu, shape):
    Mc.hist_conditions_hold(shape)
    Mc.hist_match_against_float64("cpu", shape)
    assert set(emu.calls) == {"hist_match"}


def test_guards(emu):
    Mc.metric_loss_guards("cpu")


def test_python_surfaces(emu):
    Mc.python_surfaces("cpu")
    assert {"metrics", "ssim_loss", "emd_loss", "hist_match"} <= set(emu.calls)


# ------------------------------------------------------------------------------------------------ the reference alone
@pytest.mark.parametrize("shape,kind", Mc.SSIM_CASES, ids=str)
def test_eager_fp32_ssim_lies_inside_the_bounds(shape, kind):
    Mc.ssim_reference_alone(shape, kind)


@pytest.mark.parametrize("shape,kind", Mc.EMD_CASES, ids=str)
def test_eager_fp32_emd_lies_inside_the_bounds(shape, kind):
    Mc.emd_reference_alone(shape, kind)


@pytest.mark.parametrize("shape", Mc.HIST_SHAPES, ids=str)
def test_double_interpolation_rounded_once_lies_inside_the_bounds(shape):
    Mc.hist_reference_alone(shape)


# ------------------------------------------------------------------------------------------------ mutations
def planes(ptr, d):
    return torch.from_numpy(arr(ptr, d.planes * d.H * d.W).reshape(d.planes, d.H, d.W).copy()).double()


class SsimFormulas(EmuBackend):
    """value and gradient from the kernels' closed forms in float64, with an optional planted error"""
    mutate = None

    def nirgan_image_metrics(self, ref, stream=None):
        d = obj(ref)
        x, y = planes(d.pred, d), planes(d.target, d)
        _, S, _, _ = Mc.ssim_closed_form(x, y, d.window, d.max_val, self.mutate)
        arr(d.means, 3)[:] = [(x - y).abs().mean().item(), ((x - y) ** 2).mean().item(), S.mean().item()]
        return 0

    def nirgan_ssim_loss(self, ref, stream=None):
        d = obj(ref)
        x, y = planes(d.pred, d), planes(d.target, d)
        S, _, _, gs = Mc.ssim_closed_form(x, y, d.window, d.max_val, self.mutate)
        v, n = 1.0 - S.mean().item(), x.numel()
        if d.value:
            arr(d.value, 1)[0] = v
        if d.loss:
            arr(d.loss, 1)[0] += d.weight * v
        if d.grad_pred:
            g = (-(1.0 if self.mutate == "weight ignored" else d.weight) / n * gs).reshape(-1).numpy()
            out = arr(d.grad_pred, n)
            out[:] = g if self.mutate == "overwritten" else out + g
        return 0


class ReflectWithEdgeRepeat(SsimFormulas):
    mutate = "edge repeat"


class FoldWithoutTheRightMirror(SsimFormulas):
    mutate = "fold without the right mirror"


class GradPredOverwritten(SsimFormulas):
    mutate = "overwritten"


class WeightIgnoredInTheGradient(SsimFormulas):
    mutate = "weight ignored"


class UnnormalisedTaps(SsimFormulas):
    """(dropping eps does not separate: 1e-12 against a denominator >= C1 C2 = 1.4e-6 at max_val 2 moves S by at most 7e-7 of itself,
    1e-11 on these images; ``mutate = "eps dropped"`` passes every body at max_val 2, pred == target included, where S becomes exactly 1
    and the gradient exactly 0 inside a bound of u times its cancelling terms.  So the planted error of this slot is the taps' normalisation)"""
    mutate = "unnormalised taps"


class EmdFormulas(EmuBackend):
    mutate = None

    def nirgan_emd_loss(self, ref, stream=None):
        d = obj(ref)
        n = d.B * d.N
        x, y = (torch.from_numpy(arr(p, n).reshape(d.B, d.N).copy()).double() for p in (d.pred, d.target))
        v, g = Mc.emd_formulas(x, y, d.weight, self.mutate)
        if d.value:
            arr(d.value, 1)[0] = v.item()
        if d.loss:
            arr(d.loss, 1)[0] += d.weight * v.item()
        if d.grad_pred:
            arr(d.grad_pred, n)[:] += g.reshape(-1).numpy()
        return 0


class EmdExclusiveSuffix(EmdFormulas):
    mutate = "exclusive suffix"


class EmdDividedByN(EmdFormulas):
    mutate = "divided by N"


class HistFormula(EmuBackend):
    mutate = None

    def nirgan_hist_match(self, ref, stream=None):
        d = obj(ref)
        img, tmp = (torch.from_numpy(arr(p, d.B * d.N).reshape(d.B, d.N).copy()) for p in (d.image, d.reference))
        arr(d.out, d.B * d.N)[:] = Mc.hist_formula(img, tmp, self.mutate).reshape(-1).numpy()
        return 0


class HistLowerBoundOnTheSource(HistFormula):
    mutate = "lower bound"


class HistSignedZerosApart(HistFormula):
    mutate = "signed zeros apart"


class HistTemplateOfPlaneZero(HistFormula):
    mutate = "template of plane 0"


SMALL, TILED = ((1, 6, 6, 11), "rand"), ((2, 70, 66, 11), "saturated")
MUTANTS = [
    (ReflectWithEdgeRepeat, lambda: Mc.metrics_against_float64("cpu", *SMALL)),
    (ReflectWithEdgeRepeat, lambda: Mc.ssim_loss_against_float64("cpu", *TILED)),
    (FoldWithoutTheRightMirror, lambda: Mc.ssim_loss_against_float64("cpu", *SMALL)),
    (FoldWithoutTheRightMirror, lambda: Mc.ssim_loss_against_float64("cpu", *TILED)),
    (GradPredOverwritten, lambda: Mc.ssim_loss_against_float64("cpu", *TILED)),
    (WeightIgnoredInTheGradient, lambda: Mc.ssim_loss_against_float64("cpu", *SMALL)),
    (UnnormalisedTaps, lambda: Mc.run_ssim_loss("cpu", *Mc.SSIM_VARIED, max_val=2.0)),
    (UnnormalisedTaps, lambda: Mc.metrics_against_float64("cpu", *Mc.SSIM_VARIED, max_val=2.0)),
    (EmdExclusiveSuffix, lambda: Mc.emd_loss_against_float64("cpu", (1, 15), "separated")),
    (EmdDividedByN, lambda: Mc.emd_loss_against_float64("cpu", (2, 1023), "separated")),
    (HistLowerBoundOnTheSource, lambda: Mc.hist_match_against_float64("cpu", (2, 2049))),
    (HistSignedZerosApart, lambda: Mc.hist_match_against_float64("cpu", (2, 7))),
    (HistSignedZerosApart, lambda: Mc.hist_match_against_float64("cpu", (1, 2048))),
    (HistTemplateOfPlaneZero, lambda: Mc.hist_match_against_float64("cpu", (2, 7))),
]
PLAIN = {ReflectWithEdgeRepeat: SsimFormulas, FoldWithoutTheRightMirror: SsimFormulas, GradPredOverwritten: SsimFormulas,
         WeightIgnoredInTheGradient: SsimFormulas, UnnormalisedTaps: SsimFormulas, EmdExclusiveSuffix: EmdFormulas,
         EmdDividedByN: EmdFormulas, HistLowerBoundOnTheSource: HistFormula, HistSignedZerosApart: HistFormula,
         HistTemplateOfPlaneZero: HistFormula}


@pytest.mark.parametrize("at", range(len(MUTANTS)), ids=lambda i: f"{MUTANTS[i][0].__name__}-{i}")
def test_an_emulator_with_one_planted_error_fails_the_body(at):
    mutant, body = MUTANTS[at]
    try:
        for plain in (EmuBackend, PLAIN[mutant]):
            L.set_backend(plain())
            body()                                  # the plain emulator and the plain formulas pass ...
        L.set_backend(mutant())
        with pytest.raises(AssertionError):         # ... and the mutant does not
            body()
    finally:
        L.set_backend(None)


@pytest.mark.parametrize("formulas", [SsimFormulas, EmdFormulas, HistFormula], ids=lambda c: c.__name__)
def test_the_formulas_without_a_planted_error_pass_every_body(formulas):
    try:
        L.set_backend(formulas())
        if formulas is SsimFormulas:
            for shape, kind in Mc.SSIM_CASES:
                Mc.metrics_against_float64("cpu", shape, kind)
                Mc.ssim_loss_against_float64("cpu", shape, kind)
        elif formulas is EmdFormulas:
            for shape, kind in Mc.EMD_CASES:
                Mc.emd_loss_against_float64("cpu", shape, kind)
        else:
            for shape in Mc.HIST_SHAPES:
                Mc.hist_match_against_float64("cpu", shape)
    finally:
        L.set_backend(None)
