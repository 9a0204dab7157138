"""The flat fp32 streaming entries without a GPU: the bodies of tests/streaming_cases.py on the numpy emulator (tests/emu_backend.py),
the checks that keep their derived bounds honest -- the input conditions, eager fp32 torch of the same formulas inside every bound, and
emulators with one deliberate error each that must fail a body -- and the generator with the unscaled multiply injection against the
float64 oracle.  Bodies shared with tests/test_gpu_streaming.py."""
import numpy as np
import pytest
import torch

import streaming_cases as Sc
from emu_backend import EmuBackend, arr, obj
from nirgan_hip import lib as L

BIG = {((2, 96, 100, 256), 1)}


@pytest.fixture()
def emu():
    be = EmuBackend()
    L.set_backend(be)
    yield be
    L.set_backend(None)


# ------------------------------------------------------------------------------------------------ bodies on the emulator
@pytest.mark.parametrize("shape,pad,variant", Sc.INJECT_CASES, ids=str)
def test_inject_forward_and_backward(emu, shape, pad, variant):
    Sc.inject_conditions_hold(shape, variant)
    Sc.inject_against_float64("cpu", shape, pad, variant)
    assert set(emu.calls) == {"inject_fwd", "inject_bwd"}


@pytest.mark.parametrize("src,dst", Sc.BILINEAR_CASES, ids=str)
def test_bilinear_forward_backward_and_adjoint_identity(emu, src, dst):
    Sc.bilinear_against_float64("cpu", src, dst)


@pytest.mark.parametrize("rows", Sc.COLSUM_ROWS + ("net",), ids=str)
def test_colsum(emu, rows):
    Sc.colsum_against_float64("cpu", rows)


@pytest.mark.parametrize("n", Sc.PARAM_SCALE_N)
def test_param_scale(emu, n):
    Sc.param_scale_against_float64("cpu", n)


@pytest.mark.parametrize("n", Sc.FLAT_N)
def test_fill_and_axpy(emu, n):
    Sc.fill_axpy_against_torch("cpu", n)


@pytest.mark.parametrize("n", Sc.ADAM_N)
def test_adam_three_steps(emu, n):
    Sc.adam_conditions_hold(n)
    Sc.adam_against_float64("cpu", n)


@pytest.mark.parametrize("n", Sc.LSGAN_N)
def test_lsgan(emu, n):
    Sc.lsgan_against_float64("cpu", n)


@pytest.mark.parametrize("shape", Sc.PIX_SHAPES, ids=str)
def test_pix_loss_sums_and_gradient(emu, shape):
    Sc.pix_conditions_hold(shape)
    Sc.pix_loss_against_float64("cpu", shape)


def test_pix_loss_guards(emu):
    Sc.pix_loss_guards("cpu")


@pytest.mark.parametrize("case", Sc.TAP_CASES, ids=str)
def test_tap_scatter(emu, case):
    Sc.tap_scatter_against_float64("cpu", case)


@pytest.mark.parametrize("shape", Sc.OPPOSITE_HALVES, ids=str)
def test_tap_scatter_opposite_halves_leave_the_bias_gradient_at_zero(emu, shape):
    Sc.tap_scatter_opposite_halves("cpu", shape)


def test_generator_with_the_unscaled_multiply_injection(emu):
    Sc.unscaled_multiply_generator("cpu")
    assert {"inject_fwd", "inject_bwd", "bilinear_fwd", "bilinear_bwd"} <= set(emu.calls)


# ------------------------------------------------------------------------------------------------ the reference alone
@pytest.mark.parametrize("shape,pad,variant", Sc.INJECT_CASES, ids=str)
def test_eager_fp32_inject_lies_inside_the_bounds(shape, pad, variant):
    Sc.inject_reference_alone(shape, variant)


@pytest.mark.parametrize("src,dst", Sc.BILINEAR_CASES, ids=str)
def test_eager_fp32_bilinear_lies_inside_the_bounds(src, dst):
    Sc.bilinear_reference_alone(src, dst)


def test_eager_fp32_streams_lie_inside_the_bounds():
    for rows in Sc.COLSUM_ROWS + ("net",):
        Sc.colsum_reference_alone(rows)
    for n in Sc.PARAM_SCALE_N:
        Sc.param_scale_reference_alone(n)
    for n in Sc.LSGAN_N:
        Sc.lsgan_reference_alone(n)
    for case in Sc.TAP_CASES:
        Sc.tap_reference_alone(case)


@pytest.mark.parametrize("n", Sc.ADAM_N)
def test_eager_fp32_adam_lies_inside_the_bounds(n):
    Sc.adam_reference_alone(n)


@pytest.mark.parametrize("shape", Sc.PIX_SHAPES, ids=str)
def test_eager_fp32_pix_loss_lies_inside_the_bounds(shape):
    Sc.pix_reference_alone(shape)


# ------------------------------------------------------------------------------------------------ mutations
class UnscaledMultiplyAsOnePlusE(EmuBackend):
    """multiply without a scale parameter as z * (1 + e): what the entry computed before"""

    def _with_unit_scale(self, ref, fn):
        d = obj(ref)
        if d.style == 0 and not d.scale:
            one = np.ones(1, dtype=np.float32)
            d.scale = one.ctypes.data
            try:
                return fn(ref)
            finally:
                d.scale = None
        return fn(ref)

    def nirgan_inject_fwd(self, ref, stream=None):
        return self._with_unit_scale(ref, super().nirgan_inject_fwd)

    def nirgan_inject_bwd(self, ref, stream=None):
        return self._with_unit_scale(ref, super().nirgan_inject_bwd)


class DeWithoutScale(EmuBackend):
    def nirgan_inject_bwd(self, ref, stream=None):
        rc, d = super().nirgan_inject_bwd(ref), obj(ref)
        if rc == 0 and d.scale:
            arr(d.de, d.B * d.H * d.W)[:] /= arr(d.scale, 1)[0]
        return rc


class MaskFromZ(EmuBackend):
    def nirgan_inject_bwd(self, ref, stream=None):
        d = obj(ref)
        fake = arr(d.a, d.B * d.a_hp * d.a_wp * d.C).copy().reshape(d.B, d.a_hp, d.a_wp, d.C)
        fake[:, d.a_pad:d.a_pad + d.H, d.a_pad:d.a_pad + d.W] = arr(d.z, d.B * d.H * d.W * d.C).reshape(d.B, d.H, d.W, d.C)
        keep, d.a = d.a, fake.ctypes.data
        try:
            return super().nirgan_inject_bwd(ref)
        finally:
            d.a = keep


class DscaleOverwritten(EmuBackend):
    def nirgan_inject_bwd(self, ref, stream=None):
        d = obj(ref)
        if d.dscale and d.ws and d.ws_elems >= Sc.inject_grid((d.B, d.H, d.W, d.C))[2]:
            arr(d.dscale, 1)[0] = 0
        return super().nirgan_inject_bwd(ref)


class BilinearWindowOneRowShort(EmuBackend):
    """the adjoint's window of the LAST source row ends one destination row early"""

    def nirgan_bilinear_bwd(self, ddst, B, OH, OW, dsrc, SH, SW, stream=None):
        rc = super().nirgan_bilinear_bwd(ddst, B, OH, OW, dsrc, SH, SW)
        Mh, Mw = Sc.resize_axis(SH, OH)[0], Sc.resize_axis(SW, OW)[0]
        last = torch.from_numpy(arr(ddst, B * OH * OW).reshape(B, OH, OW)[:, OH - 1].copy()).double()
        arr(dsrc, B * SH * SW).reshape(B, SH, SW)[:, SH - 1] -= (Mh[OH - 1, SH - 1] * last @ Mw).float().numpy()
        return rc


class ColsumDropsTheTail(EmuBackend):
    def nirgan_colsum(self, x, rows, cols, out, accumulate, stream=None):
        s = arr(x, rows * cols).reshape(rows, cols)[:rows // 64 * 64].sum(0)
        o = arr(out, cols)
        o[:] = o + s if accumulate else s
        return 0


class PixClosedForm(EmuBackend):
    """the gradient from the kernel's closed-form derivatives in float64, with an optional planted error"""
    mutate = None

    def nirgan_pix_loss(self, ref, stream=None):
        rc, d = super().nirgan_pix_loss(ref), obj(ref)
        if rc or not d.grad_pred:
            return rc
        n = d.B * d.H * d.W
        rgb = torch.from_numpy(arr(d.rgb, 3 * n).reshape(d.B, 3, d.H, d.W).copy()).double() if d.rgb else None
        x, y = (torch.from_numpy(arr(p, n).reshape(d.B, 1, d.H, d.W).copy()).double() for p in (d.nir, d.pred))
        w = (d.w_l1, d.w_ndvi, d.w_ndwi, d.w_gndvi, d.w_savi, d.w_msavi, d.w_evi)
        _, g = Sc.pix_closed_form(rgb, x, y, w, d.log_all, d.criterion, torch.zeros(7, dtype=torch.float64), self.mutate)
        g = g.reshape(-1).numpy()
        if d.extra:
            g = g + d.extra_scale * arr(d.extra, n * d.extra_cs)[d.extra_c::d.extra_cs]
        arr(d.grad_pred, n)[:] = g
        return rc


class MsaviFourTp(PixClosedForm):
    mutate = "msavi 4 tp"


class GndviWithoutDndp(PixClosedForm):
    mutate = "gndvi without dndp"


class ExtraScaleIgnored(EmuBackend):
    def nirgan_pix_loss(self, ref, stream=None):
        d = obj(ref)
        keep, d.extra_scale = d.extra_scale, 1.0
        try:
            return super().nirgan_pix_loss(ref)
        finally:
            d.extra_scale = keep


class TapScatterLeavesIdleChannels(EmuBackend):
    def nirgan_tap_scatter(self, ref, stream=None):
        rc, d = super().nirgan_tap_scatter(ref), obj(ref)
        arr(d.dq, d.B * d.q_hp * d.q_wp * d.q_cs).reshape(-1, d.q_cs)[:, d.ntaps:] = np.nan
        return rc


SMALL = ((2, 9, 7, 64), 1)
MUTANTS = [
    (UnscaledMultiplyAsOnePlusE, lambda: Sc.inject_against_float64("cpu", *SMALL, "multiply")),
    (DeWithoutScale, lambda: Sc.inject_against_float64("cpu", *SMALL, "multiply+scale")),
    (DeWithoutScale, lambda: Sc.inject_against_float64("cpu", *SMALL, "add+scale")),
    (MaskFromZ, lambda: Sc.inject_against_float64("cpu", *SMALL, "multiply+scale-0.8")),
    (MaskFromZ, lambda: Sc.inject_against_float64("cpu", *SMALL, "add+scale")),
    (DscaleOverwritten, lambda: Sc.inject_against_float64("cpu", *SMALL, "multiply+scale")),
    (BilinearWindowOneRowShort, lambda: Sc.bilinear_against_float64("cpu", (128, 128), (52, 36))),
    (BilinearWindowOneRowShort, lambda: Sc.bilinear_against_float64("cpu", (2, 3), (300, 2))),
    (ColsumDropsTheTail, lambda: Sc.colsum_against_float64("cpu", 65)),
    (ColsumDropsTheTail, lambda: Sc.colsum_against_float64("cpu", 1073)),
    (MsaviFourTp, lambda: Sc.pix_loss_against_float64("cpu", (2, 17, 19))),
    (GndviWithoutDndp, lambda: Sc.pix_loss_against_float64("cpu", (2, 17, 19))),
    (ExtraScaleIgnored, lambda: Sc.pix_loss_against_float64("cpu", (2, 17, 19))),
    (TapScatterLeavesIdleChannels, lambda: Sc.tap_scatter_against_float64("cpu", (2, 7, 20, 22, 3, 52))),
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


def test_the_closed_form_gradient_without_a_planted_error_passes(capsys):
    try:
        L.set_backend(PixClosedForm())
        Sc.pix_loss_against_float64("cpu", (2, 17, 19))
    finally:
        L.set_backend(None)
