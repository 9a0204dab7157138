"""The networks' boundary kernels without a GPU: the bodies of tests/boundary_cases.py on the numpy emulator (tests/emu_backend.py), and
the checks that keep their derived bounds honest -- the input conditions, eager fp32 torch of the same formulas inside every bound, and
emulators with one deliberate, subtle error each that must fail a body.  Bodies shared with tests/test_gpu_boundary.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import boundary_cases as Bc
from emu_backend import EmuBackend, arr, obj
from nirgan_hip import lib as L

# too large for eager torch on the CPU in a quick test: the two cases that exist for a grid cap only
GRID_CAP_ONLY = {Bc.HALO_GRID_CAP, Bc.DGRAD_GRID_CAP}


@pytest.fixture()
def emu():
    be = EmuBackend()
    L.set_backend(be)
    yield be
    L.set_backend(None)


# ------------------------------------------------------------------------------------------------ bodies on the emulator
@pytest.mark.parametrize("writes", Bc.HALO_CASES, ids=str)
def test_nchw_to_halo_writes_its_window_and_nothing_else(emu, writes):
    Bc.halo_against_float64("cpu", writes)
    assert emu.calls == ["nchw_to_halo"] * len(writes)


def test_nchw_to_halo_guards(emu):
    Bc.halo_guards("cpu")


@pytest.mark.parametrize("case", Bc.GATHER_CASES, ids=Bc.gather_id)
def test_tap_gather(emu, case):
    Bc.gather_conditions_hold(case)
    Bc.gather_against_float64("cpu", case)


def test_tap_gather_guards(emu):
    Bc.gather_guards("cpu")


@pytest.mark.parametrize("case", Bc.DGRAD_CASES, ids=str)
def test_conv_channel_dgrad(emu, case):
    Bc.dgrad_against_float64("cpu", case)


def test_conv_channel_dgrad_guards(emu):
    Bc.dgrad_guards("cpu")


@pytest.mark.parametrize("case", Bc.END_CASES, ids=str)
def test_endconv(emu, case):
    Bc.end_conditions_hold(case)
    Bc.end_against_float64("cpu", case)
    assert {"endconv_fwd", "endconv_dz", "endconv_dgrad", "endconv_wgrad"} <= set(emu.calls)


# ------------------------------------------------------------------------------------------------ the reference alone
@pytest.mark.parametrize("case", Bc.GATHER_CASES, ids=Bc.gather_id)
def test_eager_fp32_gather_lies_inside_the_bounds(case):
    Bc.gather_reference_alone(case)


@pytest.mark.parametrize("case", [c for c in Bc.DGRAD_CASES if c not in GRID_CAP_ONLY], ids=str)
def test_eager_fp32_channel_dgrad_lies_inside_the_bounds(case):
    Bc.dgrad_reference_alone(case)


@pytest.mark.parametrize("case", Bc.END_CASES, ids=str)
def test_eager_fp32_endconv_lies_inside_the_bounds(case):
    Bc.end_reference_alone(case)


def test_fp32_pad_is_the_float64_pad():
    """the copy has no arithmetic: fp32 F.pad of the same inputs gives the expected bits (nothing was lost by expecting in float64)"""
    for writes in Bc.HALO_CASES:
        if writes in GRID_CAP_ONLY:
            continue
        srcs, fill, exp, written = Bc.halo_case(writes)
        got = fill.clone()
        for src, (B, Cs, H, W, cs, c0, p1, p2, mode) in zip(srcs, writes):
            P = p1 + p2
            if mode == "reflect":
                win = src
                for q in (p1, p2):
                    win = F.pad(win, (q,) * 4, mode="reflect") if q else win
                got[..., c0:c0 + Cs] = win.permute(0, 2, 3, 1)
            else:
                got[:, P:P + H, P:P + W, c0:c0 + Cs] = src.permute(0, 2, 3, 1)
        assert Bc.same(got, exp) and written.any() and (writes[0][-1] == "reflect" or not written.all())


# ------------------------------------------------------------------------------------------------ mutations
def _swap(d, field, value, fn):
    keep = getattr(d, field)
    setattr(d, field, value)
    try:
        return fn()
    finally:
        setattr(d, field, keep)


class GatherDropsLastTapRightOfColumn32(EmuBackend):
    def nirgan_tap_gather(self, ref, stream=None):
        rc, d = super().nirgan_tap_gather(ref), obj(ref)
        if rc or d.ntaps < 2:
            return rc
        H2, W2 = d.OH - 2 * d.crop, d.OW - 2 * d.crop
        short = np.zeros(d.B * H2 * W2, dtype=np.float32)
        _swap(d, "dst", short.ctypes.data, lambda: _swap(d, "ntaps", d.ntaps - 1, lambda: super(GatherDropsLastTapRightOfColumn32, self).nirgan_tap_gather(ref)))
        arr(d.dst, short.size).reshape(d.B, H2, W2)[:, :, 32:] = short.reshape(d.B, H2, W2)[:, :, 32:]
        return rc


class GatherIgnoresCropAlongX(EmuBackend):
    def nirgan_tap_gather(self, ref, stream=None):
        rc, d = super().nirgan_tap_gather(ref), obj(ref)
        if rc or not d.crop:
            return rc
        c, whole = d.crop, np.zeros(d.B * d.OH * d.OW, dtype=np.float32)
        _swap(d, "dst", whole.ctypes.data, lambda: _swap(d, "crop", 0, lambda: super(GatherIgnoresCropAlongX, self).nirgan_tap_gather(ref)))
        arr(d.dst, d.B * (d.OH - 2 * c) * (d.OW - 2 * c)).reshape(d.B, d.OH - 2 * c, d.OW - 2 * c)[:] = \
            whole.reshape(d.B, d.OH, d.OW)[:, c:d.OH - c, :d.OW - 2 * c]
        return rc


class GatherSumScaled(EmuBackend):
    """a relative error of 2^-18 = 3.8e-6 in the sum"""

    def nirgan_tap_gather(self, ref, stream=None):
        rc, d = super().nirgan_tap_gather(ref), obj(ref)
        if rc == 0 and d.act == L.ACT_NONE:
            arr(d.dst, d.B * (d.OH - 2 * d.crop) * (d.OW - 2 * d.crop))[:] *= np.float32(1 + 2.0 ** -18)
        return rc


class KeepModeZeroesTheHalo(EmuBackend):
    def nirgan_nchw_to_halo(self, src, B, Cs, H, W, dst, cs, c0, pad1, pad2, mode, stream=None):
        P = pad1 + pad2
        if mode == L.BORDER_KEEP and src and dst and c0 >= 0 and c0 + Cs <= cs:
            arr(dst, B * (H + 2 * P) * (W + 2 * P) * cs).reshape(B, H + 2 * P, W + 2 * P, cs)[..., c0:c0 + Cs] = 0
        return super().nirgan_nchw_to_halo(src, B, Cs, H, W, dst, cs, c0, pad1, pad2, mode)


class KeepModeWritesTheChannelBelow(EmuBackend):
    def nirgan_nchw_to_halo(self, src, B, Cs, H, W, dst, cs, c0, pad1, pad2, mode, stream=None):
        rc, P = super().nirgan_nchw_to_halo(src, B, Cs, H, W, dst, cs, c0, pad1, pad2, mode), pad1 + pad2
        if rc == 0 and mode == L.BORDER_KEEP and c0 > 0:
            arr(dst, B * (H + 2 * P) * (W + 2 * P) * cs).reshape(B, H + 2 * P, W + 2 * P, cs)[:, P:P + H, P:P + W, c0 - 1] = \
                arr(src, B * Cs * H * W).reshape(B, Cs, H, W)[:, 0]
        return rc


class ChanDgradTakesRowMinusStride(EmuBackend):
    """nh = -stride passes ``nh % stride == 0`` and is not refused as negative: its dY row -1 is read one row late (row 0)"""

    def nirgan_conv_channel_dgrad(self, ref, stream=None):
        rc, d = super().nirgan_conv_channel_dgrad(ref), obj(ref)
        if rc:
            return rc
        OW = d.dy_wp - 2 * d.dy_pad
        dy = arr(d.dy, d.B * d.dy_hp * d.dy_wp * d.C).reshape(d.B, d.dy_hp, d.dy_wp, d.C)[:, d.dy_pad, d.dy_pad:d.dy_pad + OW].astype(np.float64)
        w = arr(d.w, d.C * d.cin * d.k * d.k).reshape(d.C, d.cin, d.k, d.k)[:, d.channel].astype(np.float64)
        out = arr(d.out, d.B * d.H * d.W).reshape(d.B, d.H, d.W)
        for kh in range(d.k):
            h = kh - d.pad - d.stride
            if not 0 <= h < d.H:
                continue
            for x in range(d.W):
                for kw in range(d.k):
                    nw = x + d.pad - kw
                    if nw >= 0 and nw % d.stride == 0 and nw // d.stride < OW:
                        out[:, h, x] += (dy[:, nw // d.stride] @ w[:, kh, kw]).astype(np.float32)
        return rc


class ChanDgradReadsTheHalo(EmuBackend):
    """taps one position outside dY are not skipped: they read the halo"""

    def nirgan_conv_channel_dgrad(self, ref, stream=None):
        rc, d = super().nirgan_conv_channel_dgrad(ref), obj(ref)
        if rc or not d.dy_pad:
            return rc
        dy = torch.from_numpy(arr(d.dy, d.B * d.dy_hp * d.dy_wp * d.C).reshape(d.B, d.dy_hp, d.dy_wp, d.C).copy()).permute(0, 3, 1, 2)
        w = torch.from_numpy(arr(d.w, d.C * d.cin * d.k * d.k).reshape(d.C, d.cin, d.k, d.k)[:, d.channel:d.channel + 1].copy())
        x = torch.zeros(d.B, 1, d.H, d.W, requires_grad=True)
        with torch.enable_grad():
            F.conv2d(x, w, stride=d.stride, padding=d.pad + d.stride * d.dy_pad).backward(dy.contiguous())
        arr(d.out, d.B * d.H * d.W)[:] = x.grad.reshape(-1).numpy()
        return rc


class ChanDgradSumScaled(EmuBackend):
    def nirgan_conv_channel_dgrad(self, ref, stream=None):
        rc, d = super().nirgan_conv_channel_dgrad(ref), obj(ref)
        if rc == 0:
            arr(d.out, d.B * d.H * d.W)[:] *= np.float32(1 + 2.0 ** -18)
        return rc


class EndWgradDropsTheLastColumnOfAnOddRow(EmuBackend):
    def nirgan_endconv_wgrad(self, ref, stream=None):
        d = obj(ref)
        if d.x_wp % 2 == 0 or not d.x:
            return super().nirgan_endconv_wgrad(ref)
        x = arr(d.x, d.B * d.x_hp * d.x_wp * 64).copy().reshape(d.B, d.x_hp, d.x_wp, 64)
        x[:, :, d.x_wp - 1] = 0
        return _swap(d, "x", x.ctypes.data, lambda: super(EndWgradDropsTheLastColumnOfAnOddRow, self).nirgan_endconv_wgrad(ref))


class EndDzWithoutTheDerivativeOnTheLastRow(EmuBackend):
    def nirgan_endconv_dz(self, ref, stream=None):
        rc, d = super().nirgan_endconv_dz(ref), obj(ref)
        if rc == 0 and d.act == L.ACT_TANH:
            c, H2, W2 = d.crop, d.OH - 2 * d.crop, d.OW - 2 * d.crop
            self._endconv_dz_image(d)[:, 6 + c + H2 - 1, 6 + c:6 + c + W2] = arr(d.dout, d.B * H2 * W2).reshape(d.B, H2, W2)[:, H2 - 1]
        return rc


class EndDzScaled(EmuBackend):
    def nirgan_endconv_dz(self, ref, stream=None):
        rc, d = super().nirgan_endconv_dz(ref), obj(ref)
        if rc == 0 and d.act == L.ACT_TANH:
            self._endconv_dz_image(d)[:] *= np.float32(1 + 2.0 ** -18)
        return rc


MUTANTS = [
    (GatherDropsLastTapRightOfColumn32, lambda: Bc.gather_against_float64("cpu", Bc.square(2, 7, 40, 40, 0, 52))),
    (GatherDropsLastTapRightOfColumn32, lambda: Bc.gather_against_float64("cpu", Bc.square(1, 7, 33, 125, 0, 52))),
    (GatherDropsLastTapRightOfColumn32, lambda: Bc.gather_against_float64("cpu", (1, 70, 70, 0, 8, Bc.CROSS))),
    (GatherIgnoresCropAlongX, lambda: Bc.gather_against_float64("cpu", Bc.square(1, 7, 9, 37, 1, 52))),
    (GatherIgnoresCropAlongX, lambda: Bc.gather_against_float64("cpu", Bc.square(2, 7, 70, 70, 3, 52))),
    (GatherSumScaled, lambda: Bc.gather_against_float64("cpu", Bc.square(3, 4, 67, 80, 0, 16))),
    (GatherSumScaled, lambda: Bc.gather_against_float64("cpu", (1, 70, 70, 0, 8, Bc.CROSS))),
    (KeepModeZeroesTheHalo, lambda: Bc.halo_against_float64("cpu", Bc.HALO_CASES[0])),
    (KeepModeZeroesTheHalo, lambda: Bc.halo_against_float64("cpu", Bc.HALO_CASES[1])),
    (KeepModeWritesTheChannelBelow, lambda: Bc.halo_against_float64("cpu", Bc.HALO_CASES[0])),
    (KeepModeWritesTheChannelBelow, lambda: Bc.halo_against_float64("cpu", Bc.HALO_CASES[2])),
    (ChanDgradTakesRowMinusStride, lambda: Bc.dgrad_against_float64("cpu", (1, 7, 9, 8, 4, 2, 1, 4, 0, 0))),
    (ChanDgradTakesRowMinusStride, lambda: Bc.dgrad_against_float64("cpu", (2, 18, 34, 64, 4, 2, 1, 4, 3, 1))),
    (ChanDgradReadsTheHalo, lambda: Bc.dgrad_against_float64("cpu", (2, 21, 25, 64, 4, 2, 1, 4, 3, 1))),
    (ChanDgradReadsTheHalo, lambda: Bc.dgrad_against_float64("cpu", (1, 2, 2, 8, 4, 2, 1, 4, 3, 1))),
    (ChanDgradSumScaled, lambda: Bc.dgrad_against_float64("cpu", (1, 9, 9, 8, 1, 1, 0, 1, 0, 0))),
    (EndWgradDropsTheLastColumnOfAnOddRow, lambda: Bc.end_against_float64("cpu", (1, 1, 1, 0))),      # (with a crop the column is never used)
    (EndWgradDropsTheLastColumnOfAnOddRow, lambda: Bc.end_against_float64("cpu", (1, 5, 65, 0))),
    (EndDzWithoutTheDerivativeOnTheLastRow, lambda: Bc.end_against_float64("cpu", (2, 9, 10, 1))),
    (EndDzWithoutTheDerivativeOnTheLastRow, lambda: Bc.end_against_float64("cpu", (1, 3, 70, 1))),
    (EndDzScaled, lambda: Bc.end_against_float64("cpu", (1, 4, 64, 0))),
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
