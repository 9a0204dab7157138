"""numpy statement of the scene histogram-matching entries of include/nirgan_hip.h (nirgan_scene_hist / nirgan_scene_match_lut /
nirgan_scene_lut_apply, the last section) -- TEST INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend``; it extends
tests/emu_tile_metrics_masked.py and is now the end of the emulator chain.

Written from the header alone.  The count is ``np.bincount``.  The table writes the header's operations out one by one in float64
(``match_table``): two cumulative sums, two rounded divisions, the last rounded reference quantile not above each rounded source
quantile by ``np.searchsorted``, then difference, quotient, difference, product and sum, each a numpy operation of its own (numpy
fuses nothing), ``np.rint`` and the nodata move.  ``match_table`` / ``match_plane`` are what the test bodies compare the device with;
tests/test_scene_match_emulated.py pins them to the oracle's ``match_histograms_plane``.
"""
import ctypes as C

import numpy as np

from emu_backend import arr, obj
from emu_tile_metrics_masked import EmuPoolTileMetricsMasked

CODES = 65536
f64 = np.float64


def histogram(codes, nodata=None):
    """int64 [65536] of a uint16 array, the code ``nodata`` left out"""
    h = np.bincount(np.asarray(codes).reshape(-1).astype(np.int64), minlength=CODES).astype(np.int64)
    if nodata is not None:
        h[int(nodata)] = 0
    return h


def move_off(code, nodata):
    """the nodata move on an integer array: nodata -> nodata + 1 (65534 for 65535)"""
    if nodata is None:
        return code
    return np.where(code == int(nodata), 65534 if int(nodata) == 65535 else int(nodata) + 1, code)


def interp_table(src_hist, ref_hist):
    """float64 [65536]: y_v of the header, before rounding; None where a histogram is empty"""
    src_hist, ref_hist = np.asarray(src_hist, dtype=np.int64), np.asarray(ref_hist, dtype=np.int64)
    ns, nr = int(src_hist.sum()), int(ref_hist.sum())
    if ns == 0 or nr == 0:
        return None
    t = np.flatnonzero(ref_hist > 0)
    q = np.cumsum(ref_hist)[t].astype(f64) / f64(nr)
    x = np.cumsum(src_hist).astype(f64) / f64(ns)
    tf = t.astype(f64)
    j = np.searchsorted(q, x, side="right") - 1                                   # the last j with q_j <= x_v; -1: x_v < q_0
    y = np.empty(CODES, dtype=f64)
    low, high = j < 0, j >= len(t) - 1
    y[low] = tf[0]
    y[high] = tf[-1]
    mid = ~low & ~high
    jm, xm = j[mid], x[mid]
    dt = tf[jm + 1] - tf[jm]
    dq = q[jm + 1] - q[jm]
    slope = dt / dq
    dx = xm - q[jm]
    rise = slope * dx
    y[mid] = np.where(xm == q[jm], tf[jm], rise + tf[jm])
    return y


def match_table(src_hist, ref_hist, nodata=None):
    """uint16 [65536]: the table of nirgan_scene_match_lut"""
    y = interp_table(src_hist, ref_hist)
    if y is None:
        return np.arange(CODES, dtype=np.uint16)
    return move_off(np.rint(y).astype(np.int64), nodata).astype(np.uint16)


def apply_table(codes, lut, nodata=None):
    codes = np.asarray(codes)
    res = np.asarray(lut)[codes.astype(np.int64)]
    return (res if nodata is None else np.where(codes == int(nodata), np.uint16(int(nodata)), res)).astype(np.uint16)


def match_plane(plane, reference, nodata=None, reference_nodata=None):
    """the whole route on two uint16 arrays -> uint16 array shaped like ``plane``"""
    lut = match_table(histogram(plane, nodata), histogram(reference, reference_nodata), nodata)
    return apply_table(plane, lut, nodata)


def u16(ptr, n):
    return np.ctypeslib.as_array((C.c_uint16 * int(n)).from_address(int(ptr)))


def i64(ptr, n):
    return np.ctypeslib.as_array((C.c_int64 * int(n)).from_address(int(ptr)))


class EmuSceneMatch(EmuPoolTileMetricsMasked):
    def _plane_error(self, d, who):
        if not d.plane:
            return f"{who}: null pointer (d or plane)"
        if not 1 <= d.n < 2 ** 31:
            return f"{who}: n outside 1 .. 2^31-1"
        if d.has_nodata and not 0 <= d.nodata <= 65535:
            return f"{who}: nodata outside 0 .. 65535"
        if int(d.plane) % 2:
            return f"{who}: the plane is not 2-byte aligned"
        return None

    def nirgan_scene_hist(self, ref, stream=None):
        who = "scene_hist"
        self.calls.append(who)
        if not ref:
            return self._fail(f"{who}: null pointer (d or plane)")
        d = obj(ref)
        err = self._plane_error(d, who)
        if err:
            return self._fail(err)
        if not d.hist:
            return self._fail(f"{who}: null pointer (hist)")
        if int(d.hist) % 8:
            return self._fail(f"{who}: hist is not 8-byte aligned")
        i64(d.hist, CODES)[...] += histogram(u16(d.plane, d.n), d.nodata if d.has_nodata else None)
        return 0

    def nirgan_scene_match_lut(self, ref, stream=None):
        who = "scene_match_lut"
        self.calls.append(who)
        if not ref:
            return self._fail(f"{who}: null pointer (d, src_hist, ref_hist or lut)")
        d = obj(ref)
        if not (d.src_hist and d.ref_hist and d.lut):
            return self._fail(f"{who}: null pointer (d, src_hist, ref_hist or lut)")
        if d.has_nodata and not 0 <= d.nodata <= 65535:
            return self._fail(f"{who}: nodata outside 0 .. 65535")
        if any(int(p or 0) % 8 for p in (d.src_hist, d.ref_hist, d.lut, d.totals)):
            return self._fail(f"{who}: src_hist, ref_hist, lut or totals is not 8-byte aligned")
        src, refh = i64(d.src_hist, CODES), i64(d.ref_hist, CODES)
        u16(d.lut, CODES)[...] = match_table(src, refh, d.nodata if d.has_nodata else None)
        if d.totals:
            i64(d.totals, 2)[...] = (src.sum(), refh.sum())
        return 0

    def nirgan_scene_lut_apply(self, ref, stream=None):
        who = "scene_lut_apply"
        self.calls.append(who)
        if not ref:
            return self._fail(f"{who}: null pointer (d or plane)")
        d = obj(ref)
        err = self._plane_error(d, who)
        if err:
            return self._fail(err)
        if not (d.lut and d.out):
            return self._fail(f"{who}: null pointer (lut or out)")
        if int(d.out) % 2:
            return self._fail(f"{who}: out is not 2-byte aligned")
        if int(d.lut) % 8:
            return self._fail(f"{who}: lut is not 8-byte aligned")
        a, b, nbytes = int(d.plane), int(d.out), 2 * d.n
        if not (a == b or a + nbytes <= b or b + nbytes <= a):
            return self._fail(f"{who}: out overlaps the plane without being the plane")
        res = apply_table(u16(d.plane, d.n).copy(), u16(d.lut, CODES), d.nodata if d.has_nodata else None)
        u16(d.out, d.n)[...] = res
        return 0
