"""numpy statement of the land-cover-stratified metrics entries of include/nirgan_hip.h (nirgan_class_metrics / _ws_elems) -- TEST
INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend`` like tests/emu_baselines.py; it extends tests/emu_val_panel.py so
that one emulator serves a whole ``fit`` run.

Float32 arithmetic restated from the descriptor alone: the evaluation window is cut out of the stored planes and of the mask by
indexing, the SSIM map is that of the whole window (reflect at the window's border), each class takes the mean over its own pixels
(sums in float64, rounded once), the index formulas are those of csrc/losses.hip in L1 form.  Contract enforced (the header's): every
computed column of ``rows`` is OVERWRITTEN, the index columns stay untouched without rgb, a class without pixels has count 0 and NaN
in its other computed columns, the workspace must hold B x (32x32 blocks of the window) x classes x 8 floats, and the argument
checks come before any work.
"""
import ctypes as C

import numpy as np

from emu_backend import arr, obj
from emu_val_panel import EmuValPanel

COLS, NV, TILE, CLASS_MAX = 8, 8, 32, 8
f32 = np.float32


def bytes_at(ptr, n):
    if hasattr(ptr, "value"):
        ptr = ptr.value
    return np.ctypeslib.as_array((C.c_uint8 * int(n)).from_address(int(ptr)))


class EmuClassMetrics(EmuValPanel):
    def nirgan_class_metrics_ws_elems(self, B, ch, cw, classes):
        if B <= 0 or ch <= 0 or cw <= 0 or classes < 1 or classes > CLASS_MAX:
            return 0
        return B * (-(-ch // TILE)) * (-(-cw // TILE)) * classes * NV

    def nirgan_class_metrics(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("class_metrics")
        if not d.nir or not d.pred or not d.mask or not d.ws or not d.rows:
            return self._fail("class_metrics: null pointer")
        if d.B <= 0 or d.H <= 0 or d.W <= 0:
            return self._fail("class_metrics: empty problem")
        if d.classes < 1 or d.classes > CLASS_MAX:
            return self._fail("class_metrics: classes must lie in 1..8")
        if d.window < 1 or d.window > 11 or d.window % 2 == 0:
            return self._fail("class_metrics: window must be odd and <= 11")
        r = d.window // 2
        if d.ch <= 0 or d.cw <= 0 or d.y0 < 0 or d.x0 < 0 or d.y0 + d.ch > d.H or d.x0 + d.cw > d.W:
            return self._fail("class_metrics: evaluation window outside the image")
        if d.ch <= r or d.cw <= r:
            return self._fail("class_metrics: evaluation window smaller than the SSIM window radius")
        if d.sigma <= 0 or d.max_val <= 0:
            return self._fail("class_metrics: sigma and max_val must be positive")
        if d.H * d.W >= 2 ** 31:
            return self._fail("class_metrics: image too large")
        if d.ch * d.cw >= 2 ** 24:
            return self._fail("class_metrics: evaluation window: the counts are exact as floats below 2^24 only")
        if d.ws_elems < self.nirgan_class_metrics_ws_elems(d.B, d.ch, d.cw, d.classes):
            return self._fail("class_metrics: workspace too small")
        B, H, W, ch, cw, K = d.B, d.H, d.W, d.ch, d.cw, d.classes
        win = (slice(None), slice(d.y0, d.y0 + ch), slice(d.x0, d.x0 + cw))
        n = arr(d.nir, B * H * W).reshape(B, H, W)[win]
        p = arr(d.pred, B * H * W).reshape(B, H, W)[win]
        m = bytes_at(d.mask, B * H * W).reshape(B, H, W)[win]
        x = np.arange(d.window, dtype=np.float64) - r
        k = np.exp(-x * x / (2.0 * float(d.sigma) ** 2))
        k = (k / k.sum()).astype(f32)

        def filt(t):                                   # separable, reflect at the WINDOW's border
            t = np.pad(t, ((0, 0), (r, r), (r, r)), mode="reflect")
            h = sum(k[i] * t[:, :, i:i + cw] for i in range(d.window))
            return sum(k[i] * h[:, i:i + ch, :] for i in range(d.window)).astype(f32)
        c1, c2 = f32((0.01 * d.max_val) ** 2), f32((0.03 * d.max_val) ** 2)
        mu1, mu2 = filt(n), filt(p)
        s1, s2, s12 = filt(n * n) - mu1 * mu1, filt(p * p) - mu2 * mu2, filt(n * p) - mu1 * mu2
        diff = p - n
        terms = {1: np.abs(diff), 2: diff * diff,
                 3: ((f32(2) * mu1 * mu2 + c1) * (f32(2) * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2) + f32(d.eps))}
        if d.rgb:
            rgb = arr(d.rgb, B * 3 * H * W).reshape(B, 3, H, W)
            R, G, Bl = (rgb[:, i][win] for i in range(3))
            e = f32(1e-6)
            c = (R - f32(7.5)) * (Bl + f32(1))
            for col, idx in ((5, lambda v: (v - R) / (v + R + e)), (6, lambda v: (v - G) / (v + G + e)),
                             (7, lambda v: f32(2.5) * ((v - R) / ((v + f32(6)) * c + e)))):
                terms[col] = np.abs(idx(p) - idx(n))
        rows = arr(d.rows, B * K * COLS).reshape(B, K, COLS)
        for b in range(B):
            for cls in range(K):
                sel = m[b] == cls
                count = int(sel.sum())
                rows[b, cls, 0] = count
                for col, t in terms.items():
                    rows[b, cls, col] = f32(t[b][sel].sum(dtype=np.float64) / count) if count else f32(np.nan)
                l2 = rows[b, cls, 2]
                with np.errstate(divide="ignore"):
                    rows[b, cls, 4] = f32(np.nan) if not count else (f32(10) * np.log10(f32(d.max_val) ** 2 / l2) if l2 > 0 else f32(np.inf))
        return 0
