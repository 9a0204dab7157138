"""numpy statement of the validation-panel entries of include/nirgan_hip.h (nirgan_val_panel / _ws_bytes) -- TEST INFRASTRUCTURE ONLY,
installed with ``nirgan_hip.lib.set_backend`` like tests/emu_baselines.py; it extends tests/emu_time_series.py so that one emulator
serves a whole ``fit`` run.

Restated from the descriptor alone with stock numpy: ``np.histogram`` on the float32 stretch, ``np.sort`` for the order statistics
(rank floor and ceil of q (n - 1), interpolated in float64 and rounded once), float32 NDVI with the association of csrc/losses.hip.
Contract enforced (the header's): every computed output is OVERWRITTEN, a NULL output is skipped, columns 6 and 7 of ``stats`` stay
untouched without rgb, the workspace must hold ``_ws_bytes`` bytes, and the argument checks come before any work.
"""
import math

import numpy as np

from emu_backend import arr, obj
from emu_time_series import EmuTimeSeries

BINS, COLS = 100, 8
PPB, TILE_INTS, PART = 2048, 9 * 2048 + 32, 8
f32 = np.float32


def clamp01(v):
    """torch.clamp(v, 0, 1): a NaN passes through"""
    with np.errstate(invalid="ignore"):
        return np.where(v < 0, f32(0), np.where(v > 1, f32(1), v)).astype(f32)


def percentile_pair(x, perc):
    """x [n] float32 -> (lo, hi) float32: torch.quantile(x, q) for q = perc / 100 and (100 - perc) / 100"""
    if np.isnan(x).any():
        return f32(np.nan), f32(np.nan)
    s = np.sort(x).astype(np.float64)
    out = []
    for q in (perc / 100.0, (100.0 - perc) / 100.0):
        pos = q * (x.size - 1)
        lo, hi = min(max(math.floor(pos), 0), x.size - 1), min(max(math.ceil(pos), 0), x.size - 1)
        with np.errstate(invalid="ignore"):
            t = pos - lo                                   # torch's lerp: from the far end for t >= 0.5
            out.append(f32(s[lo] + t * (s[hi] - s[lo]) if t < 0.5 else s[hi] - (s[hi] - s[lo]) * (1.0 - t)))
    return out[0], out[1]


class EmuValPanel(EmuTimeSeries):
    def nirgan_val_panel_ws_bytes(self, B, H, W):
        if B <= 0 or H <= 0 or W <= 0 or B * 3 * H * W >= 2 ** 31:
            return 0
        return B * TILE_INTS * 4 + B * (-(-(H * W) // PPB)) * PART * 4

    def nirgan_val_panel(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("val_panel")
        if not d.nir or not d.pred:
            return self._fail("val_panel: null pointer (nir and pred are required)")
        if d.B <= 0 or d.H <= 0 or d.W <= 0:
            return self._fail("val_panel: empty problem")
        if d.ch <= 0 or d.cw <= 0:
            return self._fail("val_panel: window extent must be positive")
        if d.y0 < 0 or d.x0 < 0 or d.y0 + d.ch > d.H or d.x0 + d.cw > d.W:
            return self._fail("val_panel: window outside the image")
        if d.B * 3 * d.H * d.W >= 2 ** 31 or d.B > 65535:
            return self._fail("val_panel: batch too large")
        if not (0 <= d.perc < 50):
            return self._fail("val_panel: perc must lie in [0, 50)")
        if not d.rgb and (d.ndvi_nir_disp or d.ndvi_pred_disp or d.rgb_disp):
            return self._fail("val_panel: the NDVI and rgb display planes need rgb")
        if not d.ws or d.ws_bytes < self.nirgan_val_panel_ws_bytes(d.B, d.H, d.W):
            return self._fail("val_panel: workspace too small")
        B, H, W, ch, cw = d.B, d.H, d.W, d.ch, d.cw
        win = (slice(None), slice(d.y0, d.y0 + ch), slice(d.x0, d.x0 + cw))
        n = arr(d.nir, B * H * W).reshape(B, H, W)
        p = arr(d.pred, B * H * W).reshape(B, H, W)
        gain = f32(d.gain)
        with np.errstate(all="ignore"):
            vn, vp = clamp01(gain * n[win]), clamp01(gain * p[win])
            if d.hist:
                hist = arr(d.hist, B * 2 * BINS, np.int32).reshape(B, 2, BINS)
                for b in range(B):
                    hist[b, 0] = np.histogram(vn[b].ravel(), bins=BINS, range=(0, 1))[0]
                    hist[b, 1] = np.histogram(vp[b].ravel(), bins=BINS, range=(0, 1))[0]
            if d.nir_disp:
                arr(d.nir_disp, B * ch * cw).reshape(B, ch, cw)[:] = vn
            if d.pred_disp:
                arr(d.pred_disp, B * ch * cw).reshape(B, ch, cw)[:] = vp
            rgb = arr(d.rgb, B * 3 * H * W).reshape(B, 3, H, W) if d.rgb else None
            for ptr, v in ((d.ndvi_nir_disp, n), (d.ndvi_pred_disp, p)):
                if ptr:
                    R = rgb[:, 0][win]
                    idx = (v[win] - R) / ((v[win] + R) + f32(1e-6))
                    arr(ptr, B * ch * cw).reshape(B, ch, cw)[:] = (np.clip(idx, f32(-1), f32(1)) + f32(1)) / f32(2)
            lohi = None
            if rgb is not None and (d.stats or d.rgb_disp):
                c = clamp01(rgb) if d.clamp_rgb else rgb
                lohi = [percentile_pair(c[b].ravel(), float(d.perc)) for b in range(B)]
            if d.stats:
                stats = arr(d.stats, B * COLS).reshape(B, COLS)
                for j, v in enumerate((n, p)):
                    v = v.reshape(B, -1)
                    stats[:, 3 * j] = v.min(axis=1)
                    stats[:, 3 * j + 1] = v.max(axis=1)
                    stats[:, 3 * j + 2] = v.mean(axis=1, dtype=np.float64).astype(f32)
                if lohi is not None:
                    stats[:, 6:8] = np.asarray(lohi, dtype=f32)
            if d.rgb_disp:
                out = arr(d.rgb_disp, B * ch * cw * 3).reshape(B, ch, cw, 3)
                for b in range(B):
                    lo, hi = lohi[b]
                    cb = np.moveaxis(c[b][:, win[1], win[2]], 0, -1)
                    out[b] = f32(0) if hi == lo else clamp01((cb - lo) / (hi - lo))
        return 0
