"""numpy statement of the window-statistics entry of include/nirgan_hip.h (nirgan_window_stats) -- TEST INFRASTRUCTURE ONLY,
installed with ``nirgan_hip.lib.set_backend`` like tests/emu_tile_metrics.py, which it extends.

Float32 arithmetic restated from the descriptor alone: the window is cut out of the stored planes by indexing, the NDVI has the
association of csrc/losses.hip, the median is the element of rank (n - 1) // 2 of the sorted window (the LOWER middle value of an
even count) and NaN with a NaN anywhere in the window.  Contract enforced (the header's): every computed column of ``rows`` is
OVERWRITTEN, columns 4 to 7 stay untouched without rgb, and the argument checks come before any work.
"""
import numpy as np

from emu_backend import arr, obj
from emu_tile_metrics import EmuTileMetrics

COLS = 8
f32 = np.float32


def lower_median(v):
    """v [T][n] float32 -> [T]"""
    out = np.sort(v, axis=1)[:, (v.shape[1] - 1) // 2].copy()
    out[np.isnan(v).any(axis=1)] = np.nan
    return out


class EmuTimeSeries(EmuTileMetrics):
    def nirgan_window_stats(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("window_stats")
        if not d.nir or not d.pred or not d.rows:
            return self._fail("window_stats: null pointer")
        if d.T <= 0 or d.H <= 0 or d.W <= 0:
            return self._fail("window_stats: empty problem")
        if d.wh <= 0 or d.ww <= 0:
            return self._fail("window_stats: window extent must be positive")
        if d.y0 < 0 or d.x0 < 0 or d.y0 + d.wh > d.H or d.x0 + d.ww > d.W:
            return self._fail("window_stats: window outside the image")
        T, H, W = d.T, d.H, d.W
        win = (slice(None), slice(d.y0, d.y0 + d.wh), slice(d.x0, d.x0 + d.ww))
        n = arr(d.nir, T * H * W).reshape(T, H, W)[win].reshape(T, -1)
        p = arr(d.pred, T * H * W).reshape(T, H, W)[win].reshape(T, -1)
        rows = arr(d.rows, T * COLS).reshape(T, COLS)
        planes = [n, p]
        if d.rgb:
            R = arr(d.rgb, T * 3 * H * W).reshape(T, 3, H, W)[:, 0][win].reshape(T, -1)
            with np.errstate(all="ignore"):
                planes += [(v - R) / ((v + R) + f32(1e-6)) for v in (n, p)]
        with np.errstate(all="ignore"):
            for q, v in enumerate(planes):
                rows[:, 2 * q] = v.mean(axis=1, dtype=f32)
                rows[:, 2 * q + 1] = lower_median(v)
        return 0
