"""numpy statement of the per-tile metrics entries of include/nirgan_hip.h (nirgan_tile_metrics / _ws_elems) -- TEST INFRASTRUCTURE
ONLY, installed with ``nirgan_hip.lib.set_backend`` like tests/emu_baselines.py, which it extends.

Float32 arithmetic restated from the descriptor alone: the evaluation window is cut out of the stored planes by indexing, the SSIM
filter reflects at the window's border, the index formulas are those of csrc/losses.hip in L1 form.  Contract enforced (the header's):
every computed column of ``rows`` is OVERWRITTEN, the index columns stay untouched without rgb and the patch means with patch == 0,
the workspace must hold B x (32x32 blocks of the window) x 8 floats, and the argument checks come before any work.
"""
import numpy as np

from emu_backend import arr, obj
from emu_baselines import EmuBaselines

COLS, NV, TILE = 9, 8, 32
f32 = np.float32


class EmuTileMetrics(EmuBaselines):
    def nirgan_tile_metrics_ws_elems(self, B, ch, cw):
        if B <= 0 or ch <= 0 or cw <= 0:
            return 0
        return B * (-(-ch // TILE)) * (-(-cw // TILE)) * NV

    def nirgan_tile_metrics(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("tile_metrics")
        if not d.nir or not d.pred or not d.ws or not d.rows:
            return self._fail("tile_metrics: null pointer")
        if d.B <= 0 or d.H <= 0 or d.W <= 0:
            return self._fail("tile_metrics: empty problem")
        if d.window < 1 or d.window > 11 or d.window % 2 == 0:
            return self._fail("tile_metrics: window must be odd and <= 11")
        r = d.window // 2
        if d.ch <= 0 or d.cw <= 0 or d.y0 < 0 or d.x0 < 0 or d.y0 + d.ch > d.H or d.x0 + d.cw > d.W:
            return self._fail("tile_metrics: evaluation window outside the image")
        if d.ch <= r or d.cw <= r:
            return self._fail("tile_metrics: evaluation window smaller than the SSIM window radius")
        if d.sigma <= 0 or d.max_val <= 0:
            return self._fail("tile_metrics: sigma and max_val must be positive")
        if d.patch < 0 or d.patch > d.ch or d.patch > d.cw:
            return self._fail("tile_metrics: patch larger than the evaluation window")
        if d.ws_elems < self.nirgan_tile_metrics_ws_elems(d.B, d.ch, d.cw):
            return self._fail("tile_metrics: workspace too small")
        B, H, W, ch, cw = d.B, d.H, d.W, d.ch, d.cw
        win = (slice(None), slice(None), slice(d.y0, d.y0 + ch), slice(d.x0, d.x0 + cw))
        n = arr(d.nir, B * H * W).reshape(B, 1, H, W)[win][:, 0]
        p = arr(d.pred, B * H * W).reshape(B, 1, H, W)[win][:, 0]
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
        ssim = ((f32(2) * mu1 * mu2 + c1) * (f32(2) * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2) + f32(d.eps))
        rows = arr(d.rows, B * COLS).reshape(B, COLS)
        diff = p - n
        rows[:, 0] = np.abs(diff).mean(axis=(1, 2), dtype=f32)
        l2 = (diff * diff).mean(axis=(1, 2), dtype=f32)
        rows[:, 1] = l2
        rows[:, 2] = ssim.mean(axis=(1, 2), dtype=f32)
        with np.errstate(divide="ignore"):
            rows[:, 3] = np.where(l2 > 0, f32(10) * np.log10(f32(d.max_val) ** 2 / l2), f32(np.inf))
        if d.rgb:
            rgb = arr(d.rgb, B * 3 * H * W).reshape(B, 3, H, W)[win]
            R, G, Bl = rgb[:, 0], rgb[:, 1], rgb[:, 2]
            e = f32(1e-6)

            def col(idx):
                return np.abs(idx(p) - idx(n)).mean(axis=(1, 2), dtype=f32)
            rows[:, 4] = col(lambda v: (v - R) / (v + R + e))
            rows[:, 5] = col(lambda v: (v - G) / (v + G + e))
            c = (R - f32(7.5)) * (Bl + f32(1))
            rows[:, 6] = col(lambda v: f32(2.5) * ((v - R) / ((v + f32(6)) * c + e)))
        if d.patch > 0:
            py, px = ch // 2 - d.patch // 2, cw // 2 - d.patch // 2
            sq = (slice(None), slice(py, py + d.patch), slice(px, px + d.patch))
            rows[:, 7] = n[sq].mean(axis=(1, 2), dtype=f32)
            rows[:, 8] = p[sq].mean(axis=(1, 2), dtype=f32)
        return 0
