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


def window_error(d, name, entry_ptrs=True):
    """the checks the window entries share, in the library's order: the message, or None.  The entries' own checks follow it (the
    library has some of them in between: with one fault at a time the message is the same)"""
    if not d.nir or not d.pred or not entry_ptrs or not d.ws or not d.rows:
        return f"{name}: null pointer"
    if d.B <= 0 or d.H <= 0 or d.W <= 0:
        return f"{name}: empty problem"
    if d.window < 1 or d.window > 11 or d.window % 2 == 0:
        return f"{name}: window must be odd and <= 11"
    if d.ch <= 0 or d.cw <= 0 or d.y0 < 0 or d.x0 < 0 or d.y0 + d.ch > d.H or d.x0 + d.cw > d.W:
        return f"{name}: evaluation window outside the image"
    if d.ch <= d.window // 2 or d.cw <= d.window // 2:
        return f"{name}: evaluation window smaller than the SSIM window radius"
    if d.sigma <= 0 or d.max_val <= 0:
        return f"{name}: sigma and max_val must be positive"
    if d.H * d.W >= 2 ** 31:
        return f"{name}: image too large"
    return None


def window_cut(d):
    """(nir, pred) [B][ch][cw] and rgb [B][3][ch][cw] or None: the evaluation window cut out of the stored planes by indexing"""
    B, H, W = d.B, d.H, d.W
    win = (Ellipsis, slice(d.y0, d.y0 + d.ch), slice(d.x0, d.x0 + d.cw))
    n, p = (arr(ptr, B * H * W).reshape(B, H, W)[win] for ptr in (d.nir, d.pred))
    return n, p, (arr(d.rgb, B * 3 * H * W).reshape(B, 3, H, W)[win] if d.rgb else None)


def ssim_map(n, p, d):
    """float32 SSIM map of the window: separable Gaussian, reflect at the WINDOW's border"""
    r, (ch, cw) = d.window // 2, n.shape[1:]
    x = np.arange(d.window, dtype=np.float64) - r
    k = np.exp(-x * x / (2.0 * float(d.sigma) ** 2))
    k = (k / k.sum()).astype(f32)

    def filt(t):
        t = np.pad(t, ((0, 0), (r, r), (r, r)), mode="reflect")
        h = sum(k[i] * t[:, :, i:i + cw] for i in range(d.window))
        return sum(k[i] * h[:, i:i + ch, :] for i in range(d.window)).astype(f32)
    c1, c2 = f32((0.01 * d.max_val) ** 2), f32((0.03 * d.max_val) ** 2)
    mu1, mu2 = filt(n), filt(p)
    s1, s2, s12 = filt(n * n) - mu1 * mu1, filt(p * p) - mu2 * mu2, filt(n * p) - mu1 * mu2
    return ((f32(2) * mu1 * mu2 + c1) * (f32(2) * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2) + f32(d.eps))


def index_terms(n, p, rgb):
    """|index(pred) - index(nir)| per pixel of NDVI, NDWI, EVI: the formulas of csrc/losses.hip"""
    R, G, Bl = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    e = f32(1e-6)
    c = (R - f32(7.5)) * (Bl + f32(1))
    return [np.abs(idx(p) - idx(n)) for idx in (lambda v: (v - R) / (v + R + e), lambda v: (v - G) / (v + G + e),
                                                lambda v: f32(2.5) * ((v - R) / ((v + f32(6)) * c + e)))]


class EmuTileMetrics(EmuBaselines):
    def nirgan_tile_metrics_ws_elems(self, B, ch, cw):
        if B <= 0 or ch <= 0 or cw <= 0:
            return 0
        return B * (-(-ch // TILE)) * (-(-cw // TILE)) * NV

    def nirgan_tile_metrics(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("tile_metrics")
        err = window_error(d, "tile_metrics")
        if err:
            return self._fail(err)
        if d.patch < 0 or d.patch > d.ch or d.patch > d.cw:
            return self._fail("tile_metrics: patch larger than the evaluation window")
        if d.ws_elems < self.nirgan_tile_metrics_ws_elems(d.B, d.ch, d.cw):
            return self._fail("tile_metrics: workspace too small")
        B, ch, cw = d.B, d.ch, d.cw
        n, p, rgb = window_cut(d)
        rows = arr(d.rows, B * COLS).reshape(B, COLS)
        diff = p - n
        rows[:, 0] = np.abs(diff).mean(axis=(1, 2), dtype=f32)
        l2 = (diff * diff).mean(axis=(1, 2), dtype=f32)
        rows[:, 1] = l2
        rows[:, 2] = ssim_map(n, p, d).mean(axis=(1, 2), dtype=f32)
        with np.errstate(divide="ignore"):
            rows[:, 3] = np.where(l2 > 0, f32(10) * np.log10(f32(d.max_val) ** 2 / l2), f32(np.inf))
        if rgb is not None:
            for col, t in zip((4, 5, 6), index_terms(n, p, rgb)):
                rows[:, col] = t.mean(axis=(1, 2), dtype=f32)
        if d.patch > 0:
            py, px = ch // 2 - d.patch // 2, cw // 2 - d.patch // 2
            sq = (slice(None), slice(py, py + d.patch), slice(px, px + d.patch))
            rows[:, 7] = n[sq].mean(axis=(1, 2), dtype=f32)
            rows[:, 8] = p[sq].mean(axis=(1, 2), dtype=f32)
        return 0
