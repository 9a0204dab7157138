"""numpy statement of the masked per-tile metrics entries of include/nirgan_hip.h (nirgan_tile_metrics_masked / _ws_elems) -- TEST
INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend``; it extends tests/emu_tile_metrics.py.

Float32 arithmetic restated from the descriptor alone: the window is cut out of the stored planes (the mask included) by indexing,
``valid != 0`` keeps a pixel, a pixel is support-clean when the reflect-padded mask is true at all (2r+1)^2 taps.  Every per-pixel
term is selected with ``np.where`` before it is summed, so that whatever lies in the images at a dropped pixel is never part of an
output (the SSIM map is computed everywhere and only its support-clean pixels are selected: those see no dropped pixel).  The selected
terms are summed over arrays laid out like those of ``EmuTileMetrics`` and divided by the count: with a mask of ones the terms, their
order and the divisor are its own, so the two agree bitwise, as the header promises of the device.  Contract enforced (the
header's): the index columns stay untouched without rgb and the patch means with patch == 0, the workspace must hold
B x (32x32 blocks) x 11 floats, ch * cw <= 2^24, and the argument checks come before any work.  ``EmuPoolTileMetricsMasked`` joins it
to the scene pool's emulator chain (tests/emu_valid_mask.py) for the tests that cut their batches from a ScenePool.
"""
import numpy as np

from emu_backend import arr, obj
from emu_tile_metrics import EmuTileMetrics, index_terms, ssim_map, window_cut, window_error
from emu_valid_mask import EmuValidMask

COLS, NV, TILE = 11, 11, 32
f32 = np.float32


def support_clean(keep, r):
    """[B][ch][cw] bool: every tap of the (2r+1)^2 support, reflected at the window's border, is kept"""
    ch, cw = keep.shape[1:]
    t = np.pad(keep, ((0, 0), (r, r), (r, r)), mode="reflect")
    out = np.ones_like(keep)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out &= t[:, dy:dy + ch, dx:dx + cw]
    return out


def selected_mean(values, keep):
    """fp32 [B]: the sum of ``values`` [B][h][w] over ``keep`` divided by its count, NaN over an empty selection"""
    return over_count(np.where(keep, values, f32(0)).sum(axis=(1, 2), dtype=f32), keep)


def over_count(total, keep):
    count = np.count_nonzero(keep, axis=(1, 2)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (total / count).astype(f32)


class EmuTileMetricsMasked(EmuTileMetrics):
    def nirgan_tile_metrics_masked_ws_elems(self, B, ch, cw):
        if B <= 0 or ch <= 0 or cw <= 0:
            return 0
        return B * (-(-ch // TILE)) * (-(-cw // TILE)) * NV

    def nirgan_tile_metrics_masked(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("tile_metrics_masked")
        err = window_error(d, "tile_metrics_masked", entry_ptrs=bool(d.valid))
        if err:
            return self._fail(err)
        if d.patch < 0 or d.patch > d.ch or d.patch > d.cw:
            return self._fail("tile_metrics_masked: patch larger than the evaluation window")
        if d.ch * d.cw > 2 ** 24:
            return self._fail("tile_metrics_masked: more than 2^24 pixels in the evaluation window")
        if d.ws_elems < self.nirgan_tile_metrics_masked_ws_elems(d.B, d.ch, d.cw):
            return self._fail("tile_metrics_masked: workspace too small")
        B, H, W, ch, cw = d.B, d.H, d.W, d.ch, d.cw
        win = (Ellipsis, slice(d.y0, d.y0 + ch), slice(d.x0, d.x0 + cw))
        n, p, rgb = window_cut(d)
        keep = arr(d.valid, B * H * W).reshape(B, H, W)[win] != 0                # -0.0 != 0 is False
        clean = support_clean(keep, d.window // 2)
        rows = arr(d.rows, B * COLS).reshape(B, COLS)
        with np.errstate(all="ignore"):                                           # garbage at dropped pixels is computed, never selected
            diff = p - n
            rows[:, 0] = selected_mean(np.abs(diff), keep)
            l2 = selected_mean(diff * diff, keep)
            rows[:, 1] = l2
            rows[:, 2] = selected_mean(ssim_map(n, p, d), clean)
            rows[:, 3] = np.where(np.isnan(l2), f32(np.nan), np.where(l2 > 0, f32(10) * np.log10(f32(d.max_val) ** 2 / l2), f32(np.inf)))
            if rgb is not None:
                for col, t in zip((4, 5, 6), index_terms(n, p, rgb)):
                    rows[:, col] = selected_mean(t, keep)
            if d.patch > 0:
                py, px = ch // 2 - d.patch // 2, cw // 2 - d.patch // 2
                sq = (slice(None), slice(py, py + d.patch), slice(px, px + d.patch))
                for col, t in ((7, n), (8, p)):
                    stored = np.zeros((B, H, W), f32)                             # the patch as a view of a stored plane, as in EmuTileMetrics
                    stored[win] = np.where(keep, t, f32(0))
                    rows[:, col] = over_count(stored[win][sq].sum(axis=(1, 2), dtype=f32), keep[sq])
        rows[:, 9] = np.count_nonzero(keep, axis=(1, 2))
        rows[:, 10] = np.count_nonzero(clean, axis=(1, 2))
        return 0


class EmuPoolTileMetricsMasked(EmuTileMetricsMasked, EmuValidMask):
    """the masked table on batches cut from a ScenePool: the whole emulator chain"""
