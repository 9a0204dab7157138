"""numpy statement of the overlapping-tile entries of include/nirgan_hip.h (nirgan_tile_count_ov / nirgan_tile_gather_ov /
nirgan_tile_blend) -- TEST INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend`` like tests/emu_backend.py, which it
extends.

Float32 arithmetic restated from the descriptor alone, one tile after the other in ascending tile number.  Contract enforced (the
header's): the scene is never read before it was written (a pixel's lowest-numbered covering tile STORES w * v, every later one adds
fma(w, v, acc)), so a scene pre-filled with NaN comes out finite; pixels past H x W are dropped; the argument checks come before any
work and name the entry.
"""
import numpy as np

from emu_backend import EmuBackend, arr, obj

f32 = np.float32


def reflect_any(i, n):
    """the gather's reflect rule continued with period 2 (n - 1): defined for every index"""
    if n == 1:
        return np.zeros_like(i)
    i = np.mod(i, 2 * (n - 1))
    return np.where(i >= n, 2 * (n - 1) - i, i)


def per_axis(extent, core, stride):
    return 1 if extent <= core else -(-(extent - core) // stride) + 1


def later_weight(t, overlap, window):
    """float32 r(t) of the later tile"""
    u = (t.astype(f32) + f32(0.5)) / f32(overlap)
    return u if window == 0 else f32(0.5) - f32(0.5) * np.cos(f32(np.pi) * u)


def axis_weights(i, nt, core, stride, overlap, window):
    """for tile i of an axis: (float32 weight, 'this tile is the position's lowest-numbered cover') per usable position 0 .. core - 1"""
    w, lowest = np.ones(core, dtype=f32), np.ones(core, dtype=bool)
    if overlap:
        t = np.arange(overlap)
        if i >= 1:
            w[:overlap] = later_weight(t, overlap, window)
            lowest[:overlap] = False
        if i < nt - 1:
            w[stride:] = f32(1) - later_weight(t, overlap, window)
    return w, lowest


class EmuTileBlend(EmuBackend):
    def nirgan_tile_count_ov(self, B, H, W, tile, margin, overlap):
        if B <= 0 or H <= 0 or W <= 0 or tile <= 0 or margin < 0 or 2 * margin >= tile or overlap < 0 or 2 * overlap > tile - 2 * margin:
            return 0
        core = tile - 2 * margin
        return B * per_axis(H, core, core - overlap) * per_axis(W, core, core - overlap)

    def _blend_geometry(self, d, who):
        if not d.scene or not d.tiles:
            return None, self._fail(f"{who}: null pointer")
        if d.B <= 0 or d.C <= 0 or d.H <= 0 or d.W <= 0 or d.tile <= 0:
            return None, self._fail(f"{who}: bad shape")
        if d.margin < 0 or 2 * d.margin >= d.tile:
            return None, self._fail(f"{who}: margin must be below tile / 2")
        core = d.tile - 2 * d.margin
        if d.overlap < 0 or 2 * d.overlap > core:
            return None, self._fail(f"{who}: overlap outside 0 .. core / 2")
        if d.window not in (0, 1):
            return None, self._fail(f"{who}: unknown window")
        if d.H >= 2 ** 30 or d.W >= 2 ** 30 or d.H * d.W >= 2 ** 31 or d.C * d.tile * d.tile >= 2 ** 31:
            return None, self._fail(f"{who}: a plane of the scene or a tile has 2^31 elements or more")
        stride = core - d.overlap
        nth, ntw = per_axis(d.H, core, stride), per_axis(d.W, core, stride)
        if d.B * nth * ntw >= 2 ** 31:
            return None, self._fail(f"{who}: 2^31 tiles or more")
        if d.first < 0 or d.n <= 0 or d.first + d.n > d.B * nth * ntw:
            return None, self._fail(f"{who}: tile range")
        return (core, stride, nth, ntw), 0

    def nirgan_tile_gather_ov(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("tile_gather_ov")
        geo, rc = self._blend_geometry(d, "tile_gather_ov")
        if rc:
            return rc
        core, stride, nth, ntw = geo
        src = arr(d.scene, d.B * d.C * d.H * d.W).reshape(d.B, d.C, d.H, d.W)
        dst = arr(d.tiles, d.n * d.C * d.tile * d.tile).reshape(d.n, d.C, d.tile, d.tile)
        for k in range(d.n):
            b, t = divmod(d.first + k, nth * ntw)
            ti, tj = divmod(t, ntw)
            hh = reflect_any(ti * stride + np.arange(d.tile) - d.margin, d.H)
            ww = reflect_any(tj * stride + np.arange(d.tile) - d.margin, d.W)
            dst[k] = src[b][:, hh][:, :, ww]
        return 0

    def nirgan_tile_blend(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("tile_blend")
        geo, rc = self._blend_geometry(d, "tile_blend")
        if rc:
            return rc
        core, stride, nth, ntw = geo
        m = d.margin
        src = arr(d.tiles, d.n * d.C * d.tile * d.tile).reshape(d.n, d.C, d.tile, d.tile)
        dst = arr(d.scene, d.B * d.C * d.H * d.W).reshape(d.B, d.C, d.H, d.W)
        for k in range(d.n):
            b, t = divmod(d.first + k, nth * ntw)
            ti, tj = divmod(t, ntw)
            h0, w0 = ti * stride, tj * stride
            nh, nw = min(core, d.H - h0), min(core, d.W - w0)                   # pixels past H x W are dropped
            wy, ly = axis_weights(ti, nth, core, stride, d.overlap, d.window)
            wx, lx = axis_weights(tj, ntw, core, stride, d.overlap, d.window)
            w = (wy[:nh, None] * wx[None, :nw]).astype(f32)
            store = ly[:nh, None] & lx[None, :nw]
            v = src[k, :, m:m + nh, m:m + nw]
            region = dst[b, :, h0:h0 + nh, w0:w0 + nw]
            acc = np.where(store, f32(0), region)                               # the stored value is not read where this tile stores
            fma = (w.astype(np.float64) * v.astype(np.float64) + acc.astype(np.float64)).astype(f32)
            region[...] = np.where(store, w * v, fma)
        return 0
