"""numpy statement of the scene-prediction entries of include/nirgan_hip.h (nirgan_scene_tile_invalid / nirgan_scene_tile_gather /
nirgan_scene_finish, the last section) -- TEST INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend``.  It joins the two
emulator chains (tests/emu_scene_split.py: the scene pool; tests/emu_tile_views.py: the blend and the views), so one backend serves
``predict_scene`` and ``ScenePool.predict`` with every ``tta``.

Written from the header alone: the usable regions as slices, the reads as index arrays (``reflect_any`` of tests/emu_tile_blend.py),
``np.float32(v) / np.float32(divisor)`` for the values, float64 for the coords, ``np.rint`` / ``astype(np.float16)`` for the outputs.
``tile_geometry`` / ``invalid_of`` / ``tile_counts`` / ``cut_tiles`` / ``tile_centres`` / ``quantise`` are what the test bodies compare
the device with.
"""
import ctypes as C

import numpy as np

from emu_backend import arr, obj
from emu_scene_pool import _pool
from emu_scene_split import EmuSceneSplit
from emu_tile_blend import per_axis, reflect_any
from emu_tile_views import EmuTileViews

f32 = np.float32
OUT_U16, OUT_F16, OUT_F32 = 0, 1, 2


def tile_geometry(H, W, tile, margin, overlap):
    """(core, stride, nth, ntw)"""
    core = tile - 2 * margin
    stride = core - overlap
    return core, stride, per_axis(H, core, stride), per_axis(W, core, stride)


def usable(t, H, W, tile, margin, overlap):
    """tile t -> (y0, x0, hy, wx): its usable region clipped to the scene"""
    core, stride, _, ntw = tile_geometry(H, W, tile, margin, overlap)
    ti, tj = divmod(t, ntw)
    return ti * stride, tj * stride, min(core, H - ti * stride), min(core, W - tj * stride)


def invalid_of(planes, nodata):
    """[3][H][W] selected planes -> bool [H][W]; nodata None: no pixel is invalid"""
    if nodata is None:
        return np.zeros(planes.shape[1:], dtype=bool)
    if planes.dtype == np.float32:
        return np.isnan(planes).any(axis=0)
    return (planes.astype(np.int64) == int(nodata)).any(axis=0)


def tile_counts(invalid, tile, margin, overlap):
    """int64 [nt]: invalid pixels per clipped usable region, by slicing"""
    H, W = invalid.shape
    _, _, nth, ntw = tile_geometry(H, W, tile, margin, overlap)
    out = np.zeros(nth * ntw, dtype=np.int64)
    for t in range(nth * ntw):
        y0, x0, hy, wx = usable(t, H, W, tile, margin, overlap)
        out[t] = int(invalid[y0:y0 + hy, x0:x0 + wx].sum())
    return out


def tiles_that_run(invalid, tile, margin, overlap):
    """the ascending list of tiles whose usable region holds a valid pixel"""
    H, W = invalid.shape
    n = tile_counts(invalid, tile, margin, overlap)
    return [t for t in range(len(n)) if n[t] < np.prod(usable(t, H, W, tile, margin, overlap)[2:])]


def cut_tiles(scene, bands, ids, tile, margin, overlap, divisor):
    """float32 [n][3][tile][tile] of the listed tiles of scene [C][H][W]"""
    _, H, W = scene.shape
    _, stride, _, ntw = tile_geometry(H, W, tile, margin, overlap)
    out = np.empty((len(ids), 3, tile, tile), dtype=f32)
    for k, t in enumerate(ids):
        ti, tj = divmod(int(t), ntw)
        hh = reflect_any(ti * stride - margin + np.arange(tile), H)
        ww = reflect_any(tj * stride - margin + np.arange(tile), W)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            out[k] = (scene[list(bands)][:, hh][:, :, ww].astype(f32) / f32(divisor)).astype(f32)
    return out


def tile_centres(geo, ids, H, W, tile, margin, overlap):
    """float32 [n][2] = (lon, lat) of the centre of every listed tile's clipped usable region; geo = (lon0, dlon, lat0, dlat)"""
    lon0, dlon, lat0, dlat = (np.float64(v) for v in geo)
    out = np.empty((len(ids), 2), dtype=f32)
    for k, t in enumerate(ids):
        y0, x0, hy, wx = usable(int(t), H, W, tile, margin, overlap)
        cx, cy = np.float64(x0 + wx // 2) + np.float64(0.5), np.float64(y0 + hy // 2) + np.float64(0.5)
        out[k] = f32(lon0 + cx * dlon), f32(lat0 + cy * dlat)
    return out


def quantise(v, invalid, kind, scale, nodata_out):
    """the finish on float32 v [..] and a bool mask of the same shape -> uint16 / float16 / float32 array"""
    v = np.asarray(v, dtype=f32)
    if kind == OUT_F32:
        return np.where(invalid, f32(nodata_out), v).astype(f32)
    if kind == OUT_F16:
        with np.errstate(over="ignore", invalid="ignore"):
            return np.where(invalid, f32(nodata_out), v).astype(np.float16)
    nd = int(nodata_out)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (v * f32(scale)).astype(f32)
    q = np.clip(np.rint(np.where(np.isnan(t), f32(0), t)), 0, 65535).astype(np.int64)
    q = np.where(q == nd, 65534 if nd == 65535 else nd + 1, q)
    return np.where(invalid | np.isnan(t), nd, q).astype(np.uint16)


class EmuScenePredict(EmuSceneSplit, EmuTileViews):
    def _scene_common(self, ref, who):
        """(descriptor, geometry, scene [C][H][W]) or (None, None, rc)"""
        if not ref:
            return None, None, self._fail(f"{who}: null pointer")
        d = obj(ref)
        if not d.scene:
            return None, None, self._fail(f"{who}: null pointer")
        if d.dtype not in (0, 1):
            return None, None, self._fail(f"{who}: unknown dtype")
        if d.C < 3 or d.H < 1 or d.W < 1:
            return None, None, self._fail(f"{who}: bad scene (C must be at least 3)")
        if d.H * d.W >= 2 ** 31:
            return None, None, self._fail(f"{who}: the plane H*W is 2^31 or more")
        if any(not 0 <= b < d.C for b in d.band):
            return None, None, self._fail(f"{who}: band outside 0 .. C-1")
        if d.has_nodata and d.dtype == 0 and not 0 <= d.nodata <= 65535:
            return None, None, self._fail(f"{who}: nodata outside 0 .. 65535")
        if d.divisor == 0 or d.divisor != d.divisor:
            return None, None, self._fail(f"{who}: divisor is 0 or NaN")
        if d.tile < 4 or d.tile % 4:
            return None, None, self._fail(f"{who}: tile is not a positive multiple of 4")
        if d.margin < 0 or 2 * d.margin >= d.tile:
            return None, None, self._fail(f"{who}: margin must be below tile / 2")
        if d.overlap < 0 or 2 * d.overlap > d.tile - 2 * d.margin:
            return None, None, self._fail(f"{who}: overlap outside 0 .. core / 2")
        geo = tile_geometry(d.H, d.W, d.tile, d.margin, d.overlap)
        if geo[2] * geo[3] >= 2 ** 31:
            return None, None, self._fail(f"{who}: 2^31 tiles or more")
        return d, geo, 0

    def _scene(self, d):
        return _pool(d.scene, d.C * d.H * d.W, d.dtype).reshape(d.C, d.H, d.W)

    def nirgan_scene_tile_invalid(self, ref, stream=None):
        who = "scene_tile_invalid"
        self.calls.append(who)
        d, geo, rc = self._scene_common(ref, who)
        if d is None:
            return rc
        if not d.counts:
            return self._fail(f"{who}: null pointer (counts)")
        scene = self._scene(d)
        bad = invalid_of(scene[list(d.band)], d.nodata if d.has_nodata else None)
        arr(d.counts, geo[2] * geo[3], np.int32)[...] = tile_counts(bad, d.tile, d.margin, d.overlap)
        return 0

    def nirgan_scene_tile_gather(self, ref, stream=None):
        who = "scene_tile_gather"
        self.calls.append(who)
        d, geo, rc = self._scene_common(ref, who)
        if d is None:
            return rc
        if not (d.ids and d.ids_host and d.tiles):
            return self._fail(f"{who}: null pointer (ids, ids_host or tiles)")
        if int(d.tiles) % 16:
            return self._fail(f"{who}: tiles is not 16-byte aligned")
        if d.n < 1 or d.n * 3 * d.tile * d.tile >= 2 ** 31:
            return self._fail(f"{who}: n or n*3*tile*tile is not in 1 .. 2^31-1")
        host = arr(d.ids_host, d.n, np.int32).tolist()
        for k, t in enumerate(host):
            if not 0 <= t < geo[2] * geo[3]:
                return self._fail(f"{who}: ids[{k}] = {t} outside 0 .. nt-1")
            if k and t <= host[k - 1]:
                return self._fail(f"{who}: ids[{k}] = {t} is not above its predecessor")
        ids = arr(d.ids, d.n, np.int32).tolist()                                  # the "device" copy
        assert ids == host
        scene = self._scene(d)
        arr(d.tiles, d.n * 3 * d.tile * d.tile).reshape(d.n, 3, d.tile, d.tile)[...] = cut_tiles(scene, d.band, ids, d.tile, d.margin, d.overlap, d.divisor)
        if d.geo and d.coords:
            arr(d.coords, d.n * 2).reshape(d.n, 2)[...] = tile_centres(arr(d.geo, 4, np.float64), ids, d.H, d.W, d.tile, d.margin, d.overlap)
        return 0

    def nirgan_scene_finish(self, ref, stream=None):
        who = "scene_finish"
        self.calls.append(who)
        d, geo, rc = self._scene_common(ref, who)
        if d is None:
            return rc
        if not (d.blended and d.out):
            return self._fail(f"{who}: null pointer (blended or out)")
        if d.out_kind not in (OUT_U16, OUT_F16, OUT_F32):
            return self._fail(f"{who}: unknown out_kind")
        if d.out_kind == OUT_U16 and not (0 <= d.nodata_out <= 65535 and d.nodata_out == int(d.nodata_out)):
            return self._fail(f"{who}: nodata_out is not an integer in 0 .. 65535")
        scene = self._scene(d)
        bad = invalid_of(scene[list(d.band)], d.nodata if d.has_nodata else None)
        v = arr(d.blended, d.H * d.W).reshape(d.H, d.W)
        res = quantise(v, bad, d.out_kind, d.scale, d.nodata_out)
        ct = {OUT_U16: C.c_uint16, OUT_F16: C.c_uint16, OUT_F32: C.c_uint32}[d.out_kind]
        dst = np.ctypeslib.as_array((ct * (d.H * d.W)).from_address(int(d.out))).reshape(d.H, d.W)
        dst[...] = res.view(dst.dtype)                                            # bit patterns: a NaN nodata_out keeps its payload
        return 0
