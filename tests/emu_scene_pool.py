"""numpy / Python-int statement of the scene-pool entries of include/nirgan_hip.h (nirgan_scene_invalid_prefix / nirgan_scene_sample)
-- TEST INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend`` like tests/emu_backend.py; it extends
tests/emu_class_metrics.py (the end of the emulator chain), so one backend serves ``fit`` on a pool's loader for every model.

Written from the header alone: Philox4x32-10 from tests/emu_dropout.py, the window index as the high word of a Python-int product,
``bisect`` for the scene, ``np.cumsum`` for the prefix table, index arrays for the views, ``np.float32(v) / np.float32(divisor)`` for
the values and float64 for the coords.  ``draw_windows`` / ``cut`` / ``centre`` are what the test bodies compare the device with.
"""
import bisect
import ctypes as C

import numpy as np

from emu_backend import arr, obj
from emu_class_metrics import EmuClassMetrics
from emu_dropout import philox4x32_10

ATTEMPTS, COLS = 8, 5
f32 = np.float32


def invalid_mask(planes, nodata):
    """[4][H][W] selected planes -> bool [H][W]: any band equal to nodata (integers) or NaN (floats)"""
    if planes.dtype == np.float32:
        return np.isnan(planes).any(axis=0)
    return (planes.astype(np.int64) == int(nodata)).any(axis=0)


def prefix_table(invalid):
    """bool [H][W] -> int32 [(H+1)][(W+1)] of inclusive 2-D prefix counts behind a zero row and column"""
    H, W = invalid.shape
    P = np.zeros((H + 1, W + 1), dtype=np.int64)
    P[1:, 1:] = np.cumsum(np.cumsum(invalid.astype(np.int64), axis=0), axis=1)
    return P.astype(np.int32)


def window_counts(shapes, T):
    """the running window counts cum_windows for tile T"""
    cum, total = [], 0
    for H, W in shapes:
        if H >= T and W >= T:
            total += (H - T + 1) * (W - T + 1)
        cum.append(total)
    return cum


def draw_windows(shapes, T, B, views, seed, draw, sample0=0, prefixes=None, max_invalid=0):
    """int64 [B][4] = (scene, y0, x0, view | attempt << 8 | exhausted << 31) -- as a non-negative Python value, compare with the
    device's int32 word after ``& 0xFFFFFFFF``.  shapes: [(H, W)]; prefixes: per scene an [(H+1)][(W+1)] table or None."""
    lo, hi = seed if isinstance(seed, (tuple, list)) else (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    cum = window_counts(shapes, T)
    total = cum[-1]
    assert total > 0
    out = np.zeros((B, 4), dtype=np.int64)
    samples = (np.arange(B, dtype=np.uint64) + np.uint64(sample0 & 0xFFFFFFFF))[:, None]
    words = philox4x32_10((draw & 0xFFFFFFFF, (draw >> 32) & 0xFFFFFFFF, samples, np.arange(ATTEMPTS, dtype=np.uint64)[None, :]), (lo, hi))
    words = np.stack(words, axis=-1).tolist()                                    # [B][ATTEMPTS][4] Python ints
    for b in range(B):
        for a in range(ATTEMPTS):
            w = words[b][a]
            u = w[0] | (w[1] << 32)
            idx = (u * total) >> 64
            s = bisect.bisect_right(cum, idx)                                    # the first scene with cum > idx
            r = idx - (cum[s - 1] if s else 0)
            nx = shapes[s][1] - T + 1
            y0, x0 = r // nx, r % nx
            view = w[2] & (views - 1)
            n = 0
            if prefixes is not None and prefixes[s] is not None:
                P = prefixes[s].astype(np.int64)
                n = int(P[y0 + T, x0 + T] - P[y0, x0 + T] - P[y0 + T, x0] + P[y0, x0])
            if n <= max_invalid:
                break
        else:
            a |= 1 << 23                                                          # exhausted: bit 31 of the word after << 8
        out[b] = (s, y0, x0, view | (a << 8))
    return out


def view_index(g, T):
    """(i', j') as [T][T] index arrays of a T x T window: view_g(x) = x[i', j'] (the rule of nirgan_tile_views_expand)"""
    i, j = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    a, b = (j, i) if g & 4 else (i, j)
    return (T - 1 - a if g & 2 else a), (T - 1 - b if g & 1 else b)


def cut(scene, bands, y0, x0, T, view, divisor):
    """float32 [4][T][T]: the window of the four selected planes, turned and divided"""
    win = scene[list(bands), y0:y0 + T, x0:x0 + T]
    ii, jj = view_index(view, T)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (win[:, ii, jj].astype(f32) / f32(divisor)).astype(f32)


def centre(geo, y0, x0, T):
    """float32 (lon, lat) of the centre of the centre pixel; geo = (lon0, dlon, lat0, dlat) as float64"""
    lon0, dlon, lat0, dlat = (np.float64(v) for v in geo)
    cx, cy = np.float64(x0 + T // 2) + np.float64(0.5), np.float64(y0 + T // 2) + np.float64(0.5)
    return f32(lon0 + cx * dlon), f32(lat0 + cy * dlat)


def _pool(ptr, n, dtype):
    ct = C.c_uint16 if dtype == 0 else C.c_float
    return np.ctypeslib.as_array((ct * int(n)).from_address(int(ptr)))


def _i64(ptr, n):
    return np.ctypeslib.as_array((C.c_int64 * int(n)).from_address(int(ptr)))


class EmuScenePool(EmuClassMetrics):
    def nirgan_scene_invalid_prefix(self, ref, stream=None):
        who = "scene_invalid_prefix"
        self.calls.append(who)
        if not ref:
            return self._fail(f"{who}: null pointer")
        d = obj(ref)
        if not d.pool or not d.prefix:
            return self._fail(f"{who}: null pointer")
        if d.dtype not in (0, 1):
            return self._fail(f"{who}: unknown dtype")
        if d.C <= 0 or d.H <= 0 or d.W <= 0:
            return self._fail(f"{who}: bad shape")
        if (d.H + 1) * (d.W + 1) >= 2 ** 31:
            return self._fail(f"{who}: the table (H+1)(W+1) is 2^31 or more")
        if any(not 0 <= b < d.C for b in d.band):
            return self._fail(f"{who}: band outside 0 .. C-1")
        if d.offset < 0 or d.pool_elems < 0 or d.offset + d.C * d.H * d.W > d.pool_elems:
            return self._fail(f"{who}: the scene lies outside the pool")
        if d.dtype == 0 and not 0 <= d.nodata <= 65535:
            return self._fail(f"{who}: nodata outside 0 .. 65535")
        scene = _pool(d.pool, d.pool_elems, d.dtype)[d.offset:d.offset + d.C * d.H * d.W].reshape(d.C, d.H, d.W)
        out = arr(d.prefix, (d.H + 1) * (d.W + 1), np.int32).reshape(d.H + 1, d.W + 1)
        out[...] = prefix_table(invalid_mask(scene[list(d.band)], d.nodata))
        return 0

    def nirgan_scene_sample(self, ref, stream=None):
        who = "scene_sample"
        self.calls.append(who)
        if not ref:
            return self._fail(f"{who}: null pointer")
        d = obj(ref)
        if not (d.pool and d.table and d.table_host and d.rgb and d.nir and d.window):
            return self._fail(f"{who}: null pointer")
        if d.dtype not in (0, 1):
            return self._fail(f"{who}: unknown dtype")
        if d.S <= 0 or d.C < 4:
            return self._fail(f"{who}: bad pool (C must be at least 4)")
        if d.views not in (1, 4, 8):
            return self._fail(f"{who}: views {d.views} is not 1, 4 or 8")
        if any(not 0 <= b < d.C for b in d.band):
            return self._fail(f"{who}: band outside 0 .. C-1")
        T, B = d.tile, d.B
        if B <= 0 or T <= 0 or T * T >= 2 ** 31 or B * T * T >= 2 ** 31:
            return self._fail(f"{who}: B, tile or B*tile*tile is not in 1 .. 2^31-1")
        if d.divisor == 0 or d.divisor != d.divisor:
            return self._fail(f"{who}: divisor is 0 or NaN")
        if d.max_invalid < 0:
            return self._fail(f"{who}: negative max_invalid")
        if d.pool_elems < 0 or d.prefix_elems < 0:
            return self._fail(f"{who}: negative pool_elems or prefix_elems")
        host = [[int(v) for v in row] for row in _i64(d.table_host, d.S * COLS).reshape(d.S, COLS)]
        total = 0
        for s, (off, H, W, cum, poff) in enumerate(host):
            if not (0 < H < 2 ** 31 and 0 < W < 2 ** 31):
                return self._fail(f"{who}: scene {s} has an extent outside 1 .. 2^31-1")
            if H >= T and W >= T:
                total += (H - T + 1) * (W - T + 1)
            if total >= 2 ** 62:
                return self._fail(f"{who}: the pool has 2^62 windows or more")
            if cum != total:
                return self._fail(f"{who}: cum_windows of scene {s} is not the running window count for tile {T}")
        if total == 0:
            return self._fail(f"{who}: no scene holds a window of tile {T}")
        for s, (off, H, W, cum, poff) in enumerate(host):
            if off < 0 or off + d.C * H * W > d.pool_elems:
                return self._fail(f"{who}: scene {s} lies outside the pool")
            if poff >= 0:
                if not d.prefix:
                    return self._fail(f"{who}: scene {s} names a prefix table but prefix is null")
                if poff + (H + 1) * (W + 1) > d.prefix_elems:
                    return self._fail(f"{who}: the prefix table of scene {s} lies outside prefix_elems")
        table = [[int(v) for v in row] for row in _i64(d.table, d.S * COLS).reshape(d.S, COLS)]     # the "device" copy
        pool = _pool(d.pool, d.pool_elems, d.dtype)
        shapes = [(r[1], r[2]) for r in table]
        prefixes = None
        if d.prefix:
            allp = arr(d.prefix, d.prefix_elems, np.int32)
            prefixes = [allp[r[4]:r[4] + (r[1] + 1) * (r[2] + 1)].reshape(r[1] + 1, r[2] + 1) if r[4] >= 0 else None for r in table]
        win = draw_windows(shapes, T, B, d.views, (d.seed_lo, d.seed_hi), int(d.draw), int(d.sample0), prefixes, d.max_invalid)
        arr(d.window, B * 4, np.int32).reshape(B, 4)[...] = win.astype(np.uint32).view(np.int32).reshape(B, 4)
        rgb, nir = arr(d.rgb, B * 3 * T * T).reshape(B, 3, T, T), arr(d.nir, B * T * T).reshape(B, 1, T, T)
        geo = arr(d.geo, d.S * 4, np.float64).reshape(d.S, 4) if d.geo else None
        coords = arr(d.coords, B * 2).reshape(B, 2) if (d.coords and geo is not None) else None
        for b, (s, y0, x0, word) in enumerate(win.tolist()):
            off, H, W = table[s][:3]
            scene = pool[off:off + d.C * H * W].reshape(d.C, H, W)
            out = cut(scene, d.band, y0, x0, T, word & 7, d.divisor)
            rgb[b], nir[b, 0] = out[:3], out[3]
            if coords is not None:
                coords[b] = centre(geo[s], y0, x0, T)
        return 0
