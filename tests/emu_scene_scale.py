"""numpy / Python-int statement of nirgan_scene_sample_scaled (include/nirgan_hip.h, the multi-scale section) -- TEST INFRASTRUCTURE
ONLY, installed with ``nirgan_hip.lib.set_backend``; it extends tests/emu_scene_pool.py and is now the end of the emulator chain.

Written from the header alone.  The scale of a sample is the fourth Philox word of attempt 0 against the running weights in Python
ints; the window of a sample of factor f is what ``emu_scene_pool.draw_windows`` draws for the tile side f*T with f*f*max_invalid
allowed (the header says the attempts ARE that entry's, so its restatement is called, not copied); the block mean is an int64
``sum`` and ``np.float32(S) / np.float32(f*f)`` for uint16 and an explicit row-major chain of float64 additions for float32; views
and centre are ``view_index`` / ``centre`` of emu_scene_pool.  ``draw_scaled`` / ``block_mean`` / ``cut_scaled`` are what the test
bodies compare the device with.
"""
import numpy as np

from emu_backend import arr, obj
from emu_dropout import philox4x32_10
from emu_scene_pool import COLS, EmuScenePool, _i64, _pool, centre, draw_windows, view_index, window_counts

MAX_SCALES, MAX_FACTOR = 8, 8
f32 = np.float32


def draw_factors(B, seed, draw, factors, weights, sample0=0):
    """the factor of each of the B samples: the first k with cumweight[k] > floor(v3 * Wtot / 2^32), v3 from attempt 0"""
    lo, hi = seed if isinstance(seed, (tuple, list)) else (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    samples = np.arange(B, dtype=np.uint64) + np.uint64(sample0 & 0xFFFFFFFF)
    v3 = philox4x32_10((draw & 0xFFFFFFFF, (draw >> 32) & 0xFFFFFFFF, samples, 0), (lo, hi))[3].tolist()
    wtot = sum(int(w) for w in weights)
    out = []
    for v in v3:
        pick, run = (int(v) * wtot) >> 32, 0
        for f, w in zip(factors, weights):
            run += int(w)
            if run > pick:
                out.append(int(f))
                break
    return out


def draw_scaled(shapes, T, B, views, seed, draw, factors, weights, sample0=0, prefixes=None, max_invalid=0):
    """int64 [B][4] = (scene, y0, x0, view | attempt << 8 | (f - 1) << 16 | exhausted << 31), non-negative Python values as
    ``draw_windows`` gives them; y0, x0 in source pixels"""
    fs = draw_factors(B, seed, draw, factors, weights, sample0)
    out = np.zeros((B, 4), dtype=np.int64)
    for f in sorted(set(fs)):                                                     # the whole batch at this side, the rows of factor f kept
        win = draw_windows(shapes, f * T, B, views, seed, draw, sample0, prefixes, max_invalid * f * f)
        rows = [b for b in range(B) if fs[b] == f]
        out[rows] = win[rows]
        out[rows, 3] |= (f - 1) << 16
    return out


def block_mean(win, f):
    """[n][f*T][f*T] uint16 or float32 -> float32 [n][T][T] of the f x f block means, as the header rounds them"""
    n, L, _ = win.shape
    T = L // f
    if win.dtype == np.float32:
        with np.errstate(invalid="ignore", over="ignore"):
            s = None
            for rr in range(f):                                                   # row-major over the block, one float64 addition each
                for e in range(f):
                    v = win[:, rr::f, e::f].astype(np.float64)
                    s = v if s is None else s + v
            return (s / np.float64(f * f)).astype(f32)
    s = win.astype(np.int64).reshape(n, T, f, T, f).sum(axis=(2, 4))
    assert s.max(initial=0) < 2 ** 24
    return (s.astype(f32) / f32(f * f)).astype(f32)


def cut_scaled(scene, bands, y0, x0, T, f, view, divisor):
    """float32 [4][T][T]: the block means of the f*T window of the four selected planes, turned and divided"""
    L = f * T
    D = block_mean(scene[list(bands), y0:y0 + L, x0:x0 + L], f)
    ii, jj = view_index(view, T)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (D[:, ii, jj] / f32(divisor)).astype(f32)


class EmuSceneScale(EmuScenePool):
    def nirgan_scene_sample_scaled(self, ref, stream=None):
        who = "scene_sample_scaled"
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
        if not 1 <= d.K <= MAX_SCALES:
            return self._fail(f"{who}: K {d.K} outside 1 .. {MAX_SCALES}")
        factors, weights = list(d.factor)[:d.K], list(d.weight)[:d.K]
        for k, (f, w) in enumerate(zip(factors, weights)):
            if not 1 <= f <= MAX_FACTOR:
                return self._fail(f"{who}: factor {f} outside 1 .. {MAX_FACTOR}")
            if k and f <= factors[k - 1]:
                return self._fail(f"{who}: the factors are not strictly increasing ({f} after {factors[k - 1]})")
            if w == 0:
                return self._fail(f"{who}: the weight of factor {f} is 0")
            if sum(weights[:k + 1]) >= 2 ** 32:
                return self._fail(f"{who}: the weights sum to 2^32 or more")
            if (f * T) ** 2 >= 2 ** 31:
                return self._fail(f"{who}: the window of factor {f}, (factor*tile)^2, is 2^31 or more")
        host = np.array(_i64(d.table_host, d.K * d.S * COLS)).reshape(d.K, d.S, COLS).tolist()
        for f, rows in zip(factors, host):
            total, side = 0, f * T
            for s, (off, H, W, cum, poff) in enumerate(rows):
                if not (0 < H < 2 ** 31 and 0 < W < 2 ** 31):
                    return self._fail(f"{who}: scene {s} has an extent outside 1 .. 2^31-1")
                if H >= side and W >= side:
                    total += (H - side + 1) * (W - side + 1)
                if total >= 2 ** 62:
                    return self._fail(f"{who}: the pool has 2^62 windows or more")
                if cum != total:
                    return self._fail(f"{who}: cum_windows of scene {s} is not the running window count for tile {side}")
            if total == 0:
                return self._fail(f"{who}: no scene holds a window of factor {f} (side {side})")
            for s, (off, H, W, cum, poff) in enumerate(rows):
                if off < 0 or off + d.C * H * W > d.pool_elems:
                    return self._fail(f"{who}: scene {s} lies outside the pool")
                if poff >= 0:
                    if not d.prefix:
                        return self._fail(f"{who}: scene {s} names a prefix table but prefix is null")
                    if poff + (H + 1) * (W + 1) > d.prefix_elems:
                        return self._fail(f"{who}: the prefix table of scene {s} lies outside prefix_elems")
        tables = np.array(_i64(d.table, d.K * d.S * COLS)).reshape(d.K, d.S, COLS).tolist()         # the "device" copy
        for f, rows in zip(factors, tables):
            assert [r[3] for r in rows] == window_counts([(r[1], r[2]) for r in rows], f * T)
        table = tables[0]
        pool = _pool(d.pool, d.pool_elems, d.dtype)
        shapes = [(r[1], r[2]) for r in table]
        prefixes = None
        if d.prefix:
            allp = arr(d.prefix, d.prefix_elems, np.int32)
            prefixes = [allp[r[4]:r[4] + (r[1] + 1) * (r[2] + 1)].reshape(r[1] + 1, r[2] + 1) if r[4] >= 0 else None for r in table]
        win = draw_scaled(shapes, T, B, d.views, (d.seed_lo, d.seed_hi), int(d.draw), factors, weights, int(d.sample0), prefixes, d.max_invalid)
        arr(d.window, B * 4, np.int32).reshape(B, 4)[...] = win.astype(np.uint32).view(np.int32).reshape(B, 4)
        rgb, nir = arr(d.rgb, B * 3 * T * T).reshape(B, 3, T, T), arr(d.nir, B * T * T).reshape(B, 1, T, T)
        geo = arr(d.geo, d.S * 4, np.float64).reshape(d.S, 4) if d.geo else None
        coords = arr(d.coords, B * 2).reshape(B, 2) if (d.coords and geo is not None) else None
        for b, (s, y0, x0, word) in enumerate(win.tolist()):
            off, H, W = table[s][:3]
            f = ((word >> 16) & 7) + 1
            scene = pool[off:off + d.C * H * W].reshape(d.C, H, W)
            out = cut_scaled(scene, d.band, y0, x0, T, f, word & 7, d.divisor)
            rgb[b], nir[b, 0] = out[:3], out[3]
            if coords is not None:
                coords[b] = centre(geo[s], y0, x0, f * T)
        return 0

