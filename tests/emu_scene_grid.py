"""numpy / Python-int statement of nirgan_scene_gather (include/nirgan_hip.h, the section after the multi-scale one) -- TEST
INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend``; it extends tests/emu_scene_scale.py and is now the end of the
emulator chain.

Written from the header alone.  The header says the pixels ARE the gather of nirgan_scene_sample_scaled and the coords those of
nirgan_scene_sample, so ``cut_scaled`` and ``centre`` of the existing restatements are called, not copied; the argument checks are
restated here.  ``grid_rows`` is the plain double loop the grid of ``ScenePool.grid`` is compared with.
"""
import numpy as np

from emu_backend import arr, obj
from emu_scene_pool import COLS, _i64, _pool, centre
from emu_scene_scale import EmuSceneScale, cut_scaled

WORD_BITS = 0x8007FF07                                                           # view, attempt, factor - 1, exhausted


def split_word(word):
    """(view, factor) of a window word given as any Python int or int32"""
    word = int(word) & 0xFFFFFFFF
    return word & 7, ((word >> 16) & 7) + 1


def starts(extent, side, stride, cover):
    """0, stride, 2 * stride, ... <= extent - side; with ``cover`` extent - side is appended if it is not the last"""
    out, p = [], 0
    while p <= extent - side:
        out.append(p)
        p += stride
    if cover and out[-1] != extent - side:
        out.append(extent - side)
    return out


def grid_rows(shapes, tile, factors=(1,), stride=None, max_invalid=0, cover=True, scenes=None, prefixes=None):
    """(kept, rejected): two lists of (s, y0, x0, word) in the order factor, scene, row, column -- Python ints throughout;
    prefixes: per scene an [(H+1)][(W+1)] table (``emu_scene_pool.prefix_table``) or None"""
    kept, rejected = [], []
    for f in sorted(factors):
        side = f * tile
        step = side if stride is None else stride
        for s in (range(len(shapes)) if scenes is None else scenes):
            H, W = shapes[s]
            if H < side or W < side:
                continue
            for y0 in starts(H, side, step, cover):
                for x0 in starts(W, side, step, cover):
                    n = 0
                    if prefixes is not None and prefixes[s] is not None:
                        P = prefixes[s]
                        n = int(P[y0 + side][x0 + side]) - int(P[y0][x0 + side]) - int(P[y0 + side][x0]) + int(P[y0][x0])
                    (kept if n <= max_invalid * f * f else rejected).append((s, y0, x0, (f - 1) << 16))
    return kept, rejected


class EmuSceneGrid(EmuSceneScale):
    def nirgan_scene_gather(self, ref, stream=None):
        who = "scene_gather"
        self.calls.append(who)
        if not ref:
            return self._fail(f"{who}: null pointer")
        d = obj(ref)
        if not (d.pool and d.table and d.table_host and d.window and d.window_host and d.rgb and d.nir):
            return self._fail(f"{who}: null pointer")
        if d.dtype not in (0, 1):
            return self._fail(f"{who}: unknown dtype")
        if d.S <= 0 or d.C < 4:
            return self._fail(f"{who}: bad pool (C must be at least 4)")
        if any(not 0 <= b < d.C for b in d.band):
            return self._fail(f"{who}: band outside 0 .. C-1")
        T, n, first = int(d.tile), int(d.n), int(d.first)
        if n <= 0 or T <= 0 or T * T >= 2 ** 31 or n * T * T >= 2 ** 31:
            return self._fail(f"{who}: n, tile or n*tile*tile is not in 1 .. 2^31-1")
        if first < 0 or first + n > d.n_windows:
            return self._fail(f"{who}: first {first}, n {n}: the rows are not inside 0 .. n_windows-1")
        if d.divisor == 0 or d.divisor != d.divisor:
            return self._fail(f"{who}: divisor is 0 or NaN")
        host = [[int(v) for v in row] for row in _i64(d.table_host, d.S * COLS).reshape(d.S, COLS)]
        for s, (off, H, W, _, _) in enumerate(host):
            if not (0 < H < 2 ** 31 and 0 < W < 2 ** 31):
                return self._fail(f"{who}: scene {s} has an extent outside 1 .. 2^31-1")
        for s, (off, H, W, _, _) in enumerate(host):
            if off < 0 or off + d.C * H * W > d.pool_elems:
                return self._fail(f"{who}: scene {s} lies outside the pool")
        rows_host = arr(d.window_host, d.n_windows * 4, np.int32).reshape(-1, 4)[first:first + n].tolist()
        for i, (s, y0, x0, word) in enumerate(rows_host, start=first):
            if (word & 0xFFFFFFFF) & ~WORD_BITS:
                return self._fail(f"{who}: row {i}: the word has a bit set outside the view, attempt, factor and exhausted fields")
            if not 0 <= s < d.S:
                return self._fail(f"{who}: row {i}: scene {s} outside 0 .. S-1")
            side = split_word(word)[1] * T
            if side * side >= 2 ** 31:
                return self._fail(f"{who}: row {i}: the window, (factor*tile)^2, is 2^31 or more")
            if y0 < 0 or x0 < 0 or y0 + side > host[s][1] or x0 + side > host[s][2]:
                return self._fail(f"{who}: row {i}: the window of side {side} at ({y0}, {x0}) is not inside scene {s}")
        table = [[int(v) for v in row] for row in _i64(d.table, d.S * COLS).reshape(d.S, COLS)]      # the "device" copies
        rows = arr(d.window, d.n_windows * 4, np.int32).reshape(-1, 4)[first:first + n].tolist()
        assert [r[:3] for r in table] == [r[:3] for r in host] and rows == rows_host
        pool = _pool(d.pool, d.pool_elems, d.dtype)
        rgb, nir = arr(d.rgb, n * 3 * T * T).reshape(n, 3, T, T), arr(d.nir, n * T * T).reshape(n, 1, T, T)
        geo = arr(d.geo, d.S * 4, np.float64).reshape(d.S, 4) if d.geo else None
        coords = arr(d.coords, n * 2).reshape(n, 2) if (d.coords and geo is not None) else None
        for i, (s, y0, x0, word) in enumerate(rows):
            off, H, W = table[s][:3]
            view, f = split_word(word)
            scene = pool[off:off + d.C * H * W].reshape(d.C, H, W)
            out = cut_scaled(scene, d.band, y0, x0, T, f, view, d.divisor)
            rgb[i], nir[i, 0] = out[:3], out[3]
            if coords is not None:
                coords[i] = centre(geo[s], y0, x0, f * T)
        return 0
