"""numpy / Python-int statement of nirgan_scene_sample_origins (include/nirgan_hip.h, the last section) -- TEST INFRASTRUCTURE ONLY,
installed with ``nirgan_hip.lib.set_backend``; it extends tests/emu_scene_grid.py and is now the end of the emulator chain.

Written from the header alone.  The scale of a sample is ``draw_factors`` of tests/emu_scene_scale.py (the header says the scale is
picked exactly as that entry picks it); the index is the high word of a Python-int product, ``bisect`` finds the row among the running
sums of ONE scale, the window is the row's corner plus ``divmod`` of the remainder; pixels and coords are ``cut_scaled`` / ``centre`` of
the existing restatements.  ``admissible_mask`` is the brute-force statement of which origins a hold-out leaves, the thing the slab
sweep of ``nirgan_hip.data.origin_rectangles`` is compared with.
"""
import bisect

import numpy as np

from emu_backend import arr, obj
from emu_dropout import philox4x32_10
from emu_scene_grid import EmuSceneGrid
from emu_scene_pool import ATTEMPTS, COLS, _i64, _pool, centre
from emu_scene_scale import MAX_FACTOR, MAX_SCALES, cut_scaled, draw_factors

OCOLS = 6


def admissible_mask(shape, side, held, guard=0):
    """bool [H-side+1][W-side+1] (or None if the scene holds no window): origin (y0, x0) is admissible iff its side x side window
    shares no pixel with any rectangle (y, x, h, w) of ``held`` widened by ``guard`` on every side -- pixel by pixel on a painted mask"""
    H, W = shape
    if H < side or W < side:
        return None
    g = guard
    paint = np.zeros((H + 2 * g, W + 2 * g), dtype=bool)                          # the scene with a margin of g, so widening needs no clipping
    for y, x, h, w in held:
        paint[y:y + h + 2 * g, x:x + w + 2 * g] = True                            # [y - g, y + h + g) shifted by g
    paint = paint[g:g + H, g:g + W]
    out = np.zeros((H - side + 1, W - side + 1), dtype=bool)
    for y0 in range(H - side + 1):
        for x0 in range(W - side + 1):
            out[y0, x0] = not paint[y0:y0 + side, x0:x0 + side].any()
    return out


def mask_of_rows(shape, side, rows):
    """(the origins the rectangles (oy, ox, oh, ow) cover as a bool mask, whether they are pairwise disjoint)"""
    H, W = shape
    hits = np.zeros((H - side + 1, W - side + 1), dtype=np.int64)
    for oy, ox, oh, ow in rows:
        assert oh >= 1 and ow >= 1 and oy >= 0 and ox >= 0 and oy + oh <= hits.shape[0] and ox + ow <= hits.shape[1]
        hits[oy:oy + oh, ox:ox + ow] += 1
    return hits > 0, int(hits.max(initial=0)) <= 1


def draw_origins(tables, T, B, views, seed, draw, factors, weights, sample0=0, prefixes=None, max_invalid=0):
    """(int64 [B][4] window rows as ``draw_scaled`` gives them, the row of its scale each sample was drawn from).
    tables: per scale the list of rows (scene, oy, ox, oh, ow, cum), cum running from the scale's first row;
    prefixes: per scene an [(H+1)][(W+1)] table or None"""
    lo, hi = seed if isinstance(seed, (tuple, list)) else (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    fs = draw_factors(B, seed, draw, factors, weights, sample0)
    samples = (np.arange(B, dtype=np.uint64) + np.uint64(sample0 & 0xFFFFFFFF))[:, None]
    words = philox4x32_10((draw & 0xFFFFFFFF, (draw >> 32) & 0xFFFFFFFF, samples, np.arange(ATTEMPTS, dtype=np.uint64)[None, :]), (lo, hi))
    words = np.stack(words, axis=-1).tolist()                                    # [B][ATTEMPTS][4] Python ints
    cums = [[int(r[5]) for r in rows] for rows in tables]
    out, which = np.zeros((B, 4), dtype=np.int64), []
    for b in range(B):
        f = fs[b]
        k = list(factors).index(f)
        rows, cum, side = tables[k], cums[k], f * T
        total = cum[-1]
        for a in range(ATTEMPTS):
            w = words[b][a]
            idx = ((w[0] | (w[1] << 32)) * total) >> 64
            i = bisect.bisect_right(cum, idx)                                    # the first row of the scale with cum > idx
            r = idx - (cum[i - 1] if i else 0)
            s, oy, ox, oh, ow = (int(v) for v in rows[i][:5])
            y0, x0 = oy + r // ow, ox + r % ow
            view = w[2] & (views - 1)
            n = 0
            if prefixes is not None and prefixes[s] is not None:
                P = prefixes[s]
                n = int(P[y0 + side][x0 + side]) - int(P[y0][x0 + side]) - int(P[y0 + side][x0]) + int(P[y0][x0])
            if n <= max_invalid * f * f:
                break
        else:
            a |= 1 << 23                                                          # exhausted: bit 31 of the word after << 8
        out[b] = (s, y0, x0, view | (a << 8) | ((f - 1) << 16))
        which.append(i)
    return out, which


class EmuSceneSplit(EmuSceneGrid):
    def nirgan_scene_sample_origins(self, ref, stream=None):
        who = "scene_sample_origins"
        self.calls.append(who)
        if not ref:
            return self._fail(f"{who}: null pointer")
        d = obj(ref)
        if not (d.pool and d.table and d.table_host and d.origins and d.origins_host and d.rgb and d.nir and d.window):
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
        host = [[int(v) for v in row] for row in _i64(d.table_host, d.S * COLS).reshape(d.S, COLS)]
        for s, (off, H, W, _, poff) in enumerate(host):
            if not (0 < H < 2 ** 31 and 0 < W < 2 ** 31):
                return self._fail(f"{who}: scene {s} has an extent outside 1 .. 2^31-1")
        for s, (off, H, W, _, poff) in enumerate(host):
            if off < 0 or off + d.C * H * W > d.pool_elems:
                return self._fail(f"{who}: scene {s} lies outside the pool")
            if poff >= 0:
                if not d.prefix:
                    return self._fail(f"{who}: scene {s} names a prefix table but prefix is null")
                if poff + (H + 1) * (W + 1) > d.prefix_elems:
                    return self._fail(f"{who}: the prefix table of scene {s} lies outside prefix_elems")
        if d.R < 1:
            return self._fail(f"{who}: R {d.R}: the origin table has no row")
        first, count = list(d.first)[:d.K], list(d.count)[:d.K]
        nxt = 0
        for k, f in enumerate(factors):
            if count[k] < 1:
                return self._fail(f"{who}: factor {f} owns no row of the origin table")
            if first[k] != nxt or nxt + count[k] > d.R:
                return self._fail(f"{who}: first / count do not tile 0 .. R-1 in order")
            nxt += count[k]
        if nxt != d.R:
            return self._fail(f"{who}: first / count do not tile 0 .. R-1 in order")
        rows_host = [[int(v) for v in row] for row in _i64(d.origins_host, d.R * OCOLS).reshape(d.R, OCOLS)]
        for k, f in enumerate(factors):
            side, total = f * T, 0
            for i in range(first[k], first[k] + count[k]):
                s, oy, ox, oh, ow, cum = rows_host[i]
                if not 0 <= s < d.S:
                    return self._fail(f"{who}: row {i}: scene {s} outside 0 .. S-1")
                if oh < 1 or ow < 1:
                    return self._fail(f"{who}: row {i}: an extent below 1")
                if oy < 0 or ox < 0:
                    return self._fail(f"{who}: row {i}: a negative origin")
                if oy + oh > host[s][1] - side + 1 or ox + ow > host[s][2] - side + 1:
                    return self._fail(f"{who}: row {i}: windows of side {side} are not inside scene {s}")
                total += oh * ow
                if total >= 2 ** 62:
                    return self._fail(f"{who}: factor {f} has 2^62 origins or more")
                if cum != total:
                    return self._fail(f"{who}: row {i}: cum is not the running sum of oh*ow of factor {f}")
        table = [[int(v) for v in row] for row in _i64(d.table, d.S * COLS).reshape(d.S, COLS)]      # the "device" copies
        rows = [[int(v) for v in row] for row in _i64(d.origins, d.R * OCOLS).reshape(d.R, OCOLS)]
        assert rows == rows_host and [r[:3] + r[4:] for r in table] == [r[:3] + r[4:] for r in host]
        pool = _pool(d.pool, d.pool_elems, d.dtype)
        prefixes = None
        if d.prefix:
            allp = arr(d.prefix, d.prefix_elems, np.int32)
            prefixes = [allp[r[4]:r[4] + (r[1] + 1) * (r[2] + 1)].reshape(r[1] + 1, r[2] + 1) if r[4] >= 0 else None for r in table]
        tables = [rows[first[k]:first[k] + count[k]] for k in range(d.K)]
        win, _ = draw_origins(tables, T, B, d.views, (d.seed_lo, d.seed_hi), int(d.draw), factors, weights, int(d.sample0), prefixes, d.max_invalid)
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
