"""numpy / Python-int statement of nirgan_scene_sample_origins (include/nirgan_hip.h, the last section) -- TEST INFRASTRUCTURE ONLY,
installed with ``nirgan_hip.lib.set_backend``; it extends tests/emu_scene_grid.py and is now the end of the emulator chain.

Written from the header alone.  The scale of a sample is ``draw_factors`` of tests/emu_scene_scale.py (the header says the scale is
picked exactly as that entry picks it); the attempts are ``draw_rows`` of tests/emu_scene_pool.py with this entry's own step from the
index to the origin: ``bisect`` finds the row among the running sums of ONE scale, the window is the row's corner plus ``divmod`` of
the remainder; pixels and coords are ``cut_scaled`` / ``centre`` of
the existing restatements.  ``admissible_mask`` is the brute-force statement of which origins a hold-out leaves, the thing the slab
sweep of ``nirgan_hip.data.origin_rectangles`` is compared with.
"""
import bisect

import numpy as np

from emu_scene_grid import EmuSceneGrid
from emu_scene_pool import (_i64, check_common, check_extents, check_sides, deliver_drawn, draw_rows, entry, need, prefixes_of,
                            table_rows)
from emu_scene_scale import check_scales, cut_scaled, draw_factors

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
    fs = draw_factors(B, seed, draw, factors, weights, sample0)
    cums = [[int(r[5]) for r in rows] for rows in tables]

    def scale_of(b):
        f = fs[b]
        k = list(factors).index(f)
        rows, cum = tables[k], cums[k]

        def origin(idx):
            i = bisect.bisect_right(cum, idx)                                    # the first row of the scale with cum > idx
            r = idx - (cum[i - 1] if i else 0)
            s, oy, ox, oh, ow = (int(v) for v in rows[i][:5])
            return s, oy + r // ow, ox + r % ow, i
        return f * T, cum[-1], max_invalid * f * f, (f - 1) << 16, origin
    return draw_rows(B, views, seed, draw, sample0, prefixes, scale_of)


class EmuSceneSplit(EmuSceneGrid):
    @entry("scene_sample_origins")
    def nirgan_scene_sample_origins(self, d):
        T, B = check_common(d, ("origins", "origins_host"))
        factors, weights = check_scales(d, T)
        host = table_rows(d.table_host, d.S)
        check_sides(host)
        check_extents(d, host)
        need(d.R >= 1, f"R {d.R}: the origin table has no row")
        first, count = list(d.first)[:d.K], list(d.count)[:d.K]
        nxt = 0
        for k, f in enumerate(factors):
            need(count[k] >= 1, f"factor {f} owns no row of the origin table")
            need(first[k] == nxt and nxt + count[k] <= d.R, "first / count do not tile 0 .. R-1 in order")
            nxt += count[k]
        need(nxt == d.R, "first / count do not tile 0 .. R-1 in order")
        rows_host = [[int(v) for v in row] for row in _i64(d.origins_host, d.R * OCOLS).reshape(d.R, OCOLS)]
        for k, f in enumerate(factors):
            side, total = f * T, 0
            for i in range(first[k], first[k] + count[k]):
                s, oy, ox, oh, ow, cum = rows_host[i]
                need(0 <= s < d.S, f"row {i}: scene {s} outside 0 .. S-1")
                need(oh >= 1 and ow >= 1, f"row {i}: an extent below 1")
                need(oy >= 0 and ox >= 0, f"row {i}: a negative origin")
                need(oy + oh <= host[s][1] - side + 1 and ox + ow <= host[s][2] - side + 1, f"row {i}: windows of side {side} are not inside scene {s}")
                total += oh * ow
                need(total < 2 ** 62, f"factor {f} has 2^62 origins or more")
                need(cum == total, f"row {i}: cum is not the running sum of oh*ow of factor {f}")
        table = table_rows(d.table, d.S)                                         # the "device" copies
        rows = [[int(v) for v in row] for row in _i64(d.origins, d.R * OCOLS).reshape(d.R, OCOLS)]
        assert rows == rows_host and [r[:3] + r[4:] for r in table] == [r[:3] + r[4:] for r in host]
        tables = [rows[first[k]:first[k] + count[k]] for k in range(d.K)]
        win, _ = draw_origins(tables, T, B, d.views, (d.seed_lo, d.seed_hi), int(d.draw), factors, weights, int(d.sample0),
                              prefixes_of(d, table), d.max_invalid)
        deliver_drawn(d, table, win, cut_scaled)
