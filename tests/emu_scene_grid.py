"""numpy / Python-int statement of nirgan_scene_gather (include/nirgan_hip.h, the section after the multi-scale one) -- TEST
INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend``; it extends tests/emu_scene_scale.py and is now the end of the
emulator chain.

Written from the header alone.  The header says the pixels ARE the gather of nirgan_scene_sample_scaled and the coords those of
nirgan_scene_sample, so ``cut_scaled`` and ``centre`` of the existing restatements are called, not copied (``deliver`` of emu_scene_pool); the checks
of the rows are restated here.  ``grid_rows`` is the plain double loop the grid of ``ScenePool.grid`` is compared with.
"""
import numpy as np

from emu_backend import arr
from emu_scene_pool import check_common, check_extents, check_sides, deliver, entry, need, table_rows
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
    @entry("scene_gather")
    def nirgan_scene_gather(self, d):
        T, n = check_common(d, ("window_host",), n="n")
        first = int(d.first)
        host = table_rows(d.table_host, d.S)
        check_sides(host)
        check_extents(d, host, with_prefix=False)
        rows_host = arr(d.window_host, d.n_windows * 4, np.int32).reshape(-1, 4)[first:first + n].tolist()
        for i, (s, y0, x0, word) in enumerate(rows_host, start=first):
            need(not (word & 0xFFFFFFFF) & ~WORD_BITS, f"row {i}: the word has a bit set outside the view, attempt, factor and exhausted fields")
            need(0 <= s < d.S, f"row {i}: scene {s} outside 0 .. S-1")
            side = split_word(word)[1] * T
            need(side * side < 2 ** 31, f"row {i}: the window, (factor*tile)^2, is 2^31 or more")
            need(y0 >= 0 and x0 >= 0 and y0 + side <= host[s][1] and x0 + side <= host[s][2],
                 f"row {i}: the window of side {side} at ({y0}, {x0}) is not inside scene {s}")
        table = table_rows(d.table, d.S)                                         # the "device" copies
        rows = arr(d.window, d.n_windows * 4, np.int32).reshape(-1, 4)[first:first + n].tolist()
        assert [r[:3] for r in table] == [r[:3] for r in host] and rows == rows_host
        deliver(d, table, rows, cut_scaled)
