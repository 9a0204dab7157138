"""numpy / Python-int statement of nirgan_scene_sample_scaled (include/nirgan_hip.h, the multi-scale section) -- TEST INFRASTRUCTURE
ONLY, installed with ``nirgan_hip.lib.set_backend``; it extends tests/emu_scene_pool.py and is now the end of the emulator chain.

Written from the header alone.  The scale of a sample is the fourth Philox word of attempt 0 against the running weights in Python
ints; the window of a sample of factor f is what ``emu_scene_pool.draw_windows`` draws for the tile side f*T with f*f*max_invalid
allowed (the header says the attempts ARE that entry's, so its restatement is called, not copied); the block mean is an int64
``sum`` and ``np.float32(S) / np.float32(f*f)`` for uint16 and an explicit row-major chain of float64 additions for float32; views
and centre are ``view_index`` / ``centre`` of emu_scene_pool, the checks and the delivery loop its shared ones.  ``draw_scaled`` / ``block_mean`` / ``cut_scaled`` are what the test
bodies compare the device with.
"""
import numpy as np

from emu_dropout import philox4x32_10
from emu_scene_pool import (EmuScenePool, check_common, check_cum, check_extents, deliver_drawn, draw_windows, entry, need,
                            prefixes_of, table_rows, view_index, window_counts)

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


def check_scales(d, T):
    """K, the factors and the weights of a descriptor -> (factors, weights)"""
    need(1 <= d.K <= MAX_SCALES, f"K {d.K} outside 1 .. {MAX_SCALES}")
    factors, weights = list(d.factor)[:d.K], list(d.weight)[:d.K]
    for k, (f, w) in enumerate(zip(factors, weights)):
        need(1 <= f <= MAX_FACTOR, f"factor {f} outside 1 .. {MAX_FACTOR}")
        need(not k or f > factors[k - 1], f"the factors are not strictly increasing ({f} after {factors[k - 1]})")
        need(w != 0, f"the weight of factor {f} is 0")
        need(sum(weights[:k + 1]) < 2 ** 32, "the weights sum to 2^32 or more")
        need((f * T) ** 2 < 2 ** 31, f"the window of factor {f}, (factor*tile)^2, is 2^31 or more")
    return factors, weights


class EmuSceneScale(EmuScenePool):
    @entry("scene_sample_scaled")
    def nirgan_scene_sample_scaled(self, d):
        T, B = check_common(d)
        factors, weights = check_scales(d, T)
        for k, f in enumerate(factors):
            host = table_rows(d.table_host, d.S, k)
            need(check_cum(host, f * T) > 0, f"no scene holds a window of factor {f} (side {f * T})")
            check_extents(d, host)
        tables = [table_rows(d.table, d.S, k) for k in range(d.K)]                # the "device" copy
        for f, rows in zip(factors, tables):
            assert [r[3] for r in rows] == window_counts([(r[1], r[2]) for r in rows], f * T)
        table = tables[0]
        win = draw_scaled([(r[1], r[2]) for r in table], T, B, d.views, (d.seed_lo, d.seed_hi), int(d.draw), factors, weights,
                          int(d.sample0), prefixes_of(d, table), d.max_invalid)
        deliver_drawn(d, table, win, cut_scaled)
