"""numpy / Python-int statement of the scene-pool entries of include/nirgan_hip.h (nirgan_scene_invalid_prefix / nirgan_scene_sample)
-- TEST INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend`` like tests/emu_backend.py; it extends
tests/emu_class_metrics.py (the end of the emulator chain), so one backend serves ``fit`` on a pool's loader for every model.

Written from the header alone: Philox4x32-10 from tests/emu_dropout.py, the window index as the high word of a Python-int product,
``bisect`` for the scene, ``np.cumsum`` for the prefix table, index arrays for the views, ``np.float32(v) / np.float32(divisor)`` for
the values and float64 for the coords.  ``draw_windows`` / ``cut`` / ``centre`` are what the test bodies compare the device with.

What the later scene entries (tests/emu_scene_scale.py, emu_scene_grid.py, emu_scene_split.py) share with this one is stated once,
here: ``entry`` (an emulated entry refuses by raising ``Refused``), the opening checks ``check_common``, the table checks
``check_sides`` / ``check_cum`` / ``check_extents``, the attempt loop ``draw_rows`` and the delivery loop ``deliver``.
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


def draw_rows(B, views, seed, draw, sample0, prefixes, scale_of):
    """The attempt loop of every draw.  ``scale_of(b)`` = (side, total, most, bits, origin): sample b draws among ``total`` windows of
    side ``side``, ``origin(idx)`` = (s, y0, x0, tag) names window ``idx`` of them, at most ``most`` invalid pixels are accepted and
    ``bits`` go into the word.  -> (int64 [B][4] rows of non-negative Python values, the tag of each window taken)"""
    lo, hi = seed if isinstance(seed, (tuple, list)) else (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    samples = (np.arange(B, dtype=np.uint64) + np.uint64(sample0 & 0xFFFFFFFF))[:, None]
    words = philox4x32_10((draw & 0xFFFFFFFF, (draw >> 32) & 0xFFFFFFFF, samples, np.arange(ATTEMPTS, dtype=np.uint64)[None, :]), (lo, hi))
    words = np.stack(words, axis=-1).tolist()                                    # [B][ATTEMPTS][4] Python ints
    out, tags = np.zeros((B, 4), dtype=np.int64), []
    for b in range(B):
        side, total, most, bits, origin = scale_of(b)
        for a in range(ATTEMPTS):
            w = words[b][a]
            s, y0, x0, tag = origin(((w[0] | (w[1] << 32)) * total) >> 64)
            view = w[2] & (views - 1)
            n = 0
            if prefixes is not None and prefixes[s] is not None:
                P = prefixes[s]
                n = int(P[y0 + side][x0 + side]) - int(P[y0][x0 + side]) - int(P[y0 + side][x0]) + int(P[y0][x0])
            if n <= most:
                break
        else:
            a |= 1 << 23                                                          # exhausted: bit 31 of the word after << 8
        out[b] = (s, y0, x0, view | (a << 8) | bits)
        tags.append(tag)
    return out, tags


def draw_windows(shapes, T, B, views, seed, draw, sample0=0, prefixes=None, max_invalid=0):
    """int64 [B][4] = (scene, y0, x0, view | attempt << 8 | exhausted << 31) -- as a non-negative Python value, compare with the
    device's int32 word after ``& 0xFFFFFFFF``.  shapes: [(H, W)]; prefixes: per scene an [(H+1)][(W+1)] table or None."""
    cum = window_counts(shapes, T)
    assert cum[-1] > 0

    def origin(idx):
        s = bisect.bisect_right(cum, idx)                                        # the first scene with cum > idx
        r = idx - (cum[s - 1] if s else 0)
        nx = shapes[s][1] - T + 1
        return s, r // nx, r % nx, None
    return draw_rows(B, views, seed, draw, sample0, prefixes, lambda b: (T, cum[-1], max_invalid, 0, origin))[0]


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


class Refused(Exception):
    """an argument error of an emulated entry; ``entry`` turns it into the library's failure"""


def need(ok, msg):
    if not ok:
        raise Refused(msg)


def entry(who):
    """an emulated entry from ``body(self, d)``: the call is logged, a null descriptor and every ``Refused`` fail as ``who: message``"""
    def wrap(body):
        def call(self, ref, stream=None):
            self.calls.append(who)
            try:
                need(ref, "null pointer")
                body(self, obj(ref))
            except Refused as e:
                return self._fail(f"{who}: {e}")
            return 0
        return call
    return wrap


def check_common(d, own_ptrs=(), n="B"):
    """the checks every entry opens with -> (T, n); an entry of ``n`` rows instead of ``B`` samples has no views, max_invalid or
    prefix_elems and places its rows inside its list here"""
    need(all(getattr(d, p) for p in ("pool", "table", "table_host", "rgb", "nir", "window") + own_ptrs), "null pointer")
    need(d.dtype in (0, 1), "unknown dtype")
    need(d.S > 0 and d.C >= 4, "bad pool (C must be at least 4)")
    need(n != "B" or d.views in (1, 4, 8), f"views {getattr(d, 'views', None)} is not 1, 4 or 8")
    need(all(0 <= b < d.C for b in d.band), "band outside 0 .. C-1")
    T, N = int(d.tile), int(getattr(d, n))
    need(N > 0 and T > 0 and T * T < 2 ** 31 and N * T * T < 2 ** 31, f"{n}, tile or {n}*tile*tile is not in 1 .. 2^31-1")
    if n != "B":
        need(0 <= d.first <= d.n_windows - N, f"first {d.first}, n {N}: the rows are not inside 0 .. n_windows-1")
    need(d.divisor != 0 and d.divisor == d.divisor, "divisor is 0 or NaN")
    if n == "B":
        need(d.max_invalid >= 0, "negative max_invalid")
        need(d.pool_elems >= 0 and d.prefix_elems >= 0, "negative pool_elems or prefix_elems")
    return T, N


def table_rows(ptr, S, k=0):
    """table k of [..][S][COLS] tables as lists of Python ints"""
    return [[int(v) for v in row] for row in _i64(ptr, (k + 1) * S * COLS)[k * S * COLS:].reshape(S, COLS)]


def check_sides(rows, scenes=None):
    for s in (range(len(rows)) if scenes is None else scenes):
        need(0 < rows[s][1] < 2 ** 31 and 0 < rows[s][2] < 2 ** 31, f"scene {s} has an extent outside 1 .. 2^31-1")


def check_cum(rows, side):
    """the checks of one host table for windows of ``side`` -> its total"""
    total = 0
    for s, (off, H, W, cum, poff) in enumerate(rows):
        check_sides(rows, [s])
        if H >= side and W >= side:
            total += (H - side + 1) * (W - side + 1)
        need(total < 2 ** 62, "the pool has 2^62 windows or more")
        need(cum == total, f"cum_windows of scene {s} is not the running window count for tile {side}")
    return total


def check_extents(d, rows, with_prefix=True):
    for s, (off, H, W, cum, poff) in enumerate(rows):
        need(off >= 0 and off + d.C * H * W <= d.pool_elems, f"scene {s} lies outside the pool")
        if with_prefix and poff >= 0:
            need(d.prefix, f"scene {s} names a prefix table but prefix is null")
            need(poff + (H + 1) * (W + 1) <= d.prefix_elems, f"the prefix table of scene {s} lies outside prefix_elems")


def prefixes_of(d, table):
    """per scene of the device table its prefix table or None; None without ``prefix``"""
    if not d.prefix:
        return None
    allp = arr(d.prefix, d.prefix_elems, np.int32)
    return [allp[r[4]:r[4] + (r[1] + 1) * (r[2] + 1)].reshape(r[1] + 1, r[2] + 1) if r[4] >= 0 else None for r in table]


def deliver(d, table, rows, cutter):
    """rgb, nir and coords of the window rows (s, y0, x0, word) from the scenes of the device table; ``cutter(scene, bands, y0, x0, T,
    f, view, divisor)`` -> float32 [4][T][T]"""
    T, n = d.tile, len(rows)
    pool = _pool(d.pool, d.pool_elems, d.dtype)
    rgb, nir = arr(d.rgb, n * 3 * T * T).reshape(n, 3, T, T), arr(d.nir, n * T * T).reshape(n, 1, T, T)
    geo = arr(d.geo, d.S * 4, np.float64).reshape(d.S, 4) if d.geo else None
    coords = arr(d.coords, n * 2).reshape(n, 2) if (d.coords and geo is not None) else None
    for i, (s, y0, x0, word) in enumerate(rows):
        off, H, W = table[s][:3]
        f = (((word & 0xFFFFFFFF) >> 16) & 7) + 1
        out = cutter(pool[off:off + d.C * H * W].reshape(d.C, H, W), d.band, y0, x0, T, f, word & 7, d.divisor)
        rgb[i], nir[i, 0] = out[:3], out[3]
        if coords is not None:
            coords[i] = centre(geo[s], y0, x0, f * T)


def deliver_drawn(d, table, win, cutter):
    """the window words of a draw ``win`` (int64 [B][4]) and their batch"""
    arr(d.window, d.B * 4, np.int32).reshape(d.B, 4)[...] = win.astype(np.uint32).view(np.int32).reshape(d.B, 4)
    deliver(d, table, win.tolist(), cutter)


class EmuScenePool(EmuClassMetrics):
    @entry("scene_invalid_prefix")
    def nirgan_scene_invalid_prefix(self, d):
        need(d.pool and d.prefix, "null pointer")
        need(d.dtype in (0, 1), "unknown dtype")
        need(d.C > 0 and d.H > 0 and d.W > 0, "bad shape")
        need((d.H + 1) * (d.W + 1) < 2 ** 31, "the table (H+1)(W+1) is 2^31 or more")
        need(all(0 <= b < d.C for b in d.band), "band outside 0 .. C-1")
        need(d.offset >= 0 and d.pool_elems >= 0 and d.offset + d.C * d.H * d.W <= d.pool_elems, "the scene lies outside the pool")
        need(d.dtype != 0 or 0 <= d.nodata <= 65535, "nodata outside 0 .. 65535")
        scene = _pool(d.pool, d.pool_elems, d.dtype)[d.offset:d.offset + d.C * d.H * d.W].reshape(d.C, d.H, d.W)
        out = arr(d.prefix, (d.H + 1) * (d.W + 1), np.int32).reshape(d.H + 1, d.W + 1)
        out[...] = prefix_table(invalid_mask(scene[list(d.band)], d.nodata))

    @entry("scene_sample")
    def nirgan_scene_sample(self, d):
        T, B = check_common(d)
        host = table_rows(d.table_host, d.S)
        need(check_cum(host, T) > 0, f"no scene holds a window of tile {T}")
        check_extents(d, host)
        table = table_rows(d.table, d.S)                                         # the "device" copy
        win = draw_windows([(r[1], r[2]) for r in table], T, B, d.views, (d.seed_lo, d.seed_hi), int(d.draw), int(d.sample0),
                           prefixes_of(d, table), d.max_invalid)
        deliver_drawn(d, table, win, lambda scene, bands, y0, x0, T, f, view, divisor: cut(scene, bands, y0, x0, T, view, divisor))
