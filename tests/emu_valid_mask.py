"""numpy / torch statement of the valid-mask entries of include/nirgan_hip.h (nirgan_scene_valid / nirgan_valid_count, the last
section; nirgan_pix_loss_masked, after nirgan_pix_loss) -- TEST INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend``; it
extends tests/emu_scene_predict.py and is now the end of the emulator chain.

Written from the header alone.  The mask: the prefix table sliced at the block corners with index arrays, int64 differences, ``== 0``,
the view as index arrays (``view_index`` of tests/emu_scene_pool.py).  ``mask_of_row`` / ``masks_of_rows`` are what the test bodies
compare the device with.  The count: ``np.count_nonzero``.  The masked loss: fp32 torch of the header's formulas, every per-pixel
term selected with ``torch.where`` before it is summed and the inputs of a dropped pixel replaced before any arithmetic sees them --
with a mask of ones the terms, their order and the divisor are those of ``EmuBackend._pix_loss``, so the two agree bitwise, as the
header promises of the device.
"""
import ctypes as C

import numpy as np
import torch

from emu_backend import arr, obj
from emu_scene_grid import WORD_BITS, split_word
from emu_scene_pool import check_sides, entry, need, table_rows, view_index
from emu_scene_predict import EmuScenePredict

f32 = np.float32


def mask_of_row(P, shape, row, T):
    """float32 [T][T] of one window row (s, y0, x0, word) on the scene of ``shape`` = (H, W) with prefix table ``P`` (None: no
    table): zeros where the window does not lie inside the scene, ones without a table"""
    _, y0, x0, word = (int(v) for v in row)
    view, f = split_word(word)
    L, (H, W) = f * T, shape
    if y0 < 0 or x0 < 0 or y0 + L > H or x0 + L > W:
        return np.zeros((T, T), f32)
    if P is None:
        return np.ones((T, T), f32)
    ys, xs = y0 + f * np.arange(T + 1), x0 + f * np.arange(T + 1)
    Q = np.asarray(P)[np.ix_(ys, xs)].astype(np.int64)
    D = ((Q[1:, 1:] - Q[:-1, 1:] - Q[1:, :-1] + Q[:-1, :-1]) == 0).astype(f32)
    ii, jj = view_index(view, T)
    return D[ii, jj]


def masks_of_rows(shapes, prefixes, rows, T):
    """float32 [n][1][T][T]; ``prefixes``: per scene a table or None, or None for a pool without tables; a row whose scene is
    outside 0 .. S-1 gives zeros"""
    out = np.zeros((len(rows), 1, T, T), f32)
    for i, row in enumerate(rows):
        s = int(row[0])
        if 0 <= s < len(shapes):
            out[i, 0] = mask_of_row(prefixes[s] if prefixes is not None else None, shapes[s], row, T)
    return out


def _i32(ptr, n):
    return np.ctypeslib.as_array((C.c_int32 * int(n)).from_address(int(ptr)))


class EmuValidMask(EmuScenePredict):
    @entry("scene_valid")
    def nirgan_scene_valid(self, d):
        need(d.table and d.table_host and d.window and d.valid, "null pointer")
        need(d.S > 0, "bad pool")
        T, n, first = int(d.tile), int(d.n), int(d.first)
        need(n > 0 and T > 0 and T * T < 2 ** 31 and n * T * T < 2 ** 31, "n, tile or n*tile*tile is not in 1 .. 2^31-1")
        need(0 <= first <= d.n_windows - n, f"first {first}, n {n}: the rows are not inside 0 .. n_windows-1")
        need(d.prefix_elems >= 0, "negative prefix_elems")
        host = table_rows(d.table_host, d.S)
        check_sides(host)
        if d.prefix:
            for s, (off, H, W, cum, poff) in enumerate(host):
                need(poff < 0 or poff + (H + 1) * (W + 1) <= d.prefix_elems, f"the prefix table of scene {s} lies outside prefix_elems")
        if d.window_host:
            rows_host = _i32(d.window_host, d.n_windows * 4).reshape(-1, 4)[first:first + n].tolist()
            for i, (s, y0, x0, word) in enumerate(rows_host, start=first):
                need(not (word & 0xFFFFFFFF) & ~WORD_BITS, f"row {i}: the word has a bit set outside the view, attempt, factor and exhausted fields")
                need(0 <= s < d.S, f"row {i}: scene {s} outside 0 .. S-1")
                side = split_word(word)[1] * T
                need(side * side < 2 ** 31, f"row {i}: the window, (factor*tile)^2, is 2^31 or more")
                need(y0 >= 0 and x0 >= 0 and y0 + side <= host[s][1] and x0 + side <= host[s][2],
                     f"row {i}: the window of side {side} at ({y0}, {x0}) is not inside scene {s}")
        table = table_rows(d.table, d.S)                                         # the "device" copies
        rows = _i32(d.window, d.n_windows * 4).reshape(-1, 4)[first:first + n].tolist()
        prefixes = None
        if d.prefix:
            allp = arr(d.prefix, d.prefix_elems, np.int32)
            prefixes = [allp[r[4]:r[4] + (r[1] + 1) * (r[2] + 1)].reshape(r[1] + 1, r[2] + 1) if r[4] >= 0 else None for r in table]
        arr(d.valid, n * T * T).reshape(n, 1, T, T)[...] = masks_of_rows([(r[1], r[2]) for r in table], prefixes, rows, T)

    def nirgan_valid_count(self, valid, n, count, stream=None):
        self.calls.append("valid_count")
        if not valid or not count:
            return self._fail("valid_count: null pointer")
        if not 0 < n < 2 ** 31:
            return self._fail(f"valid_count: n {n} is not in 1 .. 2^31-1")
        _i32(count, 1)[0] = int(np.count_nonzero(arr(valid, n)))                 # -0.0 == 0: not counted
        return 0

    def nirgan_pix_loss_masked(self, ref, stream=None):
        self.calls.append("pix_loss_masked")
        if not ref:
            return self._fail("pix_loss_masked: null pointer")
        with torch.enable_grad():
            return self._pix_loss_masked(obj(ref))

    def _pix_loss_masked(self, d):
        if not (d.nir and d.pred and d.sums):
            return self._fail("pix_loss_masked: null pointer")
        if not (d.valid and d.count):
            return self._fail("pix_loss_masked: null valid or count")
        w = [d.w_l1, d.w_ndvi, d.w_ndwi, d.w_gndvi, d.w_savi, d.w_msavi, d.w_evi]
        if not d.rgb and (d.log_all or any(v != 0 for v in w[1:])):
            return self._fail("pix_loss_masked: the spectral indices need rgb")
        if d.B <= 0 or d.H <= 0 or d.W <= 0:
            return self._fail("pix_loss_masked: bad shape")
        if d.criterion not in (0, 1):
            return self._fail("pix_loss_masked: criterion must be 0 (l1) or 1 (l2)")
        if d.extra and not 0 <= d.extra_c < d.extra_cs:
            return self._fail("pix_loss_masked: extra channel out of range")
        if not d.ws or d.ws_elems < 8192:
            return self._fail("pix_loss_masked: workspace of NIRGAN_PIX_LOSS_WS_ELEMS floats required (block partial sums)")
        B, H, W = d.B, d.H, d.W
        n = B * H * W
        keep = torch.from_numpy(arr(d.valid, n).reshape(B, 1, H, W) != 0)
        count = int(_i32(d.count, 1)[0])

        def kept(ptr, planes, benign):                                           # a dropped pixel's values are never used
            t = torch.from_numpy(arr(ptr, planes * n).reshape(B, planes, H, W).copy())
            return torch.where(keep, t, torch.tensor(benign, dtype=torch.float32))
        rgb = kept(d.rgb, 3, 0.1) if d.rgb else torch.zeros(B, 3, H, W)
        x = kept(d.nir, 1, 0.5)
        y = kept(d.pred, 1, 0.75).requires_grad_(True)
        R, Gc, Bl = rgb[:, 0:1], rgb[:, 1:2], rgb[:, 2:3]

        def idx(k, v):
            if k == 1:
                return (v - R) / (v + R + 1e-6)
            if k == 2:
                return (v - Gc) / (v + Gc + 1e-6)
            if k == 3:
                return (v - Gc) / ((v - R) / (v + R) + Gc)
            if k == 4:
                return 1.5 * (v - R) / (v + R + 0.5)
            if k == 5:
                return (2 * v + 1 - torch.sqrt((2 * v + 1) ** 2 - 8 * (v - R))) / 2
            return 2.5 * ((v - R) / ((v + 6) * (R - 7.5) * (Bl + 1) + 1e-6))

        def total_of(term):
            return torch.where(keep, term, torch.zeros(())).sum()
        crit = (lambda a, b: (a - b).abs()) if d.criterion == 0 else (lambda a, b: (a - b) ** 2)
        sums = arr(d.sums, 7)
        s0 = total_of((y - x).abs())
        sums[0] += float(s0.detach())
        total = 0.0
        total = total + w[0] * s0
        for k in range(1, 7):
            if d.log_all or w[k] != 0:
                sk = total_of(crit(idx(k, x), idx(k, y)))
                sums[k] += float(sk.detach())
                if w[k] != 0:
                    total = total + w[k] * sk
        if d.grad_pred:
            g = np.zeros(n, f32)
            if count > 0:
                (total / count).backward()
                g = np.where(keep.numpy().reshape(-1), y.grad.numpy().reshape(-1), f32(0.0)).astype(f32)
            if d.extra:
                g += d.extra_scale * arr(d.extra, n * d.extra_cs)[d.extra_c::d.extra_cs]
            arr(d.grad_pred, n)[:] = g
        return 0
