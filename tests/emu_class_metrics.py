"""numpy statement of the land-cover-stratified metrics entries of include/nirgan_hip.h (nirgan_class_metrics / _ws_elems) -- TEST
INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend`` like tests/emu_baselines.py; it extends tests/emu_val_panel.py so
that one emulator serves a whole ``fit`` run.

Float32 arithmetic restated from the descriptor alone: the evaluation window is cut out of the stored planes and of the mask by
indexing, the SSIM map is that of the whole window (reflect at the window's border), each class takes the mean over its own pixels
(sums in float64, rounded once), the index formulas are those of csrc/losses.hip in L1 form.  Contract enforced (the header's): every
computed column of ``rows`` is OVERWRITTEN, the index columns stay untouched without rgb, a class without pixels has count 0 and NaN
in its other computed columns, the workspace must hold B x (32x32 blocks of the window) x classes x 8 floats, and the argument
checks come before any work.
"""
import ctypes as C

import numpy as np

from emu_backend import arr, obj
from emu_tile_metrics import index_terms, ssim_map, window_cut, window_error
from emu_val_panel import EmuValPanel

COLS, NV, TILE, CLASS_MAX = 8, 8, 32, 8
f32 = np.float32


def bytes_at(ptr, n):
    if hasattr(ptr, "value"):
        ptr = ptr.value
    return np.ctypeslib.as_array((C.c_uint8 * int(n)).from_address(int(ptr)))


class EmuClassMetrics(EmuValPanel):
    def nirgan_class_metrics_ws_elems(self, B, ch, cw, classes):
        if B <= 0 or ch <= 0 or cw <= 0 or classes < 1 or classes > CLASS_MAX:
            return 0
        return B * (-(-ch // TILE)) * (-(-cw // TILE)) * classes * NV

    def nirgan_class_metrics(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("class_metrics")
        err = window_error(d, "class_metrics", bool(d.mask))
        if err:
            return self._fail(err)
        if d.classes < 1 or d.classes > CLASS_MAX:
            return self._fail("class_metrics: classes must lie in 1..8")
        if d.ch * d.cw >= 2 ** 24:
            return self._fail("class_metrics: evaluation window: the counts are exact as floats below 2^24 only")
        if d.ws_elems < self.nirgan_class_metrics_ws_elems(d.B, d.ch, d.cw, d.classes):
            return self._fail("class_metrics: workspace too small")
        B, H, W, K = d.B, d.H, d.W, d.classes
        n, p, rgb = window_cut(d)
        m = bytes_at(d.mask, B * H * W).reshape(B, H, W)[:, d.y0:d.y0 + d.ch, d.x0:d.x0 + d.cw]
        diff = p - n
        terms = {1: np.abs(diff), 2: diff * diff, 3: ssim_map(n, p, d)}
        if rgb is not None:
            terms.update(zip((5, 6, 7), index_terms(n, p, rgb)))
        rows = arr(d.rows, B * K * COLS).reshape(B, K, COLS)
        for b in range(B):
            for cls in range(K):
                sel = m[b] == cls
                count = int(sel.sum())
                rows[b, cls, 0] = count
                for col, t in terms.items():
                    rows[b, cls, col] = f32(t[b][sel].sum(dtype=np.float64) / count) if count else f32(np.nan)
                l2 = rows[b, cls, 2]
                with np.errstate(divide="ignore"):
                    rows[b, cls, 4] = f32(np.nan) if not count else (f32(10) * np.log10(f32(d.max_val) ** 2 / l2) if l2 > 0 else f32(np.inf))
        return 0
