"""numpy statement of the dihedral-view entries of include/nirgan_hip.h (nirgan_tile_views_expand / nirgan_tile_views_merge) -- TEST
INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend`` like tests/emu_backend.py; it extends tests/emu_tile_blend.py, so
one backend serves predict_tiled with every ``blend`` and ``tta``.

Restated from the descriptor alone with index arrays (the test bodies restate the views with np.flip / np.swapaxes instead).
Contract enforced (the header's): expand moves bit patterns (uint32 copies: NaN payloads survive); merge adds in float32 in the tree
((v0+v1)+(v2+v3))+((v4+v5)+(v6+v7)) and multiplies once by 1/k; dst is written whole and never read; the argument checks come before
any work and name the entry.
"""
import numpy as np

from emu_backend import arr, obj
from emu_tile_blend import EmuTileBlend

f32 = np.float32


def source_index(g, H, W):
    """(i', j') as [H_view][W_view] index arrays: view_g(x) = x[i', j']"""
    hv, wv = (W, H) if g & 4 else (H, W)
    i, j = np.meshgrid(np.arange(hv), np.arange(wv), indexing="ij")
    a, b = (j, i) if g & 4 else (i, j)
    return (H - 1 - a if g & 2 else a), (W - 1 - b if g & 1 else b)


class EmuTileViews(EmuTileBlend):
    def _views_check(self, d, who):
        if not d.src or not d.dst:
            return self._fail(f"{who}: null pointer")
        if d.views not in (1, 2, 4, 8):
            return self._fail(f"{who}: views {d.views} is not 1, 2, 4 or 8")
        if d.n <= 0 or d.C <= 0 or d.H <= 0 or d.W <= 0:
            return self._fail(f"{who}: bad shape")
        if d.views == 8 and d.H != d.W:
            return self._fail(f"{who}: views 8 needs a square plane")
        if d.H * d.W >= 2 ** 31 or d.n * d.views * d.C >= 2 ** 31:
            return self._fail(f"{who}: a plane or the plane count (n * views * C) is 2^31 or more")
        return 0

    def nirgan_tile_views_expand(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("tile_views_expand")
        rc = self._views_check(d, "tile_views_expand")
        if rc:
            return rc
        n, k, Cc, H, W = d.n, d.views, d.C, d.H, d.W
        src = arr(d.src, n * Cc * H * W).view(np.uint32).reshape(n, Cc, H, W)
        dst = arr(d.dst, n * k * Cc * H * W).view(np.uint32).reshape(n, k, Cc, H, W)
        for g in range(k):
            ii, jj = source_index(g, H, W)
            dst[:, g] = src[:, :, ii, jj]
        return 0

    def nirgan_tile_views_merge(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("tile_views_merge")
        rc = self._views_check(d, "tile_views_merge")
        if rc:
            return rc
        n, k, Cc, H, W = d.n, d.views, d.C, d.H, d.W
        src = arr(d.src, n * k * Cc * H * W).reshape(n, k, Cc, H, W)
        dst = arr(d.dst, n * Cc * H * W).reshape(n, Cc, H, W)
        v = []
        for g in range(k):
            ii, jj = source_index(g, H, W)
            back = np.empty((n, Cc, H, W), dtype=f32)
            back[:, :, ii, jj] = src[:, g]                                       # v_g[i'][j'] = src[g][i][j]
            v.append(back)
        while len(v) > 1:
            v = [(v[i] + v[i + 1]).astype(f32) for i in range(0, len(v), 2)]
        dst[...] = v[0] * f32(1.0 / k)
        return 0
