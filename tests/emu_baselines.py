"""numpy statement of the per-pixel baseline entries of include/nirgan_hip.h (nirgan_pixmlp_fwd / _train / _ws_elems) -- TEST
INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend`` like tests/emu_backend.py, which it extends.

Float32 arithmetic restated from the descriptor alone: the flat parameter / gradient ranges are read and written through the raw
pointers.  Contract enforced (the header's): ``loss_out[0]`` is ACCUMULATED, ``grads`` is OVERWRITTEN (padding elements zero), the
workspace must hold grid x record floats and is independent of the pixel count once the tiles outnumber the grid.
"""
import numpy as np

from emu_backend import EmuBackend, arr, obj

TILE, MLP_GRID, LIN_BLOCK, LIN_GRID = 32, 256, 256, 2048
FLAT = {0: 8, 64: 4484}                     # flat range (every tensor padded to 4 floats)
f32 = np.float32


class EmuBaselines(EmuBackend):
    def nirgan_pixmlp_ws_elems(self, B, H, W, hidden):
        if B <= 0 or H <= 0 or W <= 0 or hidden not in FLAT or B * H * W > 2 ** 31 - 1:
            return 0
        n = B * H * W
        if hidden == 64:
            return min(MLP_GRID, -(-(-(-n // TILE)) // 4)) * (FLAT[64] + 4)
        return min(LIN_GRID, -(-n // LIN_BLOCK)) * (FLAT[0] + 4)

    def _pix_forward(self, d):
        """float32 forward from the descriptor: (X [n][3], intermediates, y [n])"""
        n = d.B * d.H * d.W
        X = np.ascontiguousarray(arr(d.rgb, 3 * n).reshape(d.B, 3, d.H * d.W).transpose(0, 2, 1).reshape(n, 3))
        p = arr(d.params, FLAT[d.hidden])
        if d.hidden == 0:
            return X, None, X @ p[0:3] + p[4]
        W1, b1, W2, b2, W3, b3 = p[0:192].reshape(64, 3), p[192:256], p[256:4352].reshape(64, 64), p[4352:4416], p[4416:4480], p[4480]
        z1 = X @ W1.T + b1
        h1 = np.maximum(z1, f32(0))
        z2 = h1 @ W2.T + b2
        h2 = np.maximum(z2, f32(0))
        return X, (W2, W3, h1, z2, h2), h2 @ W3 + b3

    def _pix_check(self, d, who, train):
        if not d.rgb or not d.params or (not train and not d.pred):
            return self._fail(f"{who}: null pointer")
        if train and (not d.grads or not d.ws or not ((d.nir and d.loss_out) or d.dpred)):
            return self._fail(f"{who}: null pointer")
        if d.hidden not in FLAT:
            return self._fail(f"{who}: hidden must be 0 or 64")
        if d.B <= 0 or d.H <= 0 or d.W <= 0 or d.B * d.H * d.W > 2 ** 31 - 1:
            return self._fail(f"{who}: bad shape")
        if train and d.ws_elems < self.nirgan_pixmlp_ws_elems(d.B, d.H, d.W, d.hidden):
            return self._fail(f"{who}: workspace too small")
        return 0

    def nirgan_pixmlp_fwd(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("pixmlp_fwd")
        if self._pix_check(d, "pixmlp_fwd", False):
            return -1
        arr(d.pred, d.B * d.H * d.W)[:] = self._pix_forward(d)[2]
        return 0

    def nirgan_pixmlp_train(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("pixmlp_train")
        if self._pix_check(d, "pixmlp_train", True):
            return -1
        n = d.B * d.H * d.W
        X, mid, y = self._pix_forward(d)
        y = y.astype(f32)
        if d.pred:
            arr(d.pred, n)[:] = y
        if d.dpred:
            dy = arr(d.dpred, n).copy()
        else:
            diff = y - arr(d.nir, n)
            arr(d.loss_out, 1)[0] += f32(np.sum(diff * diff, dtype=f32) / f32(n))
            dy = diff * f32(2.0 / n)
        g = arr(d.grads, FLAT[d.hidden])
        g[:] = 0
        if d.hidden == 0:
            g[0:3], g[4] = dy @ X, dy.sum(dtype=f32)
            return 0
        W2, W3, h1, z2, h2 = mid
        dz2 = np.where(z2 > 0, dy[:, None] * W3[None, :], f32(0)).astype(f32)
        dz1 = np.where(h1 > 0, dz2 @ W2, f32(0)).astype(f32)
        g[0:192] = (dz1.T @ X).reshape(-1)
        g[192:256] = dz1.sum(0, dtype=f32)
        g[256:4352] = (dz2.T @ h1).reshape(-1)
        g[4352:4416] = dz2.sum(0, dtype=f32)
        g[4416:4480] = dy @ h2
        g[4480] = dy.sum(dtype=f32)
        return 0
