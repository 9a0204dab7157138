"""numpy statement of the pixel-discriminator entries of include/nirgan_hip.h (nirgan_pixdisc_ws_elems / _fwd / _bwd) -- TEST
INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend`` like tests/emu_backend.py, which it extends (through tests/emu_gan_loss.py).

Float32 arithmetic restated from the descriptor alone: the flat parameter / gradient ranges, x, stats, out, dout, gx are read and written
through the raw pointers.  Contract enforced (the header's): ``grads`` is OVERWRITTEN with padding elements and net.2.bias zero, the
workspace must hold what the query says, H*W >= 2, ndf == 64, the mode is one of three, bwd reads the ``stats`` fwd left.
"""
import numpy as np

from emu_backend import arr, obj
from emu_gan_loss import EmuGanLoss

TILE, NC_MAX, GRID_MAX, UREC, GREC, FLAT = 32, 64, 256, 388, 8512, 8772
O_W1, O_B1, O_W2, O_B2, O_W3, O_B3 = 0, 256, 320, 8512, 8640, 8768
f32 = np.float32


def lrelu(v):
    return np.where(v > 0, v, f32(0.2) * v).astype(f32)


class EmuPixelDisc(EmuGanLoss):         # EmuBackend + nirgan_gan_loss (the vanilla / wgangp objectives of the fused step)
    def nirgan_pixdisc_ws_elems(self, B, H, W, ndf):
        if B <= 0 or H <= 0 or W <= 0 or ndf != 64 or H * W < 2 or B * H * W > 2 ** 31 - 1:
            return 0
        T = -(-(H * W) // TILE)
        ch = -(-T // min(T, NC_MAX))
        units = B * -(-T // ch)
        return (units + B) * UREC + min(GRID_MAX, -(-units // 4)) * GREC

    def _pd_check(self, d, who, bwd):
        if not d.x or not d.params or not d.stats or not d.ws or (not bwd and not d.out) or (bwd and not d.dout):
            return self._fail(f"{who}: null pointer")
        if bwd and d.mode not in (0, 1, 2):
            return self._fail(f"{who}: mode must be PARAMS, INPUT or PRED")
        if bwd and not (d.grads if d.mode == 0 else d.gx):
            return self._fail(f"{who}: null pointer")
        if d.ndf != 64:
            return self._fail(f"{who}: ndf must be 64")
        if d.B <= 0 or d.H <= 0 or d.W <= 0 or d.H * d.W < 2 or d.B * d.H * d.W > 2 ** 31 - 1:
            return self._fail(f"{who}: bad shape")
        if d.ws_elems < self.nirgan_pixdisc_ws_elems(d.B, d.H, d.W, d.ndf):
            return self._fail(f"{who}: workspace too small")
        arr(d.ws, d.ws_elems)[:] = np.nan                       # scratch: nobody may read it between calls
        return 0

    def _pd_z(self, d):
        B, HW = d.B, d.H * d.W
        p = arr(d.params, FLAT)
        W1, b1, W2, w3, b3 = p[O_W1:O_B1].reshape(64, 4), p[O_B1:O_W2], p[O_W2:O_B2].reshape(128, 64), p[O_W3:O_B3], p[O_B3]
        X = arr(d.x, B * HW * 4).reshape(B * HW, 4)
        z1 = (X @ W1.T + b1).astype(f32)
        h1 = lrelu(z1)
        z2 = (h1.astype(np.float64) @ W2.T.astype(np.float64)).reshape(B, HW, 128)          # net.2.bias: removed by the norm, not read
        z2 = (z2 - z2[:, :1, :]).astype(f32)                   # relative to the pivot (the sample's first pixel), rounded once
        return X, W1, W2, w3, b3, z1, h1, z2

    def nirgan_pixdisc_fwd(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("pixdisc_fwd")
        if self._pd_check(d, "pixdisc_fwd", False):
            return -1
        X, W1, W2, w3, b3, z1, h1, z2 = self._pd_z(d)
        mean = z2.mean(1, dtype=np.float64)
        var = ((z2 - mean[:, None, :]) ** 2).mean(1)
        st = arr(d.stats, d.B * 256).reshape(d.B, 128, 2)
        st[:, :, 0] = mean.astype(f32)
        st[:, :, 1] = (1.0 / np.sqrt(var + 1e-5)).astype(f32)
        xh = ((z2 - st[:, :, 0].reshape(d.B, 1, 128)) * st[:, :, 1].reshape(d.B, 1, 128)).astype(f32)
        arr(d.out, d.B * d.H * d.W)[:] = (lrelu(xh) @ w3 + b3).reshape(-1)
        return 0

    def nirgan_pixdisc_bwd(self, ref, stream=None):
        d = obj(ref)
        self.calls.append(("pixdisc_bwd", int(d.mode)))
        if self._pd_check(d, "pixdisc_bwd", True):
            return -1
        B, HW = d.B, d.H * d.W
        X, W1, W2, w3, b3, z1, h1, z2 = self._pd_z(d)
        st = arr(d.stats, B * 256).reshape(B, 128, 2)
        mean, rstd = st[:, :, 0].reshape(B, 1, 128), st[:, :, 1].reshape(B, 1, 128)
        xh = ((z2 - mean) * rstd).astype(f32)
        dy = arr(d.dout, B * HW).reshape(B, HW, 1)
        dxh = (dy * w3.reshape(1, 1, 128) * np.where(xh > 0, f32(1), f32(0.2))).astype(f32)
        s1 = dxh.mean(1, dtype=np.float64, keepdims=True).astype(f32)
        s2 = (dxh * xh).mean(1, dtype=np.float64, keepdims=True).astype(f32)
        dz2 = (rstd * (dxh - s1 - xh * s2)).astype(f32).reshape(B * HW, 128)
        dz1 = ((dz2 @ W2) * np.where(z1 > 0, f32(1), f32(0.2))).astype(f32)
        if d.mode == 0:
            g = arr(d.grads, FLAT)
            g[:] = 0                                            # overwritten; padding and net.2.bias stay zero
            g[O_W1:O_B1] = (dz1.T @ X).reshape(-1)
            g[O_B1:O_W2] = dz1.sum(0, dtype=np.float64)
            g[O_W2:O_B2] = (dz2.T @ h1).reshape(-1)
            g[O_W3:O_B3] = (dy.reshape(1, -1) @ lrelu(xh).reshape(B * HW, 128)).reshape(-1)
            g[O_B3] = dy.sum(dtype=np.float64)
            return 0
        gx = (dz1 @ W1).astype(f32)
        if d.mode == 1:
            arr(d.gx, B * HW * 4)[:] = gx.reshape(-1)
        else:
            arr(d.gx, B * HW)[:] = gx[:, 3]
        return 0
