"""numpy statement of nirgan_gan_loss (include/nirgan_hip.h: the vanilla and wgangp objectives of GANLoss) -- TEST INFRASTRUCTURE ONLY,
installed with ``nirgan_hip.lib.set_backend`` like tests/emu_backend.py, which it extends.

Restated from the header alone: the scalars arrive as C floats, the terms are summed in float64, ``loss_out[0]`` takes ONE float32 add
per call, ``grad`` is overwritten (NULL: forward only), and the argument checks come before any work and name the entry.
"""
import numpy as np

from emu_backend import EmuBackend, arr

f32 = np.float32
VANILLA, WGANGP = 1, 2


class EmuGanLoss(EmuBackend):
    def nirgan_gan_loss(self, pred, n, mode, target, weight, loss_out, grad, stream=None):
        self.calls.append("gan_loss")
        if mode not in (VANILLA, WGANGP):
            return self._fail("gan_loss: mode must be 1 (vanilla) or 2 (wgangp); lsgan has nirgan_lsgan")
        if not pred or not loss_out or n <= 0:
            return self._fail("gan_loss: bad arguments")
        t, w = f32(target), f32(weight)                                  # what a float parameter of the C entry holds
        x = arr(pred, n).astype(np.float64)
        inv = f32(1) / f32(n)
        if mode == VANILLA:
            e = np.exp(-np.abs(x))
            total = (np.maximum(x, 0) - x * float(t) + np.log1p(e)).sum() / n * float(w)
            sig = np.where(x >= 0, 1 / (1 + e), e / (1 + e))
            g = (float(w) * (sig - float(t)) * float(inv)).astype(f32)
        else:
            sw = -w if t > f32(0.5) else w
            total = x.sum() / n * float(sw)
            g = np.full(n, sw * inv, dtype=f32)                          # both operations in fp32, as the header states
        out = arr(loss_out, 1)
        out[0] = out[0] + f32(total)
        if grad:
            arr(grad, n)[:] = g
        return 0
