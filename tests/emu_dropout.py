"""numpy statement of the dropout entries of include/nirgan_hip.h (nirgan_dropout_advance / nirgan_dropout_halo) -- TEST
INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend`` like tests/emu_backend.py, which it extends.

Philox4x32-10 restated from the header alone (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85) on uint64
lanes; ``keep_mask`` is what the GPU tests compare ``nirgan_hip.dropout.mask`` with, bit for bit.
"""
import ctypes as C

import numpy as np

from emu_backend import EmuBackend, arr, obj, reflect

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two 32-bit words -> four uint32 arrays."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]            # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def keep_mask(seed, call, stream_id, B, H, W, Cc, sample0=0) -> np.ndarray:
    """bool [B][H][W][C]: element kept?  seed = (lo, hi) or one 64-bit integer."""
    lo, hi = seed if isinstance(seed, (tuple, list)) else (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    assert Cc % 4 == 0
    q4 = Cc // 4
    b, h, w, cq = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(H, dtype=np.uint64), np.arange(W, dtype=np.uint64),
                              np.arange(q4, dtype=np.uint64), indexing="ij")
    q = (((np.uint64(sample0) + b) * np.uint64(H) + h) * np.uint64(W) + w) * np.uint64(q4) + cq
    words = philox4x32_10((q & MASK32, q >> np.uint64(32), stream_id, call), (lo, hi))
    keep = np.stack([(v >> np.uint32(31)).astype(bool) for v in words], axis=-1)         # [B][H][W][q4][4]
    return keep.reshape(B, H, W, Cc)


def mask_nchw(seed, call, stream_id, B, H, W, Cc, sample0=0) -> np.ndarray:
    """the {0, 2} float32 tensor [B][C][H][W] nirgan_hip.dropout.mask returns"""
    return np.ascontiguousarray(np.where(keep_mask(seed, call, stream_id, B, H, W, Cc, sample0), np.float32(2), np.float32(0)).transpose(0, 3, 1, 2))


def _u32(ptr, n):
    if hasattr(ptr, "value"):
        ptr = ptr.value
    return np.ctypeslib.as_array((C.c_uint32 * int(n)).from_address(int(ptr)))


class EmuDropout(EmuBackend):
    def nirgan_dropout_advance(self, state, stream=None):
        self.calls.append("dropout_advance")
        if not state:
            return self._fail("dropout_advance: null pointer")
        s = _u32(state, 4)
        s[2] = (int(s[2]) + 1) & 0xFFFFFFFF
        return 0

    def nirgan_dropout_halo(self, ref, stream=None):
        d = obj(ref)
        self.calls.append(("dropout_halo", int(d.stream_id), int(d.pad)))
        if not d.buf or not d.state:
            return self._fail("dropout_halo: null pointer")
        if d.B <= 0 or d.H <= 0 or d.W <= 0 or d.C < 4 or d.C % 4:
            return self._fail("dropout_halo: bad shape (C must be a multiple of 4)")
        if d.pad < 0 or d.pad >= min(d.H, d.W):
            return self._fail("dropout_halo: pad outside 0 .. min(H, W) - 1")
        if d.sample0 < 0:
            return self._fail("dropout_halo: negative sample0")
        if d.buf % 16:
            return self._fail("dropout_halo: buf must be 16-byte aligned")
        hp, wp = d.H + 2 * d.pad, d.W + 2 * d.pad
        n = d.B * hp * wp * d.C
        if n >= 2 ** 40:
            return self._fail("dropout_halo: B (H + 2 pad)(W + 2 pad) C must stay below 2^40")
        if d.buf_elems < n:
            return self._fail("dropout_halo: buf too small")
        s = _u32(d.state, 4)
        keep = keep_mask((int(s[0]), int(s[1])), int(s[2]), int(d.stream_id), d.B, d.H, d.W, d.C, d.sample0)
        ih, iw = reflect(np.arange(hp) - d.pad, d.H), reflect(np.arange(wp) - d.pad, d.W)
        keep = keep[:, ih][:, :, iw]
        x = arr(d.buf, n).reshape(d.B, hp, wp, d.C)
        with np.errstate(invalid="ignore", over="ignore"):
            x[:] = np.where(keep, np.float32(2) * x, np.float32(0))
        return 0
