"""Dropout of the generator's residual blocks: the counter-based mask of csrc/dropout.hip seen from Python.

No mask tensor exists on the training path: ``nirgan_dropout_halo`` recomputes the bits from (seed, call, stream_id, position) in
the forward and in the backward plan (include/nirgan_hip.h: nirgan_dropout_desc).  ``mask`` runs that entry on ones,
for tests and for users who want to see what a step drew.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import lib as L

RANK_STRIDE = 0x9E3779B97F4A7C15        # the seed of rank r is seed ^ (r * RANK_STRIDE mod 2^64): decorrelated masks per rank
MASK64 = (1 << 64) - 1


def split_seed(seed) -> tuple:
    """(lo, hi) 32-bit words of a seed given as one integer (taken mod 2^64) or as the pair itself."""
    if isinstance(seed, (tuple, list)):
        lo, hi = seed
        return int(lo) & 0xFFFFFFFF, int(hi) & 0xFFFFFFFF
    seed = int(seed) & MASK64
    return seed & 0xFFFFFFFF, seed >> 32


def state_words(seed, call: int) -> torch.Tensor:
    """The four state words {seed_lo, seed_hi, call, 0} as a host int32 tensor (bit patterns of the uint32 values)."""
    lo, hi = split_seed(seed)
    return torch.from_numpy(np.array([lo, hi, int(call) & 0xFFFFFFFF, 0], dtype=np.uint32).view(np.int32).copy())


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else None


def apply_halo(buf: torch.Tensor, state: torch.Tensor, B: int, H: int, W: int, Cc: int, pad: int, stream_id: int, sample0: int = 0) -> None:
    """nirgan_dropout_halo in place on a contiguous fp32 tensor holding [B][H + 2 pad][W + 2 pad][C]; state: the device words."""
    d = L.DropoutDesc()
    d.buf, d.buf_elems = buf.data_ptr(), buf.numel()
    d.B, d.H, d.W, d.C, d.pad = B, H, W, Cc, pad
    d.state, d.stream_id, d.sample0 = state.data_ptr(), stream_id, sample0
    L.call("nirgan_dropout_halo", C.byref(d), _stream(buf.device))


def mask(seed, call: int, stream_id: int, B: int, H: int, W: int, C: int, sample0: int = 0, device="cuda") -> torch.Tensor:
    """The {0, 2} multiplier [B, C, H, W] that residual block ``stream_id`` applies in the forward numbered ``call`` of a generator
    seeded with ``seed`` (ResnetGenerator.dropout_state() gives both AFTER a forward) to samples sample0 .. sample0 + B - 1 of the
    batch: the device entry run on ones."""
    device = torch.device(device)
    if device.type != "cuda" and not L.is_emulated():
        raise RuntimeError("nirgan_hip runs on MI355X (cuda device) only; there is no CPU path")
    ones = torch.ones(B, H, W, C, dtype=torch.float32, device=device)
    state = state_words(seed, call).to(device)
    apply_halo(ones, state, B, H, W, C, 0, stream_id, sample0)
    return ones.permute(0, 3, 1, 2).contiguous()
