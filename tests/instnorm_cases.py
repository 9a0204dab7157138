"""Bodies shared by tests/test_instnorm_emulated.py (numpy emulator, CPU) and tests/test_gpu_instnorm.py (MI355X): the raw entries
nirgan_instnorm_fwd and nirgan_instnorm_bwd (csrc/instnorm.hip, csrc/instnorm_dev.h) against float64 on every kernel route.

Every body takes ``dev`` ("cpu": the installed backend is an emulator).  Every expected value is float64 torch from the definition in
include/nirgan_hip.h on the fp32 (or bf16-decoded) inputs the entry receives: biased variance, eps inside the root, activation,
residual, ``F.pad(mode="reflect")``; the backward is autograd through exactly that composition (the residual left out, as the entry
leaves it out), gsum_out the autograd fold of g plus g2.  Where the entry receives a producer's partial sums instead of the tensor
(stats_chunks, sums_chunks), the expectation is the float64 value of those partial sums (raw moments, no re-basing).  Nothing is
expected from the emulator or from a kernel.

Bounds.  u = 2^-24.  Every element is held to K u A (tests/streaming_cases.py): A the float64 sum of the absolute values of the terms,
K the rounded operations on the longest chain; a division counts 3, a square root 2; a contraction to an FMA only removes roundings.
The kernels' structure (nrg = in_nrg(C) row groups of C / 4 lanes, nchunk = in_nchunk chunks of ppc = ceil(HW / nchunk) pixels, the
finalize on slices of cw = 64 channels (C >= 64 and C % 64 == 0, else C) with nrg_fin = in_nrg(cw)):

  T(chunks)   adds on the longest path of a per-(b, c) sum: a thread adds ceil(ppc / nrg) pixels, the LDS combine adds nrg row groups,
              the finalize adds ceil(chunks / nrg_fin) chunks per thread and combines nrg_fin groups:
              T = ceil(ppc / nrg) + nrg + ceil(chunks / nrg_fin) + nrg_fin;  Tf = ceil(chunks / nrg_fin) + nrg_fin for a producer's chunks.
  mean        sums about k = y[b, 0, c]: y - k (1), T adds, 1 / HW (3) and its product (1), k + m (1): K = T + 6, A = |k| + mean |y - k|.
  var         (y - k)^2: 1 + 2 roundings of its operand counted 2 -> 3, T adds, * inv 4: (T + 7) u Q, Q = mean (y - k)^2; m m:
              2 |m| (T + 5) u mean |y - k| + u m^2; the subtraction u var.  Asserted <= (2 T + 14) u (Q + m^2), the form the header
              of instnorm.hip promises (2 |m| mean |y - k| <= m^2 + Q).
  re-based    per chunk dk = k_c - K (1), n dk (1), s1 + (1): K = 3 + Tf + 4 on A1 = sum_c (|s1_c| + n_c |dk_c|) / HW; the shift and
              K + m: 2 u (|K| + |shift| + |m|).  Second moment: n dk dk (4) and its two adds: K = 6 + Tf + 4 on
              AQ = sum_c (|s2_c| + 2 |dk_c s1_c| + n_c dk_c^2) / HW; then m m and the subtraction as above.
  rstd        0.5 rstd^3 (bound of var) + (1 + 2 + 3) u rstd: the add of eps, the root, the division.
  z           rstd |d mean| + |y - mean| |d rstd| + 2 u |z|;  out: the slope's product (1) on the negative side of LeakyReLU, the
              residual's add u (|act z| + |r|).  A constant channel has z = 0 exactly on both sides: its bound is 0.
  bf16        a twin stored next to the fp32 form is bitwise its round-to-nearest-even; a twin-only run is bitwise the twin of the
              both-stored run.
  backward    fed mean, rstd = the float64 values rounded to fp32: |d mean| = u |mean|, |d rstd| = u rstd (chained on the device's own
              statistics: the forward's bounds).  g_a: (images - 1 + [g2]) u (fold |g| + |g2|).  g_z: g_a act'(z), 1 more on the negative
              side of LeakyReLU.  m1 = mean g_z: mean of the terms' bounds + (T + 4) u mean |g_z|; m2 = mean g_z z: terms
              |z| b(g_z) + |g_z| b(z) + u |g_z z|, then (T + 4) u mean |g_z z|.  dy = rstd (g_z - m1 - z m2): the operands' bounds,
              u |z m2|, two subtractions 2 u (|g_z| + |m1| + |z m2|), rstd's own rounding and the product u |dy|.
              norm = 0: dy = g_z; dbias += sum: ceil(ppc / nrg) + nrg adds per block row, then nirgan_colsum over B nchunk rows
              (ceil(rows / 64) + 3 + 2 + 16 + 1) on |dbias before| + sum |g_z|.

No element is left out: the activation mask is the sign of z, and every case's y is adjusted until every float64 |z| exceeds four times
the bound on z (asserted in the bodies); the one exception is a constant channel (z = 0 exactly; ReLU forward, no activation backward).

Two CPU checks keep this honest (tests/test_instnorm_emulated.py): a float32 numpy restatement of the documented algorithm in the
kernels' summation order lies inside every bound on every case, and emulators with one planted error each fail their body.
"""
import ctypes as C
import functools

import torch
import torch.nn.functional as F

from nirgan_hip import lib as L
from streaming_cases import U, fails, same, stream, sync, within

EPS = torch.tensor(1e-5, dtype=torch.float32).double().item()
SLOPE32 = 0.2
SLOPE = torch.tensor(SLOPE32, dtype=torch.float32).double().item()
SENT, SENT16 = -12345.5, 0xC9C9 - 0x10000          # poison: a fixed finite fp32 value, a fixed finite (negative) bf16 pattern
GUARD = 64
CONST_CH = 2
NONE, RELU, LRELU = L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU
KEEP, REFLECT = L.BORDER_KEEP, L.BORDER_REFLECT


# ------------------------------------------------------------------------------------------ the launch arithmetic, restated
def in_nrg(Cc):
    q4 = Cc // 4
    return 1 if q4 >= 256 else 256 // q4


def in_nchunk(B, HW, Cc):
    return min(max(2048 // B, 1), max(HW // (in_nrg(Cc) * 8), 1))


def in_fast_ok(H, W, pad):
    return pad == 0 or (H > 2 * pad + 1 and W > 2 * pad + 1)           # (every case here is far below 2^31 elements per sample)


def fin_cw(Cc):
    return 64 if Cc >= 64 and Cc % 64 == 0 else Cc


def geometry(shape):
    B, H, W, Cc = shape
    nchunk = in_nchunk(B, H * W, Cc)
    return {"nrg": in_nrg(Cc), "nchunk": nchunk, "ppc": -(-H * W // nchunk), "slices": Cc // fin_cw(Cc), "nrg_fin": in_nrg(fin_cw(Cc))}


def t_adds(shape, chunks=None):
    g = geometry(shape)
    chunks = g["nchunk"] if chunks is None else chunks
    return -(-g["ppc"] // g["nrg"]) + g["nrg"] + -(-chunks // g["nrg_fin"]) + g["nrg_fin"]


def tf_adds(shape, chunks):
    g = geometry(shape)
    return -(-chunks // g["nrg_fin"]) + g["nrg_fin"]


def fwd_route(sp):
    B, H, W, Cc = sp["shape"]
    if sp.get("out", "f32") is None:
        return None
    reflect = sp.get("border", KEEP) == REFLECT and sp.get("pad", 0) > 0
    return "fast" if in_fast_ok(H, W, sp["pad"] if reflect else 0) else "general"


def bwd_route(sp):
    """(first pass, second pass) as nirgan_instnorm_bwd picks them"""
    B, H, W, Cc = sp["shape"]
    norm, has_g, pre = sp.get("norm", 1), sp.get("g", True), sp.get("pre")
    fast = bool(norm and has_g and in_fast_ok(H, W, sp.get("g_pad", 0) if sp.get("fold") else 0))
    p1 = "pre" if pre else ("fast" if fast else "general")
    if not norm or sp.get("dy", "f32") is None:
        return p1, None
    fast2 = fast if has_g else pre == "gsum"
    return p1, "fast" if fast2 else "general"


PRE_CHUNKS = 5


def pre_counts(HW):
    """five chunks of unequal counts, one of them a single pixel"""
    c = [HW // 4 + 2, HW // 5 - 1, 1, HW // 3]
    return c + [HW - sum(c)]


# ------------------------------------------------------------------------------------------ cases
FWD = {
    "1": dict(shape=(2, 6, 6, 8), border=REFLECT, pad=1, act=RELU, const=True,
              route=dict(apply="fast", nrg=128, nchunk=1, ppc=36, slices=1, nrg_fin=128)),
    "2": dict(shape=(1, 5, 9, 32), border=REFLECT, pad=3, act=LRELU,
              route=dict(apply="general", nrg=32, nchunk=1, ppc=45, slices=1, nrg_fin=32)),
    "3": dict(shape=(2, 17, 13, 64), border=REFLECT, pad=1, act=NONE, r_pad=1,
              route=dict(apply="fast", nrg=16, nchunk=1, ppc=221, slices=1, nrg_fin=16)),
    "4": dict(shape=(1, 23, 19, 96), border=KEEP, pad=2, act=RELU, const=True,
              route=dict(apply="fast", nrg=10, nchunk=5, ppc=88, slices=1, nrg_fin=10)),
    "5": dict(shape=(1, 63, 65, 256), border=REFLECT, pad=1, act=LRELU, out="both",
              route=dict(apply="fast", nrg=4, nchunk=127, ppc=33, slices=4, nrg_fin=16)),
    "6": dict(shape=(3, 9, 7, 1024), border=REFLECT, pad=1, act=RELU,
              route=dict(apply="fast", nrg=1, nchunk=7, ppc=9, slices=16, nrg_fin=16)),
    "7": dict(shape=(2, 8, 10, 4), border=KEEP, pad=1, act=LRELU,
              route=dict(apply="fast", nrg=256, nchunk=1, ppc=80, slices=1, nrg_fin=256)),
    "8": dict(shape=(1, 12, 9, 192), border=REFLECT, pad=1, act=RELU, y16=True, out="twin",
              route=dict(apply="fast", nrg=5, nchunk=2, ppc=54, slices=3, nrg_fin=16)),
    "9": dict(shape=(2, 10, 10, 64), out=None,
              route=dict(apply=None, nrg=16, nchunk=1, ppc=100, slices=1, nrg_fin=16)),
    "10": dict(shape=(2, 7, 9, 32), norm=0, border=KEEP, pad=1, act=LRELU, r_pad=2,
               route=dict(apply="fast", nrg=32, nchunk=1, ppc=63, slices=1, nrg_fin=32)),
    "11-shift": dict(shape=(2, 12, 16, 64), border=REFLECT, pad=1, act=RELU, pre="shift",
                     route=dict(apply="fast", nrg=16, nchunk=1, ppc=192, slices=1, nrg_fin=16)),
    "11-noshift": dict(shape=(1, 23, 19, 96), border=KEEP, pad=0, act=NONE, pre="noshift",
                       route=dict(apply="fast", nrg=10, nchunk=5, ppc=88, slices=1, nrg_fin=10)),
    # recorded: pixel 0 at 8 standard deviations, the worst case of the shift; held to its own derived bound only
    "far-pixel-0": dict(shape=(2, 17, 13, 64), border=REFLECT, pad=1, act=LRELU, far=True,
                        route=dict(apply="fast", nrg=16, nchunk=1, ppc=221, slices=1, nrg_fin=16)),
}

BWD = {
    "1": dict(shape=(2, 6, 6, 8), fold=True, g_pad=1, act=RELU, g2=True, gsum=True, d_pad=2, route=("fast", "fast")),
    "2": dict(shape=(1, 5, 9, 32), fold=True, g_pad=3, act=LRELU, d_pad=1, route=("general", "general")),
    "3": dict(shape=(2, 17, 13, 64), fold=False, g_pad=1, act=NONE, dy="both", d_pad=1, route=("fast", "fast")),
    "4": dict(shape=(1, 23, 19, 96), g=False, g2=True, act=NONE, const=True, d_pad=1, route=("general", "general")),
    "5": dict(shape=(1, 63, 65, 256), fold=True, g_pad=1, act=RELU, y16=True, g16=True, dy="twin", d_pad=1, route=("fast", "fast")),
    "6": dict(shape=(3, 9, 7, 1024), fold=True, g_pad=1, act=RELU, d_pad=0, route=("fast", "fast")),
    "7": dict(shape=(2, 8, 10, 4), fold=False, g_pad=1, g2=True, act=LRELU, d_pad=1, route=("fast", "fast")),
    "9": dict(shape=(2, 10, 10, 64), fold=True, g_pad=1, act=LRELU, dy=None, route=("fast", None)),
    "10": dict(shape=(2, 7, 9, 32), norm=0, fold=True, g_pad=1, act=LRELU, dy="both", d_pad=1, dbias=True, route=("general", None)),
    "11-gsum": dict(shape=(2, 12, 16, 64), g=False, pre="gsum", act=RELU, d_pad=1, route=("pre", "fast")),
    "11-plain-g": dict(shape=(1, 23, 19, 96), fold=False, g_pad=1, pre="g", act=LRELU, d_pad=2, route=("pre", "fast")),
    # forward into backward on the device's own statistics
    "chained": dict(shape=(2, 17, 13, 64), fold=True, g_pad=1, act=RELU, g2=True, d_pad=1, chained=True, route=("fast", "fast")),
}


def routes_hold(kind, name):
    sp = (FWD if kind == "fwd" else BWD)[name]
    B, H, W, Cc = sp["shape"]
    g = geometry(sp["shape"])
    if kind == "fwd":
        assert dict(g, apply=fwd_route(sp)) == sp["route"], (name, g, fwd_route(sp))
    else:
        assert bwd_route(sp) == sp["route"], (name, bwd_route(sp))
    if sp["shape"] == (1, 63, 65, 256):          # ragged chunking: two empty chunks, one of 3 pixels, group remainders of 1 and 3
        fill = [max(0, min(g["ppc"], H * W - c * g["ppc"])) for c in range(g["nchunk"])]
        assert (g["nchunk"], g["ppc"]) == (127, 33) and fill[124:] == [3, 0, 0] and fill[123] == 33
        assert -(-33 // g["nrg"]) % 4 != 0 and g["nrg"] == 4
    if sp["shape"] == (2, 6, 6, 8):
        assert g["nrg"] > H * W
    if sp["shape"] in ((2, 17, 13, 64), (2, 8, 10, 4)):
        assert g["nrg"] > W                      # several rows per step of the pixel cursor
    if sp["shape"] == (1, 23, 19, 96):
        assert g["nrg"] * (Cc // 4) == 240       # 16 idle threads
    if sp["shape"] == (1, 5, 9, 32):             # three images of a row coordinate under pad 3
        assert any(sum((1 <= h <= 3, H - 4 <= h <= H - 2)) == 2 for h in range(H))


# ------------------------------------------------------------------------------------------ inputs and the float64 forward
def act64(z, act):
    if act == RELU:
        return z.clamp_min(0)
    if act == LRELU:
        return torch.where(z > 0, z, z * SLOPE)
    return z


def stats64(y64, shape, pre=None, shift=None):
    """float64 mean / rstd of y [B][HW][C] and their bounds; with ``pre`` the producer's partial sums and THEIR float64 value"""
    B, H, W, Cc = shape
    HW = H * W
    out = {}
    if pre is None:
        T = t_adds(shape)
        k = y64[:, 0]
        v = y64 - k[:, None]
        m, Mabs, Q = v.mean(1), v.abs().mean(1), (v * v).mean(1)
        mean = y64.mean(1)
        var = ((y64 - mean[:, None]) ** 2).mean(1)
        b_mean = (T + 6) * U * (k.abs() + Mabs)
        b_var = U * ((T + 7) * Q + 2 * m.abs() * (T + 5) * Mabs + m * m + var)
        assert (b_var <= (2 * T + 14) * U * (Q + m * m) * (1 + 1e-9)).all()
    else:
        s64 = shift.double() if shift is not None else torch.zeros(Cc, dtype=torch.float64)
        v = y64 - s64
        part = torch.zeros(B, PRE_CHUNKS, 4, Cc)
        at = 0
        for c, n in enumerate(pre_counts(HW)):
            seg = v[:, at:at + n]
            kc = seg[:, n // 2].float()                      # a value of the chunk itself
            dlt = seg - kc.double()[:, None]
            part[:, c, 0], part[:, c, 1], part[:, c, 2], part[:, c, 3] = kc, dlt.sum(1).float(), (dlt * dlt).sum(1).float(), float(n)
            at += n
        assert at == HW
        p = part.double()
        kc, s1, s2, n = p[:, :, 0], p[:, :, 1], p[:, :, 2], p[:, :, 3]
        mean_v = (s1 + n * kc).sum(1) / HW
        var = ((s2 + 2 * kc * s1 + n * kc * kc).sum(1) / HW - mean_v * mean_v).clamp_min(0)
        mean = s64 + mean_v
        assert ((mean - y64.mean(1)).abs() <= 8 * U * (mean.abs() + y64.abs().mean(1))).all()       # the partial sums ARE those of y
        K0 = kc[:, :1]
        dk = kc - K0
        m = mean_v - K0[:, 0]
        A1 = (s1.abs() + n * dk.abs()).sum(1) / HW
        AQ = (s2.abs() + 2 * (dk * s1).abs() + n * dk * dk).sum(1) / HW
        Tf = tf_adds(shape, PRE_CHUNKS)
        b_m = (3 + Tf + 4) * U * A1
        b_mean = b_m + 2 * U * (K0[:, 0].abs() + s64.abs() + m.abs())
        b_var = (6 + Tf + 4) * U * AQ + 2 * m.abs() * b_m + U * m * m + U * var
        out["part"] = part
    rstd = (var + EPS) ** -0.5
    out.update(mean=mean, var=var, rstd=rstd, b_mean=b_mean, b_rstd=0.5 * rstd ** 3 * b_var + 6 * U * rstd)
    return out


def z_bound(y64, st, const):
    z = (y64 - st["mean"][:, None]) * st["rstd"][:, None]
    b = st["rstd"][:, None] * st["b_mean"][:, None] + (y64 - st["mean"][:, None]).abs() * st["b_rstd"][:, None] + 2 * U * z.abs()
    if const:
        b[:, :, CONST_CH] = 0.0
    return z, b


@functools.lru_cache(maxsize=None)
def y_case(shape, y16=False, const=False, pre=None, far=False, raw=False):
    """y [B][HW][C] fp32 of a case, its float64 statistics and bounds.  Channels c % 4 == 1: mean 300, spread 0.5 (a missing shift does
    not survive it; bf16 storage has no room for it and keeps to the first); the others: mean 0.7, spread 1; channel 2 constant on
    demand.  Elements whose |z| is not safely above four times the bound on z are moved away from the kink until none is left."""
    B, H, W, Cc = shape
    gen = torch.Generator().manual_seed(61)
    y = torch.randn(B, H * W, Cc, generator=gen)
    big = ((torch.arange(Cc) % 4 == 1) & (not y16))[None, None, :]
    y = torch.where(big, 300 + 0.5 * y, 0.7 + y)
    if const:
        y[:, :, CONST_CH] = y[:, :1, CONST_CH]
    if far:
        y[:, 0] = torch.where(big[0], torch.tensor(304.0), torch.tensor(8.7))
    shift = 0.5 * torch.randn(Cc, generator=gen) if pre == "shift" else None
    rnd = (lambda t: t.bfloat16().float()) if y16 else (lambda t: t)
    y = rnd(y)
    if raw:                      # norm = 0: z = y, exactly; the kink is y = 0
        return {"y": torch.where(y.abs() < 0.01, torch.full_like(y, 0.05), y), "shift": None}
    for _ in range(60):
        st = stats64(y.double(), shape, pre, shift)
        z, b = z_bound(y.double(), st, const)
        bad = z.abs() <= 6 * b
        if const:
            bad[:, :, CONST_CH] = False
        if not bad.any():
            break
        side = torch.where(z >= 0, 1.0, -1.0) * (0.3 + 0.4 * torch.rand(z.shape, generator=gen).double())
        y = torch.where(bad, rnd((st["mean"][:, None] + side / st["rstd"][:, None]).float()), y)
    else:
        raise AssertionError(f"{shape}: some z stays near the kink")
    return {"y": y, "shift": shift, **st}


def kink_free(z, b_z, const):
    """no element is left out: every |z| exceeds four times its bound (a constant channel: exactly 0)"""
    ok = z.abs() > 4 * b_z
    if const:
        assert (z[:, :, CONST_CH] == 0).all()
        ok[:, :, CONST_CH] = True
    assert ok.all(), f"{int((~ok).sum())} elements within four bounds of the kink"


def pad64(a, P):
    return F.pad(a.permute(0, 3, 1, 2), (P,) * 4, mode="reflect").permute(0, 2, 3, 1) if P else a


def y_of(sp):
    return y_case(sp["shape"], sp.get("y16", False), sp.get("const", False), sp.get("pre") if sp.get("pre") in ("shift", "noshift") else None,
                  sp.get("far", False), not sp.get("norm", 1))


@functools.lru_cache(maxsize=None)
def fwd_case(name):
    sp = FWD[name]
    B, H, W, Cc = sp["shape"]
    yc = y_of(sp)
    y64 = yc["y"].double()
    c = {"sp": sp, "yc": yc}
    norm, act, const = sp.get("norm", 1), sp.get("act", NONE), sp.get("const", False)
    if norm:
        z, b_z = z_bound(y64, yc, const)
    else:
        z, b_z = y64, torch.zeros_like(y64)
        assert (z.abs() > 1e-3).all()
    c["z"], c["b_z"] = z, b_z
    a = act64(z, act).reshape(B, H, W, Cc)
    neg = (z < 0).reshape(B, H, W, Cc)
    b = b_z.reshape(B, H, W, Cc).clone()
    if act == RELU:
        b = torch.where(neg, torch.zeros_like(b), b)
    elif act == LRELU:
        b = torch.where(neg, SLOPE * b + U * a.abs(), b)
    if "r_pad" in sp:
        rp = sp["r_pad"]
        r = torch.randn(B, H + 2 * rp, W + 2 * rp, Cc, generator=torch.Generator().manual_seed(63))
        ri = r.double()[:, rp:rp + H, rp:rp + W]
        b = b + U * (a.abs() + ri.abs())
        a = a + ri
        c["r"] = r
    P = sp.get("pad", 0)
    if sp.get("border", KEEP) == REFLECT:
        c["out"], c["b_out"] = pad64(a, P), pad64(b, P)
    else:
        c["out"], c["b_out"] = a, b
    return c


# ------------------------------------------------------------------------------------------ buffers
def sent(n, dev):
    return torch.full((n,), SENT, device=dev)


def sent16(n, dev):
    return torch.full((n,), SENT16, dtype=torch.int16, device=dev)


def all_sent(t):
    t = t.cpu()
    return bool((t == (SENT16 if t.dtype == torch.int16 else SENT)).all())


def bf16_bits(t32):
    """round-to-nearest-even bf16 of fp32 values, as bit patterns"""
    return t32.cpu().bfloat16().view(torch.int16)


def y_dev(yc, y16, dev):
    return (yc["y"].bfloat16() if y16 else yc["y"]).contiguous().to(dev)


def halo_mask(hp, wp, P):
    m = torch.ones(hp, wp, dtype=torch.bool)
    m[P:hp - P, P:wp - P] = False
    return m


# ------------------------------------------------------------------------------------------ forward body
def fwd_desc(dev, name, out_mode):
    c = fwd_case(name)
    sp, yc = c["sp"], c["yc"]
    B, H, W, Cc = sp["shape"]
    P = sp.get("pad", 0)
    hp, wp = H + 2 * P, W + 2 * P
    norm, pre = sp.get("norm", 1), sp.get("pre")
    k = {"y": y_dev(yc, sp.get("y16", False), dev), "mean": sent(B * Cc + GUARD, dev), "rstd": sent(B * Cc + GUARD, dev)}
    need = B * PRE_CHUNKS * 4 * Cc if pre else int(L.backend().nirgan_instnorm_ws_elems(B, H, W, Cc))
    k["ws"] = sent(need + GUARD, dev)
    if pre:
        k["ws"][:need] = yc["part"].reshape(-1).to(dev)
    d = L.InFwdDesc()
    d.y, d.B, d.H, d.W, d.C, d.norm, d.eps = k["y"].data_ptr(), B, H, W, Cc, norm, 1e-5
    d.mean, d.rstd, d.act, d.slope = k["mean"].data_ptr(), k["rstd"].data_ptr(), sp.get("act", NONE), SLOPE32
    if "r" in c:
        k["r"] = c["r"].contiguous().to(dev)
        d.residual, d.r_hp, d.r_wp, d.r_pad = k["r"].data_ptr(), H + 2 * sp["r_pad"], W + 2 * sp["r_pad"], sp["r_pad"]
    if out_mode in ("f32", "both"):
        k["out"] = sent(B * hp * wp * Cc, dev)
        d.out = k["out"].data_ptr()
    if out_mode in ("twin", "both"):
        k["twin"] = sent16(B * hp * wp * Cc, dev)
        d.out_bf16 = k["twin"].data_ptr()
    d.o_hp, d.o_wp, d.o_pad, d.border = hp, wp, P, sp.get("border", KEEP)
    d.ws, d.ws_elems = k["ws"].data_ptr(), need
    if pre:
        d.stats_chunks = PRE_CHUNKS
        if yc["shift"] is not None:
            k["shift"] = yc["shift"].to(dev)
            d.stats_shift = k["shift"].data_ptr()
    d.y_bf16 = int(sp.get("y16", False))
    return d, k, need


def fwd_run(dev, name, out_mode):
    d, k, need = fwd_desc(dev, name, out_mode)
    L.call("nirgan_instnorm_fwd", C.byref(d), stream(dev))
    sync(dev)
    return {n: t.cpu() for n, t in k.items() if n in ("mean", "rstd", "ws", "out", "twin")}, need


def fwd_checks(name, got, need, out_mode, family):
    c = fwd_case(name)
    sp, yc = c["sp"], c["yc"]
    B, H, W, Cc = sp["shape"]
    P = sp.get("pad", 0)
    hp, wp = H + 2 * P, W + 2 * P
    what = f"fwd {name} {out_mode}"
    if sp.get("norm", 1):
        within(family + " mean", what, got["mean"][:B * Cc], yc["mean"], yc["b_mean"])
        within(family + " rstd", what, got["rstd"][:B * Cc], yc["rstd"], yc["b_rstd"])
        assert all_sent(got["mean"][B * Cc:]) and all_sent(got["rstd"][B * Cc:]), what + ": wrote behind mean / rstd"
    else:
        assert all_sent(got["mean"]) and all_sent(got["rstd"]) and all_sent(got["ws"]), what + ": norm = 0 touched mean / rstd / ws"
    assert all_sent(got["ws"][need:]), what + ": wrote behind ws"
    if sp.get("pre"):
        assert same(got["ws"][:need], yc["part"].reshape(-1)), what + ": the producer's partial sums changed"
    reflect = sp.get("border", KEEP) == REFLECT and P > 0
    halo = halo_mask(hp, wp, P)
    if "out" in got:
        o = got["out"].reshape(B, hp, wp, Cc)
        if reflect:
            within(family + " out", what, o, c["out"], c["b_out"])
        else:
            within(family + " out", what, o[:, P:P + H, P:P + W], c["out"], c["b_out"])
            assert all_sent(o[:, halo]), what + ": the halo of a KEEP-border out was written"
    if "twin" in got:
        t = got["twin"].reshape(B, hp, wp, Cc)
        if not reflect:
            assert all_sent(t[:, halo]), what + ": the halo of a KEEP-border twin was written"
        if "out" in got:
            o = got["out"].reshape(B, hp, wp, Cc)
            keep = torch.ones(hp, wp, dtype=torch.bool) if reflect else ~halo
            assert torch.equal(t[:, keep], bf16_bits(o[:, keep])), what + ": the twin is not the nearest-even bf16 of the fp32 store"


def fwd_against_float64(dev, name, family="in_fwd"):
    routes_hold("fwd", name)
    c = fwd_case(name)
    sp = c["sp"]
    kink_free(c["z"], c["b_z"], sp.get("const", False))
    mode = sp.get("out", "f32")
    first, need = fwd_run(dev, name, mode)
    fwd_checks(name, first, need, mode, family)
    again, _ = fwd_run(dev, name, mode)
    assert all(same(first[n], again[n]) for n in first), f"fwd {name}: a second launch from fresh poison differs"
    if mode == "twin":           # the twin alone is bitwise the twin of the run that stores both; that run's fp32 form is held to the bounds
        both, need = fwd_run(dev, name, "both")
        fwd_checks(name, both, need, "both", family)
        assert same(first["twin"], both["twin"]), f"fwd {name}: the twin-only store differs from the twin of the both-stored run"
    if sp.get("out", "f32") == "both":
        only, _ = fwd_run(dev, name, "twin")
        assert same(only["twin"], first["twin"]), f"fwd {name}: the twin-only store differs from the twin of the both-stored run"


# ------------------------------------------------------------------------------------------ backward
@functools.lru_cache(maxsize=None)
def bwd_case(name):
    sp = BWD[name]
    B, H, W, Cc = sp["shape"]
    HW = H * W
    yc = y_of(sp)
    norm, act, const, pre = sp.get("norm", 1), sp["act"], sp.get("const", False), sp.get("pre")
    P, has_g, fold = sp.get("g_pad", 0), sp.get("g", True), sp.get("fold", False)
    gen = torch.Generator().manual_seed(65)
    c = {"sp": sp, "yc": yc}
    g = torch.randn(B, H + 2 * P, W + 2 * P, Cc, generator=gen) if has_g else None
    if g is not None and sp.get("g16"):
        g = g.bfloat16().float()
    g2 = torch.randn(B, H, W, Cc, generator=gen) if sp.get("g2") or pre == "gsum" else None       # (pre "gsum": the folded gradient itself)
    c["g"], c["g2"] = g, g2
    c["dbias0"] = 3.0 * torch.randn(Cc, generator=gen)
    # autograd through the forward's composition
    y64 = yc["y"].double().reshape(B, H, W, Cc).requires_grad_(True)
    if norm:
        mu = y64.mean((1, 2), keepdim=True)
        var = ((y64 - mu) ** 2).mean((1, 2), keepdim=True)
        z = (y64 - mu) * (var + EPS) ** -0.5
    else:
        z = y64 * 1.0
    a = act64(z, act)
    a.retain_grad()
    loss = torch.zeros((), dtype=torch.float64)
    abs_terms = torch.zeros(B, H, W, Cc, dtype=torch.float64)
    images = torch.zeros(B, H, W, Cc, dtype=torch.float64)

    def fold64(t):
        """adjoint of the reflect pad (autograd of F.pad), or the interior"""
        if not fold:
            return t[:, P:P + H, P:P + W]
        x = torch.zeros(B, H, W, Cc, dtype=torch.float64, requires_grad=True)
        (pad64(x, P) * t).sum().backward()
        return x.grad
    if g is not None:
        loss = loss + ((pad64(a, P) * g.double()) if fold else (a * g.double()[:, P:P + H, P:P + W])).sum()
        abs_terms += fold64(g.double().abs())
        images += fold64(torch.ones_like(g, dtype=torch.float64))
    if g2 is not None:
        loss = loss + (a * g2.double()).sum()
        abs_terms += g2.double().abs()
        images += 1
    loss.backward()
    ga, dy_auto = a.grad.detach(), y64.grad.detach()
    z = z.detach()
    b_ga = (images - 1) * U * abs_terms
    if pre == "gsum":                       # the folded gradient is an input here: fp32 values, read as they are
        ga = ga.float().double()
        b_ga = torch.zeros_like(ga)
    c["ga"], c["b_ga"] = ga, b_ga
    # the same in closed form, term by term, for the bounds
    if norm:
        mean, rstd = yc["mean"].reshape(B, 1, 1, Cc), yc["rstd"].reshape(B, 1, 1, Cc)
        c["mean32"], c["rstd32"] = yc["mean"].float(), yc["rstd"].float()
        if sp.get("chained"):
            d_mean, d_rstd = yc["b_mean"].reshape(B, 1, 1, Cc), yc["b_rstd"].reshape(B, 1, 1, Cc)
        else:
            d_mean, d_rstd = U * mean.abs(), U * rstd
        b_z = rstd * d_mean + (y64.detach() - mean).abs() * d_rstd + 2 * U * z.abs()
        if const:
            b_z[..., CONST_CH] = 0.0
    else:
        b_z = torch.zeros_like(z)
        assert (z.abs() > 1e-3).all()
    c["z"], c["b_z"] = z.reshape(B, HW, Cc), b_z.reshape(B, HW, Cc)
    neg = z < 0
    if act == RELU:
        gz, b_gz = torch.where(neg, torch.zeros_like(ga), ga), torch.where(neg, torch.zeros_like(ga), b_ga)
    elif act == LRELU:
        gz = torch.where(neg, ga * SLOPE, ga)
        b_gz = torch.where(neg, SLOPE * b_ga + U * gz.abs(), b_ga)
    else:
        gz, b_gz = ga, b_ga
    if not norm:
        c["dy"], c["b_dy"] = gz, b_gz
        assert (gz - dy_auto).abs().max() <= 1e-12 * dy_auto.abs().max()
        geo = geometry(sp["shape"])
        rows = B * geo["nchunk"]
        kb = -(-geo["ppc"] // geo["nrg"]) + geo["nrg"] + -(-rows // 64) + 3 + 2 + 16 + 1
        c["dbias"] = c["dbias0"].double() + gz.sum((0, 1, 2))
        c["b_dbias"] = b_gz.sum((0, 1, 2)) + kb * U * (c["dbias0"].double().abs() + gz.abs().sum((0, 1, 2)))
        return c
    t2 = gz * z
    b_t2 = z.abs() * b_gz + gz.abs() * b_z + U * t2.abs()
    mean3 = lambda t: t.mean((1, 2), keepdim=True)
    if pre:
        # the producer's partial sums: a float64 split of g_z and g_z z into five chunks, rounded to fp32; the means are THEIR sums
        part = torch.zeros(B, PRE_CHUNKS, 2, Cc)
        at = 0
        for ci, n in enumerate(pre_counts(HW)):
            part[:, ci, 0] = gz.reshape(B, HW, Cc)[:, at:at + n].sum(1).float()
            part[:, ci, 1] = t2.reshape(B, HW, Cc)[:, at:at + n].sum(1).float()
            at += n
        c["part"] = part
        Tf = tf_adds(sp["shape"], PRE_CHUNKS)
        m1, m2 = (part.double()[:, :, i].sum(1).reshape(B, 1, 1, Cc) / HW for i in (0, 1))
        b_m1, b_m2 = ((Tf + 4) * U * part.double()[:, :, i].abs().sum(1).reshape(B, 1, 1, Cc) / HW for i in (0, 1))
    else:
        T = t_adds(sp["shape"])
        m1, m2 = mean3(gz), mean3(t2)
        b_m1 = mean3(b_gz) + (T + 4) * U * mean3(gz.abs())
        b_m2 = mean3(b_t2) + (T + 4) * U * mean3(t2.abs())
    inner = gz - m1 - z * m2
    dy = rstd * inner
    b_inner = b_gz + b_m1 + m2.abs() * b_z + z.abs() * b_m2 + U * (z * m2).abs() + 2 * U * (gz.abs() + m1.abs() + (z * m2).abs())
    c["dy"], c["b_dy"] = dy, rstd * b_inner + inner.abs() * d_rstd + U * dy.abs()
    c["m"], c["b_m"] = torch.cat((m1, m2), 2).reshape(B, 2, Cc), torch.cat((b_m1, b_m2), 2).reshape(B, 2, Cc)
    # the closed form IS autograd's gradient (with a producer's sums: up to their fp32 rounding)
    tol = 1e-5 if pre else 1e-10
    assert (dy - dy_auto).abs().max() <= tol * dy_auto.abs().max()
    return c


def bwd_desc(dev, name, dy_mode, stats=None):
    c = bwd_case(name)
    sp, yc = c["sp"], c["yc"]
    B, H, W, Cc = sp["shape"]
    norm, pre, P, dp = sp.get("norm", 1), sp.get("pre"), sp.get("g_pad", 0), sp.get("d_pad", 0)
    hp, wp = H + 2 * dp, W + 2 * dp
    geo = geometry(sp["shape"])
    pch = PRE_CHUNKS if pre else geo["nchunk"]
    k = {"y": y_dev(yc, sp.get("y16", False), dev), "dbias": c["dbias0"].clone().to(dev)}
    d = L.InBwdDesc()
    if c["g"] is not None:
        k["g"] = (c["g"].bfloat16() if sp.get("g16") else c["g"]).contiguous().to(dev)
        d.g, d.g_hp, d.g_wp, d.g_pad, d.g_fold = k["g"].data_ptr(), H + 2 * P, W + 2 * P, P, int(sp.get("fold", False))
    if pre == "gsum":            # g_a arrives in gsum_out; the entry wants a gradient pointer and reads neither g nor g2: NaN
        k["g2"] = torch.full((B * H * W * Cc,), float("nan"), device=dev)
        d.g2 = k["g2"].data_ptr()
    elif c["g2"] is not None:
        k["g2"] = c["g2"].contiguous().to(dev)
        d.g2 = k["g2"].data_ptr()
    d.act, d.slope, d.y, d.norm, d.B, d.H, d.W, d.C = sp["act"], SLOPE32, k["y"].data_ptr(), norm, B, H, W, Cc
    if norm:
        need = B * pch * 2 * Cc + B * 2 * Cc
        k["mean"], k["rstd"] = (stats or (c["mean32"], c["rstd32"]))
        k["mean"], k["rstd"] = k["mean"].reshape(-1).contiguous().to(dev), k["rstd"].reshape(-1).contiguous().to(dev)
        d.mean, d.rstd = k["mean"].data_ptr(), k["rstd"].data_ptr()
    else:
        need = B * geo["nchunk"] * Cc
    k["ws"] = sent(need + GUARD, dev)
    if pre:
        k["ws"][:B * pch * 2 * Cc] = c["part"].reshape(-1).to(dev)
        d.sums_chunks = PRE_CHUNKS
    d.ws, d.ws_elems = k["ws"].data_ptr(), need
    if dy_mode in ("f32", "both"):
        k["dy"] = sent(B * hp * wp * Cc, dev)
        d.dy = k["dy"].data_ptr()
    if dy_mode in ("twin", "both"):
        k["twin"] = sent16(B * hp * wp * Cc, dev)
        d.dy_bf16 = k["twin"].data_ptr()
    d.d_hp, d.d_wp, d.d_pad = hp, wp, dp
    if pre == "gsum":
        k["gsum"] = c["ga"].float().reshape(-1).contiguous().to(dev)
        d.gsum_out = k["gsum"].data_ptr()
    elif sp.get("gsum"):
        k["gsum"] = sent(B * H * W * Cc, dev)
        d.gsum_out = k["gsum"].data_ptr()
    d.dbias = k["dbias"].data_ptr()
    d.y_bf16, d.g_bf16 = int(sp.get("y16", False)), int(sp.get("g16", False))
    return d, k, need


def bwd_run(dev, name, dy_mode, stats=None):
    d, k, need = bwd_desc(dev, name, dy_mode, stats)
    L.call("nirgan_instnorm_bwd", C.byref(d), stream(dev))
    sync(dev)
    return {n: t.cpu() for n, t in k.items() if n in ("ws", "dy", "twin", "gsum", "dbias")}, need


def bwd_checks(name, got, need, dy_mode, family):
    c = bwd_case(name)
    sp = c["sp"]
    B, H, W, Cc = sp["shape"]
    norm, pre, dp = sp.get("norm", 1), sp.get("pre"), sp.get("d_pad", 0)
    hp, wp = H + 2 * dp, W + 2 * dp
    what = f"bwd {name} {dy_mode}"
    assert all_sent(got["ws"][need:]), what + ": wrote behind ws"
    if norm:
        assert same(got["dbias"], c["dbias0"]), what + ": dbias under norm = 1 must stay untouched"
        pch = PRE_CHUNKS if pre else geometry(sp["shape"])["nchunk"]
        # the two means where nirgan_wino6_input_dy_norm reads them
        within(family + " means", what, got["ws"][B * pch * 2 * Cc:need].reshape(B, 2, Cc), c["m"], c["b_m"])
        if pre:
            assert same(got["ws"][:B * pch * 2 * Cc], c["part"].reshape(-1)), what + ": the producer's partial sums changed"
    elif sp.get("dbias"):
        within(family + " dbias", what, got["dbias"], c["dbias"], c["b_dbias"])
    if "gsum" in got:
        if pre == "gsum":
            assert same(got["gsum"], c["ga"].float().reshape(-1)), what + ": gsum_out is an input here"
        else:
            within(family + " gsum", what, got["gsum"].reshape(B, H, W, Cc), c["ga"], c["b_ga"])
    halo = halo_mask(hp, wp, dp)
    if "dy" in got:
        o = got["dy"].reshape(B, hp, wp, Cc)
        within(family + " dy", what, o[:, dp:dp + H, dp:dp + W], c["dy"], c["b_dy"])
        assert all_sent(o[:, halo]), what + ": the halo of dy was written"
    if "twin" in got:
        t = got["twin"].reshape(B, hp, wp, Cc)
        assert all_sent(t[:, halo]), what + ": the halo of the dy twin was written"
        if "dy" in got:
            assert torch.equal(t[:, ~halo], bf16_bits(got["dy"].reshape(B, hp, wp, Cc)[:, ~halo])), what + ": twin is not the nearest-even bf16"


def bwd_against_float64(dev, name, family="in_bwd"):
    routes_hold("bwd", name)
    c = bwd_case(name)
    sp = c["sp"]
    if sp.get("norm", 1):
        kink_free(c["z"], c["b_z"], sp.get("const", False))
    stats = None
    if sp.get("chained"):        # the device's own statistics: a forward launch (statistics only) in front
        B, H, W, Cc = sp["shape"]
        yd = y_dev(c["yc"], False, dev)
        mean, rstd = sent(B * Cc, dev), sent(B * Cc, dev)
        n = int(L.backend().nirgan_instnorm_ws_elems(B, H, W, Cc))
        ws = sent(n, dev)
        f = L.InFwdDesc()
        f.y, f.B, f.H, f.W, f.C, f.norm, f.eps = yd.data_ptr(), B, H, W, Cc, 1, 1e-5
        f.mean, f.rstd, f.ws, f.ws_elems = mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), n
        L.call("nirgan_instnorm_fwd", C.byref(f), stream(dev))
        sync(dev)
        stats = (mean.cpu(), rstd.cpu())
    mode = sp.get("dy", "f32")
    first, need = bwd_run(dev, name, mode, stats)
    bwd_checks(name, first, need, mode, family)
    again, _ = bwd_run(dev, name, mode, stats)
    assert all(same(first[n], again[n]) for n in first), f"bwd {name}: a second launch from fresh poison differs"
    if mode == "twin":
        both, need = bwd_run(dev, name, "both", stats)
        bwd_checks(name, both, need, "both", family)
        assert same(first["twin"], both["twin"]), f"bwd {name}: the twin-only store differs from the twin of the both-stored run"
    if mode == "both":
        only, _ = bwd_run(dev, name, "twin", stats) if sp.get("norm", 1) else (first, 0)          # (norm = 0 has no twin-only form)
        assert same(only["twin"], first["twin"]), f"bwd {name}: the twin-only store differs from the twin of the both-stored run"


# ------------------------------------------------------------------------------------------ argument guards
FWD_GUARDS = [("7", {"C": 6}, b"shape"), ("7", {"C": 1028}, b"shape"), ("3", {"o_hp": 18}, b"geometry"), ("3", {"r_wp": 14}, b"geometry"),
              ("2", {"o_pad": 5, "o_hp": 15, "o_wp": 19}, b"wider"), ("3", {"ws_elems": -1}, b"too small"), ("7", {"twin": True}, b"twin")]
BWD_GUARDS = [("7", {"C": 6}, b"shape"), ("7", {"C": 1028}, b"shape"), ("1", {"g_wp": 9}, b"geometry"), ("1", {"d_hp": 9}, b"geometry"),
              ("2", {"g_pad": 5, "g_hp": 15, "g_wp": 19}, b"wider"), ("3", {"ws_elems": -1}, b"too small"), ("7", {"twin": True}, b"twin"),
              ("10", {"ws_elems": -1}, b"ws"), ("11-plain-g", {"g_fold": 1}, b"sums_chunks")]


def guards(dev):
    """every refused call leaves its message in nirgan_last_error and launches nothing"""
    be = L.backend()
    for kind, table in (("fwd", FWD_GUARDS), ("bwd", BWD_GUARDS)):
        for name, change, msg in table:
            sp = (FWD if kind == "fwd" else BWD)[name]
            mode = sp.get("out" if kind == "fwd" else "dy", "f32") or "f32"
            d, k, need = (fwd_desc if kind == "fwd" else bwd_desc)(dev, name, "f32" if mode == "twin" else mode)
            B, H, W, Cc = sp["shape"]
            for field, v in change.items():
                if field == "twin":
                    k["twin"] = sent16(B * (H + 12) * (W + 12) * Cc, dev)
                    setattr(d, "out_bf16" if kind == "fwd" else "dy_bf16", k["twin"].data_ptr())
                elif field == "ws_elems":          # (the forward asks for the partial sums' room only)
                    d.ws_elems = (B * geometry(sp["shape"])["nchunk"] * 2 * Cc if kind == "fwd" else need) - 1
                else:
                    setattr(d, field, v)
            rc = getattr(be, "nirgan_instnorm_" + kind)(C.byref(d), stream(dev))
            assert fails(rc) and msg in be.nirgan_last_error(), (kind, name, change, be.nirgan_last_error())
            sync(dev)
            for n in ("out", "dy", "twin", "ws"):
                if n in k and not (n == "ws" and sp.get("pre")):
                    assert all_sent(k[n]), f"{kind} {name} {change}: the refused call launched something"
            if kind == "bwd":
                assert same(k["dbias"], bwd_case(name)["dbias0"])
