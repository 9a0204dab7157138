"""Bodies shared by tests/test_boundary_emulated.py (numpy emulator, CPU) and tests/test_gpu_boundary.py (MI355X): the kernels at the two
ends of both networks -- csrc/layout.hip (nirgan_nchw_to_halo, nirgan_tap_gather, nirgan_conv_channel_dgrad) and csrc/endconv.hip (the
direct Conv2d(64, 1, 7): forward, dz, data gradient, weight gradient) -- each raw entry against float64 on every launch route.

Every body takes ``dev`` ("cpu": the installed backend is an EmuBackend) and drives the entry through ``L.call`` / ``L.check``.  Every
expected value is float64 torch from the operation's definition in include/nirgan_hip.h: ``F.pad(..., 'reflect')`` twice for the
reflect route of the boundary copy, sums of slices for the gather, ``F.conv2d`` and its autograd for the channel gradient and for the
last layer.  Nothing is expected from the emulator or from a kernel.  Which kernel a case takes is computed here by repeating the
dispatcher's condition from the header comment, and both kernels of the gather and of the channel gradient are asserted to be reached
by at least three cases.

Bounds: the rule of tests/streaming_cases.py.  u = 2^-24; every element is held to ``K * u * A``, A the float64 sum of the absolute
values of the terms the element adds up, K the number of rounded operations on the longest chain to it (a sum in any association is
within (adds on the deepest path) * u * sum |terms|; an FMA or an MFMA accumulate counts one rounding per term; an add to an exact 0
counts nothing).  Where an entry consumes what an earlier entry of the same body left on the device (dz reads out, the two gradients
read dz), the earlier bound is carried through the float64 derivative, so that the expectation stays float64 from the inputs alone.

nchw_to_halo  a copy: bitwise.  dst is pre-filled with distinct negative integers; the written window must equal the float64
              ``F.pad`` (reflect: pad1 then pad2; keep: the interior only) and EVERY other element the pre-fill -- the halo in keep
              mode, the channels outside [c0, c0 + Cs).
tap_gather    window kernel: s = bias, then ntaps sequential adds: K = ntaps (no bias: s = 0, the first add is exact: ntaps - 1).
              rows kernel: per kernel row a = 0 and k adds (the first exact), then one add into s (s = bias): the first row's first
              term passes k - 1 adds in a and k adds into s: K = 2k - 1 (no bias: 2k - 2).  A = |bias| + sum_t |Q_t|.
chan_dgrad    generic kernel: a lane adds, per valid tap, g = ceil((C/4) / 16) groups dv0 w0 + dv1 w1 + dv2 w2 + dv3 w3 into acc: a
              product (1), three adds inside its group (3), then one add into acc per group of every valid tap, at most
              ceil(k/stride)^2 taps per pixel, then 4 shuffle adds: K = 4 + ceil(k/stride)^2 g + 4.
              k4s2 kernel: a tap product T is C/4 groups of four products added into acc: contracted C FMAs, not contracted 4 + C/4
              roundings, C covers both; then the pixel adds its 4 taps: K = C + 4.  A = sum |dy w| (autograd of |dy|, |w|).
endconv fwd   49 FMAs per lane, 6 reduction adds (two half-wave exchanges, four DPP steps), the bias: K = 56 (no bias: 55),
              A = sum |x w| + |b|.
endconv dz    y y, 1 -, * -> K = 3, A = |dout| (1 + y^2), as tap_scatter; act none: a copy, bitwise; everything outside the crop
              window exactly 0, whatever the buffer held.  y is the forward's own output: + 2 |y dout| bound_y.
              gbias += sum dz: a thread adds ceil(n / (256 g)) elements (g = min(ceil(n / 256), 1024) blocks over the n elements of
              the bordered image), wave 6, four waves 2, ng_partials_finish ceil(g / 256) + 6 + 2, the add into gbias 1:
              K = 3 + ceil(n / (256 g)) + 8 + ceil(g / 256) + 8 + 1, A = |gbias before| + sum |dout| (1 + y^2), + sum of dz's bounds.
endconv dgrad 25 MFMA steps of 2 taps (the 50th tap has weight 0): K = 50, A = sum_t |dz| |w|, + sum_t bound_dz |w|.
endconv wgrad a wave walks ceil(units / waves) units of 8 MFMA steps x 2 pixels = 16 terms each (units = B x_hp ceil(npair / 8),
              npair = ceil(x_wp / 2), waves = 4 blocks); the 4 waves add up in LDS (4); the finish kernel adds ceil(blocks / 16)
              partials per slice and then the 16 slices: K = 16 ceil(units / waves) + 4 + ceil(blocks / 16) + 16, A = sum |dz| |x|,
              + sum bound_dz |x|.
tanh          the sum is pinned with ACT_NONE first, on the same inputs, under bound_z.  The ACT_TANH run is held to
              (1 - ref^2) bound_z + T u |ref|.  T: no accuracy table of tanhf ships with the ROCm installation, so T was measured once
              on the MI355X against float64 tanh of the device's own ACT_NONE output (the same sums bit for bit): the worst
              |tanhf(z) - tanh(z)| / (u |tanh(z)|) over every gather and endconv case here is 2.401 (1.2 ulp); T = 2 x that = 4.802.  The bodies
              print the figure on every run ("RATIO tanhf T").  Inputs keep tanh informative: the pre-activation has unit scale
              (q / sqrt(ntaps), w / sqrt(3136)), and at least 90 % of the float64 outputs of every case are asserted to have |z| < 2.

The issue's guard "a reversed k = 8 list with q_cs = 68 does not fit" does not hold: (8 + 7) (32 + 7) (68 | 1) 4 = 161 460 bytes, below the
160 KB = 163 840 the dispatcher allows.  q_cs = 68 is therefore one more case that must RUN (its planes 64 .. 67 are NaN), and the guard
is taken at q_cs = 72 (170 820 bytes), the first stride that does not fit.

Two CPU checks keep these honest (tests/test_boundary_emulated.py): eager fp32 torch of the same formula lies inside every bound, and an
emulator with one deliberate, subtle error fails the body.
"""
import ctypes as C
import functools
import math

import torch
import torch.nn.functional as F

from emu_backend import EmuBackend
from nirgan_hip import lib as L
from streaming_cases import RATIOS, U, fails, nan, same, stream, sync, within

TANH_T_MEASURED = 2.401         # worst |tanhf - tanh| / (u |tanh|) seen on the MI355X over the cases below
TANH_T = 2 * TANH_T_MEASURED    # above 8 would be a finding, not a bound
assert TANH_T <= 8
GUARD = 8                       # floats on either side of an output that must keep their value
MARK = 7.0


def guarded(n, dev):
    """an output of n NaNs with GUARD marked floats on either side"""
    buf = torch.full((n + 2 * GUARD,), MARK, device=dev)
    buf[GUARD:GUARD + n] = float("nan")
    return buf, buf[GUARD:GUARD + n]


def guard_intact(buf):
    return bool((buf[:GUARD] == MARK).all() and (buf[-GUARD:] == MARK).all())


def tanh_bound(ref, bound_z):
    return (1 - ref * ref) * bound_z + TANH_T * U * ref.abs()


def tanh_informative(z):
    return (z.abs() < 2).double().mean().item() >= 0.9


def note_tanhf(what, got_tanh, got_none):
    """T as the device shows it: tanhf against float64 tanh of the device's own ACT_NONE output"""
    t = torch.tanh(got_none.detach().double().cpu())
    ok = t != 0
    r = ((got_tanh.detach().double().cpu() - t).abs()[ok] / (U * t.abs()[ok])).max().item() if ok.any() else 0.0
    RATIOS["tanhf T"] = max(RATIOS.get("tanhf T", 0.0), r)
    print(f"RATIO tanhf T | {what} | {r:.3e}")


# ---------------------------------------------------------------------------------------------------------------- nchw_to_halo
MODES = {"keep": L.BORDER_KEEP, "reflect": L.BORDER_REFLECT}
# a case is the list of writes (B, Cs, H, W, cs, c0, pad1, pad2, mode) that go into ONE buffer
HALO_CASES = [
    ((2, 3, 5, 7, 4, 0, 0, 1, "keep"), (2, 1, 5, 7, 4, 3, 0, 1, "keep")),         # rgb, then pred beside it: the torch.cat of D's input
    ((1, 4, 1, 1, 4, 0, 0, 1, "keep"),),
    ((3, 2, 33, 17, 8, 5, 2, 0, "keep"),),
    ((1, 1, 4, 4, 4, 0, 0, 0, "keep"),),
    ((2, 1, 1030, 1030, 4, 0, 0, 1, "keep"),),                                    # 2 * 1032^2 positions > 8192 blocks x 256
    ((2, 3, 24, 20, 4, 0, 10, 3, "reflect"),),
    ((1, 3, 2, 2, 4, 0, 1, 3, "reflect"),),
    ((1, 1, 11, 4, 4, 2, 3, 0, "reflect"),),
    ((1, 3, 6, 9, 4, 0, 0, 3, "reflect"),),
]
HALO_GRID_CAP = HALO_CASES[4]
assert 2 * 1032 * 1032 > 8192 * 256


@functools.lru_cache(maxsize=2)
def halo_case(writes):
    B, _, H, W, cs, _, p1, p2, _ = writes[0]
    P = p1 + p2
    Hp, Wp = H + 2 * P, W + 2 * P
    n = B * Hp * Wp * cs
    assert n < 2 ** 24                                   # the pre-fill's integers stay distinct in fp32
    fill = -(1 + torch.arange(n, dtype=torch.float32)).reshape(B, Hp, Wp, cs)
    exp, written = fill.clone(), torch.zeros(B, Hp, Wp, cs, dtype=torch.bool)
    gen, srcs = torch.Generator().manual_seed(61), []
    for b, Cs, h, w, c, c0, q1, q2, mode in writes:
        assert (b, h, w, c, q1 + q2) == (B, H, W, cs, P)
        src = 0.5 + torch.rand(b, Cs, h, w, generator=gen)          # positive: never a pre-fill value
        win = src.double()
        if mode == "reflect":
            for q in (q1, q2):
                if q:
                    win = F.pad(win, (q,) * 4, mode="reflect")
            exp[..., c0:c0 + Cs] = win.permute(0, 2, 3, 1).float()
            written[..., c0:c0 + Cs] = True
        else:
            exp[:, P:P + h, P:P + w, c0:c0 + Cs] = win.permute(0, 2, 3, 1).float()
            written[:, P:P + h, P:P + w, c0:c0 + Cs] = True
        srcs.append(src)
    return srcs, fill, exp, written


def halo_against_float64(dev, writes):
    srcs, fill, exp, written = halo_case(writes)
    dst, keep = fill.to(dev).clone(), []
    for src, (B, Cs, H, W, cs, c0, p1, p2, mode) in zip(srcs, writes):
        keep.append(src.to(dev).contiguous())
        L.call("nirgan_nchw_to_halo", keep[-1].data_ptr(), B, Cs, H, W, dst.data_ptr(), cs, c0, p1, p2, MODES[mode], stream(dev))
    sync(dev)
    got = dst.cpu()
    bad = got.view(torch.int32) != exp.view(torch.int32)
    print(f"RATIO nchw_to_halo | {writes} | {float(bad.any()):.3e}")
    assert not bad[written].any(), f"nchw_to_halo {writes}: {int(bad[written].sum())} elements of the written window differ from F.pad"
    assert not bad[~written].any(), f"nchw_to_halo {writes}: {int(bad[~written].sum())} elements outside the window were touched"


def halo_guards(dev):
    be = L.backend()
    B, Cs, H, W, cs = 1, 3, 6, 9, 4
    src = torch.rand(B, Cs, H, W).to(dev)
    for what, (c0, p1, p2, mode) in {"c0 + Cs > cs": (2, 0, 1, "keep"), "pad1 >= H": (0, 6, 0, "reflect"),
                                     "pad2 >= H + 2 pad1": (0, 1, 8, "reflect")}.items():
        P = p1 + p2
        fill = -(1 + torch.arange(B * (H + 2 * P) * (W + 2 * P) * cs + 64, dtype=torch.float32))
        dst = fill.to(dev).clone()
        assert fails(be.nirgan_nchw_to_halo(src.data_ptr(), B, Cs, H, W, dst.data_ptr(), cs, c0, p1, p2, MODES[mode], stream(dev))), what
        sync(dev)
        assert same(dst, fill), what + ": the refused call launched something"


# ---------------------------------------------------------------------------------------------------------------- tap_gather
def rowmajor(k):
    return tuple((t // k, t % k) for t in range(k * k))


def square(B, k, OH, OW, crop, q_cs):
    return (B, OH, OW, crop, q_cs, rowmajor(k))


CROSS = ((0, 1), (1, 0), (1, 1), (1, 2), (2, 1))
# (B, OH, OW, crop, q_cs, taps)
GATHER_CASES = [
    square(2, 7, 40, 40, 0, 52), square(2, 4, 31, 31, 0, 16), square(1, 7, 9, 37, 1, 52), square(1, 4, 1, 1, 0, 16),
    square(1, 7, 63, 65, 0, 52),                                                 # 4095 outputs: still the window kernel
    square(1, 7, 64, 64, 0, 52),                                                 # 4096 outputs: the rows kernel
    square(3, 4, 67, 80, 0, 16), square(2, 7, 70, 70, 3, 52), square(1, 7, 33, 125, 0, 52),
    (1, 70, 70, 0, 8, CROSS), (1, 70, 70, 0, 52, rowmajor(7)[::-1]),
    square(1, 8, 70, 70, 0, 64), (1, 70, 70, 0, 64, rowmajor(8)[::-1]),
    (1, 70, 70, 0, 68, rowmajor(8)[::-1]),                                       # 161 460 bytes of LDS: fits (see the docstring)
]
GATHER_ROUTES = ["window"] * 5 + ["rows"] * 4 + ["window", "window", "rows", "window", "window"]


def gather_id(case):
    B, OH, OW, crop, q_cs, taps = case
    kind = "rowmajor" if taps == rowmajor(int(math.isqrt(len(taps)))) else "cross" if taps == CROSS else "reversed"
    return f"B{B}-{OH}x{OW}-crop{crop}-cs{q_cs}-{len(taps)}{kind}"


def gather_extent(taps):
    return 1 + max(dh for dh, _ in taps), 1 + max(dw for _, dw in taps)


def gather_window_bytes(case):
    kh, kw = gather_extent(case[5])
    return (8 + kh - 1) * (32 + kw - 1) * (case[4] | 1) * 4


def gather_route(case):
    """the dispatcher's condition (include/nirgan_hip.h): full row-major k x k list on a map of >= 4096 outputs -> rows kernel"""
    B, OH, OW, crop, q_cs, taps = case
    kh, kw = gather_extent(taps)
    if kh == kw and taps == rowmajor(kw) and (OH - 2 * crop) * (OW - 2 * crop) >= 4096:
        return "rows"
    assert gather_window_bytes(case) <= 160 * 1024
    return "window"


assert [gather_route(c) for c in GATHER_CASES] == GATHER_ROUTES
assert all(GATHER_ROUTES.count(r) >= 3 for r in ("window", "rows"))
assert gather_window_bytes(GATHER_CASES[-1]) == 161460 and gather_window_bytes((1, 70, 70, 0, 72, rowmajor(8)[::-1])) > 160 * 1024


def gather_k(case, with_bias):
    taps = case[5]
    if gather_route(case) == "rows":
        k = gather_extent(taps)[0]
        return 2 * k - 1 if with_bias else 2 * k - 2
    return len(taps) if with_bias else len(taps) - 1


@functools.lru_cache(maxsize=None)
def gather_case(case):
    B, OH, OW, crop, q_cs, taps = case
    kh, kw = gather_extent(taps)
    qh, qw, H2, W2, nt = OH + kh - 1, OW + kw - 1, OH - 2 * crop, OW - 2 * crop, len(taps)
    gen = torch.Generator().manual_seed(63)
    q = torch.randn(B, qh, qw, q_cs, generator=gen) / math.sqrt(nt)
    q[..., nt:] = float("nan")                          # planes t >= ntaps must not be read into the result
    bias = 0.05 + 0.1 * torch.rand(1, generator=gen)
    z, A = torch.zeros(B, H2, W2, dtype=torch.float64), torch.zeros(B, H2, W2, dtype=torch.float64)
    for t, (dh, dw) in enumerate(taps):
        term = q[:, crop + dh:crop + dh + H2, crop + dw:crop + dw + W2, t].double()
        z, A = z + term, A + term.abs()
    return {"q": q, "bias": bias, "z": z, "A": A}


def gather_ref(case, act, with_bias):
    c = gather_case(case)
    b = c["bias"].double().item() if with_bias else 0.0
    z, bound = c["z"] + b, gather_k(case, with_bias) * U * (c["A"] + abs(b))
    if act == "tanh":
        ref = torch.tanh(z)
        return ref, tanh_bound(ref, bound)
    return z, bound


def gather_conditions_hold(case):
    c = gather_case(case)
    assert tanh_informative(c["z"]) and tanh_informative(c["z"] + c["bias"].double()), f"{case}: tanh would saturate"
    assert torch.isnan(c["q"][..., len(case[5]):]).all() and torch.isfinite(c["q"][..., :len(case[5])]).all()


def gather_desc(case, q, bias, act, dst):
    B, OH, OW, crop, q_cs, taps = case
    kh, kw = gather_extent(taps)
    d = L.TapGatherDesc()
    d.q, d.q_hp, d.q_wp, d.q_cs, d.ntaps = q.data_ptr(), OH + kh - 1, OW + kw - 1, q_cs, len(taps)
    for t, (dh, dw) in enumerate(taps):
        d.tap_dh[t], d.tap_dw[t] = dh, dw
    d.bias, d.act = None if bias is None else bias.data_ptr(), L.ACT_TANH if act == "tanh" else L.ACT_NONE
    d.B, d.OH, d.OW, d.crop, d.dst = B, OH, OW, crop, dst.data_ptr()
    return d


def gather_against_float64(dev, case):
    B, OH, OW, crop, q_cs, taps = case
    c, n = gather_case(case), B * (OH - 2 * crop) * (OW - 2 * crop)
    q, bias = c["q"].to(dev), c["bias"].to(dev)
    fam = "tap_gather " + gather_route(case)
    for with_bias in (True, False):
        got = {}
        for act in ("none", "tanh"):
            buf, dst = guarded(n, dev)
            L.call("nirgan_tap_gather", C.byref(gather_desc(case, q, bias if with_bias else None, act, dst)), stream(dev))
            sync(dev)
            within(fam if act == "none" else fam + " tanh", f"{gather_id(case)} bias {with_bias}", dst, *gather_ref(case, act, with_bias))
            assert guard_intact(buf), "tap_gather wrote outside its output"
            got[act] = dst
        note_tanhf(gather_id(case), got["tanh"], got["none"])


def gather_eager32(case, act, with_bias):
    """the same sum in eager fp32 torch, in the kernel's tap order"""
    B, OH, OW, crop, q_cs, taps = case
    c, H2, W2 = gather_case(case), OH - 2 * crop, OW - 2 * crop
    s = (c["bias"] if with_bias else torch.zeros(1)).expand(B, H2, W2).clone()
    for t, (dh, dw) in enumerate(taps):
        s = s + c["q"][:, crop + dh:crop + dh + H2, crop + dw:crop + dw + W2, t]
    return torch.tanh(s) if act == "tanh" else s


def gather_reference_alone(case):
    for with_bias in (True, False):
        for act in ("none", "tanh"):
            within("eager tap_gather", f"{gather_id(case)} {act} bias {with_bias}", gather_eager32(case, act, with_bias),
                   *gather_ref(case, act, with_bias))


GATHER_GUARDS = {"ntaps > q_cs": {"q_cs": 48}, "q_cs % 4 != 0": {"q_cs": 50}, "a tap past q_hp": {"tap": (7, 6)},
                 "OH <= 2 crop": {"crop": 5}}


def gather_guards(dev):
    be = L.backend()
    case = square(1, 7, 9, 37, 1, 52)
    q = torch.zeros(1, 9 + 6, 37 + 6, 52).to(dev)
    for what, change in GATHER_GUARDS.items():
        dst = nan(9 * 37, dev=dev)
        d = gather_desc(case, q, None, "none", dst)
        for k, v in change.items():
            if k == "tap":
                d.tap_dh[48], d.tap_dw[48] = v
            else:
                setattr(d, k, v)
        assert fails(be.nirgan_tap_gather(C.byref(d), stream(dev))), what
        sync(dev)
        assert torch.isnan(dst).all(), what + ": the refused call launched something"
    case = (1, 70, 70, 0, 72, rowmajor(8)[::-1])
    q, dst = torch.zeros(1, 77, 77, 72).to(dev), nan(70 * 70, dev=dev)
    assert fails(be.nirgan_tap_gather(C.byref(gather_desc(case, q, None, "none", dst)), stream(dev))) and b"LDS" in be.nirgan_last_error()
    sync(dev)
    assert torch.isnan(dst).all(), "the window that does not fit was launched"


# ---------------------------------------------------------------------------------------------------------------- conv_channel_dgrad
# (B, H, W, C, k, stride, pad, cin, channel, dy_pad)
DGRAD_CASES = [
    (2, 21, 25, 64, 4, 2, 1, 4, 3, 1), (1, 7, 9, 8, 4, 2, 1, 4, 0, 0), (2, 12, 10, 32, 3, 1, 1, 4, 2, 1), (1, 13, 13, 16, 7, 1, 3, 2, 1, 2),
    (1, 9, 9, 8, 1, 1, 0, 1, 0, 0), (1, 20, 20, 8, 5, 3, 2, 3, 1, 1),
    (2, 181, 183, 8, 4, 2, 1, 4, 3, 1),                 # 66 246 pixels > 4096 blocks x 16: the grid stride
    (1, 6, 8, 928, 4, 2, 1, 4, 3, 1),                   # even, but 16 C + 1600 floats > 64 KB: generic
    (1, 2, 2, 8, 4, 2, 1, 4, 3, 1), (2, 18, 34, 64, 4, 2, 1, 4, 3, 1),
    (1, 6, 8, 924, 4, 2, 1, 4, 3, 1),                   # exactly 64 KB of LDS: k4s2
    (9, 496, 496, 8, 4, 2, 1, 4, 3, 1),                 # 8649 tiles > the cap of 8192 blocks
]
DGRAD_ROUTES = ["generic"] * 8 + ["k4s2"] * 4
DGRAD_GRID_CAP = DGRAD_CASES[-1]
assert 2 * 181 * 183 > 4096 * 16 and 9 * 31 * 31 > 8192


def dgrad_out_hw(case):
    B, H, W, Cc, k, s, p, cin, ch, dp = case
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def dgrad_route(case):
    """the dispatcher's condition (include/nirgan_hip.h)"""
    B, H, W, Cc, k, s, p, cin, ch, dp = case
    OH, OW = dgrad_out_hw(case)
    if k == 4 and s == 2 and p == 1 and H == 2 * OH and W == 2 * OW and (16 * Cc + 1600) * 4 <= 65536:
        return "k4s2"
    assert k <= 7 and k * k * Cc * 4 <= 65536
    return "generic"


assert [dgrad_route(c) for c in DGRAD_CASES] == DGRAD_ROUTES
assert all(DGRAD_ROUTES.count(r) >= 3 for r in ("generic", "k4s2"))
assert (16 * 924 + 1600) * 4 == 65536


def dgrad_k(case):
    B, H, W, Cc, k, s, p, cin, ch, dp = case
    if dgrad_route(case) == "k4s2":
        return Cc + 4
    return 4 + (-(-k // s)) ** 2 * -(-(Cc // 4) // 16) + 4


def dgrad_through(x, w, dy, case):
    B, H, W, Cc, k, s, p, cin, ch, dp = case
    x = x.clone().requires_grad_(True)
    F.conv2d(x, w[:, ch:ch + 1], stride=s, padding=p).backward(dy.permute(0, 3, 1, 2))
    return x.grad[:, 0]


@functools.lru_cache(maxsize=2)
def dgrad_case(case):
    B, H, W, Cc, k, s, p, cin, ch, dp = case
    OH, OW = dgrad_out_hw(case)
    gen = torch.Generator().manual_seed(65)
    w = torch.randn(Cc, cin, k, k, generator=gen) / math.sqrt((-(-k // s)) ** 2 * Cc)
    dy = torch.randn(B, OH, OW, Cc, generator=gen)
    zero = torch.zeros(B, 1, H, W, dtype=torch.float64)
    ref = dgrad_through(zero, w.double(), dy.double(), case)
    A = dgrad_through(zero, w.double().abs(), dy.double().abs(), case)
    return {"w": w, "dy": dy, "ref": ref, "bound": dgrad_k(case) * U * A}


def dgrad_desc(case, dyh, w, out):
    B, H, W, Cc, k, s, p, cin, ch, dp = case
    OH, OW = dgrad_out_hw(case)
    d = L.ChanDgradDesc()
    d.dy, d.dy_hp, d.dy_wp, d.dy_pad, d.C = dyh.data_ptr(), OH + 2 * dp, OW + 2 * dp, dp, Cc
    d.w, d.cin, d.k, d.stride, d.pad, d.channel = w.data_ptr(), cin, k, s, p, ch
    d.B, d.H, d.W, d.out = B, H, W, out.data_ptr()
    return d


def dgrad_against_float64(dev, case):
    B, H, W, Cc, k, s, p, cin, ch, dp = case
    OH, OW = dgrad_out_hw(case)
    c = dgrad_case(case)
    dyh = nan(B, OH + 2 * dp, OW + 2 * dp, Cc)                  # the halo must never reach the output
    dyh[:, dp:dp + OH, dp:dp + OW] = c["dy"]
    dyh, w = dyh.to(dev), c["w"].to(dev)
    buf, out = guarded(B * H * W, dev)
    L.call("nirgan_conv_channel_dgrad", C.byref(dgrad_desc(case, dyh, w, out)), stream(dev))
    sync(dev)
    within("chan_dgrad " + dgrad_route(case), str(case), out, c["ref"], c["bound"])
    assert guard_intact(buf), "conv_channel_dgrad wrote outside its output"


def dgrad_reference_alone(case):
    c = dgrad_case(case)
    B, H, W = case[:3]
    got = dgrad_through(torch.zeros(B, 1, H, W), c["w"], c["dy"], case)
    within("eager chan_dgrad", str(case), got, c["ref"], c["bound"])


def dgrad_guards(dev):
    be = L.backend()
    base = (1, 7, 9, 8, 4, 2, 1, 4, 0, 1)
    for what, case, change in (("C % 4 != 0", base, {"C": 6}), ("channel >= cin", base, {"channel": 4}),
                               ("wrong dy_hp", base, {"dy_hp": dgrad_out_hw(base)[0] + 3}),
                               ("k = 8", (1, 9, 9, 8, 8, 1, 0, 1, 0, 1), {}), ("k = 7, C = 512", (1, 9, 9, 512, 7, 1, 3, 1, 0, 1), {})):
        B, H, W, Cc, k, s, p, cin, ch, dp = case
        OH, OW = dgrad_out_hw(case)
        dyh, w, out = torch.zeros(B, OH + 2 * dp + 1, OW + 2 * dp, Cc).to(dev), torch.zeros(Cc, cin, k, k).to(dev), nan(B * H * W, dev=dev)
        d = dgrad_desc(case, dyh, w, out)
        for f, v in change.items():
            setattr(d, f, v)
        assert fails(be.nirgan_conv_channel_dgrad(C.byref(d), stream(dev))), what
        sync(dev)
        assert torch.isnan(out).all(), what + ": the refused call launched something"
    assert b"LDS" in be.nirgan_last_error()


# ---------------------------------------------------------------------------------------------------------------- endconv
END_CASES = [(1, 1, 1, 0), (1, 4, 64, 0), (1, 5, 65, 0), (2, 9, 10, 1), (2, 9, 11, 1), (3, 5, 130, 2), (1, 3, 70, 1)]
END_NULLS = (2, 9, 10, 1)       # here also bias = NULL, and gbias = NULL
GB0 = 0.25
WS_MARK = 9.0


def end_variants(case):
    full = [(act, True, True) for act in ("none", "tanh")]
    if case == END_NULLS:
        full += [(act, wb, wg) for act in ("none", "tanh") for wb, wg in ((False, True), (True, False))]
    return full


def end_dz_geometry(case):
    B, OH, OW, crop = case
    return OH + 12, (OW + 12 + 3) // 4 * 4 + 8


def end_wgrad_grid(case):
    B, OH, OW, crop = case
    x_hp, x_wp = OH + 6, OW + 6
    blocks = min((B * x_hp + 3) // 4, 512)
    npair = (x_wp + 1) // 2
    units = B * x_hp * -(-npair // 8)
    return blocks, units, npair, -(-npair // 8)


assert [end_wgrad_grid(c)[2:] for c in ((2, 9, 10, 1), (2, 9, 11, 1))] == [(8, 1), (9, 2)]


def end_through(x, w, cot):
    """the adjoint of the 7x7 convolution at cotangent ``cot`` on the full OH x OW map: (gx as NHWC, gw [64][7][7])"""
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    F.conv2d(x, w).backward(cot)
    return x.grad.permute(0, 2, 3, 1), w.grad[0]


@functools.lru_cache(maxsize=None)
def end_inputs(case):
    B, OH, OW, crop = case
    H2, W2 = OH - 2 * crop, OW - 2 * crop
    gen = torch.Generator().manual_seed(67)
    x = torch.randn(B, OH + 6, OW + 6, 64, generator=gen)
    w = torch.randn(1, 64, 7, 7, generator=gen) / 56.0                # sqrt(3136): a pre-activation of unit scale
    bias = 0.05 + 0.1 * torch.rand(1, generator=gen)
    dout = torch.randn(B, H2, W2, generator=gen)
    x64, w64 = x.double().permute(0, 3, 1, 2).contiguous(), w.double()
    sl = (slice(None), 0, slice(crop, OH - crop), slice(crop, OW - crop))
    return {"x": x, "w": w, "bias": bias, "dout": dout, "x64": x64, "w64": w64, "z": F.conv2d(x64, w64)[sl],
            "Az": F.conv2d(x64.abs(), w64.abs())[sl]}


@functools.lru_cache(maxsize=None)
def end_case(case, act, with_bias):
    B, OH, OW, crop = case
    c = end_inputs(case)
    b = c["bias"].double().item() if with_bias else 0.0
    d64 = c["dout"].double()
    z, bz = c["z"] + b, (49 + 6 + (1 if with_bias else 0)) * U * (c["Az"] + abs(b))
    rows, S = end_dz_geometry(case)
    n = B * rows * S
    g = min(-(-n // 256), 1024)
    kgb = -(-n // (256 * g)) + 8 + -(-g // 256) + 8 + 1
    if act == "tanh":
        y = torch.tanh(z)
        by = tanh_bound(y, bz)
        dz, adz = d64 * (1 - y * y), d64.abs() * (1 + y * y)
        bdz = 3 * U * adz + 2 * (y * d64).abs() * by
        bgb = (3 + kgb) * U * (GB0 + adz.sum()) + bdz.sum()
    else:
        y, by, dz, bdz = z, bz, d64, torch.zeros_like(d64)
        bgb = kgb * U * (GB0 + d64.abs().sum())
    full = lambda t: F.pad(t, (crop,) * 4)[:, None]
    gx, gw = end_through(c["x64"], c["w64"], full(dz))
    Ax, Aw = end_through(c["x64"].abs(), c["w64"].abs(), full(dz.abs()))
    Ex, Ew = end_through(c["x64"].abs(), c["w64"].abs(), full(bdz))
    blocks, units, _, _ = end_wgrad_grid(case)
    kw = 16 * -(-units // (4 * blocks)) + 4 + -(-blocks // 16) + 16
    img, bimg = (torch.zeros(B, rows, S, dtype=torch.float64) for _ in range(2))
    win = (slice(None), slice(6 + crop, 6 + crop + OH - 2 * crop), slice(6 + crop, 6 + crop + OW - 2 * crop))
    img[win], bimg[win] = dz, bdz
    return {"y": y, "by": by, "z": z, "img": img, "bimg": bimg, "gb": GB0 + dz.sum(), "bgb": bgb,
            "gx": gx, "bgx": 50 * U * Ax + Ex, "gw": gw, "bgw": kw * U * Aw + Ew}


def end_conditions_hold(case):
    c = end_inputs(case)
    if c["z"].numel() >= 100:
        assert tanh_informative(c["z"]) and tanh_informative(c["z"] + c["bias"].double()), f"{case}: tanh would saturate"
    else:
        assert c["z"].abs().max() < 3.5


def end_sizes_hold(case):
    """the two size entries of the installed backend: dz_elems is the header's closed form, ws_elems covers the emulator's figure"""
    B, OH, OW, crop = case
    be = L.backend()
    rows, S = end_dz_geometry(case)
    assert be.nirgan_endconv_dz_elems(B, OH, OW) == B * rows * S
    assert be.nirgan_endconv_ws_elems(B, OH, OW) >= EmuBackend().nirgan_endconv_ws_elems(B, OH, OW) >= end_wgrad_grid(case)[0] * 49 * 64 + 1024


def end_against_float64(dev, case):
    B, OH, OW, crop = case
    be, st, c = L.backend(), stream(dev), end_inputs(case)
    end_sizes_hold(case)
    hp, wp, H2, W2 = OH + 6, OW + 6, OH - 2 * crop, OW - 2 * crop
    x, bias, dout = c["x"].to(dev), c["bias"].to(dev), c["dout"].to(dev)
    wt = c["w"][0].permute(1, 2, 0).reshape(49, 64).contiguous().to(dev)            # [t][c], the tap-plane forward pack
    outs = {}
    for act, with_bias, with_gbias in end_variants(case):
        r = end_case(case, act, with_bias)
        what = f"{case} {act} bias {with_bias} gbias {with_gbias}"
        fam = "endconv" if act == "none" else "endconv tanh"
        obuf, out = guarded(B * H2 * W2, dev)
        dz = torch.full((be.nirgan_endconv_dz_elems(B, OH, OW),), 3.0, device=dev)   # stale contents: the kernel rewrites the border
        ws = torch.full((be.nirgan_endconv_ws_elems(B, OH, OW),), WS_MARK, device=dev)
        gx, gw, gb = torch.full((B, hp, wp, 64), 5.0, device=dev), torch.full((64 * 49,), 5.0, device=dev), torch.full((1,), GB0, device=dev)
        d = L.EndConvDesc()
        d.x, d.x_hp, d.x_wp, d.B, d.OH, d.OW, d.crop, d.C, d.k = x.data_ptr(), hp, wp, B, OH, OW, crop, 64, 7
        d.w, d.bias, d.act = wt.data_ptr(), bias.data_ptr() if with_bias else None, L.ACT_TANH if act == "tanh" else L.ACT_NONE
        d.out, d.dout, d.dz, d.dz_elems = out.data_ptr(), dout.data_ptr(), dz.data_ptr(), dz.numel()
        d.gx, d.gw, d.gbias, d.ws, d.ws_elems = gx.data_ptr(), gw.data_ptr(), gb.data_ptr() if with_gbias else None, ws.data_ptr(), ws.numel()
        L.call("nirgan_endconv_fwd", C.byref(d), st)
        sync(dev)
        within(fam + " fwd", what, out, r["y"], r["by"])
        assert guard_intact(obuf), "endconv_fwd wrote outside its output"
        if with_bias:
            outs[act] = out
        # refused: a dz image or a partials workspace one float short
        d.dz_elems -= 1
        assert fails(be.nirgan_endconv_dz(C.byref(d), st))
        d.dz_elems += 1
        d.ws_elems -= 1
        assert fails(be.nirgan_endconv_wgrad(C.byref(d), st)) and (not with_gbias or fails(be.nirgan_endconv_dz(C.byref(d), st)))
        d.ws_elems += 1
        sync(dev)
        assert (dz == 3.0).all() and (ws == WS_MARK).all() and (gw == 5.0).all() and gb.item() == GB0, "a refused call launched something"
        L.call("nirgan_endconv_dz", C.byref(d), st)
        sync(dev)
        within(fam + " dz", what, dz, r["img"], r["bimg"])
        if with_gbias:
            within(fam + " gbias", what, gb[0], r["gb"], r["bgb"])
        else:
            assert gb.item() == GB0 and (ws == WS_MARK).all(), what + ": the dz launch without gbias touched the accumulator or the partials"
        L.call("nirgan_endconv_wgrad", C.byref(d), st)
        L.call("nirgan_endconv_dgrad", C.byref(d), st)
        sync(dev)
        within(fam + " dgrad", what, gx, r["gx"], r["bgx"])
        within(fam + " wgrad", what, gw.reshape(64, 7, 7), r["gw"], r["bgw"])
        gw2 = torch.zeros_like(gw)                      # a second launch gives the same bits (fixed summation order)
        d.gw = gw2.data_ptr()
        L.call("nirgan_endconv_wgrad", C.byref(d), st)
        sync(dev)
        assert same(gw2, gw), what + ": the weight gradient is not reproducible"
        d.C = 32
        assert be.nirgan_endconv_fwd(C.byref(d), st) == -1 and b"Conv2d(64, 1, 7)" in be.nirgan_last_error()
    note_tanhf(str(case), outs["tanh"], outs["none"])


def end_reference_alone(case):
    """eager fp32 torch: conv2d, tanh and their autograd"""
    B, OH, OW, crop = case
    c = end_inputs(case)
    for act, with_bias in sorted({v[:2] for v in end_variants(case)}):
        r = end_case(case, act, with_bias)
        x = c["x"].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        w, b = c["w"].clone().requires_grad_(True), c["bias"].clone().requires_grad_(True)
        z = F.conv2d(x, w, b if with_bias else None)[:, 0, crop:OH - crop, crop:OW - crop]
        y = torch.tanh(z) if act == "tanh" else z
        y.backward(c["dout"])
        what = f"{case} {act} bias {with_bias}"
        within("eager endconv", what + " fwd", y, r["y"], r["by"])
        within("eager endconv", what + " dgrad", x.grad.permute(0, 2, 3, 1), r["gx"], r["bgx"])
        within("eager endconv", what + " wgrad", w.grad[0], r["gw"], r["bgw"])
        if with_bias:
            within("eager endconv", what + " gbias", GB0 + b.grad[0], r["gb"], r["bgb"])
        dz = c["dout"] * (1 - y.detach() * y.detach()) if act == "tanh" else c["dout"]
        rows, S = end_dz_geometry(case)
        img = torch.zeros(B, rows, S)
        img[:, 6 + crop:6 + OH - crop, 6 + crop:6 + OW - crop] = dz
        within("eager endconv", what + " dz", img, r["img"], r["bimg"])
