"""Bodies shared by tests/test_streaming_emulated.py (numpy emulator, CPU) and tests/test_gpu_streaming.py (MI355X): the flat fp32
kernels of csrc/elementwise.hip (inject, bilinear, colsum, param_scale, fill, axpy, adam), csrc/losses.hip (lsgan, pix_loss) and the
tap adjoint of csrc/layout.hip (tap_scatter), each raw entry against float64.

Every body takes ``dev`` ("cpu": the installed backend is an EmuBackend) and drives the entry through ``L.call`` / ``L.check``.
Every expected value is float64 torch from the operation's definition (the header comment of include/nirgan_hip.h and the reference
lines it cites; ``F.interpolate(mode="bilinear", align_corners=False)`` and its autograd for the resize; autograd through
``O.rs_index_pairs``, the float64 restatement of utils/remote_sensing_indices.py, for the loss gradients).  Nothing is expected from
the emulator or from a kernel.

Bounds.  u = 2^-24 (fp32 unit roundoff).  Every element is held to ``K * u * A``: A is the float64 sum of the absolute values of
the terms the element adds up, K the number of rounded operations on the longest chain to it (first-order running error analysis:
a sum of n terms in ANY association is within (adds on the deepest path) * u * sum|terms|).  A division counts 3 and a square root 2
(HIP documents them to 2.5 and 1 ulp when not correctly rounded); a contraction to an FMA only removes roundings.  Per family:

inject_fwd    multiply + scale: s*e, 1 +, z * -> K = 3, A = |z| (1 + |s e|).  multiply, no scale: z * e -> K = 1, A = |z e|.
              add: s*e, z + -> K = 2, A = |z| + |s e|.  The ReLU is exact given the sign (input condition: |pre| >= 1e-4).
inject_bwd    dz = gm * (1 + s e): K = 3, A = |gm| (1 + |s e|); gm * e: K = 1; add: dz = gm, K = 0 (bitwise).
              de = sum_c gm z s: two products, then the kernel's adds: a thread adds its 4 * ceil((C/4) / q4) channels, lane 0 of
              the pixel adds the q4 partial sums in LDS (q4 = min(C/4, 256)): K = 2 + 4 ceil((C/4)/q4) + q4, A = sum_c |gm z s|.
              dscale += sum gm z e: two products, T = ceil(npix / (g ppi)) * 4 ceil((C/4)/q4) adds per thread (g blocks of ppi = 256/q4
              pixels), wave sum 6, four waves 2, the finish kernel ceil(g/256) + 6 + 2, the add into dscale 1:
              K = 2 + T + 8 + ceil(g/256) + 8 + 1, A = |dscale before| + sum |gm z e|.
bilinear_fwd  the value: 1 - lw, * s, +, 1 - lh and its product (2), + -> K = 6, A = the float64 resize of |src|.  The source
              coordinate: scale = fl(S / O) (u S), fl(scale * (o + .5)) (u S; the - 0.5 and the - i0 are exact): |d lambda| <=
              2 u scale (o + .5), each of the two only where the quantity is not an fp32 number to begin with.  The resize is piecewise linear in the coordinate with the neighbour differences as slopes, so the
              coordinate costs 2 u scale_h (oh + .5) * Dh + the same in w, Dh / Dw the largest vertical / horizontal neighbour
              difference of src in the 5 x 5 cells around (h0, w0) (a coordinate that crosses an integer lands in the next cell).
bilinear_bwd  coefficient ch = (1 - lh) (+ lh at the clamped end): 2, cw: 2, ch * cw, * d: 2, then one add per non-zero
              contribution: K = 6 + nnz_h(h) nnz_w(w), A = M_h^T |d| M_w (M the 1-D float64 resize matrices).  Every coefficient is a
              hat function of the coordinate (1-Lipschitz): the coordinate costs E_h^T |d| M_w + M_h^T |d| E_w with E[o][j] =
              2 u scale (o + .5) on the rows j = i0 - 1 .. i0 + 2 the coordinate can touch.
              The project's bounds for the resize (1e-6 forward, 1e-5 backward, max-norm relative to max |ref|, in
              test_gpu_kernels.py) are against fp32 torch, which rounds the coordinate exactly as the kernel does; against float64
              that rounding is visible (1e-5 of max |ref| at 128 -> 52 x 36 in eager fp32 torch), so it is in the bound here.  Where
              the coordinate is exact (128 -> 256, 128, 64) the bound here is asserted to lie below 1e-6 / 1e-5 of max |ref|, and the
              fp32-torch comparison at 1e-6 / 1e-5 is kept for EVERY case, so that no case is held more loosely than before.
adjoint       |<fwd x, d> - <x, bwd d>| <= sum |d| bound_fwd + sum |x| bound_bwd (float64 products of the device outputs).
colsum        a lane adds ceil(rows / 64) rows into each of 4 partial sums (+ 3 tail rows into the first), combines them (2), lane 0
              adds the 16 lanes, accumulate adds 1: K = ceil(rows/64) + 3 + 2 + 16 + 1, A = |out before| + sum_r |x|.
param_scale   out = x c, gx = g c: K = 1.  dparam += sum g x: 1 product, ceil(n / (256 g)) adds per thread, then as dscale:
              K = 1 + ceil(n/(256 g)) + 8 + ceil(g/256) + 8 + 1, A = |dparam before| + sum |g x|.
fill / axpy   bitwise against fp32 torch (alpha = -0.5: the product is exact, so the fused and the two-step forms agree); a second
              alpha, -0.37: alpha x, y + -> K = 2, A = |y| + |alpha x|.
adam          three steps; the error bounds of m, v, p are carried along in float64 with the rule above (m: 3 u (|b1 m| + |(1-b1) g|);
              v: 3 u (b2 v + (1-b2) g^2); denom = sqrt(v) c + eps: sqrt 2, *, + -> 4 u denom + c E_v / (2 sqrt v); the update
              step * (m / denom): the two host constants 2, division 3, product 1 -> 6 u |upd| + its operands' errors; p: + u |p|).
              The float64 Adam takes b1, b2, eps, lr as the fp32 values the entry receives.
lsgan         loss += w mean (p - t)^2: p - t, square, 4 ceil(n / 4096) adds per thread, w * (1/n) and its product (3), wave 6,
              16 waves, the add into loss_out: K = 2 + 4 ceil(n/4096) + 3 + 6 + 16 + 1, A = |loss before| + w mean d^2.
              grad = w 2 d / n: p - t, w * 2, * d, 1/n, * -> K = 5, A = |grad|.
pix_loss      the index formulas and their closed-form derivatives (csrc/losses.hip) are replayed operation by operation on
              (value, error bound) pairs with the rule above, so that every subtraction of rounded quantities -- dp - (y - R),
              tp^2 - 8 (y - R), tp - sp, f - a -- carries its conditioning |operands' errors| / |result| exactly; 1e-6f differs from
              1e-6 by u 1e-6.  Operation counts to the index value: ndvi / ndwi 6, gndvi 10, savi 7, msavi 9, evi 9.  The sums: the
              terms' own bounds + K u (|sums before| + sum |term|), K = ceil(n / (256 g)) + 6 + 4 + ceil(g/256) + 8 + 1.  The values
              the pairs carry are asserted to equal the autograd gradient to 1e-11: the expectation is autograd's.
tap_scatter   dq = dout (1 - y^2): y y, 1 -, * -> K = 3, A = |dout| (1 + y^2) (act none: a copy, K = 0, bitwise); channels t >= ntaps
              exactly 0.  dbias += sum dz: 3 + 3 ceil(n / 4096) + 6 + 16 + 1, A = |dbias before| + sum |dout| (1 + y^2).  The gather's
              project bound (5e-6 max-norm) is looser than 3 u (1 + y^2) <= 3.6e-7 of |dout|.

Two CPU checks keep these honest (tests/test_streaming_emulated.py): eager fp32 torch of the same formula lies inside every bound, and
an emulator with one deliberate error fails the body.
"""
import ctypes as C
import functools
import math

import torch
import torch.nn.functional as F

import nirgan_oracle as O
from nirgan_hip import lib as L

U = 2.0 ** -24
DIV, SQRT = 3, 2
RATIOS = {}                     # family -> the worst err / bound this process has seen


def stream(dev):
    return torch.cuda.current_stream().cuda_stream if torch.device(dev).type == "cuda" else None


def sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same(a, b):
    """bitwise, NaN equal to NaN"""
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def nan(*shape, dev="cpu"):
    return torch.full(shape, float("nan"), device=dev)


def within(family, what, got, ref, bound):
    """every element of ``got`` within ``bound`` of float64 ``ref`` (bound 0: equal); prints the worst err / bound before it asserts"""
    got = torch.as_tensor(got).detach().double().cpu().reshape(ref.shape)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand(ref.shape)
    assert torch.isfinite(got).all(), f"{family} {what}: non-finite"
    err = (got - ref).abs()
    zero = bound == 0
    ratio = (err[~zero] / bound[~zero]).max().item() if (~zero).any() else 0.0
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)
    print(f"RATIO {family} | {what} | {ratio:.3e}")
    assert (err[zero] == 0).all(), f"{family} {what}: an element that must be exact differs by {err[zero].max().item():.3e}"
    assert ratio <= 1.0, f"{family} {what}: err / bound {ratio:.3e}"


def fails(rc):
    return rc != 0


# ---------------------------------------------------------------------------------------------------------------- injection
INJECT_SHAPES = [((1, 3, 5, 4), 0), ((2, 9, 7, 64), 1), ((1, 6, 5, 96), 3), ((2, 130, 129, 64), 0), ((2, 96, 100, 256), 1),
                 ((1, 2, 3, 1028), 3)]
INJECT_VARIANTS = {"multiply+scale": (0, 0.5), "multiply": (0, None), "add+scale": (1, 0.5)}
# 1 + 0.5 e stays positive on e in [-1.5, 1.5]; one more run with a scale of -0.8, where the factor does change sign
INJECT_CASES = [(s, p, v) for s, p in INJECT_SHAPES for v in INJECT_VARIANTS] + [((2, 9, 7, 64), 1, "multiply+scale-0.8")]
DSCALE0 = 3.0


def inject_variant(variant):
    if variant == "multiply+scale-0.8":
        return 0, -0.8
    return INJECT_VARIANTS[variant]


def inject_grid(shape):
    B, H, W, Cc = shape
    q4 = min(Cc // 4, 256)
    ppi = 256 // q4
    g = min(-(-B * H * W // ppi), 2048)
    return q4, ppi, g


@functools.lru_cache(maxsize=4)
def inject_case(shape, variant):
    """inputs, float64 expectation and bounds of a case; computed once, nobody writes to them"""
    B, H, W, Cc = shape
    style, s = inject_variant(variant)
    gen = torch.Generator().manual_seed(41)
    z = torch.randn(B, H, W, Cc, generator=gen)
    e = (0.05 + 1.45 * torch.rand(B, H, W, generator=gen)) * (torch.randint(0, 2, (B, H, W), generator=gen) * 2 - 1)
    g = torch.randn(B, H, W, Cc, generator=gen)
    s32 = None if s is None else torch.tensor([s], dtype=torch.float32)
    sv = 1.0 if s is None else s32.double().item()
    e64 = e.double()[..., None]

    def pre_of(z64):
        if style == 0:
            return z64 * ((1 + sv * e64) if s is not None else e64)
        return z64 + sv * e64
    z = torch.where(pre_of(z.double()).abs() < 2e-4, torch.ones_like(z), z)       # keep the pre-activation off the kink
    z64, g64 = z.double(), g.double()
    pre = pre_of(z64)
    gm = torch.where(pre > 0, g64, torch.zeros_like(g64))
    q4, ppi, blocks = inject_grid(shape)
    qtrips = -(-(Cc // 4) // q4)
    k_de = 2 + 4 * qtrips + q4
    k_ds = 2 + -(-B * H * W // (blocks * ppi)) * 4 * qtrips + 8 + -(-blocks // 256) + 8 + 1
    if style == 0 and s is not None:
        f = 1 + sv * e64
        ref = {"a": pre.clamp_min(0), "dz": gm * f, "de": (gm * z64 * sv).sum(-1), "dscale": DSCALE0 + (gm * z64 * e64).sum()}
        bound = {"a": 3 * U * z64.abs() * (1 + (sv * e64).abs()), "dz": 3 * U * gm.abs() * (1 + (sv * e64).abs()),
                 "de": k_de * U * (gm * z64 * sv).abs().sum(-1), "dscale": k_ds * U * (DSCALE0 + (gm * z64 * e64).abs().sum())}
    elif style == 0:
        ref = {"a": pre.clamp_min(0), "dz": gm * e64, "de": (gm * z64).sum(-1)}
        bound = {"a": U * pre.abs(), "dz": U * (gm * e64).abs(), "de": k_de * U * (gm * z64).abs().sum(-1)}
    else:
        ref = {"a": pre.clamp_min(0), "dz": gm, "de": (gm * sv).sum(-1), "dscale": DSCALE0 + (gm * e64).sum()}
        bound = {"a": 2 * U * (z64.abs() + (sv * e64).abs()), "dz": torch.zeros_like(gm), "de": k_de * U * (gm * sv).abs().sum(-1),
                 "dscale": k_ds * U * (DSCALE0 + (gm * e64).abs().sum())}
    return {"z": z, "e": e, "g": g, "scale": s32, "style": style, "pre": pre, "ref": ref, "bound": bound}


def inject_conditions_hold(shape, variant):
    c = inject_case(shape, variant)
    assert (c["pre"].abs() >= 1e-4).all()
    assert (c["pre"] > 0).any() and (c["pre"] < 0).any()
    assert c["e"].abs().max() <= 1.5 and c["e"].abs().min() >= 0.05 and (c["e"] > 0).any() and (c["e"] < 0).any()
    if c["e"].numel() > 100:
        assert c["e"].min() < -1.4 and c["e"].max() > 1.4
    if variant == "multiply+scale-0.8":
        f = 1 + c["scale"].double() * c["e"].double()
        assert (f > 0).any() and (f < 0).any()


def inject_eager32(shape, variant):
    """the same formulas in eager fp32 torch"""
    c = inject_case(shape, variant)
    z, e, g, s = c["z"], c["e"][..., None], c["g"], c["scale"]
    if c["style"] == 0:
        f = (1 + s * e) if s is not None else e
        a = torch.relu(z * f)
        gm = torch.where(a > 0, g, torch.zeros_like(g))
        out = {"a": a, "dz": gm * f, "de": (gm * z * (s if s is not None else 1.0)).sum(-1)}
        if s is not None:
            out["dscale"] = DSCALE0 + (gm * z * e).sum()
    else:
        a = torch.relu(z + s * e)
        gm = torch.where(a > 0, g, torch.zeros_like(g))
        out = {"a": a, "dz": gm, "de": (gm * s).sum(-1), "dscale": DSCALE0 + (gm * e).sum()}
    return out


def inject_against_float64(dev, shape, pad, variant):
    B, H, W, Cc = shape
    c = inject_case(shape, variant)
    be, st = L.backend(), stream(dev)
    z, e, g = (c[k].to(dev).contiguous() for k in ("z", "e", "g"))
    scale = None if c["scale"] is None else c["scale"].to(dev)
    hp, wp = H + 2 * pad, W + 2 * pad
    out = nan(B, hp, wp, Cc, dev=dev)
    d = L.InjectFwdDesc()
    d.z, d.e, d.scale, d.style = z.data_ptr(), e.data_ptr(), None if scale is None else scale.data_ptr(), c["style"]
    d.B, d.H, d.W, d.C, d.out, d.o_hp, d.o_wp, d.o_pad = B, H, W, Cc, out.data_ptr(), hp, wp, pad
    L.call("nirgan_inject_fwd", C.byref(d), st)
    sync(dev)
    inside = torch.zeros(hp, wp, dtype=torch.bool)
    inside[pad:pad + H, pad:pad + W] = True
    host = out.cpu()
    assert same(host[:, ~inside], nan(B, int((~inside).sum()), Cc)), "inject_fwd wrote into the halo"
    fam = "inject " + variant.split("-")[0]
    what = f"{shape} pad {pad}"
    within(fam, what + " a", host[:, pad:pad + H, pad:pad + W], c["ref"]["a"], c["bound"]["a"])
    # backward: a is the forward's own output, halo and all
    _, _, blocks = inject_grid(shape)
    dz, de = nan(B, H, W, Cc, dev=dev), nan(B, H, W, dev=dev)
    dscale = None if scale is None else torch.full((1,), DSCALE0, device=dev)
    ws = None if scale is None else torch.zeros(blocks, device=dev)
    b = L.InjectBwdDesc()
    b.g, b.a, b.a_hp, b.a_wp, b.a_pad, b.z, b.e = g.data_ptr(), out.data_ptr(), hp, wp, pad, z.data_ptr(), e.data_ptr()
    b.scale, b.style, b.B, b.H, b.W, b.C = d.scale, c["style"], B, H, W, Cc
    b.dz, b.de = dz.data_ptr(), de.data_ptr()
    if scale is not None:
        b.dscale, b.ws, b.ws_elems = dscale.data_ptr(), ws.data_ptr(), blocks - 1
        assert fails(be.nirgan_inject_bwd(C.byref(b), st)) and b"workspace" in be.nirgan_last_error()
        sync(dev)
        assert torch.isnan(dz).all() and torch.isnan(de).all() and dscale.item() == DSCALE0, "the refused call launched something"
        b.ws_elems = blocks
    else:
        b.dscale, b.ws, b.ws_elems = None, None, 0            # no scale: no dscale, and no workspace is needed
    L.call("nirgan_inject_bwd", C.byref(b), st)
    sync(dev)
    within(fam, what + " dz", dz, c["ref"]["dz"], c["bound"]["dz"])
    within(fam, what + " de", de, c["ref"]["de"], c["bound"]["de"])
    if scale is not None:
        within(fam, what + " dscale", dscale[0], c["ref"]["dscale"], c["bound"]["dscale"])


def inject_reference_alone(shape, variant):
    c, got = inject_case(shape, variant), inject_eager32(shape, variant)
    assert set(got) == set(c["ref"])
    for k, v in got.items():
        within("eager inject", f"{shape} {variant} {k}", v, c["ref"][k], c["bound"][k])


# ---------------------------------------------------------------------------------------------------------------- bilinear
BILINEAR_CASES = [((128, 128), (256, 256)), ((128, 128), (128, 128)), ((128, 128), (64, 64)), ((128, 128), (52, 36)),
                  ((7, 5), (1, 1)), ((1, 1), (5, 3)), ((2, 3), (300, 2)), ((5, 3), (3, 5)), ((128, 128), (25, 15))]
EXACT_COORDINATE = BILINEAR_CASES[:3]           # 2x, 1x, 1/2: scale * (o + .5) - .5 is exact in fp32
BILINEAR_B = (1, 3)


def resize_axis(S, Osz):
    """float64 1-D statement of the align_corners=False resize: matrix M [O][S], the coordinate's error matrix E, first index i0"""
    scale = S / Osz
    o = torch.arange(Osz, dtype=torch.float64)
    raw = scale * (o + 0.5)
    s = (raw - 0.5).clamp_min(0)
    i0 = s.floor().clamp_max(S - 1).long()
    i1 = (i0 + 1).clamp_max(S - 1)
    lam = s - i0
    M = torch.zeros(Osz, S, dtype=torch.float64)
    M[torch.arange(Osz), i0] += 1 - lam
    M[torch.arange(Osz), i1] += lam
    # fl(S / O) and fl(scale * (o + .5)) each cost u * raw, unless exact (the 2x, 1x and 1/2 resizes of the nets)
    scale32 = (torch.tensor(float(S), dtype=torch.float32) / torch.tensor(float(Osz), dtype=torch.float32)).double().item()
    prod = scale32 * (o + 0.5)                      # exact in float64: 24 bits times 10
    cs = U * raw * (float(scale32 != scale) + (prod.float().double() != prod).double())
    E = torch.zeros(Osz, S, dtype=torch.float64)
    for j in range(-1, 3):
        col = i0 + j
        ok = (col >= 0) & (col < S)
        E[torch.arange(Osz)[ok], col[ok]] = cs[ok]
    return M, E, i0, cs


@functools.lru_cache(maxsize=None)
def bilinear_case(src_hw, dst_hw, B):
    (SH, SW), (OH, OW) = src_hw, dst_hw
    gen = torch.Generator().manual_seed(43)
    x = torch.randn(B, SH, SW, generator=gen)
    d = torch.randn(B, OH, OW, generator=gen)
    x64 = x.double()[:, None].requires_grad_(True)
    y = F.interpolate(x64, size=(OH, OW), mode="bilinear", align_corners=False)
    y.backward(d.double()[:, None])
    Mh, Eh, h0, csh = resize_axis(SH, OH)
    Mw, Ew, w0, csw = resize_axis(SW, OW)
    ax = x.double().abs()
    A = torch.einsum("oh,bhw,pw->bop", Mh, ax, Mw)
    # largest neighbour difference in the 5 x 5 cells around (h0, w0)
    dv, dh = torch.zeros(B, SH, SW, dtype=torch.float64), torch.zeros(B, SH, SW, dtype=torch.float64)
    dv[:, :SH - 1] = (x.double()[:, 1:] - x.double()[:, :-1]).abs()
    dh[:, :, :SW - 1] = (x.double()[:, :, 1:] - x.double()[:, :, :-1]).abs()
    pool = lambda t: F.max_pool2d(t[:, None], 5, 1, 2)[:, 0][:, h0][:, :, w0]
    bound_f = csh[None, :, None] * pool(dv) + csw[None, None, :] * pool(dh) + 6 * U * A
    ad = d.double().abs()
    nnz = (Mh > 0).sum(0)[:, None] * (Mw > 0).sum(0)[None, :]
    bound_b = torch.einsum("oh,bop,pw->bhw", Eh, ad, Mw) + torch.einsum("oh,bop,pw->bhw", Mh, ad, Ew) + \
        (6 + nnz)[None] * U * torch.einsum("oh,bop,pw->bhw", Mh, ad, Mw)
    return {"x": x, "d": d, "fwd": y.detach()[:, 0], "bwd": x64.grad[:, 0], "bound_f": bound_f, "bound_b": bound_b, "Mh": Mh, "Mw": Mw}


def bilinear_eager32(src_hw, dst_hw, B):
    c = bilinear_case(src_hw, dst_hw, B)
    x = c["x"][:, None].clone().requires_grad_(True)
    y = F.interpolate(x, size=dst_hw, mode="bilinear", align_corners=False)
    y.backward(c["d"][:, None])
    return y.detach()[:, 0], x.grad[:, 0]


def bilinear_reference_alone(src_hw, dst_hw):
    for B in BILINEAR_B:
        c = bilinear_case(src_hw, dst_hw, B)
        # the matrices behind the bounds state the same resize as F.interpolate in float64
        assert (torch.einsum("oh,bhw,pw->bop", c["Mh"], c["x"].double(), c["Mw"]) - c["fwd"]).abs().max() <= 1e-12
        assert (torch.einsum("oh,bop,pw->bhw", c["Mh"], c["d"].double(), c["Mw"]) - c["bwd"]).abs().max() <= 1e-12
        y, gx = bilinear_eager32(src_hw, dst_hw, B)
        within("eager bilinear", f"{src_hw}->{dst_hw} B{B} fwd", y, c["fwd"], c["bound_f"])
        within("eager bilinear", f"{src_hw}->{dst_hw} B{B} bwd", gx, c["bwd"], c["bound_b"])
        if (src_hw, dst_hw) in EXACT_COORDINATE:          # never looser than the project's max-norm bounds where the coordinate is exact
            assert c["bound_f"].max() <= 1e-6 * c["fwd"].abs().max() and c["bound_b"].max() <= 1e-5 * c["bwd"].abs().max()


def bilinear_against_float64(dev, src_hw, dst_hw):
    (SH, SW), (OH, OW) = src_hw, dst_hw
    st = stream(dev)
    for B in BILINEAR_B:
        c = bilinear_case(src_hw, dst_hw, B)
        x, d = c["x"].to(dev), c["d"].to(dev)
        y, gx = nan(B, OH, OW, dev=dev), nan(B, SH, SW, dev=dev)
        L.call("nirgan_bilinear_fwd", x.data_ptr(), B, SH, SW, y.data_ptr(), OH, OW, st)
        L.call("nirgan_bilinear_bwd", d.data_ptr(), B, OH, OW, gx.data_ptr(), SH, SW, st)
        sync(dev)
        what = f"{src_hw}->{dst_hw} B{B}"
        within("bilinear_fwd", what, y, c["fwd"], c["bound_f"])
        within("bilinear_bwd", what, gx, c["bwd"], c["bound_b"])
        y64, g64, x64, d64 = y.double().cpu(), gx.double().cpu(), c["x"].double(), c["d"].double()
        lhs, rhs = (y64 * d64).sum(), (x64 * g64).sum()
        slack = (d64.abs() * c["bound_f"]).sum() + (x64.abs() * c["bound_b"]).sum()
        within("bilinear adjoint", what, lhs, rhs, slack)
        # the project's earlier bounds, against the reference they were set for (fp32 torch)
        y32, g32 = bilinear_eager32(src_hw, dst_hw, B)
        assert (y.cpu() - y32).abs().max() <= 1e-6 * max(y32.abs().max().item(), 1e-20), what
        assert (gx.cpu() - g32).abs().max() <= 1e-5 * max(g32.abs().max().item(), 1e-20), what


# ---------------------------------------------------------------------------------------------------------------- colsum
COLSUM_ROWS = (1, 2, 15, 16, 17, 63, 64, 65, 113, 1073)
COLSUM_COLS = (1, 63, 65, 200)
COLSUM_NET = (2, 16384)


def colsum_shapes(rows):
    return [COLSUM_NET] if rows == "net" else [(rows, c) for c in COLSUM_COLS]


@functools.lru_cache(maxsize=None)
def colsum_case(rows, cols):
    gen = torch.Generator().manual_seed(45)
    x, out0 = torch.randn(rows, cols, generator=gen), torch.randn(cols, generator=gen) * 3
    return x, out0


def colsum_ref(rows, cols, accumulate):
    x, out0 = colsum_case(rows, cols)
    k = -(-rows // 64) + 3 + 2 + 16 + 1
    base = out0.double() if accumulate else torch.zeros(cols, dtype=torch.float64)
    return base + x.double().sum(0), k * U * (base.abs() + x.double().abs().sum(0))


def colsum_against_float64(dev, rows):
    for r, cols in colsum_shapes(rows):
        x, out0 = colsum_case(r, cols)
        xd = x.to(dev)
        for accumulate in (0, 1):
            out = out0.to(dev).clone() if accumulate else nan(cols, dev=dev)
            L.call("nirgan_colsum", xd.data_ptr(), r, cols, out.data_ptr(), accumulate, stream(dev))
            sync(dev)
            within("colsum", f"{r} x {cols} accumulate {accumulate}", out, *colsum_ref(r, cols, accumulate))


def colsum_reference_alone(rows):
    for r, cols in colsum_shapes(rows):
        x, out0 = colsum_case(r, cols)
        within("eager colsum", f"{r} x {cols}", out0 + x.sum(0), *colsum_ref(r, cols, 1))
        within("eager colsum", f"{r} x {cols}", x.sum(0), *colsum_ref(r, cols, 0))


# ---------------------------------------------------------------------------------------------------------------- param_scale
PARAM_SCALE_N = (1, 255, 257, 65536, 524365)
DPARAM0 = -2.0


@functools.lru_cache(maxsize=None)
def param_scale_case(n):
    gen = torch.Generator().manual_seed(47)
    x, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    c = torch.tensor([0.8125 + 1 / 3], dtype=torch.float32)
    blocks = min(-(-n // 256), 1024)
    k = 1 + -(-n // (256 * blocks)) + 8 + -(-blocks // 256) + 8 + 1
    x64, g64, c64 = x.double(), g.double(), c.double()
    ref = {"out": x64 * c64, "gx": g64 * c64, "dparam": DPARAM0 + (g64 * x64).sum()}
    bound = {"out": U * ref["out"].abs(), "gx": U * ref["gx"].abs(), "dparam": k * U * (abs(DPARAM0) + (g64 * x64).abs().sum())}
    return x, g, c, blocks, ref, bound


def param_scale_against_float64(dev, n):
    x, g, c, blocks, ref, bound = param_scale_case(n)
    be, st = L.backend(), stream(dev)
    xd, gd, cd = x.to(dev), g.to(dev), c.to(dev)
    out, gx, dparam, ws = nan(n, dev=dev), nan(n, dev=dev), torch.full((1,), DPARAM0, device=dev), torch.zeros(blocks, device=dev)
    L.call("nirgan_param_scale_fwd", xd.data_ptr(), cd.data_ptr(), out.data_ptr(), n, st)
    assert fails(be.nirgan_param_scale_bwd(gd.data_ptr(), xd.data_ptr(), cd.data_ptr(), gx.data_ptr(), dparam.data_ptr(), ws.data_ptr(),
                                           blocks - 1, n, st))
    sync(dev)
    assert torch.isnan(gx).all() and dparam.item() == DPARAM0, "the refused call launched something"
    L.call("nirgan_param_scale_bwd", gd.data_ptr(), xd.data_ptr(), cd.data_ptr(), gx.data_ptr(), dparam.data_ptr(), ws.data_ptr(), blocks, n, st)
    sync(dev)
    for k, v in (("out", out), ("gx", gx), ("dparam", dparam[0])):
        within("param_scale", f"n {n} {k}", v, ref[k], bound[k])


def param_scale_reference_alone(n):
    x, g, c, _, ref, bound = param_scale_case(n)
    for k, v in (("out", x * c), ("gx", g * c), ("dparam", DPARAM0 + (g * x).sum())):
        within("eager param_scale", f"n {n} {k}", v, ref[k], bound[k])


# ---------------------------------------------------------------------------------------------------------------- fill / axpy
FLAT_N = (1, 257, 1048833)


def fill_axpy_against_torch(dev, n):
    gen = torch.Generator().manual_seed(49)
    x, y = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    st = stream(dev)
    buf = nan(n + 2, dev=dev)
    L.call("nirgan_fill", buf[1:].data_ptr(), n, -1.25, st)
    sync(dev)
    assert same(buf[1:n + 1], torch.full((n,), -1.25)) and torch.isnan(buf[0]) and torch.isnan(buf[n + 1])
    xd, yd = x.to(dev), y.to(dev).clone()
    L.call("nirgan_axpy", yd.data_ptr(), xd.data_ptr(), n, -0.5, st)
    sync(dev)
    assert same(yd, y + (-0.5) * x), "axpy, alpha -0.5"
    alpha = torch.tensor(-0.37, dtype=torch.float32)
    yd = y.to(dev).clone()
    L.call("nirgan_axpy", yd.data_ptr(), xd.data_ptr(), n, alpha.item(), st)
    sync(dev)
    ax = alpha.double() * x.double()
    within("axpy", f"n {n}", yd, y.double() + ax, 2 * U * (y.double().abs() + ax.abs()))
    within("eager axpy", f"n {n}", y + alpha * x, y.double() + ax, 2 * U * (y.double().abs() + ax.abs()))


# ---------------------------------------------------------------------------------------------------------------- adam
ADAM_N = (3, 4, 7, 2098355)
ADAM_HYPER = (2e-4, 0.5, 0.999, 1e-8)


@functools.lru_cache(maxsize=2)
def adam_case(n):
    """three steps of float64 Adam on the fp32 hyper-parameters the entry receives, with the running error bound of p"""
    gen = torch.Generator().manual_seed(51)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * 10.0 ** (5 * torch.rand(n, generator=gen) - 3) for _ in range(3)]
    lr, b1, b2, eps = (torch.tensor(v, dtype=torch.float32).double().item() for v in ADAM_HYPER)
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    Ep, Em, Ev = (torch.zeros(n, dtype=torch.float64) for _ in range(3))
    steps = []
    for t, g32 in enumerate(grads, start=1):
        g = g32.double()
        Em = b1 * Em + 3 * U * ((b1 * m).abs() + ((1 - b1) * g).abs())
        Ev = b2 * Ev + 3 * U * (b2 * v + (1 - b2) * g * g)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        c = 1 / math.sqrt(1 - b2 ** t)
        denom = v.sqrt() * c + eps
        Eden = c * Ev / (2 * v.sqrt()) + 4 * U * denom
        upd = (lr / (1 - b1 ** t)) * (m / denom)
        Eupd = (lr / (1 - b1 ** t)) * (Em / denom + m.abs() * Eden / denom ** 2) + 6 * U * upd.abs()
        p = p - upd
        Ep = Ep + Eupd + U * p.abs()
        steps.append((p.clone(), Ep.clone(), m.clone(), Em.clone(), v.clone(), Ev.clone()))
    return p0, grads, steps


def adam_conditions_hold(n):
    _, grads, steps = adam_case(n)
    g = torch.cat(grads).abs()
    if n > 1000:
        assert g.min() < 1e-3 and g.max() > 1e2
    assert all((v > 0).all() for _, _, _, _, v, _ in steps)


def adam_eager32(n):
    p0, grads, _ = adam_case(n)
    q = p0.clone().requires_grad_(True)
    lr, b1, b2, eps = ADAM_HYPER
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps)
    out = []
    for g in grads:
        q.grad = g.clone()
        opt.step()
        out.append(q.detach().clone())
    return out


def adam_against_float64(dev, n):
    p0, grads, steps = adam_case(n)
    guard = 4
    buf = [torch.zeros(n + 2 * guard, device=dev) for _ in range(3)]          # p, m, v with a guard band on either side
    p, m, v = (b[guard:guard + n] for b in buf)
    p.copy_(p0)
    lr, b1, b2, eps = ADAM_HYPER
    for t, g in enumerate(grads, start=1):
        gd = g.to(dev)
        L.call("nirgan_adam", p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, b1, b2, eps, t, stream(dev))
        sync(dev)
        rp, ep, rm, em, rv, ev = steps[t - 1]
        within("adam", f"n {n} step {t} m", m, rm, em)
        within("adam", f"n {n} step {t} v", v, rv, ev)
        within("adam", f"n {n} step {t} p", p, rp, ep)
    assert all((b[:guard] == 0).all() and (b[guard + n:] == 0).all() for b in buf), "adam wrote outside its n elements"


def adam_reference_alone(n):
    _, _, steps = adam_case(n)
    for t, q in enumerate(adam_eager32(n), start=1):
        within("eager adam", f"n {n} step {t}", q, steps[t - 1][0], steps[t - 1][1])


# ---------------------------------------------------------------------------------------------------------------- lsgan
LSGAN_N = (1, 1023, 4097, 14400)
LOSS0 = 0.75


@functools.lru_cache(maxsize=None)
def lsgan_case(n, target):
    gen = torch.Generator().manual_seed(53)
    pred = 0.5 + 0.5 * torch.randn(n, generator=gen)
    w = 0.5
    d = pred.double() - target
    k = 2 + 4 * -(-n // 4096) + 3 + 6 + 16 + 1
    loss = LOSS0 + w * (d * d).mean()
    grad = w * 2 * d / n
    return pred, w, loss, k * U * loss.abs(), grad, 5 * U * grad.abs()


def lsgan_against_float64(dev, n):
    for target in (0.0, 1.0):
        pred, w, loss, bl, grad, bg = lsgan_case(n, target)
        pd_ = pred.to(dev)
        for with_grad in (False, True):
            out, g = torch.full((1,), LOSS0, device=dev), nan(n, dev=dev)
            L.call("nirgan_lsgan", pd_.data_ptr(), n, target, w, out.data_ptr(), g.data_ptr() if with_grad else None, stream(dev))
            sync(dev)
            within("lsgan", f"n {n} target {target} loss", out[0], loss, bl)
            if with_grad:
                within("lsgan", f"n {n} target {target} grad", g, grad, bg)
            else:
                assert torch.isnan(g).all()


def lsgan_reference_alone(n):
    for target in (0.0, 1.0):
        pred, w, loss, bl, grad, bg = lsgan_case(n, target)
        d = pred - target
        within("eager lsgan", f"n {n} loss", LOSS0 + w * (d * d).mean(), loss, bl)
        within("eager lsgan", f"n {n} grad", w * 2 * d / n, grad, bg)


# ---------------------------------------------------------------------------------------------------------------- pix_loss
class Fx:
    """a float64 value with a bound on the error of its fp32 evaluation"""

    def __init__(self, v, e=None):
        self.v = torch.as_tensor(v, dtype=torch.float64)
        self.e = torch.zeros_like(self.v) if e is None else e


def fx(a):
    return a if isinstance(a, Fx) else Fx(a)


def fadd(a, b):
    a, b = fx(a), fx(b)
    v = a.v + b.v
    return Fx(v, a.e + b.e + U * v.abs())


def fsub(a, b):
    a, b = fx(a), fx(b)
    v = a.v - b.v
    return Fx(v, a.e + b.e + U * v.abs())


def fmul(a, b):
    a, b = fx(a), fx(b)
    v = a.v * b.v
    return Fx(v, a.v.abs() * b.e + b.v.abs() * a.e + U * v.abs())


def fdiv(a, b):
    a, b = fx(a), fx(b)
    v = a.v / b.v
    return Fx(v, (a.e + v.abs() * b.e) / b.v.abs() + DIV * U * v.abs())


def fsqrt(a):
    v = a.v.sqrt()
    return Fx(v, a.e / (2 * v) + SQRT * U * v)


EPS6 = Fx(1e-6, torch.tensor(U * 1e-6, dtype=torch.float64))
PIX_NAMES = ("l1", "ndvi", "ndwi", "gndvi", "savi", "msavi", "evi")
PIX_SHAPES = [(1, 1, 1), (2, 17, 19), (3, 64, 65), (5, 256, 256)]
ALL_W = (0.7, 0.31, 0.23, 0.17, 0.13, 0.11, 0.29)
SUMS0 = torch.tensor([1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0])
EXTRA = (4, 3, -0.5)


def one_hot(k, w=0.6):
    return tuple(w if i == k else 0.0 for i in range(7))


# name -> (weights, log_all, rgb, grad, extra)
PIX_VARIANTS = {**{n + " alone": (one_hot(k), 0, True, True, False) for k, n in enumerate(PIX_NAMES) if k},
                "all seven": (ALL_W, 0, True, True, False),
                "log_all, l1 only": (one_hot(0), 1, True, True, False),
                "no rgb": (one_hot(0), 0, False, True, False),
                "no grad": (ALL_W, 0, True, False, False),
                "extra": (ALL_W, 0, True, True, True)}


def pix_variants(shape):
    return ["all seven"] if shape == PIX_SHAPES[-1] else list(PIX_VARIANTS)


@functools.lru_cache(maxsize=None)
def pix_inputs(shape):
    B, H, W = shape
    gen = torch.Generator().manual_seed(55)
    rgb = 0.05 + 0.25 * torch.rand(B, 3, H, W, generator=gen)
    nir = 0.35 + 0.65 * torch.rand(B, 1, H, W, generator=gen)
    step = 0.02 + 0.2 * torch.rand(B, 1, H, W, generator=gen)
    rgb = rgb.clamp(0.05, 0.3)
    pred = torch.where(nir + step <= 0.995, nir + step, nir - step)
    for _ in range(20):         # an index that is not monotonic in the band can agree at two values: draw those pixels' step again
        pairs = O.rs_index_pairs(rgb.double(), nir.double(), pred.double(), "loss")
        flat = torch.stack([(a - b).abs() for a, b in pairs.values()]).min(0).values < 2e-4
        if not flat.any():
            break
        step = 0.02 + 0.2 * torch.rand(B, 1, H, W, generator=gen)
        pred = torch.where(flat, torch.where(nir + step <= 0.995, nir + step, nir - step), pred)
    extra = torch.randn(B, H, W, EXTRA[0], generator=gen)
    return rgb, nir, pred, extra


def fx_index(k, y, R, G, Bl):
    """index k of band y and its derivative wrt y, operation by operation as pix_loss_kernel evaluates them"""
    if k in (1, 2):
        band = R if k == 1 else G
        num, dp = fsub(y, band), fadd(fadd(y, band), EPS6)
        return fdiv(num, dp), fdiv(fsub(dp, num), fmul(dp, dp))
    if k == 3:
        yr = fadd(y, R)
        denp = fadd(fdiv(fsub(y, R), yr), G)
        num = fsub(y, G)
        dndp = fdiv(fmul(2.0, R), fmul(yr, yr))
        return fdiv(num, denp), fdiv(fsub(denp, fmul(num, dndp)), fmul(denp, denp))
    if k == 4:
        num, dp = fsub(y, R), fadd(fadd(y, R), 0.5)
        return fdiv(fmul(1.5, num), dp), fdiv(fmul(1.5, fsub(dp, num)), fmul(dp, dp))
    if k == 5:
        tp = fadd(fmul(2.0, y), 1.0)
        sp = fsqrt(fsub(fmul(tp, tp), fmul(8.0, fsub(y, R))))
        return fmul(fsub(tp, sp), 0.5), fmul(0.5, fsub(2.0, fdiv(fsub(fmul(4.0, tp), 8.0), fmul(2.0, sp))))
    c = fmul(fsub(R, 7.5), fadd(Bl, 1.0))
    num, dp = fsub(y, R), fadd(fmul(fadd(y, 6.0), c), EPS6)
    return fmul(2.5, fdiv(num, dp)), fdiv(fmul(2.5, fsub(dp, fmul(num, c))), fmul(dp, dp))


def pix_grid(n):
    return min(-(-n // 256), L.PIX_LOSS_WS_ELEMS // 8)


@functools.lru_cache(maxsize=8)
def pix_case(shape, variant, criterion):
    """float64 sums and gradient (autograd through O.rs_index_pairs) and their bounds (the kernel's operations on Fx pairs)"""
    w, log_all, with_rgb, with_grad, with_extra = PIX_VARIANTS[variant]
    w32 = [torch.tensor(v, dtype=torch.float32).double().item() for v in w]
    rgb, nir, pred, extra = pix_inputs(shape)
    n = nir.numel()
    y = pred.double().requires_grad_(True)
    x = nir.double()
    active = [k for k in range(1, 7) if log_all or w32[k] != 0]
    pairs = O.rs_index_pairs(rgb.double(), x, y, "loss") if with_rgb else {}
    crit = (lambda a, b: (a - b).abs().sum()) if criterion == 0 else (lambda a, b: ((a - b) ** 2).sum())
    terms = {0: (y - x).abs().sum()}
    for k in active:
        terms[k] = crit(*pairs[PIX_NAMES[k]])
    total = sum(w32[k] * t for k, t in terms.items()) / n
    total.backward()
    grad = y.grad.clone()
    blocks = pix_grid(n)
    ksum = -(-n // (256 * blocks)) + 6 + 4 + -(-blocks // 256) + 8 + 1
    sums, sums_b = SUMS0.double().clone(), torch.zeros(7, dtype=torch.float64)
    R, G, Bl = (Fx(rgb[:, i:i + 1].double()) for i in range(3))
    d0 = fsub(Fx(pred.double()), Fx(x))
    g = Fx(w32[0] * torch.sign(d0.v))
    term_b = {0: (d0.v.abs(), d0.e)}
    for k in active:
        f, df = fx_index(k, Fx(pred.double()), R, G, Bl)
        a, _ = fx_index(k, Fx(x), R, G, Bl)
        d = fsub(f, a)
        val, dval = (Fx(d.v.abs(), d.e), Fx(torch.sign(d.v))) if criterion == 0 else (fmul(d, d), fmul(2.0, d))
        term_b[k] = (val.v, val.e)
        if w32[k] != 0:
            g = fadd(g, fmul(fmul(w32[k], dval), df))
    for k, (v, e) in term_b.items():
        sums[k] += terms[k].detach()
        assert abs(v.sum() - terms[k].detach()) <= 1e-11 * v.sum()
        sums_b[k] = e.sum() + ksum * U * (SUMS0[k].double() + v.sum())
    g = fmul(g, Fx(1.0 / n, torch.tensor(U / n, dtype=torch.float64)))
    assert (g.v - grad).abs().max() <= 1e-11 * grad.abs().max()                   # the closed forms ARE the derivatives
    if with_extra:
        ex = extra[..., EXTRA[1]].double().reshape(grad.shape)
        s = torch.tensor(EXTRA[2], dtype=torch.float32).double().item()
        grad = grad + s * ex
        g = fadd(g, fmul(s, ex))
    return {"sums": sums, "sums_b": sums_b, "grad": grad, "grad_b": g.e, "active": active, "w": w}


def pix_conditions_hold(shape):
    rgb, nir, pred, _ = (t.double() for t in pix_inputs(shape))
    R, G, Bl = rgb[:, 0:1], rgb[:, 1:2], rgb[:, 2:3]
    assert rgb.min() >= 0.05 and rgb.max() <= 0.3 + 1e-7 and min(nir.min(), pred.min()) >= 0.35 and max(nir.max(), pred.max()) <= 1
    assert (pred - nir).abs().min() >= 0.02 - 1e-6
    for v in (nir, pred):
        dens = (v + R, v + G, (v - R) / (v + R) + G, (v + 6) * (R - 7.5) * (Bl + 1), torch.sqrt((2 * v + 1) ** 2 - 8 * (v - R)), v + R + 0.5)
        assert all(d.abs().min() >= 0.05 for d in dens)
    for a, b in O.rs_index_pairs(rgb, nir, pred, "loss").values():
        assert (a - b).abs().min() > 1e-4


def pix_desc(dev, shape, variant, criterion, keep):
    w, log_all, with_rgb, with_grad, with_extra = PIX_VARIANTS[variant]
    rgb, nir, pred, extra = (t.to(dev).contiguous() for t in pix_inputs(shape))
    sums, grad, ws = SUMS0.to(dev).clone(), nan(*nir.shape, dev=dev), torch.zeros(L.PIX_LOSS_WS_ELEMS, device=dev)
    d = L.PixLossDesc()
    d.rgb, d.nir, d.pred = rgb.data_ptr() if with_rgb else None, nir.data_ptr(), pred.data_ptr()
    d.B, d.H, d.W = shape
    d.w_l1, d.w_ndvi, d.w_ndwi, d.w_gndvi, d.w_savi, d.w_msavi, d.w_evi = w
    d.criterion, d.log_all = criterion, log_all
    if with_extra:
        d.extra, d.extra_cs, d.extra_c, d.extra_scale = extra.data_ptr(), EXTRA[0], EXTRA[1], EXTRA[2]
    d.sums, d.grad_pred, d.ws, d.ws_elems = sums.data_ptr(), grad.data_ptr() if with_grad else None, ws.data_ptr(), ws.numel()
    keep.extend((rgb, nir, pred, extra, ws))
    return d, sums, grad


def pix_loss_against_float64(dev, shape):
    for variant in pix_variants(shape):
        for criterion in (0, 1):
            c, keep = pix_case(shape, variant, criterion), []
            d, sums, grad = pix_desc(dev, shape, variant, criterion, keep)
            L.call("nirgan_pix_loss", C.byref(d), stream(dev))
            sync(dev)
            what = f"{shape} {variant} criterion {criterion}"
            within("pix_loss", what + " sums", sums, c["sums"], c["sums_b"])
            idle = [k for k in range(1, 7) if k not in c["active"]]
            assert same(sums[idle], SUMS0[idle]), what + ": an index that is off moved its sum"
            if PIX_VARIANTS[variant][3]:
                within("pix_loss", what + " grad", grad, c["grad"], c["grad_b"])
            else:
                assert torch.isnan(grad).all()


def pix_loss_guards(dev):
    be, shape = L.backend(), (2, 17, 19)
    for variant, change, msg in (("ndvi alone", {"rgb": None}, b"rgb"), ("log_all, l1 only", {"rgb": None}, b"rgb"),
                                 ("all seven", {"criterion": 2}, b"criterion"), ("extra", {"extra_c": EXTRA[0]}, b"extra"),
                                 ("extra", {"extra_c": -1}, b"extra")):
        keep = []
        d, sums, grad = pix_desc(dev, shape, variant, 0, keep)
        for k, v in change.items():
            setattr(d, k, v)
        assert fails(be.nirgan_pix_loss(C.byref(d), stream(dev))) and msg in be.nirgan_last_error(), variant
        sync(dev)
        assert same(sums, SUMS0) and torch.isnan(grad).all(), "the refused call launched something"


def pix_closed_form(rgb, x, y, w, log_all, criterion, sums0, mutate=None):
    """the kernel's own formulas (values and closed-form derivatives) in eager torch of the inputs' dtype; ``mutate`` plants an error"""
    R, G, Bl = (rgb[:, 0:1], rgb[:, 1:2], rgb[:, 2:3]) if rgb is not None else (None, None, None)
    n = x.numel()
    w = [torch.tensor(v, dtype=torch.float32).to(x.dtype) for v in w]

    def index(k, v):
        if k in (1, 2):
            band = R if k == 1 else G
            dp = v + band + 1e-6
            return (v - band) / dp, (dp - (v - band)) / (dp * dp)
        if k == 3:
            denp = (v - R) / (v + R) + G
            dndp = 0 if mutate == "gndvi without dndp" else 2 * R / ((v + R) * (v + R))
            return (v - G) / denp, (denp - (v - G) * dndp) / (denp * denp)
        if k == 4:
            dp = v + R + 0.5
            return 1.5 * (v - R) / dp, 1.5 * (dp - (v - R)) / (dp * dp)
        if k == 5:
            tp = 2 * v + 1
            sp = torch.sqrt(tp * tp - 8 * (v - R))
            return (tp - sp) * 0.5, 0.5 * (2 - (4 * tp - (0 if mutate == "msavi 4 tp" else 8)) / (2 * sp))
        c = (R - 7.5) * (Bl + 1)
        dp = (v + 6) * c + 1e-6
        return 2.5 * ((v - R) / dp), 2.5 * (dp - (v - R) * c) / (dp * dp)
    sums = sums0.clone()
    sums[0] += (y - x).abs().sum()
    g = w[0] * torch.sign(y - x)
    for k in range(1, 7):
        if log_all or w[k] != 0:
            f, df = index(k, y)
            d = f - index(k, x)[0]
            sums[k] += (d.abs() if criterion == 0 else d * d).sum()
            if w[k] != 0:
                g = g + w[k] * (torch.sign(d) if criterion == 0 else 2 * d) * df
    return sums, g * (1.0 / n)


def pix_eager32(shape, variant, criterion):
    w, log_all, with_rgb, with_grad, with_extra = PIX_VARIANTS[variant]
    rgb, x, y, extra = pix_inputs(shape)
    sums, g = pix_closed_form(rgb if with_rgb else None, x, y, w, log_all, criterion, SUMS0)
    if with_extra:
        g = g + EXTRA[2] * extra[..., EXTRA[1]].reshape(g.shape)
    return sums, g


def pix_reference_alone(shape):
    for variant in pix_variants(shape):
        for criterion in (0, 1):
            c = pix_case(shape, variant, criterion)
            sums, g = pix_eager32(shape, variant, criterion)
            within("eager pix_loss", f"{shape} {variant} {criterion} sums", sums, c["sums"], c["sums_b"])
            within("eager pix_loss", f"{shape} {variant} {criterion} grad", g, c["grad"], c["grad_b"])


# ---------------------------------------------------------------------------------------------------------------- tap_scatter
TAP_CASES = [(2, 7, 20, 22, 3, 52), (1, 7, 70, 70, 0, 52), (3, 4, 9, 11, 0, 16)]
DBIAS0 = 0.25


@functools.lru_cache(maxsize=None)
def tap_case(case, act):
    """the float64 adjoint of the gather as test_tap_gather_kernels states it: out = act(bias + sum_t Q[y+crop+dh_t][x+crop+dw_t][t])"""
    B, k, OH, OW, crop, qcs = case
    H2, W2, qh, qw = OH - 2 * crop, OW - 2 * crop, OH + k - 1, OW + k - 1
    gen = torch.Generator().manual_seed(57)
    dout = torch.randn(B, H2, W2, generator=gen)
    out = torch.tanh(torch.randn(B, H2, W2, generator=gen))
    o64, d64 = out.double(), dout.double()
    dz = d64 * (1 - o64 * o64) if act else d64
    a = d64.abs() * (1 + o64 * o64) if act else torch.zeros_like(d64)

    def adjoint(cot):
        q = torch.zeros(B, qh, qw, qcs, dtype=torch.float64, requires_grad=True)
        y = sum(q[:, crop + t // k:crop + t // k + H2, crop + t % k:crop + t % k + W2, t] for t in range(k * k))
        y.backward(cot)
        return q.grad
    n = dout.numel()
    kb = 3 + 3 * -(-n // 4096) + 6 + 16 + 1
    return {"dout": dout, "out": out, "dq": adjoint(dz), "dq_b": 3 * U * adjoint(a), "dbias": DBIAS0 + dz.sum(),
            "dbias_b": kb * U * (DBIAS0 + (a if act else d64.abs()).sum()), "dz": dz}


def tap_scatter_against_float64(dev, case):
    B, k, OH, OW, crop, qcs = case
    qh, qw = OH + k - 1, OW + k - 1
    for act in (True, False):
        c = tap_case(case, act)
        dout, out = c["dout"].to(dev), c["out"].to(dev)
        for with_bias in (True, False):
            dq, dbias = nan(B, qh, qw, qcs, dev=dev), torch.full((1,), DBIAS0, device=dev)
            d = L.TapScatterDesc()
            d.dout, d.out, d.act = dout.data_ptr(), out.data_ptr() if act else None, L.ACT_TANH if act else L.ACT_NONE
            d.B, d.OH, d.OW, d.crop, d.ntaps = B, OH, OW, crop, k * k
            for t in range(k * k):
                d.tap_dh[t], d.tap_dw[t] = t // k, t % k
            d.dq, d.q_hp, d.q_wp, d.q_cs, d.dbias = dq.data_ptr(), qh, qw, qcs, dbias.data_ptr() if with_bias else None
            L.call("nirgan_tap_scatter", C.byref(d), stream(dev))
            sync(dev)
            what = f"{case} tanh {act} dbias {with_bias}"
            within("tap_scatter", what + " dq", dq, c["dq"], c["dq_b"])
            assert same(dq[..., k * k:], torch.zeros(B, qh, qw, qcs - k * k)), what + ": channels t >= ntaps"
            if with_bias:
                within("tap_scatter", what + " dbias", dbias[0], c["dbias"], c["dbias_b"])
            else:
                assert dbias.item() == DBIAS0


OPPOSITE_HALVES = [(4, 6, 6), (6, 5, 7), (2, 30, 30)]        # the PatchGAN's last map: 2B samples of a [fake ; real] batch, no power of two


def tap_scatter_opposite_halves(dev, shape):
    """dout = +w/n on the first half of the batch and -w/n on the second (a wgangp discriminator step): the bias gradient is a sum of
    equal and opposite terms and has to leave dbias bitwise where it was -- a residue of the summation order would be a gradient of
    rounding noise, which Adam turns into a step (step_matrix_cases row w01 found the fused and the Lightning route one step of the
    last bias apart).  Beside its fp32 sum the library sums the terms in float64, where every partial sum of such terms is exact, and adds
    nothing when that sum is exactly 0."""
    B, OH, OW = shape
    k, qcs = 4, 16
    qh, qw = OH + k - 1, OW + k - 1
    a = (torch.tensor(0.37) * (torch.tensor(1.0) / torch.tensor(float(B // 2 * OH * OW)))).item()      # fp32((w) * (1.f / n))
    dout = torch.full((B, OH, OW), a)
    dout[B // 2:] = -a
    dout = dout.to(dev)
    dq, dbias = nan(B, qh, qw, qcs, dev=dev), torch.full((1,), DBIAS0, device=dev)
    d = L.TapScatterDesc()
    d.dout, d.out, d.act = dout.data_ptr(), None, L.ACT_NONE
    d.B, d.OH, d.OW, d.crop, d.ntaps = B, OH, OW, 0, k * k
    for t in range(k * k):
        d.tap_dh[t], d.tap_dw[t] = t // k, t % k
    d.dq, d.q_hp, d.q_wp, d.q_cs, d.dbias = dq.data_ptr(), qh, qw, qcs, dbias.data_ptr()
    L.call("nirgan_tap_scatter", C.byref(d), stream(dev))
    sync(dev)
    assert dbias.item() == DBIAS0, f"{shape}: dbias moved by {dbias.item() - DBIAS0:.3e}"
    assert torch.isfinite(dq.cpu()).all()


def tap_reference_alone(case):
    for act in (True, False):
        c = tap_case(case, act)
        dz = c["dout"] * (1 - c["out"] * c["out"]) if act else c["dout"]
        within("eager tap_scatter", f"{case} dz", dz, c["dz"], 3 * U * c["dout"].double().abs() * (1 + c["out"].double() ** 2) if act else 0.0)
        within("eager tap_scatter", f"{case} dbias", DBIAS0 + dz.sum(), c["dbias"], c["dbias_b"])


# ---------------------------------------------------------------------------------------------------------------- whole path
def unscaled_multiply_generator(dev, size=32, B=2):
    """ResnetGenerator_inject with scaling_param=False and the multiply style (generator_inject.py:126-127: x * embeds), forward and
    backward through the autograd bridge against the float64 oracle, with the bounds of test_golden_inject_generator (1e-3 of the
    prediction's max; gradients rel-L2 1e-3 and 1e-2 of their max)"""
    import types
    from model.generator_inject import define_G_inject
    ns = types.SimpleNamespace
    cfg = ns(base_configs=ns(input_nc=3, output_nc=1, ngf=8, netG="resnet_9blocks", norm="instance", no_dropout=True,
                             init_type="normal", init_gain=0.02),
             satclip=ns(satclip_inject_style="multiply", post_correction=False, post_correction_init=1.0,
                        scaling_param=False, scaling_param_init=0.01))
    torch.manual_seed(0)
    net = define_G_inject(cfg)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    assert "scale_param" not in sd
    gen = torch.Generator().manual_seed(59)
    sd["fc.weight"], sd["fc.bias"] = torch.randn(16384, 256, generator=gen) * 0.05, torch.randn(16384, generator=gen) * 0.05
    net.load_state_dict(sd)
    rgb = 0.02 + 0.58 * torch.rand(B, 3, size, size, generator=gen)
    emb = torch.randn(B, 256, generator=gen)
    dout = torch.randn(B, 1, size, size, generator=gen)
    net = net.to(dev)
    pred = net(rgb.to(dev), emb.to(dev))
    pred.backward(dout.to(dev))
    p64 = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    ref = O.px_forward(p64, rgb.double(), 9, 0, emb.double(), {"style": "multiply", "use_scale": False})
    ref.backward(dout.double())
    with torch.no_grad():                       # what the entry computed before: x * (1 + embeds), a visibly different function
        old = O.px_forward({**p64, "scale_param": torch.tensor(1.0, dtype=torch.float64)}, rgb.double(), 9, 0, emb.double(),
                           {"style": "multiply", "use_scale": True})
    assert (old - ref).abs().max() > 2e-2 * ref.abs().max()
    got = pred.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    print(f"unscaled multiply: pred err {err:.3e} of {scale:.3e}")
    assert err <= 1e-3 * scale
    shadow, seen = O.shadowed_bias_keys("G", 9), set()
    for k, p in net.named_parameters():
        if k in shadow or p64[k].grad is None:
            continue
        a, b = p.grad.detach().double().cpu(), p64[k].grad
        e2, em = ((a - b).norm() / b.norm().clamp_min(1e-30)).item(), ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()
        print(f"unscaled multiply: grad {k} rel-L2 {e2:.3e} max {em:.3e}")
        assert torch.isfinite(a).all() and e2 <= 1e-3 and em <= 1e-2, k
        seen.add(k)
    assert {"fc.weight", "fc.bias", "model.1.weight"} <= seen
