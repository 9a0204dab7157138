"""Bodies shared by tests/test_metric_loss_emulated.py (numpy emulator, CPU) and tests/test_gpu_metric_loss.py (MI355X): the raw entries
nirgan_image_metrics (csrc/metrics.hip), nirgan_ssim_loss (csrc/ssimloss.hip), nirgan_emd_loss (csrc/emdloss.hip) and nirgan_hist_match
(csrc/histmatch.hip), each against float64.

Every body takes ``dev`` ("cpu": the installed backend is an EmuBackend) and drives the entry through ``L.call`` / ``L.check``.  Every
expected value is float64 torch or numpy from the operation's definition: ``O.ssim_map`` and its autograd, the softmax / cumsum / mean
definition of the EMD (include/nirgan_hip.h) and its autograd, ``O.histogram_match``.  Nothing is expected from the emulator or from a
kernel.  Every output sits between NaN guard bands that must stay NaN bitwise, every workspace is NaN before the call, and the inputs
must be bitwise what they were after it.

Bounds.  u = 2^-24, every element is held to ``K * u * A`` (tests/streaming_cases.py: K the rounded operations on the longest chain, A
the float64 sum of the absolute terms; a division counts 3); ``Fx`` pairs (value, bound) of streaming_cases replay a formula operation
by operation, so that a subtraction of rounded quantities carries its operands' bounds: that IS the conditioning of m_xx - mu^2 on a
flat bright image.  An exact doubling or negation adds nothing.

ssim map       taps: the double Gaussian exp(-x^2 / (2 sigma^2)) / sum rounded once to fp32 (ng_ssim_taps): (k, u k).  Horizontal then
               vertical pass: every term k * v (1), k * v * w (2), summed by 2r adds (the first lands on 0).  Then the formula of the
               kernel on pairs.  metrics.hip: mu1^2, mu2^2, mu1 mu2, the three subtractions, (2 mu12 + C1)(2 s12 + C2),
               (mu1^2 + mu2^2 + C1)(s1 + s2 + C2), / (den + eps).  ssimloss.hip: A1 = 2 mu nu + C1, A2 = 2 (m_xy - mu nu) + C2,
               B1 = mu^2 + nu^2 + C1, B2 = (m_xx - mu^2) + (m_yy - nu^2) + C2, inv = 1 / (B1 B2 + eps), S = A1 A2 inv.
               C1 = (0.01f max_val)^2 in fp32 is held to 5 u (0.01f 1, two products 2 each after squaring, the square 1 -> 5), eps to u.
sums           a thread adds its 4 pixels, the wave 6, the four waves 2, the one-block second launch ceil(blocks / 256) + 6 + 2:
               Ks = 20 + ceil(blocks / 256), sum within (terms' own bounds) + Ks u sum |term|.  means[j] = sum * fl(1 / n): 3 + 1.
               means[0] terms |x - y|: 1 u each; means[1] terms (x - y)^2: 2 u each.  ssim value: 1 - sum / n: 3, then 1.
               loss += weight * value: one product, one add.  A second call of nirgan_image_metrics is bitwise the first.
ssim gradient  the maps a = (2 nu (A2 - A1) - 2 mu S (B2 - B1)) inv, b = -S B1 inv, c = 2 A1 inv on the same pairs; the adjoint filter
               on the zero-padded (H + 2r) x (W + 2r) domain (two sums of 2r + 1 terms); the fold over the reflect images of a pixel
               (F's entries at every padded coordinate that reflects onto it, from the definition of the reflect border:
               nh * nw <= 9 adds per map); f_a + 2 x f_b + y f_c (2 products, 2 adds); * fl(-weight / n) (3, 1); + grad_pred (1).
               The values the pairs carry are asserted to equal weight * the float64 autograd gradient of 1 - mean O.ssim_map to
               1e-10 of its maximum: the expectation is autograd's.  pred == target: S = 1 - eps / D, and the gradient is NOT zero:
               with A1 = B1, A2 = B2, t = eps / (A1 A2 + eps) it is  -weight / n * (G^T[2 mu (A2 - A1) t / D] + x G^T[2 A1 t / D]),
               1e-9 of its cancelling terms 2 x G^T[b] and y G^T[c].  float64 autograd carries those terms' rounding (2^-53 of
               them, 1e-6 of the result), so this case expects the cancellation-free form above and asserts autograd within
               1e-13 of the cancelling terms (2^-53 times some hundred operations) instead of 1e-10 of the result.
emd value      expectation: float64 softmax and cumsum, each CDF rounded to fp32 before the subtraction (the header: the reference
               compares fp32 CDFs).  The kernel's terms are double(expf(fl(x - max))): relative rho_i = 2 ulp (2 * 2^-23) + u |x_i - max|
               each, against exact ones.  c_i = sum_{j<=i} e_j / sum_j e_j moves by at most
               (1 - c_i) sum_{j<=i} p_j rho_j + c_i sum_{j>i} p_j rho_j =: E_i.  The fp32 CDFs add u c_i + u d_i (half an ulp each), the
               fp32 subtraction u |c - d|, the double accumulation N 2^-53 (negligible; counted).  ||a| - |b|| <= |a - b|: the value is
               within the mean of these + u value (the cast).  loss += weight value: 2 more.
emd gradient   dL/dx_k = weight / (B N) p_k (g_k - sum_j p_j g_j), g the inclusive suffix sums of sign(c - d) (asserted against autograd
               to 1e-10).  With equal signs the kernel's p moves by p_k (rho_k + rbar), rbar = sum_j p_j rho_j, the dot product by
               sum_j p_j rho_j |g_j - dot|; the cast and the add into grad_pred 1 each.  Sign-free elements: where the float64 |c_i - d_i|
               is below E_i(c) + E_i(d) + u (c_i + d_i) the kernel's sign is any of -1, 0, 1; a flip moves g_k by 2 for k <= i, dL/dx_k by
               at most 2 p_k max(c_i, 1 - c_i) weight / (B N), added to element k's bound.  The last element of a sample is always
               sign-free and contributes 0 (a constant shift of g cancels against the dot product).  Condition (emd_conditions_hold):
               at most 0.2 % of B N sign-free elements for N >= 1000, at most two per sample below.  pred == target bitwise: value 0,
               gradient exactly 0, loss untouched bitwise.
hist_match     within u |want| + 1e-12 max(1, |want|) of the float64 O.histogram_match: one fp32 rounding of a double result.  Where
               np.interp returns a template value unchanged (the cumulative count of the source value is that of a template value, or
               lies below the first one's) the element equals that template value and is bitwise one of the template's elements;
               tie-free inputs: the output is bitwise a permutation of the template.

Two CPU checks keep these honest (tests/test_metric_loss_emulated.py): the kernels' formulas in eager fp32 torch (EMD: fp32 exp, double
cumsum; hist: double interpolation, one rounding) lie inside every bound of every case, and an emulator with one planted error fails a
named body.
"""
import ctypes as C
import functools

import numpy as np
import torch
import torch.nn.functional as F

import nirgan_oracle as O
from nirgan_hip import lib as L
from streaming_cases import RATIOS, U, Fx, bits, fadd, fdiv, fmul, fsub, nan, same, stream, sync, within  # noqa: F401 (RATIOS: one table for all families)

GUARD = 8
ULP = 2.0 ** -23
LOSS0 = 2.0
SIGMA = 1.5
EPS = 1e-12


def banded(n, dev, dtype=torch.float32):
    """n elements between two NaN guard bands: (the whole buffer, the view the entry gets)"""
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def bands_intact(buf, n):
    edge = torch.full((GUARD,), float("nan"), dtype=buf.dtype)
    a, b = buf[:GUARD].cpu(), buf[GUARD + n:].cpu()
    return torch.equal(a.view(torch.uint8), edge.view(torch.uint8)) and torch.equal(b.view(torch.uint8), edge.view(torch.uint8))


def all_nan_bitwise(t):
    return same(t, torch.full(t.shape, float("nan"), dtype=t.dtype)) if t.dtype == torch.float32 else bool(torch.isnan(t).all())


def fdbl(a):
    return Fx(2 * a.v, 2 * a.e)


def fneg(a):
    return Fx(-a.v, a.e)


def fsum(terms, adds):
    v = sum(t.v for t in terms)
    return Fx(v, sum(t.e for t in terms) + adds * U * sum(t.v.abs() for t in terms))


def cut(a, axis, t, n):
    return Fx(a.v.narrow(axis, t, n), a.e.narrow(axis, t, n))


def f32(v):
    return torch.tensor(v, dtype=torch.float32).double().item()


# ---------------------------------------------------------------------------------------------------------------- ssim: definition
SSIM_SHAPES = [(1, 6, 6, 11), (2, 12, 9, 11), (3, 33, 31, 5), (2, 70, 66, 11), (1, 8, 8, 5), (1, 5, 7, 1)]
SSIM_KINDS = ("rand", "bright", "saturated", "equal")
SSIM_CASES = [(s, k) for s in ((1, 6, 6, 11), (2, 70, 66, 11)) for k in SSIM_KINDS] + \
    [((2, 12, 9, 11), "rand"), ((3, 33, 31, 5), "saturated"), ((1, 8, 8, 5), "bright"), ((1, 5, 7, 1), "rand")]
SSIM_VARIED = ((2, 12, 9, 11), "rand")          # the case that also runs weight 0, the NULL forms and max_val 2
WEIGHT = 0.75


def taps64(window):
    x = torch.arange(window, dtype=torch.float64) - window // 2
    k = torch.exp(-x * x / (2.0 * SIGMA ** 2))
    return k / k.sum()


def reflect_source(j, n):
    """the image coordinate a reflect border (no edge repeat) shows at coordinate j"""
    j = abs(j)
    return 2 * (n - 1) - j if j >= n else j


def fold_matrix(n, r, mutate=None):
    """R[h][j] = 1 where padded coordinate j of the (n + 2r) domain shows image coordinate h: the adjoint of the reflect border"""
    R = torch.zeros(n, n + 2 * r, dtype=torch.float64)
    for j in range(n + 2 * r):
        if mutate == "fold without the right mirror" and j >= n + r:
            continue
        R[reflect_source(j - r, n), j] = 1
    return R


@functools.lru_cache(maxsize=None)
def ssim_images(shape, kind):
    P, H, W, _ = shape
    gen = torch.Generator().manual_seed(61)
    if kind == "bright":
        x = 0.9 + 1e-3 * torch.randn(P, H, W, generator=gen)
        y = (x + 0.01 * torch.randn(P, H, W, generator=gen)).clamp(0, 1)
    elif kind == "saturated":          # 4 x 4 patches of one coarse value: those above 1 clamp to flat patches
        coarse = torch.rand(P, -(-H // 4), -(-W // 4), generator=gen).repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W]
        x = (1.2 * coarse + 0.4 + 0.01 * torch.randn(P, H, W, generator=gen)).clamp(0, 1)
        y = (x + 0.1 * torch.randn(P, H, W, generator=gen)).clamp(0, 1)
    else:
        x = torch.rand(P, H, W, generator=gen)
        y = x.clone() if kind == "equal" else (x + 0.1 * torch.randn(P, H, W, generator=gen)).clamp(0, 1)
    base = 1e-4 * torch.randn(P, H, W, generator=gen)
    return x.contiguous(), y.contiguous(), base


def ssim_conditions_hold(shape, kind):
    x, y, _ = ssim_images(shape, kind)
    assert x.min() >= 0 and max(x.max(), y.max()) <= 1.01 and y.min() >= 0
    if kind == "equal":
        assert same(x, y)
    if kind == "saturated":
        assert (x == 1).float().mean() > 0.15 and (x < 1).any()
        if shape[1] >= 8 and shape[2] >= 8:
            assert (F.avg_pool2d((x == 1).float()[:, None], 4, 4) == 1).any(), "no saturated patch"
    if kind == "bright":
        assert x.std() < 2e-3 and x.mean() > 0.89


def ssim_pairs(x, y, window, max_val, form):
    """the five filtered moments and the kernel's formula on (value, bound) pairs; form "metrics" or "loss" """
    P, H, W = x.shape
    r, n = window // 2, window
    K = [Fx(k, U * k) for k in taps64(window)]
    pad = (lambda t: F.pad(t[:, None], (r, r, r, r), mode="reflect")[:, 0]) if r else (lambda t: t)
    xp, yp = Fx(pad(x)), Fx(pad(y))
    hpass = []
    for first, second in ((xp, None), (yp, None), (xp, xp), (yp, yp), (xp, yp)):
        terms = []
        for t in range(n):
            term = fmul(K[t], cut(first, 2, t, W))
            terms.append(term if second is None else fmul(term, cut(second, 2, t, W)))
        hpass.append(fsum(terms, n - 1))
    mu, nu, mxx, myy, mxy = (fsum([fmul(K[t], cut(h, 1, t, H)) for t in range(n)], n - 1) for h in hpass)
    c1v, c2v = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    c1, c2 = Fx(c1v, torch.tensor(5 * U * c1v, dtype=torch.float64)), Fx(c2v, torch.tensor(5 * U * c2v, dtype=torch.float64))
    eps = Fx(EPS, torch.tensor(U * EPS, dtype=torch.float64))
    if form == "metrics":
        m11, m22, m12 = fmul(mu, mu), fmul(nu, nu), fmul(mu, nu)
        s1, s2, s12 = fsub(mxx, m11), fsub(myy, m22), fsub(mxy, m12)
        num = fmul(fadd(fdbl(m12), c1), fadd(fdbl(s12), c2))
        den = fmul(fadd(fadd(m11, m22), c1), fadd(fadd(s1, s2), c2))
        return {"S": fdiv(num, fadd(den, eps))}
    munu, mumu, nunu = fmul(mu, nu), fmul(mu, mu), fmul(nu, nu)
    A1, A2 = fadd(fdbl(munu), c1), fadd(fdbl(fsub(mxy, munu)), c2)
    B1, B2 = fadd(fadd(mumu, nunu), c1), fadd(fadd(fsub(mxx, mumu), fsub(myy, nunu)), c2)
    D = fadd(fmul(B1, B2), eps)
    inv = fdiv(1.0, D)
    S = fmul(fmul(A1, A2), inv)
    a = fmul(fsub(fmul(fdbl(nu), fsub(A2, A1)), fmul(fmul(fdbl(mu), S), fsub(B2, B1))), inv)
    b = fmul(fmul(fneg(S), B1), inv)
    c = fmul(fdbl(A1), inv)
    return {"S": S, "maps": (a, b, c), "mu": mu, "A1": A1, "A2": A2, "D": D}


def adjoint_pairs(m, window):
    """G^T m on pairs: the zero-padded correlation on the (H + 2r) x (W + 2r) domain, then the fold over the reflect images"""
    P, H, W = m.v.shape
    r, n = window // 2, window
    K = [Fx(k, U * k) for k in taps64(window)]
    z = Fx(F.pad(m.v, (2 * r,) * 4), F.pad(m.e, (2 * r,) * 4))
    h = fsum([fmul(K[t], cut(z, 2, t, W + 2 * r)) for t in range(n)], n - 1)
    Fm = fsum([fmul(K[t], cut(h, 1, t, H + 2 * r)) for t in range(n)], n - 1)
    Rh, Rw = fold_matrix(H, r), fold_matrix(W, r)
    fold = lambda t: torch.einsum("hi,pij,wj->phw", Rh, t, Rw)
    adds = (Rh.sum(1)[:, None] * Rw.sum(1)[None, :])[None]
    return Fx(fold(Fm.v), fold(Fm.e) + adds * U * fold(Fm.v.abs()))


def sum_adds(blocks):
    return 4 + 6 + 2 + -(-blocks // 256) + 6 + 2


def tiles(shape):
    P, H, W, _ = shape
    return P * -(-H // 32) * -(-W // 32)


def mean_of(terms, shape, scale_ops):
    """(float64 mean, bound) of the block sums of ``terms`` followed by ``scale_ops`` rounded operations on the mean"""
    n = terms.v.numel()
    mean = terms.v.sum() / n
    return mean, (terms.e.sum() + sum_adds(tiles(shape)) * U * terms.v.abs().sum()) / n + scale_ops * U * mean.abs()


@functools.lru_cache(maxsize=None)
def metrics_case(shape, kind, max_val=1.0):
    x, y, _ = ssim_images(shape, kind)
    x64, y64, window = x.double(), y.double(), shape[3]
    d = x64 - y64
    S = ssim_pairs(x64, y64, window, max_val, "metrics")["S"]
    ref_map = O.ssim_map(x64[:, None], y64[:, None], window, max_val, EPS)[:, 0]
    assert (S.v - ref_map).abs().max() <= 1e-10 * ref_map.abs().max()            # the pairs carry O.ssim_map
    rows = [mean_of(Fx(d.abs(), U * d.abs()), shape, 4), mean_of(Fx(d * d, 2 * U * d * d), shape, 4), mean_of(Fx(ref_map, S.e), shape, 4)]
    return {"means": torch.stack([v for v, _ in rows]), "means_b": torch.stack([b for _, b in rows]), "map": ref_map, "map_b": S.e}


@functools.lru_cache(maxsize=None)
def ssim_case(shape, kind, max_val=1.0, weight=WEIGHT, preload=True):
    """float64 value, loss and gradient of nirgan_ssim_loss with their bounds"""
    x, y, base = ssim_images(shape, kind)
    if not preload:
        base = torch.zeros_like(base)
    P, H, W, window = shape
    n = P * H * W
    w = f32(weight)
    loss0 = LOSS0 if preload else 0.0
    x64 = x.double().requires_grad_(True)
    y64 = y.double()
    ref_map = O.ssim_map(x64[:, None], y64[:, None], window, max_val, EPS)[:, 0]
    ref_v = 1.0 - ref_map.mean()
    auto, = torch.autograd.grad(w * ref_v, x64)
    x64, ref_map, ref_v = x64.detach(), ref_map.detach(), ref_v.detach()
    q = ssim_pairs(x64, y64, window, max_val, "loss")
    assert (q["S"].v - ref_map).abs().max() <= 1e-10 * ref_map.abs().max()
    mean, mean_b = mean_of(Fx(ref_map, q["S"].e), shape, 3)
    value_b = mean_b + U * ref_v.abs()
    loss = loss0 + w * ref_v
    loss_b = w * value_b + U * (w * ref_v).abs() + U * loss.abs()
    fa, fb, fc = (adjoint_pairs(m, window) for m in q["maps"])
    scale = Fx(-w / n, torch.tensor(3 * U * w / n, dtype=torch.float64))
    g = fmul(scale, fadd(fadd(fa, fmul(fdbl(Fx(x64)), fb)), fmul(Fx(y64), fc)))
    if kind == "equal":
        t = EPS / (q["A1"].v * q["A2"].v + EPS)
        lone = lambda m: adjoint_pairs(Fx(m), window).v
        want = -w / n * (lone(2 * q["mu"].v * (q["A2"].v - q["A1"].v) * t / q["D"].v) + x64 * lone(2 * q["A1"].v * t / q["D"].v))
        cancelling = w / n * (lone(q["maps"][0].v.abs()) + 2 * x64.abs() * lone(q["maps"][1].v.abs()) + y64.abs() * lone(q["maps"][2].v.abs()))
        assert (auto - want).abs().max() <= 1e-13 * cancelling.max()
        assert want.abs().max() > 0
    else:
        want = auto
        assert (g.v - auto).abs().max() <= 1e-10 * auto.abs().max()             # the closed forms ARE the derivative
    out = fadd(Fx(base.double()), g)
    return {"x": x, "y": y, "base": base, "value": ref_v, "value_b": value_b, "loss": loss, "loss_b": loss_b, "loss0": loss0,
            "grad": base.double() + want, "grad_b": out.e, "w": weight, "max_val": max_val}


# ---------------------------------------------------------------------------------------------------------------- ssim: formulas in eager torch
def ssim_closed_form(x, y, window, max_val, mutate=None):
    """the kernels' formulas in eager torch of the inputs' dtype with the fp32 taps: S, the maps, d(sum S)/dx; ``mutate`` plants an error"""
    P, H, W = x.shape
    r, n, dt = window // 2, window, x.dtype
    k = taps64(window).float().to(dt)
    if mutate == "unnormalised taps":
        k = torch.exp(-(torch.arange(window, dtype=torch.float64) - r) ** 2 / (2.0 * SIGMA ** 2)).float().to(dt)

    def source(j, size):
        if mutate == "edge repeat":
            return -j - 1 if j < 0 else (2 * size - 1 - j if j >= size else j)
        return reflect_source(j, size)
    ih = torch.tensor([source(j, H) for j in range(-r, H + r)])
    iw = torch.tensor([source(j, W) for j in range(-r, W + r)])

    def passes(t, oh, ow):
        h = sum(k[i] * t[:, :, i:i + ow] for i in range(n))
        return sum(k[i] * h[:, i:i + oh] for i in range(n))

    def moments(a, b=None):
        ap = a[:, ih][:, :, iw]
        bp = None if b is None else b[:, ih][:, :, iw]
        h = sum((k[i] * ap[:, :, i:i + W]) if bp is None else (k[i] * ap[:, :, i:i + W] * bp[:, :, i:i + W]) for i in range(n))
        return sum(k[i] * h[:, i:i + H] for i in range(n))
    mu, nu, mxx, myy, mxy = moments(x), moments(y), moments(x, x), moments(y, y), moments(x, y)
    c1 = (torch.tensor(0.01) * torch.tensor(max_val, dtype=torch.float32)) ** 2
    c2 = (torch.tensor(0.03) * torch.tensor(max_val, dtype=torch.float32)) ** 2
    c1, c2, eps = c1.to(dt), c2.to(dt), torch.tensor(0.0 if mutate == "eps dropped" else EPS, dtype=torch.float32).to(dt)
    A1, A2 = 2 * mu * nu + c1, 2 * (mxy - mu * nu) + c2
    B1, B2 = mu * mu + nu * nu + c1, (mxx - mu * mu) + (myy - nu * nu) + c2
    inv = 1 / (B1 * B2 + eps)
    S = A1 * A2 * inv
    S_metrics = ((2 * (mu * nu) + c1) * (2 * (mxy - mu * nu) + c2)) / ((mu * mu + nu * nu + c1) * ((mxx - mu * mu) + (myy - nu * nu) + c2) + eps)
    maps = ((2 * nu * (A2 - A1) - 2 * mu * S * (B2 - B1)) * inv, -S * B1 * inv, 2 * A1 * inv)
    Rh, Rw = fold_matrix(H, r, mutate).to(dt), fold_matrix(W, r, mutate).to(dt)
    f = [Rh @ passes(F.pad(m, (2 * r,) * 4), H + 2 * r, W + 2 * r) @ Rw.T for m in maps]
    return S, S_metrics, maps, f[0] + 2 * x * f[1] + y * f[2]


def ssim_eager32(shape, kind, max_val=1.0, weight=WEIGHT):
    x, y, base = ssim_images(shape, kind)
    S, S_metrics, _, gs = ssim_closed_form(x, y, shape[3], max_val)
    n = x.numel()
    value = 1 - S.sum() / n
    w = torch.tensor(weight, dtype=torch.float32)
    d = x - y
    return {"value": value, "loss": LOSS0 + w * value, "grad": base + (-w / n) * gs, "map": S_metrics,
            "means": torch.stack([d.abs().sum() * (1.0 / n), (d * d).sum() * (1.0 / n), S_metrics.sum() * (1.0 / n)])}


def ssim_reference_alone(shape, kind):
    for max_val, weight in [(1.0, WEIGHT)] + ([(2.0, WEIGHT), (1.0, 0.0)] if (shape, kind) == SSIM_VARIED else []):
        c, m, got = ssim_case(shape, kind, max_val, weight), metrics_case(shape, kind, max_val), ssim_eager32(shape, kind, max_val, weight)
        what = f"{shape} {kind} max_val {max_val} weight {weight}"
        within("eager ssim map", what, got["map"], m["map"], m["map_b"])
        within("eager metrics", what, got["means"], m["means"], m["means_b"])
        within("eager ssim value", what + " value", got["value"], c["value"], c["value_b"])
        within("eager ssim value", what + " loss", got["loss"], c["loss"], c["loss_b"])
        within("eager ssim gradient", what, got["grad"], c["grad"], c["grad_b"])


# ---------------------------------------------------------------------------------------------------------------- ssim: bodies
def metrics_against_float64(dev, shape, kind, max_val=1.0):
    P, H, W, window = shape
    c = metrics_case(shape, kind, max_val)
    x, y, _ = ssim_images(shape, kind)
    xd, yd = x.to(dev).contiguous(), y.to(dev).contiguous()
    be, st = L.backend(), stream(dev)
    elems = int(be.nirgan_image_metrics_ws_elems(P, H, W))
    assert elems == 3 * tiles(shape)
    runs = []
    for _ in range(2):
        ws_buf, ws = banded(elems, dev)
        out_buf, out = banded(3, dev)
        d = L.MetricsDesc()
        d.pred, d.target, d.planes, d.H, d.W = xd.data_ptr(), yd.data_ptr(), P, H, W
        d.window, d.sigma, d.max_val, d.eps = window, SIGMA, max_val, EPS
        d.ws, d.ws_elems, d.means = ws.data_ptr(), elems, out.data_ptr()
        L.call("nirgan_image_metrics", C.byref(d), st)
        sync(dev)
        assert bands_intact(out_buf, 3) and bands_intact(ws_buf, elems), "image_metrics wrote outside its outputs"
        runs.append(out.cpu().clone())
    assert same(xd, x) and same(yd, y), "image_metrics changed its inputs"
    assert same(runs[0], runs[1]), "image_metrics: a second call differs bitwise"
    within("metrics", f"{shape} {kind} max_val {max_val}", runs[0], c["means"], c["means_b"])


def run_ssim_loss(dev, shape, kind, max_val=1.0, weight=WEIGHT, skip=None):
    """one call of nirgan_ssim_loss; ``skip`` names the output passed as NULL"""
    P, H, W, window = shape
    r, n = window // 2, P * H * W
    c = ssim_case(shape, kind, max_val, weight)
    xd, yd = c["x"].to(dev).contiguous(), c["y"].to(dev).contiguous()
    be, st = L.backend(), stream(dev)
    elems = int(be.nirgan_ssim_loss_ws_elems(P, H, W, window))
    n_maps, n_f = 3 * n, 3 * P * (H + 2 * r) * (W + 2 * r)
    assert elems == n_maps + n_f + tiles(shape)
    ws_buf, ws = banded(elems, dev)
    loss_buf, loss = banded(1, dev)
    value_buf, value = banded(1, dev)
    grad_buf, grad = banded(n, dev)
    loss.fill_(LOSS0)
    grad.copy_(c["base"].reshape(-1))
    d = L.SsimLossDesc()
    d.pred, d.target, d.planes, d.H, d.W = xd.data_ptr(), yd.data_ptr(), P, H, W
    d.window, d.sigma, d.max_val, d.eps, d.weight = window, SIGMA, max_val, EPS, weight
    d.ws, d.ws_elems = ws.data_ptr(), elems
    d.loss = None if skip == "loss" else loss.data_ptr()
    d.value = None if skip == "value" else value.data_ptr()
    d.grad_pred = None if skip == "grad_pred" else grad.data_ptr()
    L.call("nirgan_ssim_loss", C.byref(d), st)
    sync(dev)
    what = f"{shape} {kind} max_val {max_val} weight {weight} without {skip}"
    assert all(bands_intact(b, k) for b, k in ((ws_buf, elems), (loss_buf, 1), (value_buf, 1), (grad_buf, n))), what + ": wrote outside its outputs"
    assert same(xd, c["x"]) and same(yd, c["y"]), what + ": changed its inputs"
    if skip == "loss":
        assert same(loss, torch.full((1,), LOSS0))
    else:
        within("ssim value", what + " loss", loss[0], c["loss"], c["loss_b"])
    if skip == "value":
        assert all_nan_bitwise(value)
    else:
        within("ssim value", what + " value", value[0], c["value"], c["value_b"])
    if skip == "grad_pred":
        assert same(grad, c["base"].reshape(-1)), what + ": grad_pred is NULL and the buffer moved"
        assert all_nan_bitwise(ws[n_maps:n_maps + n_f]), what + ": value only, and the adjoint's region of the workspace was written"
    else:
        within("ssim gradient", what, grad, c["grad"].reshape(-1), c["grad_b"].reshape(-1))


def ssim_loss_against_float64(dev, shape, kind):
    run_ssim_loss(dev, shape, kind)
    if (shape, kind) == SSIM_VARIED:
        run_ssim_loss(dev, shape, kind, weight=0.0)
        run_ssim_loss(dev, shape, kind, max_val=2.0)
        for skip in ("loss", "value", "grad_pred"):
            run_ssim_loss(dev, shape, kind, skip=skip)


# ---------------------------------------------------------------------------------------------------------------- emd
EMD_CASES = [((1, 1), "separated"), ((1, 15), "separated"), ((2, 1023), "separated"), ((2, 1024), "separated"), ((2, 1025), "separated"),
             ((3, 2046), "separated"), ((2, 5000), "separated"), ((2, 2000), "uniform"), ((2, 1025), "equal"), ((1, 15), "equal")]
EMD_VARIED = ((2, 1025), "separated")           # the case that also runs the NULL forms
EMD_WEIGHT = 3.0


@functools.lru_cache(maxsize=None)
def emd_inputs(shape, kind):
    B, N = shape
    gen = torch.Generator().manual_seed(63)
    r = torch.rand(B, N, generator=gen)
    noise = torch.randn(B, N, generator=gen)
    ramp = torch.linspace(-1, 1, N)
    base = 1e-4 * torch.randn(B, N, generator=gen)
    if kind == "uniform":
        return r, (r + 0.2 * noise).clamp(0, 1), base
    pred = 8 * r + 2 * ramp
    return pred, (pred.clone() if kind == "equal" else 8 * (r + 0.2 * noise).clamp(0, 1) - 2 * ramp), base


def suffix_sums(s):
    return s.flip(1).cumsum(1).flip(1)


@functools.lru_cache(maxsize=None)
def emd_case(shape, kind, weight=EMD_WEIGHT, preload=True):
    B, N = shape
    x, y, base = emd_inputs(shape, kind)
    if not preload:
        base = torch.zeros_like(base)
    loss0 = LOSS0 if preload else 0.0
    w = f32(weight)
    x64, y64 = x.double().requires_grad_(True), y.double()
    p, q = torch.softmax(x64, 1), torch.softmax(y64, 1)
    c, d = p.cumsum(1), q.cumsum(1)
    auto, = torch.autograd.grad(w * (c - d).abs().mean(), x64)
    x64, p, c = x64.detach(), p.detach(), c.detach()

    def moved(v, pr, cdf):
        rho = 2 * ULP + U * (v - v.max(1, keepdim=True).values).abs()
        below = (pr * rho).cumsum(1)
        return rho, (1 - cdf).clamp_min(0) * below + cdf * ((pr * rho).sum(1, keepdim=True) - below).clamp_min(0)
    rho, Ec = moved(x64, p, c)
    _, Ed = moved(y64, q, d)
    diff = c.float().double() - d.float().double()
    value = diff.abs().mean()
    round_b = Ec + Ed + U * (c + d)
    value_b = (round_b + U * diff.abs() + N * 2.0 ** -53).mean() + U * value
    loss = loss0 + w * value
    loss_b = w * value_b + U * w * value + U * loss.abs()
    # gradient: the closed form is autograd's
    scale = w / (B * N)
    g = suffix_sums(torch.sign(c - d))
    dot = (p * g).sum(1, keepdim=True)
    closed = scale * p * (g - dot)
    assert (closed - auto).abs().max() <= 1e-10 * max(auto.abs().max().item(), 1e-300)
    free = (c - d).abs() < round_b
    assert free[:, -1].all()
    rbar = (p * rho).sum(1, keepdim=True)
    gb = scale * p * ((g - dot).abs() * (rho + rbar) + (p * rho * (g - dot).abs()).sum(1, keepdim=True))
    inner = free.clone()
    inner[:, -1] = False
    flips = (torch.maximum(c, 1 - c) * inner).sum(1, keepdim=True)
    grad = base.double() + auto
    grad_b = gb + 2 * scale * p * flips + U * auto.abs() + U * grad.abs()
    return {"x": x, "y": y, "base": base, "value": value, "value_b": value_b, "loss": loss, "loss_b": loss_b, "grad": grad,
            "grad_b": grad_b, "free": free, "loss0": loss0}


def emd_conditions_hold(shape, kind):
    B, N = shape
    c = emd_case(shape, kind)
    if kind == "equal":
        assert same(c["x"], c["y"])
        return
    per_sample = c["free"].sum(1)
    print(f"emd {shape} {kind}: value {c['value'].item():.4g}, sign-free {per_sample.tolist()} of {N}")
    if N >= 1000:
        assert c["free"].sum().item() <= 0.002 * B * N
    else:
        assert per_sample.max().item() <= 2
    if kind == "separated" and N >= 1000:
        assert c["value"] > 0.1           # the CDFs separate


def emd_formulas(x, y, weight, mutate=None):
    """the kernel's formulas on the exponentials of the inputs' dtype, everything after them in double; ``mutate`` plants an error"""
    B, N = x.shape
    ex, ey = torch.exp(x - x.max(1, keepdim=True).values).double(), torch.exp(y - y.max(1, keepdim=True).values).double()
    p, q = ex / ex.sum(1, keepdim=True), ey / ey.sum(1, keepdim=True)
    diff = p.cumsum(1).float() - q.cumsum(1).float()
    count = N if mutate == "divided by N" else B * N
    value = (diff.double().abs().sum() / count).float()
    s = torch.sign(diff).double()
    g = suffix_sums(s) - (s if mutate == "exclusive suffix" else 0)
    return value, (float(weight) / count * p * (g - (p * g).sum(1, keepdim=True))).float()


def emd_reference_alone(shape, kind):
    c = emd_case(shape, kind)
    w = torch.tensor(EMD_WEIGHT, dtype=torch.float32)
    value, grad = emd_formulas(c["x"], c["y"], w)
    within("eager emd value", f"{shape} {kind} value", value, c["value"], c["value_b"])
    within("eager emd value", f"{shape} {kind} loss", LOSS0 + w * value, c["loss"], c["loss_b"])
    within("eager emd gradient", f"{shape} {kind}", c["base"] + grad, c["grad"], c["grad_b"])


def run_emd_loss(dev, shape, kind, skip=None):
    B, N = shape
    c = emd_case(shape, kind)
    xd, yd = c["x"].to(dev).contiguous(), c["y"].to(dev).contiguous()
    be, st = L.backend(), stream(dev)
    nbytes = int(be.nirgan_emd_loss_ws_bytes(B, N, 0 if skip == "grad_pred" else 1))
    assert nbytes == 8 * B + (0 if skip == "grad_pred" else 4 * B * N)
    ws_buf, ws = banded(-(-nbytes // 8), dev, torch.float64)
    loss_buf, loss = banded(1, dev)
    value_buf, value = banded(1, dev)
    grad_buf, grad = banded(B * N, dev)
    loss.fill_(LOSS0)
    grad.copy_(c["base"].reshape(-1))
    d = L.EmdLossDesc()
    d.pred, d.target, d.B, d.N, d.weight = xd.data_ptr(), yd.data_ptr(), B, N, EMD_WEIGHT
    d.ws, d.ws_bytes = ws.data_ptr(), nbytes
    d.loss = None if skip == "loss" else loss.data_ptr()
    d.value = None if skip == "value" else value.data_ptr()
    d.grad_pred = None if skip == "grad_pred" else grad.data_ptr()
    L.call("nirgan_emd_loss", C.byref(d), st)
    sync(dev)
    what = f"{shape} {kind} without {skip}"
    assert all(bands_intact(b, k) for b, k in ((ws_buf, ws.numel()), (loss_buf, 1), (value_buf, 1), (grad_buf, B * N))), what + ": wrote outside its outputs"
    assert same(xd, c["x"]) and same(yd, c["y"]), what + ": changed its inputs"
    if kind == "equal":
        assert skip is None
        assert same(value, torch.zeros(1)) and same(loss, torch.full((1,), LOSS0)) and same(grad, c["base"].reshape(-1)), what
        return
    if skip == "loss":
        assert same(loss, torch.full((1,), LOSS0))
    else:
        within("emd value", what + " loss", loss[0], c["loss"], c["loss_b"])
    if skip == "value":
        assert all_nan_bitwise(value)
    else:
        within("emd value", what + " value", value[0], c["value"], c["value_b"])
    if skip == "grad_pred":
        assert same(grad, c["base"].reshape(-1)), what + ": grad_pred is NULL and the buffer moved"
    else:
        within("emd gradient", what, grad, c["grad"].reshape(-1), c["grad_b"].reshape(-1))


def emd_loss_against_float64(dev, shape, kind):
    run_emd_loss(dev, shape, kind)
    if (shape, kind) == EMD_VARIED:
        for skip in ("loss", "value", "grad_pred"):
            run_emd_loss(dev, shape, kind, skip=skip)


# ---------------------------------------------------------------------------------------------------------------- hist_match
HIST_SHAPES = [(1, 1), (1, 2), (2, 7), (1, 2047), (1, 2048), (2, 2049), (1, 4100), (3, 8200)]
HIST_KINDS = ("randn", "ties", "constant image", "constant template", "two-valued template", "ascending", "descending", "wide")


@functools.lru_cache(maxsize=None)
def hist_inputs(shape, kind):
    B, N = shape
    gen = torch.Generator().manual_seed(65)
    img = torch.randn(B, N, generator=gen)
    ref = torch.rand(B, N, generator=gen) * 2 - 0.5
    plane = torch.arange(B, dtype=torch.float32)[:, None]
    if kind == "ties":
        img, ref = (img * 4).round() / 4, (ref * 16).round() / 16
        img[0, 0] = 0.0
        img[0, N - 1] = -0.0
    elif kind == "constant image":
        img = (0.37 + plane).expand(B, N).clone()
    elif kind == "constant template":
        ref = (-1.25 - plane).expand(B, N).clone()
    elif kind == "two-valued template":
        ref = torch.where(torch.rand(B, N, generator=gen) < 0.3 + 0.2 * plane, torch.full((B, N), -0.5), 2.0 + plane.expand(B, N))
    elif kind == "ascending":
        img = img.sort(1).values
    elif kind == "descending":
        img = img.sort(1, descending=True).values
    elif kind == "wide":
        wide = lambda n: ((torch.randint(0, 2, (n,), generator=gen) * 2 - 1) * 10.0 ** (60 * torch.rand(n, generator=gen, dtype=torch.float64) - 30)).float()
        img, ref = wide(B * N).reshape(B, N), wide(B * N).reshape(B, N)
        without_ties(img, wide)
        without_ties(ref, wide)
    elif kind == "randn":
        without_ties(img, lambda n: torch.randn(n, generator=gen))
        without_ties(ref, lambda n: torch.rand(n, generator=gen) * 2 - 0.5)
    return img.contiguous(), ref.contiguous()


def without_ties(t, draw):
    """draws the elements of a plane that tie with another one again (8200 fp32 draws do tie now and then)"""
    for b in range(t.shape[0]):
        for _ in range(20):
            _, inverse, counts = torch.unique(t[b], return_inverse=True, return_counts=True)
            tied = counts[inverse] > 1
            if not tied.any():
                break
            t[b, tied] = draw(int(tied.sum()))


@functools.lru_cache(maxsize=None)
def hist_case(shape, kind):
    B, N = shape
    img, ref = hist_inputs(shape, kind)
    assert torch.isfinite(img).all() and torch.isfinite(ref).all()
    want = O.histogram_match(img.double().reshape(B, 1, 1, N), ref.double().reshape(B, 1, 1, N)).reshape(B, N)
    assert want.dtype == torch.float64
    # np.interp returns fp[i] where x == xp[i], and fp[0] below xp[0]: those elements are template values, untouched
    a, t = img.double().numpy(), ref.double().numpy()
    kept, tv = np.zeros((B, N), dtype=bool), np.zeros((B, N))
    for b in range(B):
        ss, ts = np.sort(a[b]), np.sort(t[b])
        r = np.searchsorted(ss, a[b], side="right")
        tv[b] = ts[r - 1]
        kept[b] = (np.searchsorted(ts, tv[b], side="right") == r) | (np.searchsorted(ts, tv[b], side="left") == 0)
    tie_free = all(np.unique(v[b]).size == N for v in (a, t) for b in range(B))
    return {"img": img, "ref": ref, "want": want, "bound": U * want.abs() + 1e-12 * want.abs().clamp_min(1.0),
            "kept": torch.from_numpy(kept), "tv": torch.from_numpy(tv), "tie_free": tie_free}


def hist_conditions_hold(shape):
    B, N = shape
    for kind in HIST_KINDS:
        c = hist_case(shape, kind)
        if B > 1:
            assert not same(c["img"][0], c["img"][1])
            assert not same(c["ref"][0], c["ref"][1])
        if kind in ("randn", "wide") and N > 1:
            assert c["tie_free"]
        if kind == "wide" and N > 1000:
            assert c["img"].abs().min() < 1e-25 and c["img"].abs().max() > 1e25 and (c["img"] < 0).any() and (c["img"] > 0).any()
        if kind == "ties" and N >= 7:
            assert (bits(c["img"]) == 0).any() and (bits(c["img"]) == -2 ** 31).any() and not c["kept"].all()
        if kind == "constant template":
            assert c["kept"].all()
        assert (c["want"][c["kept"]] == c["tv"][c["kept"]]).all()


def hist_formula(img, ref, mutate=None):
    """the kernel's route in numpy: ranks by binary search in the sorted planes, interpolation in double, one rounding"""
    B, N = img.shape
    a, t = img.numpy(), ref.numpy()
    out = np.zeros((B, N), dtype=np.float32)
    for b in range(B):
        ss, ts = np.sort(a[b]), np.sort(t[0 if mutate == "template of plane 0" else b]).astype(np.float64)
        if mutate == "signed zeros apart":
            key = lambda v: np.where(np.signbit(v), -1.0, 1.0) * 1e-45 + v.astype(np.float64)
            r = np.searchsorted(np.sort(key(a[b])), key(a[b]), side="right")
        elif mutate == "lower bound":
            r = np.searchsorted(ss, a[b], side="left") + 1
        else:
            r = np.searchsorted(ss, a[b], side="right")
        tv = ts[r - 1]
        hi, lo = np.searchsorted(ts, tv, side="right"), np.searchsorted(ts, tv, side="left")
        prev = ts[np.maximum(lo - 1, 0)]
        inv_n = 1.0 / N
        with np.errstate(divide="ignore", invalid="ignore"):
            res = (tv - prev) / (hi * inv_n - lo * inv_n) * (r * inv_n - lo * inv_n) + prev
        out[b] = np.where((hi == r) | (lo == 0), tv, res).astype(np.float32)
    return torch.from_numpy(out)


def hist_check(c, got, what, family="hist"):
    got = got.cpu().reshape(c["want"].shape)
    within(family, what, got, c["want"], c["bound"])
    kept = c["kept"]
    assert (got.double()[kept] == c["tv"][kept]).all(), what + ": an element np.interp returns unchanged is not the template's value"
    for b in range(got.shape[0]):
        assert np.isin(bits(got[b][kept[b]]).numpy(), bits(c["ref"][b]).numpy()).all(), what + ": not bitwise an element of the template"
    if c["tie_free"]:
        assert same(got.sort(1).values, c["ref"].sort(1).values), what + ": tie-free inputs, and the output is no permutation of the template"


def hist_reference_alone(shape):
    for kind in HIST_KINDS:
        c = hist_case(shape, kind)
        hist_check(c, hist_formula(c["img"], c["ref"]), f"{shape} {kind}", "eager hist")


def hist_match_against_float64(dev, shape):
    B, N = shape
    be, st = L.backend(), stream(dev)
    nbytes = int(be.nirgan_hist_match_ws_bytes(B, N))
    P = 2048
    while P < N:
        P *= 2
    assert nbytes == 12 * B * P
    for kind in HIST_KINDS:
        c = hist_case(shape, kind)
        img, ref = c["img"].to(dev).contiguous(), c["ref"].to(dev).contiguous()
        ws_buf, ws = banded(nbytes // 8, dev, torch.float64)
        out_buf, out = banded(B * N, dev)
        d = L.HistMatchDesc()
        d.image, d.reference, d.B, d.N = img.data_ptr(), ref.data_ptr(), B, N
        d.ws, d.ws_bytes, d.out = ws.data_ptr(), nbytes, out.data_ptr()
        L.call("nirgan_hist_match", C.byref(d), st)
        sync(dev)
        what = f"{shape} {kind}"
        assert bands_intact(out_buf, B * N) and bands_intact(ws_buf, ws.numel()), what + ": wrote outside its outputs"
        assert same(img, c["img"]) and same(ref, c["ref"]), what + ": changed its inputs"
        hist_check(c, out, what)


# ---------------------------------------------------------------------------------------------------------------- guards
def refused(rc, be, entry):
    return rc == -1 and entry in be.nirgan_last_error()


def metric_loss_guards(dev):
    """every refused call returns -1, names its entry and launches nothing"""
    be, st = L.backend(), stream(dev)
    shape, kind = (2, 12, 9, 11), "rand"
    P, H, W, window = shape
    x, y, _ = ssim_images(shape, kind)
    xd, yd = x.to(dev).contiguous(), y.to(dev).contiguous()
    bad_geometry = [{"window": 10}, {"window": 13}, {"H": 5}, {"W": 5}]

    def metrics_desc(out, ws):
        d = L.MetricsDesc()
        d.pred, d.target, d.planes, d.H, d.W = xd.data_ptr(), yd.data_ptr(), P, H, W
        d.window, d.sigma, d.max_val, d.eps = window, SIGMA, 1.0, EPS
        d.ws, d.ws_elems, d.means = ws.data_ptr(), ws.numel(), out.data_ptr()
        return d
    for change in bad_geometry + [{"ws_elems": 3 * tiles(shape) - 1}, {"pred": None}, {"target": None}, {"ws": None}, {"means": None}]:
        out, ws = nan(3, dev=dev), nan(3 * tiles(shape), dev=dev)
        d = metrics_desc(out, ws)
        for k, v in change.items():
            setattr(d, k, v)
        assert refused(be.nirgan_image_metrics(C.byref(d), st), be, b"image_metrics"), change
        sync(dev)
        assert all_nan_bitwise(out) and all_nan_bitwise(ws), f"image_metrics {change}: the refused call launched something"

    elems = int(be.nirgan_ssim_loss_ws_elems(P, H, W, window))
    for change in bad_geometry + [{"ws_elems": elems - 1}, {"pred": None}, {"target": None}, {"ws": None}]:
        ws, loss, value, grad = nan(elems, dev=dev), nan(1, dev=dev), nan(1, dev=dev), nan(P * H * W, dev=dev)
        d = L.SsimLossDesc()
        d.pred, d.target, d.planes, d.H, d.W = xd.data_ptr(), yd.data_ptr(), P, H, W
        d.window, d.sigma, d.max_val, d.eps, d.weight = window, SIGMA, 1.0, EPS, WEIGHT
        d.ws, d.ws_elems, d.loss, d.value, d.grad_pred = ws.data_ptr(), elems, loss.data_ptr(), value.data_ptr(), grad.data_ptr()
        for k, v in change.items():
            setattr(d, k, v)
        assert refused(be.nirgan_ssim_loss(C.byref(d), st), be, b"ssim_loss"), change
        sync(dev)
        assert all(all_nan_bitwise(t) for t in (ws, loss, value, grad)), f"ssim_loss {change}: the refused call launched something"

    B, N = 2, 15
    ex, ey, _ = emd_inputs((B, N), "separated")
    exd, eyd = ex.to(dev).contiguous(), ey.to(dev).contiguous()
    nbytes = int(be.nirgan_emd_loss_ws_bytes(B, N, 1))
    for change in [{"ws_bytes": nbytes - 1}, {"ws": "misaligned"}, {"N": 1 << 24}, {"pred": None}, {"target": None}, {"ws": None}]:
        ws = torch.full((nbytes // 8 + 2,), float("nan"), dtype=torch.float64, device=dev)
        loss, value, grad = nan(1, dev=dev), nan(1, dev=dev), nan(B * N, dev=dev)
        d = L.EmdLossDesc()
        d.pred, d.target, d.B, d.N, d.weight = exd.data_ptr(), eyd.data_ptr(), B, N, EMD_WEIGHT
        d.ws, d.ws_bytes, d.loss, d.value, d.grad_pred = ws.data_ptr(), nbytes, loss.data_ptr(), value.data_ptr(), grad.data_ptr()
        for k, v in change.items():
            setattr(d, k, ws.data_ptr() + 4 if v == "misaligned" else v)
        assert refused(be.nirgan_emd_loss(C.byref(d), st), be, b"emd_loss"), change
        sync(dev)
        assert all(all_nan_bitwise(t) for t in (ws, loss, value, grad)), f"emd_loss {change}: the refused call launched something"

    B, N = 2, 7
    img, ref = (t.to(dev).contiguous() for t in hist_inputs((B, N), "randn"))
    nbytes = int(be.nirgan_hist_match_ws_bytes(B, N))
    for change in [{"ws_bytes": nbytes - 1}, {"ws": "misaligned"}, {"image": None}, {"reference": None}, {"out": None}, {"ws": None}]:
        ws = torch.full((nbytes // 8 + 2,), float("nan"), dtype=torch.float64, device=dev)
        out = nan(B * N, dev=dev)
        d = L.HistMatchDesc()
        d.image, d.reference, d.B, d.N = img.data_ptr(), ref.data_ptr(), B, N
        d.ws, d.ws_bytes, d.out = ws.data_ptr(), nbytes, out.data_ptr()
        for k, v in change.items():
            setattr(d, k, ws.data_ptr() + 4 if v == "misaligned" else v)
        assert refused(be.nirgan_hist_match(C.byref(d), st), be, b"hist_match"), change
        sync(dev)
        assert all_nan_bitwise(ws) and all_nan_bitwise(out), f"hist_match {change}: the refused call launched something"


# ---------------------------------------------------------------------------------------------------------------- the Python surfaces
def python_surfaces(dev):
    """utils.losses.ssim_loss / emd_loss with their autograd bridges, utils.calculate_metrics.image_metrics_device and
    nirgan_hip.inference.histogram_match, one small case each under the bounds of the raw entries (weight 1, nothing preloaded)"""
    from nirgan_hip.inference import histogram_match
    from utils.calculate_metrics import image_metrics_device
    from utils.losses import emd_loss, ssim_loss
    shape, kind = (2, 12, 9, 11), "rand"
    P, H, W, window = shape
    c = ssim_case(shape, kind, 1.0, 1.0, False)
    pa, t = c["x"].reshape(P, 1, H, W).to(dev).requires_grad_(True), c["y"].reshape(P, 1, H, W).to(dev)
    v = ssim_loss(pa, t, window)
    (2.0 * v).backward()
    within("ssim value", "utils.losses.ssim_loss", v.detach(), c["value"], c["value_b"])
    within("ssim gradient", "utils.losses.ssim_loss, scaled by 2", pa.grad.reshape(P, H, W), 2 * c["grad"], 2 * c["grad_b"])
    within("ssim value", "utils.losses.ssim_loss, value only", ssim_loss(pa.detach(), t, window), c["value"], c["value_b"])
    m = metrics_case(shape, kind)
    within("metrics", "image_metrics_device", image_metrics_device(pa.detach(), t, window_size=window), m["means"], m["means_b"])
    eshape = (2, 1025)
    e = emd_case(eshape, "separated", 1.0, False)
    pa, t = e["x"].reshape(2, 1, 25, 41).to(dev).requires_grad_(True), e["y"].reshape(2, 1, 25, 41).to(dev)
    v = emd_loss(pa, t)
    (2.0 * v).backward()
    within("emd value", "utils.losses.emd_loss", v.detach(), e["value"], e["value_b"])
    within("emd gradient", "utils.losses.emd_loss, scaled by 2", pa.grad.reshape(eshape), 2 * e["grad"], 2 * e["grad_b"])
    within("emd value", "utils.losses.emd_loss, value only", emd_loss(pa.detach(), t), e["value"], e["value_b"])
    hshape = (2, 2049)
    h = hist_case(hshape, "ties")
    got = histogram_match(h["img"].reshape(2, 1, 3, 683).to(dev), h["ref"].reshape(2, 1, 3, 683).to(dev))
    assert got.shape == (2, 1, 3, 683)
    hist_check(h, got.reshape(hshape), "inference.histogram_match")
