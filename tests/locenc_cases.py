"""nirgan_location_encoder (csrc/locenc.hip: lon/lat -> real spherical harmonics -> SirenNet, fp64) against extended precision: the cases,
references, bounds and bodies shared by tests/test_gpu_locenc.py (the MI355X) and tests/test_locenc_emulated.py (the numpy emulator, the
conditions on the bounds, and emulators with one planted error each).  Bodies launch the RAW entry through L.LocEncDesc, so the options
the LocationEncoder module never produces (one and eight layers, null biases, an identity in the middle, a sine at the end, no
`features`, odd and tiny widths) are reached; every output sits between 64 sentinel elements which must stay untouched.

THE REFERENCE is numpy longdouble (x87 extended, eps 1.08e-19; asserted at import), in the reference project's operation order
(oracle/nirgan_oracle.py::spherical_harmonics and the emulator's loop), with the constant K from exact fractions.Fraction factorial
ratios converted once to longdouble (exact_norm).

HARMONICS.  phi, theta and m * phi are single IEEE operations in the same order on every side: they are computed in float64 on the host
and nothing is asked of them.  Only cos / sin and the arithmetic can differ, so feature f of coordinate i is held to

    |got - ref| <= 4 * A * S + E(i, f)

  E  the envelope of the longdouble reference while x = cos(theta) ranges over [x - k ulp, x + k ulp] (clamped to [-1, 1]) and
     cos(m phi) / sin(|m| phi) over +- k ulp: evaluated at both ends against the centre, plus |dP/dx| * k ulp from a longdouble
     central difference (step ulp / 16) so that a sign change inside the interval does not escape.  Near a pole this is where the
     whole bound comes from: sqrt((1 - x)(1 + x)) loses all relative accuracy in 1 + x, and at |lat| = 89.999999 one ulp of x moves
     the m = +-1 features by 1e-7 (L = 10) to 1e-6 (L = 45); E is 1e-14 and less away from the poles.
  k  the accuracy of OCML's double cos / sin in ulps.  SOURCE: the ROCm installation carries no accuracy table for the OCML / HIP
     math functions (nothing under its documentation or include directories states one), so k = 2 is used, the fallback this
     suite's plan names.  glibc's cos / sin stay inside 1 ulp: with k = 1 the float64 restatement (the emulator) passes every case,
     which tests/test_locenc_emulated.py asserts.
  S  max |Y| of the case.
  A  MEASURED, not chosen: the worst error, relative to S, of the float64 restatement (float64_harmonics, sh_normalisation's K)
     against the longdouble reference on the same 33 coordinates, both fed the SAME float64 x and phi.  The device gets 4 times
     that, which covers FMA contraction and another evaluation order of the same recurrence and nothing else.  Measured here
     (measure_arithmetic; the emulated file asserts that the measurement stays at or below the record):

         L          1        2        10        10 generator-text   16        32        33        45
         A * S      3.9e-18  7.0e-17  2.1e-15   6.9e-15             7.7e-15   6.3e-14   6.7e-14   1.7e-13
         S          0.282    0.489    1.230     3.863               1.571     2.239     2.274     2.661
         A          1.36e-17 1.42e-16 1.71e-15  1.78e-15            4.87e-15  2.79e-14  2.93e-14  6.28e-14

     For L >= 10 the worst feature is at (13.4, 89.999999); away from the poles and the three near-pole points the figures are
     1.3e-15 (L = 10) and 5.6e-14 (L = 45).  The records in ARITH are the row A, rounded up in the third digit.

  At the exact poles x = -+1 comes out of cos exactly, every m != 0 feature must be exactly 0.0 and the zonal ones K * (-+1)^l within
  the arithmetic term alone.  A standalone SphericalHarmonics launch returns the encoder launch's `features` bit for bit.

SIREN LAYERS, teacher-forced: the longdouble reference is fed the launch's OWN `features`, so pole conditioning does not leak into the
layer check.  A running bound is carried through the layers as tests/streaming_cases.py does for Adam, with u = 2^-53:
    dot product   e_z = (din + 8) * u * (sum |w||x| + |b|) + sum |w| * e_x
    sine          e   = w0 * e_z + k * u              (identity: e = e_z)
and `out` is compared within the final bound, on the device and on the emulator alike.

FOUND: nothing in the kernel.  On the MI355X every case passes: at |lat| <= 84 the worst feature error is 4.5e-15 (L = 10) and 1.9e-14
(L = 45), 0.16 and 0.02 of its bound; over all coordinates the worst error / bound is 0.25 (L = 1: the rounding of K) and 0.09 - 0.18
elsewhere, and the near-pole errors (2e-8 at L = 10, 2e-7 at L = 45) are those of one ulp in cos(theta), the same as libm's.  cos of
fl(pi) and of 0 come out as exactly -1 and 1.  The layers stay below 2e-15 of the longdouble reference (bounds 3e-16 .. 3e-10).
The case "identity-inside-sine-last" has three layers and is given four frequencies (30, 0, 1, 1), as the plan lists them: the
entry reads the first three, so the identity is the middle layer and the last layer has a sine.
"""
import ctypes as C
import fractions
import functools
import math
import os

import numpy as np
import torch

from nirgan_hip import lib as L
from model.satclip.location_encoder import (HARMONICS_VARIANTS, LocationEncoder, SphericalHarmonics, get_neural_network,
                                            get_positional_encoding, sh_normalisation)

LD = np.longdouble
assert np.finfo(LD).eps <= 1.1e-19, f"numpy longdouble is not x87 extended precision here (eps {np.finfo(LD).eps}): the reference of these tests needs it"

U = 2.0 ** -53
K_ULP = 2                       # OCML double cos / sin (see above); glibc: 1
ARITH_FACTOR = 4                # the device's multiple of the measured arithmetic error
GUARD = 64
SENTINEL = 0x7FF8DEADBEEF0123   # a quiet NaN with a payload: an element nobody wrote is not finite, a guard is compared as bits
D2R = math.pi / 180.0           # torch.deg2rad, the kernel: x * (pi / 180)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# measured arithmetic error of the float64 restatement relative to max |Y| (A above), per L; rounded up from measure_arithmetic
ARITH = {1: 1.36e-17, 2: 1.42e-16, 10: 1.78e-15, 16: 4.87e-15, 32: 2.79e-14, 33: 2.93e-14, 45: 6.28e-14}

HARMONICS_CASES = [(1, "closed-form"), (2, "closed-form")] + [(10, v) for v in HARMONICS_VARIANTS] + \
                  [(16, "closed-form"), (32, "closed-form"), (33, "closed-form"), (45, "closed-form")]

# (name, L, widths, w0, layers without a bias)
SIREN_CASES = [
    ("one-layer-4-1", 2, (4, 1), (0.0,), ()),
    ("4-2", 2, (4, 2), (0.0,), ()),
    ("odd-widths-null-biases", 2, (4, 31, 33, 63, 65, 1), (30.0, 1.0, 1.0, 1.0, 0.0), (1, 3)),
    ("eight-layers-of-3", 2, (4,) + (3,) * 8, (30.0,) + (1.0,) * 6 + (0.0,), ()),
    ("identity-inside-sine-last", 10, (100, 65, 64, 7), (30.0, 0.0, 1.0, 1.0), ()),      # three layers: the fourth frequency is never read
    ("gates-2025-33-2048-5", 45, (2025, 33, 2048, 5), (30.0, 1.0, 0.0), ()),
    ("satclip-100-512-512-256", 10, (100, 512, 512, 256), (30.0, 1.0, 0.0), ()),
]
SIREN = {c[0]: c for c in SIREN_CASES}
BITWISE_CASES = ["odd-widths-null-biases", "identity-inside-sine-last"]


# ---------------------------------------------------------------------------------------------------- exact constants
def ld_fraction(fr) -> LD:
    """a Fraction as longdouble, correct to an ulp of longdouble whatever the size of its terms"""
    fr = fractions.Fraction(fr)
    p, q = abs(fr.numerator), fr.denominator
    if p == 0:
        return LD(0)
    s = 160 - (p.bit_length() - q.bit_length())
    n = (p << s) // q if s >= 0 else p // (q << -s)
    acc = LD(0)
    for i in reversed(range((n.bit_length() + 31) // 32)):
        acc = acc * LD(4294967296.0) + LD(float((n >> (32 * i)) & 0xFFFFFFFF))
    return np.ldexp(acc, -s) * (-1 if fr < 0 else 1)


PI = ld_fraction(fractions.Fraction(31415926535897932384626433832795028841971693993751, 10 ** 49))


def exact_norm(L_, variant="closed-form"):
    """the constant in front of P_l^|m| * {1, cos(m phi), sin(|m| phi)} (model/satclip/location_encoder.py::sh_normalisation) from exact
    factorial ratios, longdouble [L*L]"""
    assert variant in HARMONICS_VARIANTS
    out = np.zeros(L_ * L_, dtype=LD)
    for l in range(L_):
        for m in range(-l, l + 1):
            am = abs(m)
            ratio = fractions.Fraction((2 * l + 1) * math.factorial(l - am), 4 * math.factorial(l + am))
            if m != 0:
                k = np.sqrt(ld_fraction(2 * ratio) / PI) * (1 if variant == "closed-form" else (-1) ** am)
            elif variant == "analytic-generator-text":
                k = np.sqrt(ld_fraction(fractions.Fraction(2 * l + 1, 4)) * PI)
            else:
                k = np.sqrt(ld_fraction(ratio) / PI)
            out[l * l + l + m] = k
    return out


# ---------------------------------------------------------------------------------------------------- coordinates
@functools.lru_cache(maxsize=None)
def _coordinates():
    fixed = [(0, 90), (0, -90), (180, 90), (-180, -90),
             (180, 0), (-180, 0), (0, 0), (179.999999, 45), (0, 1e-9),
             (13.4, 89.999999), (-77, -89.999999), (10, 89.9),
             (20, 84), (20, -84)]
    f6 = np.load(os.path.join(GOLDEN, "f6_locenc.npz"))["lonlat"].astype(np.float64)
    assert f6.shape == (12, 2)
    rng = np.random.RandomState(20)
    rest = np.stack((rng.uniform(-180, 180, 7), rng.uniform(-90, 90, 7)), -1)
    ll = np.concatenate((np.array(fixed, dtype=np.float64), f6, rest))
    assert ll.shape == (33, 2)
    return ll


def coordinates():
    """[33][2] (lon, lat): the poles, the date line, the equator, three near-pole points, the Sentinel-2 limit, fixture f6, seeded points"""
    return _coordinates().copy()


POLES = {0: 90.0, 1: -90.0, 2: 90.0, 3: -90.0}        # row -> latitude of the exact poles
NEAR_POLE = (9, 10, 11)


def angles(ll):
    """phi, theta in float64, as every implementation forms them"""
    return (ll[:, 0] + 180.0) * D2R, (ll[:, 1] + 90.0) * D2R


# ---------------------------------------------------------------------------------------------------- the recurrence, any precision
def legendre_table(x, L_):
    """P_l^|m|(x) at [..., l*l+l+m] in x's dtype, in the reference's operation order.  One run per order |m| serves every degree: the
    reference's loop for (l, m) passes through the values of (m, m), (m+1, m), ... with the same operations."""
    P = np.zeros(x.shape + (L_ * L_,), dtype=x.dtype)
    somx2 = np.sqrt((1 - x) * (1 + x))
    pmm, fact = np.ones_like(x), 1.0
    for am in range(L_):
        if am > 0:
            pmm = pmm * (-fact) * somx2
            fact += 2.0
        seq = [pmm]
        if am + 1 < L_:
            seq.append(x * (2.0 * am + 1.0) * pmm)
        for q in range(am + 2, L_):
            seq.append(((2.0 * q - 1.0) * x * seq[-1] - (q + am - 1.0) * seq[-2]) / (q - am))
        for l, v in zip(range(am, L_), seq):
            P[..., l * l + l + am] = v
            P[..., l * l + l - am] = v
    return P


def azimuth_table(phi, L_, dtype):
    """1, cos(m phi), sin(|m| phi) at [B, l*l+l+m]; m * phi is the float64 product on every side, the function is evaluated in dtype"""
    T = np.ones(phi.shape + (L_ * L_,), dtype=dtype)
    for am in range(1, L_):
        arg = (float(am) * phi).astype(dtype)
        c, s = np.cos(arg), np.sin(arg)
        for l in range(am, L_):
            T[:, l * l + l + am] = c
            T[:, l * l + l - am] = s
    return T


def float64_harmonics(x, phi, K, L_):
    """the float64 restatement of the kernel on given float64 x = cos(theta) and phi"""
    assert x.dtype == np.float64 and phi.dtype == np.float64 and K.dtype == np.float64
    return (K * azimuth_table(phi, L_, np.float64)) * legendre_table(x, L_)


def product_norm(L_, variant):
    return sh_normalisation(L_, variant).numpy().copy()


@functools.lru_cache(maxsize=None)
def measure_arithmetic(L_, variant):
    """(worst error, S): float64 restatement with the product's K against longdouble with the exact K, on the same float64 x and phi"""
    phi, theta = angles(coordinates())
    x = np.cos(theta)
    ref = (exact_norm(L_, variant) * azimuth_table(phi, L_, LD)) * legendre_table(x.astype(LD), L_)
    got = float64_harmonics(x, phi, product_norm(L_, variant), L_)
    return float(np.abs(got.astype(LD) - ref).max()), float(np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def _geometry(L_, k):
    """what the bound needs and K does not touch: P at the centre, its envelope over x +- k ulp, the azimuth factor and its k ulp"""
    phi, theta = angles(coordinates())
    xc = np.cos(theta.astype(LD))
    ulp = np.spacing(np.abs(xc).astype(np.float64)).astype(LD)
    clamp = lambda v: np.minimum(np.maximum(v, LD(-1)), LD(1))
    lo, hi, dlo, dhi = clamp(xc - k * ulp), clamp(xc + k * ulp), clamp(xc - ulp / 16), clamp(xc + ulp / 16)
    P = legendre_table(np.stack((xc, lo, hi, dlo, dhi)), L_)
    slope = np.abs(P[4] - P[3]) / (dhi - dlo)[:, None]
    T = azimuth_table(phi, L_, LD)
    dT = k * np.spacing(np.abs(T).astype(np.float64)).astype(LD)
    zonal = [l * l + l for l in range(L_)]
    dT[:, zonal] = 0
    env = np.maximum(np.abs(P[1] - P[0]), np.abs(P[2] - P[0]))
    spread = (np.abs(T) + dT) * env + dT * np.abs(P[0]) + np.abs(T) * slope * (k * ulp)[:, None]
    return P[0], T, spread


@functools.lru_cache(maxsize=None)
def harmonics_reference(L_, variant, k):
    """(Y, E, S): the longdouble reference, the envelope E(i, f) for k ulp in cos / sin, max |Y|.  Shared; left unchanged."""
    Pc, T, spread = _geometry(L_, k)
    K = exact_norm(L_, variant)
    Y, E = K * T * Pc, np.abs(K) * spread
    Y.setflags(write=False)
    E.setflags(write=False)
    return Y, E, float(np.abs(Y).max())


# ---------------------------------------------------------------------------------------------------- one raw launch
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _guarded(n, dev):
    return torch.from_numpy(np.full(n + 2 * GUARD, SENTINEL, dtype=np.int64)).to(dev)


def _unguard(buf, what):
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), f"{what}: a sentinel next to the buffer was overwritten"
    return host[GUARD:-GUARD].view(np.float64).copy()


def launch(dev, lonlat, L_, K, weights, biases, w0, features=True):
    """one nirgan_location_encoder launch on numpy inputs; (out [B][dout], features [B][L*L] or None) as numpy.  Both outputs lie
    between GUARD sentinel elements, asserted untouched; an element the launch did not write stays a NaN."""
    dev = torch.device(dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    B, nf, n = lonlat.shape[0], L_ * L_, len(weights)
    dims = [weights[0].shape[1]] + [w.shape[0] for w in weights]
    keep = [t(lonlat), t(K)] + [t(w) for w in weights] + [None if b is None else t(b) for b in biases]
    out, feat = _guarded(B * dims[-1], dev), _guarded(B * nf, dev)
    d = L.LocEncDesc()
    d.lonlat, d.B, d.L, d.sh_norm, d.nlayers = keep[0].data_ptr(), B, L_, keep[1].data_ptr(), n
    wp, bp = (L.fp * n)(), (L.fp * n)()
    for i in range(n):
        wp[i] = keep[2 + i].data_ptr()
        bp[i] = None if keep[2 + n + i] is None else keep[2 + n + i].data_ptr()
    d.weights, d.biases = C.cast(wp, C.POINTER(L.fp)), C.cast(bp, C.POINTER(L.fp))
    d.dims, d.w0 = (L.i32 * (n + 1))(*dims), (C.c_double * len(w0))(*w0)
    d.out = out.data_ptr() + 8 * GUARD
    d.features = feat.data_ptr() + 8 * GUARD if features else None
    st = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    L.check(L.backend().nirgan_location_encoder(C.byref(d), st), "location_encoder")
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    o, f = _unguard(out, "out").reshape(B, dims[-1]), _unguard(feat, "features").reshape(B, nf)
    del keep
    if not features:
        assert (bits(f) == SENTINEL).all(), "features were written though the descriptor has none"
        return o, None
    return o, f


def siren_weights(name):
    """random float64 weights scaled as the SIREN initialisation (location_encoder.py::Siren), seeded by the case"""
    _, L_, dims, w0, nobias = SIREN[name]
    rng = np.random.RandomState(sum(dims) * 31 + len(dims))
    Ws, bs = [], []
    for i in range(len(dims) - 1):
        std = 1.0 / dims[i] if i == 0 else math.sqrt(6.0 / dims[i]) / (w0[i] if w0[i] != 0.0 else 1.0)
        Ws.append(rng.uniform(-std, std, (dims[i + 1], dims[i])))
        bs.append(None if i in nobias else rng.uniform(-std, std, dims[i + 1]))
    return Ws, bs


def _probe_layer(L_):
    """the one 1-wide linear layer behind the harmonics in the harmonics bodies (the entry needs a layer)"""
    rng = np.random.RandomState(L_)
    return [rng.uniform(-1.0, 1.0, (1, L_ * L_)) / (L_ * L_)], [None], (0.0,)


# ---------------------------------------------------------------------------------------------------- bodies: harmonics
def harmonics_against_longdouble(dev, L_, variant, k=K_ULP, arith=ARITH_FACTOR, report=None):
    ll = coordinates()
    K = product_norm(L_, variant)
    Ws, bs, w0 = _probe_layer(L_)
    _, got = launch(dev, ll, L_, K, Ws, bs, w0)
    Y, E, S = harmonics_reference(L_, variant, k)
    floor = arith * ARITH[L_] * S
    assert np.isfinite(got).all(), f"L={L_} {variant}: a feature is not finite"
    err = np.abs(got.astype(LD) - Y)
    if report is not None:
        calm, ratio = np.abs(ll[:, 1]) <= 84.0, err / np.maximum(floor + E, LD(1e-300))
        report(f"locenc harmonics L={L_} {variant}: S {S:.3f}, arithmetic term {floor:.2e}; worst error {float(err.max()):.2e}, "
               f"at |lat| <= 84: {float(err[calm].max()):.2e} (envelope there <= {float(E[calm].max()):.2e}); "
               f"worst error / bound {float(ratio.max()):.3f}, at |lat| <= 84: {float(ratio[calm].max()):.3f}")
    bad = np.argwhere(~(err <= floor + E))
    assert bad.size == 0, (f"L={L_} {variant}: {len(bad)} features outside 4AS + E, first at coordinate {tuple(ll[bad[0][0]])} feature {bad[0][1]}: "
                           f"error {float(err[tuple(bad[0])]):.3e}, bound {float(floor + E[tuple(bad[0])]):.3e}")
    # the exact poles: x = -+1 exactly, so every m != 0 feature is +-0 and the zonal ones are K (-+1)^l to the arithmetic term alone
    zonal = np.array([l * l + l for l in range(L_)])
    other = np.setdiff1d(np.arange(L_ * L_), zonal)
    Kx = exact_norm(L_, variant)
    for row, lat in POLES.items():
        assert (got[row, other] == 0.0).all(), f"L={L_} {variant}: an m != 0 feature at latitude {lat} is not exactly zero"
        want = Kx[zonal] * np.array([(-1.0 if lat > 0 else 1.0) ** l for l in range(L_)], dtype=LD)
        assert (np.abs(got[row, zonal].astype(LD) - want) <= floor).all(), f"L={L_} {variant}: zonal features at latitude {lat}"
    # the identity-layer path of the module: the same features, bit for bit
    alone = SphericalHarmonics(L_, variant).to(dev)(torch.from_numpy(ll).to(dev))
    assert alone.dtype == torch.float64 and same_bits(alone.cpu().numpy(), got), f"L={L_} {variant}: the standalone launch differs"
    return got


# ---------------------------------------------------------------------------------------------------- bodies: the layers
def siren_reference(feat, Ws, bs, w0, k=K_ULP):
    """(out, bound): the layers in longdouble on the given features, and the running float64 bound of the header"""
    h = feat.astype(LD)
    e = np.zeros(feat.shape)
    for W, b, f in zip(Ws, bs, w0):
        din = W.shape[1]
        mag = np.abs(h).astype(np.float64) @ np.abs(W).T + (0.0 if b is None else np.abs(b))
        e = (din + 8) * U * mag + e @ np.abs(W).T
        h = h @ W.astype(LD).T
        if b is not None:
            h = h + b.astype(LD)
        if f != 0.0:
            h, e = np.sin(LD(f) * h), f * e + k * U
    return h, e


def siren_teacher_forced(dev, name, k=K_ULP, report=None):
    _, L_, dims, w0, _ = SIREN[name]
    Ws, bs = siren_weights(name)
    out, feat = launch(dev, coordinates(), L_, product_norm(L_, "closed-form"), Ws, bs, w0)
    assert np.isfinite(feat).all() and np.isfinite(out).all(), f"{name}: an output is not finite"
    ref, bound = siren_reference(feat, Ws, bs, w0, k)
    err = np.abs(out.astype(LD) - ref)
    if report is not None:
        report(f"locenc siren {name}: worst error {float(err.max()):.2e}, bound {bound.min():.2e} .. {bound.max():.2e}, "
               f"worst error / bound {float((err / bound).max()):.3f}")
    bad = np.argwhere(~(err <= bound))
    assert out.shape == (33, dims[-1]) and bad.size == 0, \
        f"{name}: {len(bad)} outputs outside the running bound, first at {tuple(bad[0])}: error {float(err[tuple(bad[0])]):.3e}, bound {bound[tuple(bad[0])]:.3e}"


# ---------------------------------------------------------------------------------------------------- bodies: placement and bits
def placement_and_bits(dev, name):
    """a second launch and a launch without `features` give the same bits; row i of the batch is a launch of coordinate i alone"""
    _, L_, dims, w0, _ = SIREN[name]
    Ws, bs = siren_weights(name)
    ll, K = coordinates(), product_norm(L_, "closed-form")
    out, feat = launch(dev, ll, L_, K, Ws, bs, w0)
    assert np.isfinite(out).all() and np.isfinite(feat).all()
    again, fagain = launch(dev, ll, L_, K, Ws, bs, w0)
    assert same_bits(again, out) and same_bits(fagain, feat), f"{name}: two launches differ"
    bare, none = launch(dev, ll, L_, K, Ws, bs, w0, features=False)
    assert none is None and same_bits(bare, out), f"{name}: `out` depends on whether `features` is asked for"
    for i in range(ll.shape[0]):
        o1, f1 = launch(dev, ll[i:i + 1], L_, K, Ws, bs, w0)
        assert same_bits(o1[0], out[i]) and same_bits(f1[0], feat[i]), f"{name}: coordinate {i} alone differs from its row of the batch"


def module_end_to_end(dev, tmp_path):
    """LocationEncoder and SatClIP_wrapper.predict at |lat| <= 84 against the oracle within 1e-11 * max(1, |ref|); the wrapper's float32
    embedding is bitwise .float() of the float64 one"""
    import nirgan_oracle as O
    from model.satclip.satclip_wrapper import SatClIP_wrapper
    ll = coordinates()
    ll = torch.from_numpy(ll[np.abs(ll[:, 1]) <= 84.0])
    assert ll.shape[0] >= 20
    hp = {"le_type": "sphericalharmonics", "legendre_polys": 10, "harmonics_calculation": "analytic", "min_radius": 1,
          "max_radius": 360, "frequency_num": 10, "pe_type": "siren", "embed_dim": 33, "capacity": 65, "num_hidden_layers": 2}
    torch.manual_seed(11)
    net = get_neural_network("siren", 100, hp["embed_dim"], hp["capacity"], hp["num_hidden_layers"]).double()
    p = {"nnet." + k_: v.detach().clone() for k_, v in net.state_dict().items()}
    ref = O.location_encoder_forward(p, ll, 10, 2, "analytic")
    enc = LocationEncoder(get_positional_encoding("sphericalharmonics", 10, "analytic"), net).double().eval().to(dev)
    got = enc(ll.to(dev)).cpu()
    assert got.dtype == torch.float64 and torch.isfinite(got).all()
    assert ((got - ref).abs() <= 1e-11 * ref.abs().clamp(min=1.0)).all(), f"LocationEncoder: {(got - ref).abs().max().item():.3e}"
    path = os.path.join(str(tmp_path), "satclip.ckpt")
    sd = {"model.location." + k_: v for k_, v in p.items()}
    sd["model.visual.conv1.weight"] = torch.zeros(1)
    torch.save({"hyper_parameters": hp, "state_dict": sd}, path)
    emb = SatClIP_wrapper(path, device=dev).predict(ll.to(dev)).cpu()
    assert emb.dtype == torch.float32 and not emb.requires_grad
    assert torch.equal(emb.view(torch.int32), got.float().view(torch.int32)), "the wrapper's float32 embedding is not .float() of the float64 one"


# ---------------------------------------------------------------------------------------------------- bodies: refusals
FAKE = 0x10000      # a non-null address nobody dereferences: every call below is refused before anything is launched


def _fake_problem():
    keep = {"wp": (L.fp * 2)(FAKE, FAKE), "bp": (L.fp * 2)(FAKE, None), "dims": (L.i32 * 3)(4, 3, 2), "w0": (C.c_double * 2)(30.0, 0.0)}
    d = L.LocEncDesc()
    d.lonlat, d.B, d.L, d.sh_norm, d.nlayers, d.out, d.features = FAKE, 3, 2, FAKE, 2, FAKE, None
    d.weights, d.biases = C.cast(keep["wp"], C.POINTER(L.fp)), C.cast(keep["bp"], C.POINTER(L.fp))
    d.dims, d.w0 = keep["dims"], keep["w0"]
    return keep, d


def _set(field, value):
    return lambda d, keep: setattr(d, field, value)


def _item(table, i, value):
    def mutate(d, keep):
        keep[table][i] = value
    return mutate


def _many_layers(d, keep):
    keep["wp9"], keep["bp9"] = (L.fp * 9)(*[FAKE] * 9), (L.fp * 9)()
    keep["dims9"], keep["w09"] = (L.i32 * 10)(*[4] * 10), (C.c_double * 9)()
    d.weights, d.biases = C.cast(keep["wp9"], C.POINTER(L.fp)), C.cast(keep["bp9"], C.POINTER(L.fp))
    d.dims, d.w0, d.nlayers = keep["dims9"], keep["w09"], 9


REFUSALS = [(f"null {f}", _set(f, None), b"null pointer") for f in ("lonlat", "sh_norm", "weights", "biases", "dims", "w0", "out")] + [
    ("B = 0", _set("B", 0), b"empty batch"),
    ("B < 0", _set("B", -1), b"empty batch"),
    ("L = 0", _set("L", 0), b"legendre_polys=0 out of range (L*L <= 2048)"),
    ("L = 46", _set("L", 46), b"legendre_polys=46 out of range (L*L <= 2048)"),
    ("no layers", _set("nlayers", 0), b"0 linear layers (1..8)"),
    ("nine layers", _many_layers, b"9 linear layers (1..8)"),
    ("dims[0] != L*L", _item("dims", 0, 5), b"first layer expects 5 inputs, the harmonics give 4"),
    ("width 2049 inside", _item("dims", 1, 2049), b"layer 0 is 4 -> 2049 (width <= 2048)"),
    ("width 2049 at the end", _item("dims", 2, 2049), b"layer 1 is 3 -> 2049 (width <= 2048)"),
    ("width 0", _item("dims", 2, 0), b"layer 1 is 3 -> 0 (width <= 2048)"),
    ("null weights[0]", _item("wp", 0, None), b"layer 0 has no weight"),
    ("null weights[1]", _item("wp", 1, None), b"layer 1 has no weight"),
]


def refusals(be):
    """every NG_REQUIRE of the entry, on the given backend (the library or an emulator): -1, its message, nothing launched"""
    assert be.nirgan_location_encoder(None, None) == -1 and b"location_encoder: null pointer" in be.nirgan_last_error()
    for what, mutate, words in REFUSALS:
        keep, d = _fake_problem()
        mutate(d, keep)
        assert be.nirgan_location_encoder(C.byref(d), None) == -1, what
        msg = be.nirgan_last_error()
        assert b"location_encoder: " in msg and words in msg, (what, msg)


# ---------------------------------------------------------------------------------------------------- CPU only: the constant
def norm_against_exact(L_=45):
    """sh_normalisation against the exact constant: 4 float64 ulps per entry, the sign pattern, the zonal constants of the variants"""
    zonal = np.array([l * l + l for l in range(L_)])
    sign = np.ones(L_ * L_)
    for l in range(L_):
        for m in range(-l, l + 1):
            sign[l * l + l + m] = (-1.0) ** abs(m)
    exact = {v: exact_norm(L_, v) for v in HARMONICS_VARIANTS}
    for v in HARMONICS_VARIANTS:
        got = product_norm(L_, v)
        assert got.dtype == np.float64 and got.shape == (L_ * L_,)
        ulps = np.abs(got.astype(LD) - exact[v]) / np.spacing(np.abs(exact[v]).astype(np.float64)).astype(LD)
        assert (ulps <= 4).all(), f"{v}: entry {int(ulps.argmax())} is {float(ulps.max()):.2f} ulps from the exact constant"
        assert np.array_equal(np.sign(got), np.ones(L_ * L_) if v == "closed-form" else sign), f"{v}: sign pattern"
    cf, an, gt = (product_norm(L_, v) for v in ("closed-form", "analytic", "analytic-generator-text"))
    assert np.array_equal(an[zonal], cf[zonal]) and np.array_equal(np.abs(an), cf)
    other = np.setdiff1d(np.arange(L_ * L_), zonal)
    assert np.array_equal(gt[other], an[other])
    want = np.sqrt(np.array([ld_fraction(fractions.Fraction(2 * l + 1, 4)) for l in range(L_)], dtype=LD) * PI)
    assert (np.abs(gt[zonal].astype(LD) - want) <= 4 * np.spacing(want.astype(np.float64)).astype(LD)).all()
    assert abs(float(cf[0]) - 0.28209479177387814) <= 1e-16 and abs(float(gt[0]) - 0.886226925452758) <= 1e-15
