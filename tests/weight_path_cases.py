"""Bodies shared by tests/test_weight_path_emulated.py (numpy emulator, CPU) and tests/test_gpu_weight_path.py (MI355X): the small launches
that move the parameters into the kernels' layouts and the gradients back out on every training step -- the weight packs
(nirgan_pack_rows / _bf16 / _batch, csrc/igemm_wgrad.hip), the slab sums (nirgan_reduce_rows / _part / _batch), the Winograd weight
transforms (nirgan_wino6_weights / _r / _x3 / _batch, csrc/wino6.hip), their inverse for the weight gradient
(nirgan_wino6_wgrad_finish / _r / _batch) and the host code that builds the device-side job tables of the batch forms
(Plan.fuse_packs, Plan.fuse_wino6_weights, emit_deferred_reduce_rows, emit_w6_deferred_finishes in nirgan_hip/engine.py).

Every body takes ``dev`` ("cpu": the installed backend is an EmuBackend) and drives the raw entry through ``L.call``.  Nothing is expected
from the emulator or from a kernel: copies and roundings are expected as bit patterns computed here with integer arithmetic, sums and
transforms in float64 from the definitions in include/nirgan_hip.h.

Ownership.  Every output is allocated with GUARD elements behind it and pre-filled with a sentinel bit pattern (a quiet NaN no kernel
computes: SENTINEL_BITS of tests/wgrad_replay.py for fp32, SENT16 for bf16).  Every body asserts (1) each element the entry owns was
written, (2) each element it does not own still holds the sentinel -- the guard, the gap between dst_row_stride rows, columns no map
entry addresses, the padding between bf16 planes -- and (3) the values.  Where an entry accumulates, the elements it owns hold the old
value instead and everything else the sentinel.

Bounds.  u = 2^-24; the rule of tests/streaming_cases.py: an element is held to ``Kr * u * A``, A the float64 sum of the absolute values
of the terms it adds up, Kr the number of rounded operations on the longest chain to it.

pack_rows       no arithmetic: bitwise.  fp32 an exact copy (zeros where map < 0, -0.0 kept), bf16 the round-to-nearest-even upper half
                (integer restatement rne_bf16_bits; tests/test_weight_path_emulated.py holds it against torch's own conversion).
split planes    h = rne(x), m = rne(x - h), l = rne(x - h - m): both subtractions are exact in fp32 for normal-range inputs, so the host
                restatement is bitwise, and h + m + l == x is asserted exactly in float64.
reduce_rows     sum_s slab_s (+ old dst): ANY association of nsplit terms costs at most nsplit - 1 roundings on the deepest path, the
                accumulate one more, and one is slack: |got - ref| <= (nsplit + 1) u (sum_s |slab_s| + |old dst|).  With slabs and old
                values drawn from {-2, -1, 1, 2} every partial sum is an integer below 2^24: the result must be bitwise the float64 sum.
wino6_weights   U = G g G^T: two stages of at most R <= 4 fused multiply-adds each, with coefficients that are themselves rounded to
                fp32: (R + 2) roundings per stage to first order, 2 (R + 2) <= 12 for both; the hand-written forms of the F(4x4,3x3)
                variant (csrc/wino6.hip::w6_g) add before they scale and may associate differently, the rest is slack:
                |got - ref| <= 16 u (|G| |g| |G|^T).
wgrad_finish    dW = G^T (sum_s dU_s) G: the split sum (nsplit - 1 roundings, in order) in front of the same two stages.  A column of G has
                at most 7 non-zero entries (the zeros are dropped at compile time): 7 multiply-adds and the coefficient's own rounding
                per stage, 16 for both, nsplit + 15 on the longest chain and one of slack:
                |got - ref| <= (nsplit + 16) u (|G|^T (sum_s |dU_s|) |G|), plus u |result| for the one more add when the entry
                accumulates into the old gradient.

The Winograd matrices G, B^T, A^T the references use are W6M below; tests/test_weight_path_emulated.py checks them once against the
operation itself (the full identity reproduces a direct correlation to 1e-12).  It also holds eager fp32 torch of every bounded formula
inside its bound, checks the stated input conditions, and fails each body with an emulator that has one planted error.
"""
import ctypes as C
import functools

import numpy as np
import torch

from nirgan_hip import engine as E
from nirgan_hip import geometry as G
from nirgan_hip import lib as L
from streaming_cases import U, fails, stream, sync, within
from wgrad_replay import SENTINEL_BITS

GUARD = 64                      # elements behind every output that must keep the sentinel
SENT32 = SENTINEL_BITS
SENT16 = 0x7FDE                 # a bf16 quiet NaN: rounding a finite value never gives it
KINDS = ("cf", "cd1", "cd2", "tf", "syn")


# ---------------------------------------------------------------------------------------------------------------- buffers and bits
class Armed:
    """n elements (fp32, or bf16) with ``extra`` more behind them, every one the sentinel"""

    def __init__(self, n, dev, bf16=False, extra=GUARD):
        self.n, self.bf16 = int(n), bf16
        self.t = torch.full((self.n + extra,), SENT16 if bf16 else SENT32, dtype=torch.int16 if bf16 else torch.int32, device=dev)

    @property
    def ptr(self):
        return self.t.data_ptr()

    @property
    def sent(self):
        return SENT16 if self.bf16 else SENT32

    def f32(self):
        return self.t.view(torch.float32)

    def bits(self):
        a = self.t.cpu().numpy()
        return a.view(np.uint16) if self.bf16 else a.view(np.uint32)

    def preload(self, index, values):
        """old values under an accumulating entry: fp32 ``values`` at the elements ``index`` (numpy int64)"""
        self.f32()[torch.from_numpy(index).to(self.t.device)] = torch.as_tensor(values, dtype=torch.float32).to(self.t.device)


def first_n(total, n):
    m = np.zeros(total, dtype=bool)
    m[:n] = True
    return m


def owned_check(what, got, owned, sent):
    assert (got[~owned] == sent).all(), f"{what}: {int((got[~owned] != sent).sum())} elements the entry does not own were touched"
    assert (got[owned] != sent).all(), f"{what}: {int((got[owned] == sent).sum())} elements the entry owns were not written"


def to_dev(bits, dev):
    """uint32 bit patterns as an fp32 tensor on dev"""
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint32).view(np.int32)).view(torch.float32).to(dev)


def as_f32(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def rne_bf16_bits(bits32):
    """uint32 patterns of finite fp32 values -> the uint16 patterns of their nearest-even bf16"""
    b = np.asarray(bits32, dtype=np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_f32(b16):
    return (np.asarray(b16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def split3_host(x):
    """nirgan_split3's rule on fp32 values of the normal range: three uint16 planes"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = rne_bf16_bits(x.view(np.uint32))
    r1 = x - bf16_f32(h)
    m = rne_bf16_bits(r1.view(np.uint32))
    r2 = r1 - bf16_f32(m)
    return h, m, rne_bf16_bits(r2.view(np.uint32))


def planes_sum_exactly(planes, x):
    s = sum(bf16_f32(p).astype(np.float64) for p in planes)
    return bool((s == np.asarray(x, dtype=np.float32).astype(np.float64)).all())


def plane_mask(total, plane, n):
    m = np.zeros(total, dtype=bool)
    for t in range(3):
        m[t * plane:t * plane + n] = True
    return m


# ---------------------------------------------------------------------------------------------------------------- maps
@functools.lru_cache(maxsize=None)
def pack_spec(kind, N, K):
    """(index_map int32 [K], row stride, elements of the parameter) of the engine's own pack specs at small channel counts: cf =
    conv_fwd_pack, cd1 = conv_dgrad_pack over a stride-1 tap list, cd2 = conv_dgrad_pack for one stride-2 phase, tf = convT_fwd_pack for
    one phase; syn = a synthetic map with -1 entries, repeated indices and a row stride larger than K"""
    k = 3 if K % 9 == 0 else 2
    if kind == "cf":
        s, elems = G.conv_fwd_pack(N, K // (k * k), k), N * K
    elif kind == "cd1":
        cout = K // (k * k)
        s, elems = G.conv_dgrad_pack(cout, N, k, [(a, b) for a in range(k) for b in range(k)]), cout * N * k * k
    elif kind == "cd2":
        ph = G.conv_dgrad_s2_phases(8, 8, 4, 1)[1]
        assert len(ph.taps_hw) == 4
        s, elems = G.conv_dgrad_pack(K // 4, N, 4, ph.taps_hw), (K // 4) * N * 16
    elif kind == "tf":
        ph = G.convT_fwd_phases(4, 4, 3, 1)[3]
        assert len(ph.taps_hw) == 4
        s, elems = G.convT_fwd_pack(K // 4, N, 3, ph.taps_hw), (K // 4) * N * 9
    else:
        rng = np.random.default_rng(1000 + K)
        stride = K + 12
        m = rng.integers(0, stride, K).astype(np.int32)
        m[rng.random(K) < 0.2] = -1
        m[0], m[1], m[2], m[K - 1] = 3, 3, -1, stride - 1
        return m, stride, N * stride
    assert (s.N, s.K) == (N, K) and s.index_map.dtype == np.int32
    return s.index_map, s.row_stride, elems


@functools.lru_cache(maxsize=None)
def reduce_map(kind, N, K):
    """(map, dst_row_stride, dst_elems) for a slab sum: the same specs (they are the weight gradients' scatter maps: injective); syn = a
    partial permutation with -1 entries into rows of 2 K + 8"""
    if kind != "syn":
        return pack_spec(kind, N, K)
    rng = np.random.default_rng(2000 + K)
    stride = 2 * K + 8
    m = rng.permutation(stride)[:K].astype(np.int32)
    m[rng.random(K) < 0.2] = -1
    m[K - 1] = -1
    return m, stride, N * stride


def scatter_index(imap, stride, rows):
    """(flat destination index [rows][live columns], the live columns)"""
    ok = imap >= 0
    return (np.arange(rows, dtype=np.int64)[:, None] * stride + imap[None, :].astype(np.int64))[:, ok], ok


# ---------------------------------------------------------------------------------------------------------------- 1. packs
def pack_values(n, seed):
    """n fp32 bit patterns of the normal range: magnitudes 2^-60 .. 2^60, every sixth an exact bf16 tie, its neighbours one ulp either
    side, bf16-exact values, +-0.  pack_inputs puts HEAD where the map reads first, so that the smallest case packs them all: a tie
    with an even and one with an odd upper half, one ulp below and above a tie, +0, -0, 2^-60 and -2^60"""
    rng = np.random.default_rng(seed)
    up = (rng.integers(0, 2, n) << 15) | (rng.integers(67, 188, n) << 7) | rng.integers(0, 128, n)
    low = rng.integers(0, 65536, n)
    sel = np.arange(n) % 6
    for s, v in ((0, 0x8000), (1, 0x7FFF), (2, 0x8001), (3, 0)):
        low[sel == s] = v
    bits = ((up << 16) | low).astype(np.uint32)
    bits[11::17] = 0
    bits[12::17] = 0x80000000
    return bits


PACK_SHAPES32 = [(1, 4), (3, 1020), (5, 1024), (2, 1028), (65, 2304)]
PACK_SHAPES16 = [(1, 8), (3, 1032)]
PACK_CASES = [(kind, N, K, False) for N, K in PACK_SHAPES32 for kind in KINDS] + [(kind, N, K, True) for N, K in PACK_SHAPES16 for kind in KINDS]


HEAD = np.array([0x3F808000, 0x3F818000, 0x40017FFF, 0xC0018001, 0x00000000, 0x80000000, 0x21800000, 0xDD800000], dtype=np.uint32)


@functools.lru_cache(maxsize=8)
def pack_inputs(kind, N, K):
    """(map, row stride, the parameter's bits, the packed bits [N][K]); the first eight elements the map reads hold HEAD"""
    imap, stride, elems = pack_spec(kind, N, K)
    src = pack_values(elems, 7 * N + K)
    idx = np.arange(N, dtype=np.int64)[:, None] * stride + np.where(imap >= 0, imap, 0)[None, :]
    assert idx.max() < elems
    live = np.unique(idx[:, imap >= 0])
    src[live[:8]] = HEAD[:min(8, live.size)]
    return imap, stride, src, np.where(imap[None, :] >= 0, src[idx], 0).astype(np.uint32)


def pack_conditions_hold(case):
    kind, N, K, bf16 = case
    imap, stride, src, exp = pack_inputs(kind, N, K)
    assert K % 4 == 0 and (not bf16 or K % 8 == 0) and imap.shape == (K,)
    if kind == "cf":        # the last source index is the parameter's last element
        assert (N - 1) * stride + imap.max() == src.size - 1
    if kind == "syn":
        assert (imap < 0).any() and stride > K and len(set(imap[imap >= 0])) < (imap >= 0).sum()
    packed = exp[:, imap >= 0].reshape(-1)
    mag = np.abs(as_f32(packed[(packed << 1) != 0]).astype(np.float64))
    assert mag.min() >= 2.0 ** -60 and mag.max() < 2.0 ** 61, "normal range only: the host restatement of the split holds there"
    if np.unique(packed).size < 8:
        assert N * K < 8 or (kind == "syn" and N * K == 8)  # the smallest legal row; a map that reads fewer than eight distinct elements
        return
    hi, lo = packed >> 16, packed & 0xFFFF
    ties = lo == 0x8000
    assert (ties & (hi & 1 == 0)).any() and (ties & (hi & 1 == 1)).any() and (lo == 0x7FFF).any() and (lo == 0x8001).any()
    assert (packed == 0).any() and (packed == 0x80000000).any(), "+0 and -0 must reach the packed rows"
    assert mag.min() < 2.0 ** -55 and mag.max() > 2.0 ** 55


def pack_launch(dev, name, src, stride, mp, out, N, K):
    L.call(name, src.data_ptr(), src.numel(), stride, mp.data_ptr(), out.ptr, N, K, stream(dev))


def pack_against_host(dev, case):
    kind, N, K, bf16 = case
    imap, stride, src_bits, exp = pack_inputs(kind, N, K)
    src, mp, out = to_dev(src_bits, dev), i32(imap, dev), Armed(N * K, dev, bf16)
    pack_launch(dev, "nirgan_pack_rows_bf16" if bf16 else "nirgan_pack_rows", src, stride, mp, out, N, K)
    sync(dev)
    got = out.bits()
    owned_check(f"pack_rows {case}", got, first_n(got.size, N * K), out.sent)
    want = rne_bf16_bits(exp) if bf16 else exp
    bad = got[:N * K] != want.reshape(-1)
    assert not bad.any(), f"pack_rows {case}: {int(bad.sum())} packed elements differ, the first at {int(np.flatnonzero(bad)[0])}"


# a job is (kind, N, K, mode): "f32", "bf16", or "x3" (fp32 with the three bf16 planes)
PACK_TABLES = {
    1: [("cf", 5, 1024, "x3")],
    2: [("cd1", 3, 1020, "f32"), ("cf", 2, 1028, "x3")],
    7: [("syn", 1, 4, "f32"), ("cf", 3, 1032, "bf16"), ("cd2", 2, 1028, "x3"), ("tf", 65, 2304, "f32"), ("cf", 1, 8, "bf16"),
        ("cd1", 5, 1024, "x3"), ("tf", 3, 1020, "f32")],
}
PLANE_PAD = 16                  # w_x3_plane = N K + PLANE_PAD: the padding between the planes must keep the sentinel


def pack_table_conditions_hold(njobs):
    jobs = PACK_TABLES[njobs]
    assert len(jobs) == njobs
    firsts, first = {}, 0
    for kind, N, K, mode in jobs:
        firsts.setdefault(mode, []).append(first)
        first += N * -(-K // 1024)
        if mode == "x3":
            assert N * K % 8 == 0 and (N * K + PLANE_PAD) % 8 == 0
        if mode == "bf16":
            assert K % 8 == 0
    if njobs == 7:              # every kind of job also at a first_block other than 0, behind jobs of different block counts
        assert all(any(f > 0 for f in v) for v in firsts.values()) and set(firsts) == {"f32", "bf16", "x3"}
        assert len({N * -(-K // 1024) for _, N, K, _ in jobs}) >= 4 and jobs[-1][2] % 1024 != 0


class PackJob:
    def __init__(self, dev, job):
        kind, N, K, mode = job
        self.N, self.K, self.mode, self.n = N, K, mode, N * K
        self.imap, self.stride, self.src_bits, self.exp = pack_inputs(kind, N, K)
        self.src, self.mp = to_dev(self.src_bits, dev), i32(self.imap, dev)
        self.plane = self.n + PLANE_PAD
        self.out = [Armed(self.n, dev, mode == "bf16") for _ in range(2)]                       # the batch's, the single launch's
        self.tw = [Armed(3 * self.plane, dev, True) if mode == "x3" else None for _ in range(2)]

    def row(self, first):
        """the job's table row, as Plan.fuse_packs writes it"""
        return [self.src.data_ptr(), self.out[0].ptr, self.mp.data_ptr(), self.src.numel(), self.N, self.K,
                self.stride | ((1 << 32) if self.mode == "bf16" else 0), first, self.tw[0].ptr if self.tw[0] else 0, self.plane if self.tw[0] else 0]

    def single(self, dev):
        pack_launch(dev, "nirgan_pack_rows_bf16" if self.mode == "bf16" else "nirgan_pack_rows", self.src, self.stride, self.mp, self.out[1], self.N, self.K)
        if self.tw[1]:
            L.call("nirgan_split3", self.out[1].ptr, self.tw[1].ptr, self.n, self.plane, stream(dev))

    def check(self, what, host=True):
        got, one = self.out[0].bits(), self.out[1].bits()
        owned_check(what, got, first_n(got.size, self.n), self.out[0].sent)
        assert np.array_equal(got, one), f"{what}: the batch's packed rows differ from the single launch's"
        want = (rne_bf16_bits(self.exp) if self.mode == "bf16" else self.exp).reshape(-1)
        assert np.array_equal(got[:self.n], want), f"{what}: the packed rows differ from the host's"
        if self.tw[0]:
            tw, tw1 = self.tw[0].bits(), self.tw[1].bits()
            owned_check(what + " planes", tw, plane_mask(tw.size, self.plane, self.n), SENT16)
            assert np.array_equal(tw, tw1), f"{what}: the batch's planes differ from nirgan_split3's"
            planes = [tw[t * self.plane:t * self.plane + self.n] for t in range(3)]
            if host:
                assert planes_sum_exactly(planes, as_f32(want)), f"{what}: h + m + l != x"
                for name, p, q in zip("hml", planes, split3_host(as_f32(want))):
                    assert np.array_equal(p, q), f"{what}: plane {name} differs from the host's round-to-nearest-even split"


def run_pack_table(dev, jobs):
    rows, first = [], 0
    for j in jobs:
        rows.append(j.row(first))
        first += j.N * -(-j.K // 1024)
    table = torch.tensor(rows, dtype=torch.int64).to(dev)
    L.call("nirgan_pack_rows_batch", table.data_ptr(), len(rows), first, stream(dev))
    for j in jobs:
        j.single(dev)
    sync(dev)
    return table


def pack_batch_against_host(dev, njobs):
    jobs = [PackJob(dev, job) for job in PACK_TABLES[njobs]]
    run_pack_table(dev, jobs)
    for i, j in enumerate(jobs):
        j.check(f"pack_rows_batch of {njobs}, job {i} {PACK_TABLES[njobs][i]}")


SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000, 0x80400000,
                     0x7F000000, 0xFF000000, 0x00800000, 0x80800000, 0x00008000, 0x00018000, 0x3F800000, 0xBF808000], dtype=np.uint32)


def pack_batch_specials(dev):
    """+-0, subnormals and +-2^127: the batch's planes against nirgan_split3's, bitwise (no host restatement: the roundings of
    subnormal remainders are the hardware's on both sides)"""
    jobs = []
    for first in (0, 8):
        j = PackJob(dev, ("cf", 1, 8, "x3"))
        j.src_bits = SPECIALS[first:first + 8].copy()
        j.src, j.exp = to_dev(j.src_bits, dev), j.src_bits[np.where(j.imap >= 0, j.imap, 0)][None, :]
        jobs.append(j)
    run_pack_table(dev, jobs)
    for i, j in enumerate(jobs):
        j.check(f"pack_rows_batch specials, job {i}", host=False)


# ---------------------------------------------------------------------------------------------------------------- 2. slab sums
NSPLITS = [1, 2, 4, 5, 12, 13, 16, 17, 29, 32, 35]         # both sides of every hand-over between the four-way loop and the remainder
REDUCE_KS = [4, 252, 256, 260, 516]
REDUCE_NS = [1, 3]
PART_BANDS = [(0, 2), (1, 2)]                               # (row0, rows) of N = 3: from the first row; up to the last


def slab_values(shape, integer, seed):
    gen = torch.Generator().manual_seed(seed)
    if integer:
        return torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, shape, generator=gen)]
    return torch.randn(shape, generator=gen)


def reduce_expect(slabs, old, imap, stride, dst_elems, acc, row0, rows):
    """float64: (ref, A) over the dst_elems elements, and the owned mask"""
    idx, ok = scatter_index(imap, stride, rows)
    assert idx.max() < dst_elems and np.unique(idx).size == idx.size
    s = slabs.double().sum(0)[row0:row0 + rows].numpy()[:, ok]
    a = slabs.double().abs().sum(0)[row0:row0 + rows].numpy()[:, ok]
    ref, A, owned = np.zeros(dst_elems), np.zeros(dst_elems), np.zeros(dst_elems, dtype=bool)
    o = old.double().numpy()
    ref[idx], A[idx], owned[idx] = s + (o[idx] if acc else 0), a + (np.abs(o[idx]) if acc else 0), True
    return ref, A, owned


def reduce_check(what, family, out, ref, A, owned, nsplit, integer):
    got = out.bits()
    full = np.concatenate([owned, np.zeros(got.size - owned.size, dtype=bool)])
    owned_check(what, got, full, SENT32)
    val = as_f32(got[:owned.size])[owned]
    if integer:
        assert np.array_equal(val.view(np.uint32), ref[owned].astype(np.float32).view(np.uint32)), f"{what}: an exact integer sum differs"
    else:
        within(family, what, torch.from_numpy(val.copy()), torch.from_numpy(ref[owned]), torch.from_numpy((nsplit + 1) * U * A[owned]))


def reduce_one(dev, nsplit, N, K, kind, acc, integer, band=None):
    row0, rows = band or (0, N)
    imap, stride, dst_elems = reduce_map(kind, rows, K)
    slabs = slab_values((nsplit, N, K), integer, 31 * nsplit + K + N)
    old = slab_values((dst_elems,), integer, 17 * nsplit + K)
    ref, A, owned = reduce_expect(slabs, old, imap, stride, dst_elems, acc, row0, rows)
    sd, mp, out = slabs.to(dev), i32(imap, dev), Armed(dst_elems, dev)
    if acc:
        out.preload(np.flatnonzero(owned), old[torch.from_numpy(owned)])
    if band:
        L.call("nirgan_reduce_rows_part", sd.data_ptr(), nsplit, N, row0, rows, K, mp.data_ptr(), out.ptr, dst_elems, stride, acc, stream(dev))
    else:
        L.call("nirgan_reduce_rows", sd.data_ptr(), nsplit, N, K, mp.data_ptr(), out.ptr, dst_elems, stride, acc, stream(dev))
    sync(dev)
    what = f"nsplit {nsplit} N {N} K {K} {kind} acc {acc} {'integer' if integer else 'random'} band {band}"
    reduce_check(what, "reduce_rows_part" if band else "reduce_rows", out, ref, A, owned, nsplit, integer)


def reduce_combos():
    """(K, N, accumulate, map kind): every K x N x accumulate, the map kinds taken in turn"""
    return [(K, N, acc, KINDS[i % len(KINDS)]) for i, (K, N, acc) in enumerate((K, N, acc) for K in REDUCE_KS for N in REDUCE_NS for acc in (0, 1))]


assert {k for _, _, _, k in reduce_combos()} == set(KINDS) and {(N, a) for _, N, a, k in reduce_combos() if k == "syn"} >= {(1, 0), (3, 1)}


def reduce_against_float64(dev, nsplit):
    for K, N, acc, kind in reduce_combos():
        for integer in (True, False):
            reduce_one(dev, nsplit, N, K, kind, acc, integer)
            if N == 3:
                for band in PART_BANDS:
                    reduce_one(dev, nsplit, N, K, kind, acc, integer, band)


# a job is (taps, map kind, N, K, nsplit, accumulate): taps = T > 0 is the Conv2d layout (K = T Cin, the map conv_fwd_pack's, and a
# dst_row_stride of K + TAPS_PAD > Cin T)
REDUCE_TABLES = {
    2: [(9, "cf", 3, 9 * 64, 5, 1), (0, "syn", 3, 260, 13, 0)],
    5: [(0, "cf", 1, 516, 2, 0), (16, "cf", 2, 16 * 128, 17, 1), (1, "cf", 3, 64, 4, 0), (0, "cd1", 3, 252, 16, 1), (9, "cf", 1, 9 * 128, 1, 0)],
}
TAPS_PAD = 12


def reduce_table_conditions_hold(njobs):
    jobs = REDUCE_TABLES[njobs]
    assert len(jobs) == njobs and len({j[5] for j in jobs}) == 2 and {bool(j[0]) for j in jobs} == {True, False}
    for T, kind, N, K, nsplit, acc in jobs:
        if T:
            k = {1: 1, 9: 3, 16: 4}[T]
            cin = K // T
            assert cin in (64, 128) and np.array_equal(G.conv_fwd_pack(N, cin, k).index_map.reshape(T, cin), np.arange(cin)[None, :] * T + np.arange(T)[:, None])
    both = [j for n in REDUCE_TABLES for j in REDUCE_TABLES[n] if j[0]]
    assert {(K // T) for T, _, _, K, _, _ in both} == {64, 128} and {T for T, *_ in both} == {1, 9, 16}


class ReduceJob:
    def __init__(self, dev, job, integer):
        self.T, kind, self.N, self.K, self.nsplit, self.acc = job
        T, N, K = self.T, self.N, self.K
        if T:
            self.imap, self.stride = G.conv_fwd_pack(N, K // T, {1: 1, 9: 3, 16: 4}[T]).index_map, K + TAPS_PAD
            self.dst_elems = N * self.stride
        else:
            self.imap, self.stride, self.dst_elems = reduce_map(kind, N, K)
        slabs = slab_values((self.nsplit, N, K), integer, 13 * self.nsplit + K)
        old = slab_values((self.dst_elems,), integer, 19 * self.nsplit + K)
        self.ref, self.A, self.owned = reduce_expect(slabs, old, self.imap, self.stride, self.dst_elems, self.acc, 0, N)
        self.slabs, self.mp = slabs.to(dev), i32(self.imap, dev)
        self.out = [Armed(self.dst_elems, dev) for _ in range(2)]
        if self.acc:
            for o in self.out:
                o.preload(np.flatnonzero(self.owned), old[torch.from_numpy(self.owned)])

    def row(self, first):
        """as emit_deferred_reduce_rows writes it"""
        return [self.slabs.data_ptr(), self.out[0].ptr, self.mp.data_ptr(), self.nsplit, self.N, self.K, self.dst_elems,
                self.stride | (self.acc << 32), first, self.T]

    def blocks(self):
        return self.N * ((self.K // self.T // 64) if self.T else -(-self.K // 256))


def reduce_batch_against_float64(dev, njobs):
    for integer in (True, False):
        jobs = [ReduceJob(dev, job, integer) for job in REDUCE_TABLES[njobs]]
        rows, first = [], 0
        for j in jobs:
            rows.append(j.row(first))
            first += j.blocks()
        table = torch.tensor(rows, dtype=torch.int64).to(dev)
        L.call("nirgan_reduce_rows_batch", table.data_ptr(), njobs, first, stream(dev))
        for j in jobs:
            L.call("nirgan_reduce_rows", j.slabs.data_ptr(), j.nsplit, j.N, j.K, j.mp.data_ptr(), j.out[1].ptr, j.dst_elems, j.stride, j.acc, stream(dev))
        sync(dev)
        for i, j in enumerate(jobs):
            what = f"reduce_rows_batch of {njobs}, job {i} {REDUCE_TABLES[njobs][i]} {'integer' if integer else 'random'}"
            reduce_check(what, "reduce_rows_batch", j.out[0], j.ref, j.A, j.owned, j.nsplit, integer)
            assert np.array_equal(j.out[0].bits(), j.out[1].bits()), f"{what}: differs from nirgan_reduce_rows"


# ---------------------------------------------------------------------------------------------------------------- Winograd matrices
def _m(rows):
    return np.array(rows, dtype=np.float64)


# variant -> (G [n][r], B^T [n][n], A^T [mo][n]); 3 = F(4x4,3x3) over 0, 1, -1, 2, -1/2, inf; 4 = F(4x4,4x4) over 0, 1, -1, 2, -2, 1/2, inf;
# 6 = F(6x6,3x3) over 0, 1, -1, 2, -2, 1/2, -1/2, inf (include/nirgan_hip.h, nirgan_wino6_desc)
W6M = {
    3: (_m([[1 / 2, 0, 0], [1 / 6, 1 / 6, 1 / 6], [1 / 6, -1 / 6, 1 / 6], [1 / 30, 1 / 15, 2 / 15], [16 / 15, -8 / 15, 4 / 15], [0, 0, 1 / 2]]),
        _m([[2, 3, -4, -3, 2, 0], [0, 2, 5, 1, -2, 0], [0, 2, 1, -5, 2, 0], [0, -1, -2, 1, 2, 0], [0, -2, 1, 2, -1, 0], [0, 2, 3, -4, -3, 2]]),
        _m([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -1 / 2, 0], [0, 1, 1, 4, 1 / 4, 0], [0, 1, -1, 8, -1 / 8, 1]])),
    4: (_m([[1 / 4, 0, 0, 0], [1 / 6, 1 / 6, 1 / 6, 1 / 6], [1 / 18, -1 / 18, 1 / 18, -1 / 18], [1 / 72, 1 / 36, 1 / 18, 1 / 9],
            [1 / 120, -1 / 60, 1 / 30, -1 / 15], [32 / 45, 16 / 45, 8 / 45, 4 / 45], [0, 0, 0, 1 / 2]]),
        _m([[4, -8, -5, 10, 1, -2, 0], [0, -4, 4, 9, -1, -2, 0], [0, -4, 12, -7, -3, 2, 0], [0, 2, -3, -4, 3, 2, 0], [0, 2, -5, 0, 5, -2, 0],
            [0, 4, 0, -5, 0, 1, 0], [0, -4, 8, 5, -10, -1, 2]]),
        _m([[1, 1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 1 / 2, 0], [0, 1, 1, 4, 4, 1 / 4, 0], [0, 1, -1, 8, -8, 1 / 8, 1]])),
    6: (_m([[1 / 4, 0, 0], [1 / 18, 1 / 18, 1 / 18], [1 / 18, -1 / 18, 1 / 18], [1 / 360, 1 / 180, 1 / 90], [1 / 360, -1 / 180, 1 / 90],
            [16 / 45, 8 / 45, 4 / 45], [16 / 45, -8 / 45, 4 / 45], [0, 0, 1 / 4]]),
        _m([[4, 0, -21, 0, 21, 0, -4, 0], [0, -4, -4, 17, 17, -4, -4, 0], [0, 4, -4, -17, 17, 4, -4, 0], [0, 2, 1, -10, -5, 8, 4, 0],
            [0, -2, 1, 10, -5, -8, 4, 0], [0, 4, 8, -5, -10, 1, 2, 0], [0, -4, 8, 5, -10, -1, 2, 0], [0, -4, 0, 21, 0, -21, 0, 4]]),
        _m([[1, 1, 1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 1 / 2, -1 / 2, 0], [0, 1, 1, 4, 4, 1 / 4, 1 / 4, 0], [0, 1, -1, 8, -8, 1 / 8, -1 / 8, 0],
            [0, 1, 1, 16, 16, 1 / 16, 1 / 16, 0], [0, 1, -1, 32, -32, 1 / 32, -1 / 32, 1]])),
}
VARIANTS = (3, 4, 6)


def w6_geo(v):
    """variant -> (filter size r, outputs per tile and dimension, points per dimension n)"""
    r, mo = (3, 6) if v == 6 else (v, 4)
    return r, mo, mo + r - 1


def winograd_identity_error(v, seed=5):
    """max |A^T ((G g G^T) o (B^T d B)) A - the direct r x r correlation of d| for a random patch d and filter g, in float64"""
    Gm, Bt, At = W6M[v]
    r, mo, n = w6_geo(v)
    assert Gm.shape == (n, r) and Bt.shape == (n, n) and At.shape == (mo, n)
    rng = np.random.default_rng(seed)
    d, g = rng.standard_normal((n, n)), rng.standard_normal((r, r))
    y = At @ ((Gm @ g @ Gm.T) * (Bt @ d @ Bt.T)) @ At.T
    direct = np.array([[(d[i:i + r, j:j + r] * g).sum() for j in range(mo)] for i in range(mo)])
    return np.abs(y - direct).max()


# ---------------------------------------------------------------------------------------------------------------- 3. weight transforms
WINO_KC = [(1, 1), (3, 85), (16, 16), (257, 1), (1, 257), (64, 32)]      # 1, 255, 256, 257 threads either side of a block edge; K != C


@functools.lru_cache(maxsize=None)
def wino_w_case(v, K, Cc, flip):
    """the stored weight (flip: [C][K][r][r], the forward weight of the layer whose data gradient this is), float64 U [n n][K][C], bound"""
    r, _, n = w6_geo(v)
    gen = torch.Generator().manual_seed(100 * v + K + 3 * Cc + flip)
    w = torch.randn((Cc, K, r, r) if flip else (K, Cc, r, r), generator=gen)
    g = w.double().permute(1, 0, 2, 3).flip(2, 3) if flip else w.double()
    Gm = torch.from_numpy(W6M[v][0])
    ref = torch.einsum("ai,kcij,bj->abkc", Gm, g, Gm).reshape(n * n, K, Cc)
    A = torch.einsum("ai,kcij,bj->abkc", Gm.abs(), g.abs(), Gm.abs()).reshape(n * n, K, Cc)
    return w, ref, 16 * U * A


def wino_w_eager32(v, K, Cc, flip):
    w, ref, bound = wino_w_case(v, K, Cc, flip)
    g = w.permute(1, 0, 2, 3).flip(2, 3) if flip else w
    Gm = torch.from_numpy(W6M[v][0]).float()
    return torch.einsum("ai,kcij,bj->abkc", Gm, g, Gm).reshape(ref.shape)


def wino_launch(dev, name, w, K, Cc, v, flip, U_, U3=None):
    if name == "nirgan_wino6_weights":
        L.call(name, w.data_ptr(), K, Cc, flip, U_.ptr, stream(dev))
    elif name == "nirgan_wino6_weights_r":
        L.call(name, w.data_ptr(), K, Cc, v, flip, U_.ptr, stream(dev))
    else:
        L.call(name, w.data_ptr(), K, Cc, v, flip, U_.ptr if U_ else None, U3.ptr, stream(dev))


def check_u3(what, U3, u_bits, n_u):
    """the planes of one transform: each n_u elements, nothing between or behind them, the three-term split of the U given as bits"""
    tw = U3.bits()
    owned_check(what + " planes", tw, first_n(tw.size, 3 * n_u), SENT16)
    planes = [tw[t * n_u:(t + 1) * n_u] for t in range(3)]
    assert planes_sum_exactly(planes, as_f32(u_bits)), f"{what}: h + m + l != U"
    for name, p, q in zip("hml", planes, split3_host(as_f32(u_bits))):
        assert np.array_equal(p, q), f"{what}: plane {name} is not the round-to-nearest-even split of the U the call wrote"


def wino_weights_against_float64(dev, v, flip):
    r, _, n = w6_geo(v)
    for K, Cc in WINO_KC:
        w, ref, bound = wino_w_case(v, K, Cc, flip)
        what, n_u = f"r{v} K {K} C {Cc} flip {flip}", n * n * K * Cc
        wd = w.to(dev)
        U1, U2, P2, P3 = Armed(n_u, dev), Armed(n_u, dev), Armed(3 * n_u, dev, True), Armed(3 * n_u, dev, True)
        wino_launch(dev, "nirgan_wino6_weights_r", wd, K, Cc, v, flip, U1)
        wino_launch(dev, "nirgan_wino6_weights_x3", wd, K, Cc, v, flip, U2, P2)
        wino_launch(dev, "nirgan_wino6_weights_x3", wd, K, Cc, v, flip, None, P3)
        if v == 3:
            U0 = Armed(n_u, dev)
            wino_launch(dev, "nirgan_wino6_weights", wd, K, Cc, v, flip, U0)
        sync(dev)
        got = U1.bits()
        owned_check("wino6_weights_r " + what, got, first_n(got.size, n_u), SENT32)
        within(f"wino6_weights r{v}", what, torch.from_numpy(as_f32(got[:n_u]).copy()), ref.reshape(-1), bound.reshape(-1))
        assert np.array_equal(U2.bits(), got), f"wino6_weights_x3 {what}: its U differs from nirgan_wino6_weights_r's"
        check_u3("wino6_weights_x3 " + what, P2, got[:n_u], n_u)
        assert np.array_equal(P3.bits(), P2.bits()), f"wino6_weights_x3 {what}: the planes without U differ from the planes with U"
        if v == 3:
            assert np.array_equal(U0.bits(), got), f"nirgan_wino6_weights {what}: differs from nirgan_wino6_weights_r with r = 3"


# a job is (variant, K, C, flip, planes, with U)
WINO_TABLES = {
    2: [(3, 3, 85, 0, False, True), (6, 16, 16, 1, True, True)],
    6: [(4, 1, 1, 0, True, True), (3, 257, 1, 1, False, True), (6, 1, 257, 0, False, True), (4, 64, 32, 1, True, False), (3, 16, 16, 0, True, True),
        (6, 3, 85, 1, False, True)],
}


def wino_batch_against_single(dev, njobs):
    jobs, rows, first, keep = WINO_TABLES[njobs], [], 0, []
    for v, K, Cc, flip, planes, with_u in jobs:
        n_u = w6_geo(v)[2] ** 2 * K * Cc
        wd = wino_w_case(v, K, Cc, flip)[0].to(dev)
        Us = [Armed(n_u, dev) if with_u else None for _ in range(2)]
        Ps = [Armed(3 * n_u, dev, True) if planes else None for _ in range(2)]
        keep.append((wd, Us, Ps, n_u))
        rows.append([wd.data_ptr(), Us[0].ptr if with_u else 0, K, Cc, flip, first, v, Ps[0].ptr if planes else 0])      # as Plan.fuse_wino6_weights
        first += (K * Cc + 255) // 256
    table = torch.tensor(rows, dtype=torch.int64).to(dev)
    L.call("nirgan_wino6_weights_batch", table.data_ptr(), njobs, first, stream(dev))
    for (v, K, Cc, flip, planes, with_u), (wd, Us, Ps, n_u) in zip(jobs, keep):
        wino_launch(dev, "nirgan_wino6_weights_x3" if planes else "nirgan_wino6_weights_r", wd, K, Cc, v, flip, Us[1], Ps[1])
    sync(dev)
    for i, (job, (wd, Us, Ps, n_u)) in enumerate(zip(jobs, keep)):
        what = f"wino6_weights_batch of {njobs}, job {i} {job}"
        v, K, Cc, flip, planes, with_u = job
        if with_u:
            got = Us[0].bits()
            owned_check(what, got, first_n(got.size, n_u), SENT32)
            assert np.array_equal(got, Us[1].bits()), f"{what}: U differs from the single launch's"
            w, ref, bound = wino_w_case(v, K, Cc, flip)
            within(f"wino6_weights_batch r{v}", what, torch.from_numpy(as_f32(got[:n_u]).copy()), ref.reshape(-1), bound.reshape(-1))
        if planes:
            tw = Ps[0].bits()
            owned_check(what + " planes", tw, first_n(tw.size, 3 * n_u), SENT16)
            assert np.array_equal(tw, Ps[1].bits()), f"{what}: the planes differ from the single launch's"
            if with_u:
                check_u3(what, Ps[0], Us[0].bits()[:n_u], n_u)


# ---------------------------------------------------------------------------------------------------------------- 4. weight-gradient finish
FIN_NSPLITS = [1, 4, 5]
FIN_KC = [(1, 1), (7, 9), (8, 8), (5, 13), (64, 64)]       # K C = 1, 63, 64, 65, 4096: a block takes 64 pairs
assert [k * c for k, c in FIN_KC] == [1, 63, 64, 65, 4096]


@functools.lru_cache(maxsize=20)
def finish_case(v, nsplit, K, Cc, layer=0):
    """slabs [n n][nsplit][K][C], the old gradient [K][C][r][r], float64 G^T (sum dU) G and its scale"""
    r, _, n = w6_geo(v)
    gen = torch.Generator().manual_seed(1000 * v + 10 * nsplit + K + Cc + 77 * layer)
    slabs, old = torch.randn(n * n, nsplit, K, Cc, generator=gen), torch.randn(K, Cc, r, r, generator=gen)
    Gm = torch.from_numpy(W6M[v][0])
    g = torch.einsum("ai,abkc,bj->kcij", Gm, slabs.double().sum(1).reshape(n, n, K, Cc), Gm)
    A = torch.einsum("ai,abkc,bj->kcij", Gm.abs(), slabs.double().abs().sum(1).reshape(n, n, K, Cc), Gm.abs())
    return slabs, old, g, A


def finish_ref(v, nsplit, K, Cc, acc, layer=0):
    slabs, old, g, A = finish_case(v, nsplit, K, Cc, layer)
    ref = g + old.double() if acc else g
    return ref, (nsplit + 16) * U * A + (U * ref.abs() if acc else 0)


def finish_eager32(v, nsplit, K, Cc, acc):
    slabs, old, g, A = finish_case(v, nsplit, K, Cc)
    r, _, n = w6_geo(v)
    Gm = torch.from_numpy(W6M[v][0]).float()
    u = slabs[:, 0].clone()
    for s in range(1, nsplit):
        u = u + slabs[:, s]
    out = torch.einsum("ai,abkc,bj->kcij", Gm, u.reshape(n, n, K, Cc), Gm)
    return old + out if acc else out


def finish_grad(dev, old, acc):
    g = Armed(old.numel(), dev)
    if acc:
        g.f32()[:old.numel()] = old.reshape(-1).to(dev)
    return g


def finish_against_float64(dev, v, nsplit):
    r = w6_geo(v)[0]
    for K, Cc in FIN_KC:
        slabs, old, _, _ = finish_case(v, nsplit, K, Cc)
        sd = slabs.to(dev)
        for acc in (0, 1):
            ref, bound = finish_ref(v, nsplit, K, Cc, acc)
            what, n_g = f"r{v} nsplit {nsplit} K {K} C {Cc} acc {acc}", K * Cc * r * r
            g1 = finish_grad(dev, old, acc)
            L.call("nirgan_wino6_wgrad_finish_r", sd.data_ptr(), nsplit, K, Cc, v, g1.ptr, acc, stream(dev))
            if v == 3:
                g0 = finish_grad(dev, old, acc)
                L.call("nirgan_wino6_wgrad_finish", sd.data_ptr(), nsplit, K, Cc, g0.ptr, acc, stream(dev))
            sync(dev)
            got = g1.bits()
            owned_check("wino6_wgrad_finish_r " + what, got, first_n(got.size, n_g), SENT32)
            within(f"wino6_wgrad_finish r{v}", what, torch.from_numpy(as_f32(got[:n_g]).copy()), ref.reshape(-1), bound.reshape(-1))
            if v == 3:
                assert np.array_equal(g0.bits(), got), f"nirgan_wino6_wgrad_finish {what}: differs from nirgan_wino6_wgrad_finish_r with r = 3"


FIN_BATCH_LAYERS = [1, 3, 16]
FIN_BATCH_GEO = (5, 5, 13)       # nsplit, K, C: 65 pairs, a second block holding one


def finish_batch_against_single(dev, v, layers):
    nsplit, K, Cc = FIN_BATCH_GEO
    r = w6_geo(v)[0]
    n_g = K * Cc * r * r
    for acc in (0, 1):
        cases = [finish_case(v, nsplit, K, Cc, layer) for layer in range(layers)]
        sds = [c[0].to(dev) for c in cases]
        gb, gs = [finish_grad(dev, c[1], acc) for c in cases], [finish_grad(dev, c[1], acc) for c in cases]
        sp, gp = (C.c_void_p * layers)(*[s.data_ptr() for s in sds]), (C.c_void_p * layers)(*[g.ptr for g in gb])
        L.call("nirgan_wino6_wgrad_finish_batch", sp, gp, layers, nsplit, K, Cc, v, acc, stream(dev))
        for s, g in zip(sds, gs):
            L.call("nirgan_wino6_wgrad_finish_r", s.data_ptr(), nsplit, K, Cc, v, g.ptr, acc, stream(dev))
        sync(dev)
        for layer in range(layers):
            what = f"wino6_wgrad_finish_batch r{v} of {layers}, layer {layer} acc {acc}"
            got = gb[layer].bits()
            owned_check(what, got, first_n(got.size, n_g), SENT32)
            ref, bound = finish_ref(v, nsplit, K, Cc, acc, layer)
            within(f"wino6_wgrad_finish_batch r{v}", what, torch.from_numpy(as_f32(got[:n_g]).copy()), ref.reshape(-1), bound.reshape(-1))
            assert np.array_equal(got, gs[layer].bits()), f"{what}: differs from nirgan_wino6_wgrad_finish_r"


# ---------------------------------------------------------------------------------------------------------------- 5. the table builders
BUILDER_CONTEXTS = ("fp32", "bf16", "bf16x3")


def _snapshot(tensors):
    return [t.cpu().view(torch.uint8).clone() if t.dtype != torch.uint8 else t.cpu().clone() for t in tensors]


def _arm(tensors):
    for t in tensors:
        (t.view(torch.int16).fill_(SENT16) if t.dtype == torch.bfloat16 else t.view(torch.int32).fill_(SENT32))


def _same_bytes(what, a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"{what}: output {i} of the fused plan differs from the unfused plan's"


def _launches(plan):
    return [n for n, _ in plan.ops if n is not E.HOOK]


def pack_plan(ctx):
    """a pack plan over the real specs, as Weights.packed emits them (one row more than the spec allocated behind every buffer: the
    row, and the padding it puts between the bf16 planes, must stay untouched); returns (plan, every output tensor)"""
    dev = ctx.device
    gen = torch.Generator().manual_seed(23)
    wc = torch.randn(64, 32, 3, 3, generator=gen).to(dev)          # Conv2d(32, 64, 3)
    wd = torch.randn(32, 64, 4, 4, generator=gen).to(dev)          # Conv2d(64, 32, 4, stride 2): rows of its data gradient are the 64 inputs
    wt = torch.randn(32, 64, 3, 3, generator=gen).to(dev)          # ConvTranspose2d(32, 64, 3)
    w1 = torch.randn(8, 3, 7, 7, generator=gen).to(dev)            # the first layer, row-packed: map entries of -1
    ph2, pht = G.conv_dgrad_s2_phases(8, 8, 4, 1), G.convT_fwd_phases(4, 4, 3, 1)
    specs = [(wc, G.conv_fwd_pack(64, 32, 3)), (wc, G.conv_dgrad_pack(64, 32, 3, [(a, b) for a in range(3) for b in range(3)])),
             (wd, G.conv_dgrad_pack(32, 64, 4, ph2[0].taps_hw)), (wd, G.conv_dgrad_pack(32, 64, 4, ph2[3].taps_hw)),
             (wt, G.convT_fwd_pack(32, 64, 3, pht[3].taps_hw)), (wt, G.convT_fwd_pack(32, 64, 3, pht[1].taps_hw)),
             (w1, G.conv_rowpacked_pack(8, 3, 7, 4))]
    plan, W = E.Plan(ctx), E.Weights(ctx)
    outs, padded = [], []
    for param, spec in specs:
        buf = W.packed(plan, param, spec, rows_alloc=spec.N + 1)
        outs.append(buf)
        if hasattr(buf, "x3"):
            outs.append(buf.x3[0])
    padded = [True] * len(outs)
    if ctx.precision == 0:
        buf = W.packed_pair(plan, wt, [G.convT_fwd_pack(32, 64, 3, pht[3].taps_hw), G.convT_fwd_pack(32, 64, 3, pht[3].taps_hw[::-1])])
        outs += [buf, buf.x3[0]]
        padded += [False, False]
    ctx.keep += [wc, wd, wt, w1]
    return plan, outs, padded


def _sentinel_hits(snap, out):
    """per element of a snapshot: does it still hold the sentinel"""
    return snap.view(torch.int16) == SENT16 if out.dtype == torch.bfloat16 else snap.view(torch.int32) == SENT32


def pack_plan_fused_equals_unfused(dev, precision):
    ctx = E.Ctx(dev, precision)
    plan, outs, padded = pack_plan(ctx)
    names = _launches(plan)
    npacks = sum(n in ("nirgan_pack_rows", "nirgan_pack_rows_bf16") for n in names)
    assert npacks >= 6 and ("nirgan_split3" in names) == (precision == "fp32") and ("nirgan_pack_rows_bf16" in names) == (precision == "bf16")
    _arm(outs)
    plan.run()
    sync(dev)
    unfused = _snapshot(outs)
    for u, o, pad in zip(unfused, outs, padded):
        hits = _sentinel_hits(u, o)
        assert not hits.all() and bool(hits.any()) == pad, "the unfused plan: an output never written, or the row allocated behind it touched"
    _arm(outs)
    plan.fuse_packs()
    assert _launches(plan) == ["nirgan_pack_rows_batch"] and plan.ops[0][1][1] == npacks
    plan.run()
    sync(dev)
    _same_bytes(f"fuse_packs {precision}", _snapshot(outs), unfused)


def wino_plan_fused_equals_unfused(dev):
    ctx = E.Ctx(dev, "fp32")
    plan, outs, keep = E.Plan(ctx), [], []
    # the ops as emit_wino6 adds them: _r with U, _x3 with the planes only (U = None); one _x3 with both
    for v, K, Cc, flip, planes, with_u in [(6, 64, 32, 0, False, True), (6, 32, 64, 1, True, False), (4, 16, 16, 0, True, True), (3, 3, 85, 1, False, True)]:
        n_u = w6_geo(v)[2] ** 2 * K * Cc
        wd = wino_w_case(v, K, Cc, flip)[0].to(dev)
        U_ = torch.zeros(n_u + GUARD, device=dev) if with_u else None
        P = torch.zeros(3 * n_u + GUARD, dtype=torch.bfloat16, device=dev) if planes else None
        keep.append(wd)
        outs += [t for t in (U_, P) if t is not None]
        if planes:
            plan.add("nirgan_wino6_weights_x3", wd.data_ptr(), K, Cc, v, flip, U_.data_ptr() if with_u else None, P.data_ptr())
        else:
            plan.add("nirgan_wino6_weights_r", wd.data_ptr(), K, Cc, v, flip, U_.data_ptr())
    _arm(outs)
    plan.run()
    sync(dev)
    unfused = _snapshot(outs)
    _arm(outs)
    plan.fuse_wino6_weights()
    assert _launches(plan) == ["nirgan_wino6_weights_batch"] and plan.ops[0][1][1] == 4
    plan.run()
    sync(dev)
    _same_bytes("fuse_wino6_weights", _snapshot(outs), unfused)
    for u, o in zip(unfused, outs):
        tail = u.view(torch.int16)[-GUARD:] if o.dtype == torch.bfloat16 else u.view(torch.int32)[-GUARD:]
        assert (tail == (SENT16 if o.dtype == torch.bfloat16 else SENT32)).all() and (u.view(torch.int16)[:64] != SENT16).any()


def deferred_reduce_equals_single(dev):
    ctx = E.Ctx(dev, "fp32")
    # (taps of the Conv2d layout or 0, spec, nsplit, accumulate)
    items = [(9, G.conv_fwd_pack(3, 64, 3), 5, 0), (0, G.conv_dgrad_pack(63, 3, 2, [(0, 0), (0, 1), (1, 0), (1, 1)]), 13, 1),
             (0, G.convT_dgrad_pack(2, 65, 2), 4, 0)]
    for count in (3, 1):
        plan, ctx.rr_deferred, keep = E.Plan(ctx), [], []
        for T, spec, nsplit, acc in items[:count]:
            elems = {"cf": spec.N * spec.K, "cd": 63 * 3 * 4, "td": 2 * 65 * 4}[spec.key[0]]
            slabs, old = slab_values((nsplit, spec.N, spec.K), False, 5 * nsplit).to(dev), slab_values((elems,), False, 3 * nsplit)
            bufs = [Armed(elems, dev) for _ in range(2)]
            for b in bufs if acc else []:
                b.f32()[:elems] = old.to(dev)
            imap = ctx.i32(spec.index_map)
            grad = bufs[0].f32()[:elems]
            # the tuple emit_wgrad defers: (slabs, nsplit, N, K, map, gradient, row stride, accumulate, taps of the Conv2d layout or 0)
            ctx.rr_deferred.append((slabs, nsplit, spec.N, spec.K, imap, grad, spec.row_stride, acc, T))
            keep.append((slabs, imap, bufs, spec, nsplit, acc, elems))
        E.emit_deferred_reduce_rows(plan, ctx)
        assert ctx.rr_deferred is None and _launches(plan) == (["nirgan_reduce_rows_batch"] if count > 1 else ["nirgan_reduce_rows"])
        plan.run()
        for slabs, imap, bufs, spec, nsplit, acc, elems in keep:
            L.call("nirgan_reduce_rows", slabs.data_ptr(), nsplit, spec.N, spec.K, imap.data_ptr(), bufs[1].ptr, elems, spec.row_stride, acc, stream(dev))
        sync(dev)
        for i, (slabs, imap, bufs, spec, nsplit, acc, elems) in enumerate(keep):
            got = bufs[0].bits()
            assert np.array_equal(got, bufs[1].bits()), f"emit_deferred_reduce_rows of {count}, item {i}: differs from nirgan_reduce_rows"
            assert (got[elems:] == SENT32).all() and (got[:elems] != SENT32).all()


def deferred_finishes_equal_single(dev):
    ctx = E.Ctx(dev, "fp32")
    plan, ctx.w6_deferred, keep = E.Plan(ctx), [], []
    for layer, (v, nsplit, K, Cc, acc) in enumerate([(6, 5, 5, 13, 0), (4, 4, 8, 8, 1), (6, 5, 5, 13, 0)]):
        slabs, old, _, _ = finish_case(v, nsplit, K, Cc, layer)
        sd, bufs = slabs.to(dev), [finish_grad(dev, old, acc) for _ in range(2)]
        # the tuple emit_wino6_backward defers: (slabs, nsplit, K, C, variant, gradient, accumulate)
        ctx.w6_deferred.append((sd, nsplit, K, Cc, v, bufs[0].f32()[:old.numel()], acc))
        keep.append((sd, bufs, v, nsplit, K, Cc, acc, old.numel()))
    E.emit_w6_deferred_finishes(plan, ctx)
    assert ctx.w6_deferred is None and sorted(_launches(plan)) == ["nirgan_wino6_wgrad_finish_batch", "nirgan_wino6_wgrad_finish_r"]
    plan.run()
    for sd, bufs, v, nsplit, K, Cc, acc, n_g in keep:
        L.call("nirgan_wino6_wgrad_finish_r", sd.data_ptr(), nsplit, K, Cc, v, bufs[1].ptr, acc, stream(dev))
    sync(dev)
    for i, (sd, bufs, v, nsplit, K, Cc, acc, n_g) in enumerate(keep):
        got = bufs[0].bits()
        assert np.array_equal(got, bufs[1].bits()), f"emit_w6_deferred_finishes, layer {i}: differs from nirgan_wino6_wgrad_finish_r"
        assert (got[n_g:] == SENT32).all() and (got[:n_g] != SENT32).all()


def table_builders(dev):
    for precision in BUILDER_CONTEXTS:
        pack_plan_fused_equals_unfused(dev, precision)
    wino_plan_fused_equals_unfused(dev)
    deferred_reduce_equals_single(dev)
    deferred_finishes_equal_single(dev)


# ---------------------------------------------------------------------------------------------------------------- 6. guards
def _refused(be, dev, what, rc, outs):
    assert fails(rc), f"{what}: accepted"
    assert be.nirgan_last_error(), f"{what}: no error message"
    sync(dev)
    for o in outs:
        assert (o.bits() == o.sent).all(), f"{what}: the refused call launched something"


def guards(dev):
    be, st = L.backend(), stream(dev)
    src, mp = torch.zeros(4096, device=dev), i32(np.arange(64), dev)
    out, out16 = Armed(4096, dev), Armed(4096, dev, True)
    slabs = torch.ones(8192, device=dev)
    tw = Armed(3 * 64, dev, True)
    table = torch.zeros(257 * 10, dtype=torch.int64, device=dev)
    s, m, o, o16, sl = src.data_ptr(), mp.data_ptr(), out.ptr, out16.ptr, slabs.data_ptr()
    outs = [out, out16, tw]
    R = lambda what, rc: _refused(be, dev, what, rc, outs)
    R("pack_rows K % 4 != 0", be.nirgan_pack_rows(s, 4096, 64, m, o, 2, 6, st))
    R("pack_rows_bf16 K % 8 != 0", be.nirgan_pack_rows_bf16(s, 4096, 64, m, o16, 2, 12, st))
    R("pack_rows unaligned dst", be.nirgan_pack_rows(s, 4096, 64, m, o + 4, 2, 8, st))
    R("pack_rows N = 0", be.nirgan_pack_rows(s, 4096, 0, m, o, 0, 8, st))
    R("pack_rows N = 65536", be.nirgan_pack_rows(s, 4096, 0, m, o, 65536, 8, st))
    R("reduce_rows K % 4 != 0", be.nirgan_reduce_rows(sl, 2, 2, 6, m, o, 4096, 64, 0, st))
    R("reduce_rows unaligned slabs", be.nirgan_reduce_rows(sl + 4, 2, 2, 8, m, o, 4096, 64, 0, st))
    R("reduce_rows N = 0", be.nirgan_reduce_rows(sl, 2, 0, 8, m, o, 4096, 64, 0, st))
    R("reduce_rows N = 65536", be.nirgan_reduce_rows(sl, 1, 65536, 8, m, o, 4096, 0, 0, st))
    R("reduce_rows_part unaligned slabs", be.nirgan_reduce_rows_part(sl + 4, 2, 4, 0, 2, 8, m, o, 4096, 64, 0, st))
    R("reduce_rows_part rows past the slab", be.nirgan_reduce_rows_part(sl, 2, 4, 3, 2, 8, m, o, 4096, 64, 0, st))
    R("reduce_rows_part row0 < 0", be.nirgan_reduce_rows_part(sl, 2, 4, -1, 2, 8, m, o, 4096, 64, 0, st))
    R("reduce_rows_part no rows", be.nirgan_reduce_rows_part(sl, 2, 4, 0, 0, 8, m, o, 4096, 64, 0, st))
    R("split3 n % 8 != 0", be.nirgan_split3(s, tw.ptr, 60, 64, st))
    R("split3 plane < n", be.nirgan_split3(s, tw.ptr, 64, 56, st))
    for name, bad in (("nirgan_reduce_rows_batch", (0, 65)), ("nirgan_pack_rows_batch", (0, 257)), ("nirgan_wino6_weights_batch", (0, 257))):
        for njobs in bad:
            R(f"{name} njobs = {njobs}", getattr(be, name)(table.data_ptr(), njobs, max(njobs, 1), st))
    R("wino6_weights_r variant 5", be.nirgan_wino6_weights_r(s, 2, 2, 5, 0, o, st))
    R("wino6_weights_x3 variant 5", be.nirgan_wino6_weights_x3(s, 2, 2, 5, 0, o, tw.ptr, st))
    R("wino6_wgrad_finish_r variant 5", be.nirgan_wino6_wgrad_finish_r(sl, 1, 2, 2, 5, o, 0, st))
    grads = [Armed(36, dev) for _ in range(17)]
    outs += grads
    sp, gp = (C.c_void_p * 17)(*[sl] * 17), (C.c_void_p * 17)(*[g.ptr for g in grads])
    R("wino6_wgrad_finish_batch variant 5", be.nirgan_wino6_wgrad_finish_batch(sp, gp, 2, 1, 2, 2, 5, 0, st))
    R("wino6_wgrad_finish_batch of 17 layers", be.nirgan_wino6_wgrad_finish_batch(sp, gp, 17, 1, 2, 2, 3, 0, st))
    R("wino6_wgrad_finish_batch of 0 layers", be.nirgan_wino6_wgrad_finish_batch(sp, gp, 0, 1, 2, 2, 3, 0, st))
    gp[1] = None
    R("wino6_wgrad_finish_batch with a null gradient", be.nirgan_wino6_wgrad_finish_batch(sp, gp, 3, 1, 2, 2, 3, 0, st))
    gp[1], sp[2] = grads[1].ptr, None
    R("wino6_wgrad_finish_batch with null slabs", be.nirgan_wino6_wgrad_finish_batch(sp, gp, 3, 1, 2, 2, 3, 0, st))


CLAMP_REAL = 2                  # the real allocations are CLAMP_REAL x the declared *_elems: a broken clamp stays inside the test's buffers


def pack_clamps_past_src_elems(dev):
    """nirgan_pack_rows reads 0 for a source index >= src_elems (include/nirgan_hip.h); the memory behind the declared elements is
    there and holds ones, so a missing clamp shows as a 1 and reads nothing foreign"""
    N, K, stride, declared = 3, 8, 8, 20
    src = torch.ones(CLAMP_REAL * N * stride, device=dev)
    src[:declared] = torch.arange(1, declared + 1, dtype=torch.float32) + 1
    mp = i32(np.arange(K), dev)
    for name, bf16 in (("nirgan_pack_rows", False), ("nirgan_pack_rows_bf16", True)):
        out = Armed(N * K, dev, bf16)
        L.call(name, src.data_ptr(), declared, stride, mp.data_ptr(), out.ptr, N, K, stream(dev))
        sync(dev)
        got = out.bits()
        owned_check(name + " clamp", got, first_n(got.size, N * K), out.sent)
        want = np.where(np.arange(N * K) < declared, np.arange(N * K) + 2, 0).astype(np.float32)
        val = bf16_f32(got[:N * K]) if bf16 else as_f32(got[:N * K])
        assert np.array_equal(val, want), f"{name}: a source index >= src_elems must read 0"
    rows = [[src.data_ptr(), 0, mp.data_ptr(), declared, N, K, stride, 0, 0, 0]]
    out = Armed(N * K, dev)
    rows[0][1] = out.ptr
    table = torch.tensor(rows, dtype=torch.int64).to(dev)
    L.call("nirgan_pack_rows_batch", table.data_ptr(), 1, N, stream(dev))
    sync(dev)
    assert np.array_equal(as_f32(out.bits()[:N * K]), np.where(np.arange(N * K) < declared, np.arange(N * K) + 2, 0).astype(np.float32))


def reduce_clamps_past_dst_elems(dev):
    """nirgan_reduce_rows drops a store at an index >= dst_elems: the declared tail keeps its sentinel"""
    nsplit, N, K, stride, declared = 2, 3, 8, 8, 20
    slabs, mp = torch.ones(nsplit, N, K, device=dev), i32(np.arange(K), dev)
    outs = [Armed(declared, dev, extra=CLAMP_REAL * N * stride) for _ in range(3)]
    L.call("nirgan_reduce_rows", slabs.data_ptr(), nsplit, N, K, mp.data_ptr(), outs[0].ptr, declared, stride, 0, stream(dev))
    L.call("nirgan_reduce_rows_part", slabs.data_ptr(), nsplit, N, 0, N, K, mp.data_ptr(), outs[1].ptr, declared, stride, 0, stream(dev))
    table = torch.tensor([[slabs.data_ptr(), outs[2].ptr, mp.data_ptr(), nsplit, N, K, declared, stride, 0, 0]], dtype=torch.int64).to(dev)
    L.call("nirgan_reduce_rows_batch", table.data_ptr(), 1, N, stream(dev))
    sync(dev)
    for o, name in zip(outs, ("reduce_rows", "reduce_rows_part", "reduce_rows_batch")):
        got = o.bits()
        owned_check(name + " clamp", got, first_n(got.size, declared), SENT32)
        assert (as_f32(got[:declared]) == 2.0).all(), name


def clamps_refused_by_the_emulator(dev):
    """the emulator's stricter refusal: an index past the declared elements is an error there"""
    be = L.backend()
    src, mp, out = torch.ones(48), i32(np.arange(8), dev), Armed(24, dev)
    assert fails(be.nirgan_pack_rows(src.data_ptr(), 20, 8, mp.data_ptr(), out.ptr, 3, 8, None))
    assert fails(be.nirgan_reduce_rows(src.data_ptr(), 2, 3, 8, mp.data_ptr(), out.ptr, 20, 8, 0, None))
    assert (out.bits() == SENT32).all()
