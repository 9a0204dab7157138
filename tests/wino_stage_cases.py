"""Bodies shared by tests/test_wino_stages_emulated.py (numpy emulator, CPU) and tests/test_gpu_wino_stages.py (MI355X): the launches between
the two ends of a Winograd layer's chain that tests/weight_path_cases.py and tests/test_gpu_wgrad.py already pin (csrc/wino6.hip) --

    stage 1   V = B^T d B                 nirgan_wino6_input / _input_norm / _input_dy / _input_dy_norm / nirgan_wino6_dy (Yt = A dY A^T)
    stage 2   M[f] = V[f] U[f]^T          nirgan_wino6_gemm (every plane-GEMM route, the split tile included) and
                                          nirgan_wino6_gemm_wgrad_pair (M and the transform-domain weight-gradient slabs)
    stage 3   y = A^T M A (+ bias)        nirgan_wino6_output: plain (with the instance-norm partial sums) and the fused mode (reflect
                                          fold, skip gradient, g_a and the per-tile sums of g_z and g_z z)

each stage ALONE against a float64 reference taken from the definitions in include/nirgan_hip.h with the matrices W6M of
tests/weight_path_cases.py.  Every body takes ``dev`` ("cpu": the installed backend is an EmuBackend) and drives the raw entry through
``L.call``.

Two passes per case (the scheme of tests/test_gpu_conv.py).

Integer pass, bitwise.  Inputs from {-2, -1, 1, 2}.  B^T is integer, A^T dyadic (multiples of 2^-GRAN[v]: 2^-3 for the 4x4-output
variants, 2^-5 for F(6x6,3x3)), so a two-stage result is a multiple of 2^-2 GRAN and every partial sum is exact in fp32 in any
association and under any contraction while A 2^(2 GRAN) < 2^24, A the sum of the absolute terms.  ``exact_or_die`` asserts that per element
on the CPU for the inputs drawn (both stages); V, Yt, y, fuse_gz and the shift k of stats_ws must then equal the float64 reference bit for
bit (the sign of a zero aside: the reference's own depends on the association).  The per-tile sums (stats_ws[1..2], fuse_part) are bitwise
where the record's absolute sum stays below 2^24 in units of its granularity and take the bound elsewhere.

Random pass, derived bound ``Kr u A`` (u = 2^-24, A the float64 sum of the absolute terms, Kr the rounded operations on the longest chain):

one 1-D stage   a row with nnz non-zero coefficients: nnz products and nnz - 1 adds, uncontracted: 2 nnz - 1.  nnz is the row maximum read
                from W6M (NNZ below: B^T 5 / 6 / 6, A^T 5 / 6 / 7, A 4 / 4 / 6 for the variants 3 / 4 / 6).
two stages      the two counts and 2 of slack: KR_IN, KR_OUT, KR_YT.
output          one more and |bias| for the bias add.
fused mode      up to three more (two fold adds, fuse_g2); the fold is applied to A as well.
input_norm      x = act((y - mean) rstd) in fp32 is off by e_x = 3 u (|y| + |mean|) rstd (the activation is continuous: no element is
                excluded); |B^T| e_x |B| on top of the transform's own bound.
stats_ws        k is the tile's first output without the bias (element bound); the two sums are referenced in float64 against the kernel's
                own k under conv_replay.stats_bound's rule with the tile's stored-output count (exact) in place of 64.
fuse_part       conv_replay.fuse_bound's rule with the tile's interior pixel count in place of 128; every |z| is kept above Z_MARGIN (|y| +
                |mean|) rstd by construction (an offending fuse_y is moved by 1/2; none may be left), so act'(z) is the same on both sides.
input_dy_norm   dY is the instance-norm backward's second pass: its float64 value and bound are tests/instnorm_cases.py's (bwd_case), the
                bound goes through |B^T| . |B| and |A| . |A^T| on top of the transforms' own.  Random pass only.
plane GEMMs     the convolution replay's rule: (C PRODUCTS_PER_FP32[precision] + 8) u sum_c |V| |U| -- the launch is that 1x1 convolution.
pair            M as above; the slabs against wgrad_replay.restate_with_scale under tests/test_gpu_wgrad.py's bound for a plane problem,
                (rows_per_split + nsplit + 8) u |P|^T |Q|.

Ownership.  Every output (V, Yt, M, y, stats_ws, fuse_gz, fuse_part) sits in an Armed buffer: SLACK elements more than the entry needs
are declared to it (V_elems, M_elems, Yt_elems exceed the need), weight_path_cases.GUARD more lie behind, all pre-filled with the sentinel.  After the launch
every owned element was written, everything else still holds the sentinel, and a second launch gives the same bits.  In the fused mode y
is passed and must stay untouched.

Worst err / bound measured on the MI355X per family (RATIO lines; integer passes are bitwise and have no ratio).  The kernel in a family's
name is the one the launch ran on: every case asserts on the device that the library's routing (nirgan_wino6_transform_kernel_name,
_gemm_kernel_name, _pair_kernel_name: the functions the launchers switch on) names its table's kernel; nirgan_wino6_dy has one per variant:

    in_bwd means (ws)                                                      0.409
    wino6_dy r3 Yt wino6_dy_kernel<3>                                      0.144
    wino6_dy r4 Yt wino6_dy_kernel<4>                                      0.135
    wino6_dy r6 Yt wino6_dy_kernel<6>                                      0.146
    wino6_gemm conv_x3_kernel<128> (planes)                                0.009
    wino6_gemm conv_x3_kernel<64> (planes)                                 0.010
    wino6_gemm conv_x3r_kernel<128> (planes)                               0.008
    wino6_gemm wino6_gemm16_kernel                                         0.183
    wino6_gemm wino6_gemm32p_kernel                                        0.022
    wino6_gemm wino6_gemm_kernel                                           0.241
    wino6_input r3 V wino6_input_kernel<3,0>                               0.100
    wino6_input r4 V wino6_input_coop_kernel<4,0>                          0.095
    wino6_input r4 V wino6_input_kernel<4,0>                               0.109
    wino6_input r6 V wino6_input_coop_kernel<6,0>                          0.115
    wino6_input r6 V wino6_input_kernel<6,0>                               0.112
    wino6_input_dy r3 V wino6_input_kernel<3,0>                            0.107
    wino6_input_dy r3 Yt wino6_input_kernel<3,0>                           0.134
    wino6_input_dy r4 V wino6_input_coop_kernel<4,0>                       0.106
    wino6_input_dy r4 V wino6_input_kernel<4,0>                            0.089
    wino6_input_dy r4 Yt wino6_input_coop_kernel<4,0>                      0.133
    wino6_input_dy r4 Yt wino6_input_kernel<4,0>                           0.088
    wino6_input_dy r6 V wino6_input_coop_kernel<6,0>                       0.111
    wino6_input_dy r6 V wino6_input_kernel<6,0>                            0.085
    wino6_input_dy r6 Yt wino6_input_coop_kernel<6,0>                      0.129
    wino6_input_dy r6 Yt wino6_input_kernel<6,0>                           0.106
    wino6_input_dy_norm V wino6_input_coop_kernel<6,2>                     0.504
    wino6_input_dy_norm Yt wino6_input_coop_kernel<6,2>                    0.775
    wino6_input_norm r3 V wino6_input_kernel<3,1>                          0.107
    wino6_input_norm r6 V wino6_input_coop_kernel<6,1>                     0.088
    wino6_input_norm r6 V wino6_input_kernel<6,1>                          0.086
    wino6_output fuse_part wino6_output_inbwd_coop_kernel                  0.049
    wino6_output fuse_part wino6_output_inbwd_kernel<6>                    0.037
    wino6_output fused g_a wino6_output_inbwd_coop_kernel                  0.115
    wino6_output fused g_a wino6_output_inbwd_kernel<6>                    0.096
    wino6_output r3 stats k                                                0.067
    wino6_output r3 stats sums                                             0.076
    wino6_output r3 y                                                      0.155
    wino6_output r4 stats k                                                0.052
    wino6_output r4 stats sums                                             0.103
    wino6_output r4 y                                                      0.110
    wino6_output r6 stats k                                                0.044
    wino6_output r6 stats sums                                             0.125
    wino6_output r6 y                                                      0.135
    wino6_pair two launches M                                              0.062
    wino6_pair two launches slabs                                          0.085
    wino6_pair wino6_pair16_kernel M                                       0.015
    wino6_pair wino6_pair16_kernel slabs                                   0.087
    wino6_pair wino6_pair16p_kernel M                                      0.017
    wino6_pair wino6_pair16p_kernel slabs                                  0.102
    wino6_pair wino6_pair_kernel M                                         0.045
    wino6_pair wino6_pair_kernel slabs                                     0.093
"""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np
import torch

from conv_replay import PRODUCTS_PER_FP32, Z_MARGIN
from nirgan_hip import lib as L
from streaming_cases import U, fails, stream, sync, within
from weight_path_cases import SENT32, W6M, Armed, as_f32, first_n, owned_check, slab_values, split3_host, w6_geo

SLACK = 40                       # elements a workspace is declared larger than the entry needs
VARIANTS = (3, 4, 6)
GRAN = {3: 3, 4: 3, 6: 5}        # A^T's entries are multiples of 2^-GRAN
NONE, RELU, LRELU = 0, 1, 2      # NIRGAN_ACT_*
SLOPE = 0.2
INT_SLOPE = 0.25                 # the integer pass's LeakyReLU slope: a power of two keeps the values dyadic


def mats(v):
    """(B^T [n][n], A^T [mo][n], A [n][mo])"""
    return W6M[v][1], W6M[v][2], np.ascontiguousarray(W6M[v][2].T)


NNZ = {name: {v: int((mats(v)[i] != 0).sum(1).max()) for v in VARIANTS} for i, name in enumerate(("BT", "AT", "A"))}
assert NNZ == {"BT": {3: 5, 4: 6, 6: 6}, "AT": {3: 5, 4: 6, 6: 7}, "A": {3: 4, 4: 4, 6: 6}}
for _v in VARIANTS:
    assert (mats(_v)[0] == np.round(mats(_v)[0])).all() and (mats(_v)[1] * 2 ** GRAN[_v] == np.round(mats(_v)[1] * 2 ** GRAN[_v])).all()


def kr(name, v):
    return 2 * (2 * NNZ[name][v] - 1) + 2


KR_IN, KR_OUT, KR_YT = ({v: kr(n, v) for v in VARIANTS} for n in ("BT", "AT", "A"))


def tiles_of(H, W, v):
    mo = w6_geo(v)[1]
    return -(-H // mo), -(-W // mo)


# ---------------------------------------------------------------------------------------------------------------- plumbing
def dev_t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def draw(shape, integer, seed):
    return slab_values(tuple(shape), integer, seed).numpy()


def exact_or_die(what, stages):
    """stages: (A, g): the sums of absolute terms of a stage and the granularity exponent of its results"""
    for A, g in stages:
        assert float(np.max(A)) * 2.0 ** g < 2.0 ** 24, f"{what}: an element of the integer pass is not exactly representable ({np.max(A)} 2^{g})"


def bitwise(what, got, ref):
    """fp32 ``got`` equal to float64 ``ref`` bit for bit (ref exactly representable; +0 and -0 alike)"""
    want = np.asarray(ref, dtype=np.float64).astype(np.float32)
    assert (want.astype(np.float64) == ref).all(), f"{what}: the reference is not an fp32 value"
    g = np.asarray(got, dtype=np.float32).reshape(want.shape)
    bad = (g + np.float32(0)).view(np.uint32) != (want + np.float32(0)).view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ from the exact result, the first at {np.argwhere(bad)[0].tolist()}: {g[bad][0]!r} for {want[bad][0]!r}"


def held(family, what, got, ref, bound, integer, exact=None):
    """integer pass: bitwise (where ``exact``, the rest under the bound); random pass: the bound"""
    got, ref, bound = np.asarray(got, dtype=np.float32).reshape(ref.shape), np.asarray(ref), np.broadcast_to(bound, ref.shape)
    if integer and exact is None:
        return bitwise(f"{family} {what}", got, ref)
    if integer:
        exact = np.broadcast_to(exact, ref.shape)
        bitwise(f"{family} {what} (exact records)", got[exact], ref[exact])
        if exact.all():
            return
        got, ref, bound = got[~exact], ref[~exact], bound[~exact]
    within(family, what, torch.from_numpy(got.copy()), torch.from_numpy(np.array(ref, dtype=np.float64)), torch.from_numpy(np.array(bound, dtype=np.float64)))


def owned(what, a, need):
    """the ownership check of an Armed output; returns its ``need`` owned fp32 elements"""
    b = a.bits()
    owned_check(what, b, first_n(b.size, need), SENT32)
    return as_f32(b[:need]).copy()


def twice(dev, launch, outs):
    """launch; the outputs' bits; re-arm; launch again: the same bits"""
    launch()
    sync(dev)
    first = [o.bits().copy() for o in outs]
    for o in outs:
        o.t.fill_(SENT32)
    launch()
    sync(dev)
    for i, (o, f) in enumerate(zip(outs, first)):
        assert np.array_equal(o.bits(), f), f"output {i}: a second launch over the same inputs gives other bits"


def untouched(what, a):
    assert (a.bits() == SENT32).all(), f"{what}: a buffer the entry must not write was written"


# ---------------------------------------------------------------------------------------------------------------- float64 references
def patches(x, v, TH, TW):
    """halo'd x [B][hp][wp][C] float64 -> the n x n patches [B][TH][TW][n][n][C] at stride mo; rows and columns past the buffer read 0"""
    r, mo, n = w6_geo(v)
    B, hp, wp, Cc = x.shape
    xp = np.zeros((B, mo * (TH - 1) + n, mo * (TW - 1) + n, Cc))
    xp[:, :hp, :wp] = x
    out = np.empty((B, TH, TW, n, n, Cc))
    for i in range(n):
        for j in range(n):
            out[:, :, :, i, j] = xp[:, i:i + mo * TH:mo, j:j + mo * TW:mo]
    return out


def two_stage(Mx, P):
    """Mx [p][i], P [B][TH][TW][i][j][c] -> [p p][T][c] with element (p1 p + p2, t, c) = sum Mx[p1][i] Mx[p2][j] P[t][i][j][c]"""
    o = np.einsum("ai,btsijc,lj->albtsc", Mx, P, Mx)
    return o.reshape(Mx.shape[0] ** 2, -1, P.shape[-1])


def one_stage_abs(Mx, P):
    return np.einsum("ai,btsijc->btsajc", np.abs(Mx), np.abs(P))


def v_ref(x, H, W, v):
    """(V, A, A of the first stage) of a halo'd buffer x [B][H+r-1][W+r-1][C]"""
    TH, TW = tiles_of(H, W, v)
    P = patches(x, v, TH, TW)
    BT = mats(v)[0]
    return two_stage(BT, P), two_stage(np.abs(BT), np.abs(P)), one_stage_abs(BT, P)


def dy_blocks(dy, v):
    """dense dY [B][H][W][K] -> its mo x mo blocks [B][TH][TW][mo][mo][K], zero past the extent"""
    mo = w6_geo(v)[1]
    B, H, W, K = dy.shape
    TH, TW = tiles_of(H, W, v)
    z = np.zeros((B, mo * TH, mo * TW, K))
    z[:, :H, :W] = dy
    return z.reshape(B, TH, mo, TW, mo, K).transpose(0, 1, 3, 2, 4, 5)


def yt_ref(dy, v):
    """(Yt = A dY A^T per tile, A, A of the first stage) of a dense dY"""
    P = dy_blocks(dy, v)
    A = mats(v)[2]
    return two_stage(A, P), two_stage(np.abs(A), np.abs(P)), one_stage_abs(A, P)


def out_ref(M, B, H, W, v):
    """M [n n][T][K] -> (R = A^T M A over the tiled extent [B][mo TH][mo TW][K], its A, A of the first stage)"""
    r, mo, n = w6_geo(v)
    TH, TW = tiles_of(H, W, v)
    K = M.shape[-1]
    Mt = M.reshape(n, n, B, TH, TW, K)
    AT = mats(v)[1]
    R = np.einsum("pa,albtsk,ql->btpsqk", AT, Mt, AT).reshape(B, mo * TH, mo * TW, K)
    A = np.einsum("pa,albtsk,ql->btpsqk", np.abs(AT), np.abs(Mt), np.abs(AT)).reshape(B, mo * TH, mo * TW, K)
    A1 = np.einsum("pa,albtsk->plbtsk", np.abs(AT), np.abs(Mt))
    return R, A, A1


def act64(z, act, slope):
    return z if act == NONE else np.where(z > 0, z, z * (0.0 if act == RELU else slope))


def reflect_idx(n):
    i = np.abs(np.arange(n + 2) - 1)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def fold(R, H, W):
    """the adjoint of ReflectionPad2d(1) on R [B][>= H][>= W][K]: rows, then columns; returns the interior [B][H-2][W-2][K]"""
    R = R[:, :H, :W].copy()
    R[:, 2] += R[:, 0]
    R[:, H - 3] += R[:, H - 1]
    R[:, :, 2] += R[:, :, 0]
    R[:, :, W - 3] += R[:, :, W - 1]
    return R[:, 1:H - 1, 1:W - 1]


def f32_slope(s):
    return float(np.float32(s))


# ---------------------------------------------------------------------------------------------------------------- stage 1: input transforms
# entry: "input" | "input_norm" | "input_dy" | "dy".  hw: the layer's extent (for input_dy and dy: dY's extent).  opt: input_norm the
# activation, dy the halo width dy_pad.  kernel: as nirgan_wino6_transform_kernel_name reports it (asserted on the device in every case;
# nirgan_wino6_dy has one kernel per variant and no query); the table must name every instantiation
In = namedtuple("In", "entry v C hw B algo opt kernel")
PT, PL = L.W6_PATCH_PER_THREAD, L.W6_PATCH_PER_LANES
IN_CASES = [
    # patch per thread, plain
    In("input", 3, 4, (2, 3), 1, 0, 0, "wino6_input_kernel<3,0>"),
    In("input", 3, 36, (5, 9), 2, 0, 0, "wino6_input_kernel<3,0>"),
    In("input", 3, 32, (11, 7), 3, 0, 0, "wino6_input_kernel<3,0>"),
    In("input", 4, 4, (4, 4), 1, 0, 0, "wino6_input_kernel<4,0>"),
    In("input", 4, 36, (11, 7), 2, 0, 0, "wino6_input_kernel<4,0>"),
    In("input", 4, 32, (8, 12), 1, PT, 0, "wino6_input_kernel<4,0>"),
    In("input", 6, 4, (2, 3), 1, 0, 0, "wino6_input_kernel<6,0>"),
    In("input", 6, 8, (6, 6), 3, 0, 0, "wino6_input_kernel<6,0>"),
    In("input", 6, 36, (7, 13), 2, 0, 0, "wino6_input_kernel<6,0>"),
    In("input", 6, 96, (17, 11), 1, PT, 0, "wino6_input_kernel<6,0>"),
    In("input", 6, 100, (12, 18), 2, 0, 0, "wino6_input_kernel<6,0>"),          # 3 blocks
    In("input", 6, 252, (17, 11), 3, 0, 0, "wino6_input_kernel<6,0>"),          # 9 blocks
    In("input", 6, 360, (12, 18), 3, 0, 0, "wino6_input_kernel<6,0>"),          # 13 blocks
    # the lane-spread form, plain
    In("input", 6, 32, (2, 3), 1, 0, 0, "wino6_input_coop_kernel<6,0>"),
    In("input", 6, 32, (7, 13), 2, 0, 0, "wino6_input_coop_kernel<6,0>"),        # 12 units: 3 blocks
    In("input", 6, 96, (6, 6), 1, 0, 0, "wino6_input_coop_kernel<6,0>"),         # 3 units: a dead wave at the barriers
    In("input", 6, 96, (12, 18), 2, 0, 0, "wino6_input_coop_kernel<6,0>"),       # 36 units: 9 blocks
    In("input", 6, 544, (6, 6), 3, 0, 0, "wino6_input_coop_kernel<6,0>"),        # 51 units: 13 blocks, one dead wave
    In("input", 6, 32, (17, 11), 3, PL, 0, "wino6_input_coop_kernel<6,0>"),
    In("input", 4, 32, (2, 3), 1, 0, 0, "wino6_input_coop_kernel<4,0>"),
    In("input", 4, 32, (5, 9), 2, 0, 0, "wino6_input_coop_kernel<4,0>"),
    In("input", 4, 96, (11, 7), 3, 0, 0, "wino6_input_coop_kernel<4,0>"),
    In("input", 4, 96, (4, 4), 1, 0, 0, "wino6_input_coop_kernel<4,0>"),
    In("input", 4, 32, (6, 10), 2, 0, 0, "wino6_input_coop_kernel<4,0>"),        # the extents the engines' layers leave modulo the tile
    In("input", 6, 32, (9, 10), 1, 0, 0, "wino6_input_coop_kernel<6,0>"),
    In("input", 6, 32, (10, 8), 2, 0, 0, "wino6_input_coop_kernel<6,0>"),
    # the normalising variant
    In("input_norm", 3, 4, (2, 3), 1, 0, NONE, "wino6_input_kernel<3,1>"),
    In("input_norm", 3, 36, (5, 9), 2, 0, LRELU, "wino6_input_kernel<3,1>"),
    In("input_norm", 3, 32, (11, 7), 1, PL, RELU, "wino6_input_kernel<3,1>"),
    In("input_norm", 6, 8, (2, 3), 2, 0, RELU, "wino6_input_kernel<6,1>"),
    In("input_norm", 6, 36, (7, 13), 1, 0, LRELU, "wino6_input_kernel<6,1>"),
    In("input_norm", 6, 32, (17, 11), 2, 0, RELU, "wino6_input_kernel<6,1>"),
    In("input_norm", 6, 32, (7, 13), 1, 0, RELU, "wino6_input_kernel<6,1>"),
    In("input_norm", 6, 32, (8, 9), 2, 0, RELU, "wino6_input_kernel<6,1>"),
    In("input_norm", 6, 64, (9, 10), 1, 0, RELU, "wino6_input_kernel<6,1>"),
    In("input_norm", 6, 32, (10, 8), 1, 0, RELU, "wino6_input_kernel<6,1>"),
    In("input_norm", 6, 32, (13, 6), 1, 0, RELU, "wino6_input_kernel<6,1>"),
    In("input_norm", 6, 32, (7, 13), 3, PL, RELU, "wino6_input_coop_kernel<6,1>"),
    In("input_norm", 6, 96, (6, 6), 1, PL, LRELU, "wino6_input_coop_kernel<6,1>"),
    In("input_norm", 6, 96, (12, 18), 2, PL, NONE, "wino6_input_coop_kernel<6,1>"),
    # V and Yt of one output-gradient buffer
    In("input_dy", 3, 36, (5, 9), 2, 0, 0, "wino6_input_kernel<3,0>"),
    In("input_dy", 3, 4, (2, 3), 1, 0, 0, "wino6_input_kernel<3,0>"),            # TH = 1 = yTH, TW = 2 > yTW = 1
    In("input_dy", 4, 8, (4, 4), 3, 0, 0, "wino6_input_kernel<4,0>"),            # 7 x 7 data gradient: TH = 2 > yTH = 1
    In("input_dy", 4, 32, (11, 7), 2, 0, 0, "wino6_input_coop_kernel<4,0>"),
    In("input_dy", 6, 36, (6, 6), 2, 0, 0, "wino6_input_kernel<6,0>"),           # 8 x 8 data gradient: TH = 2 > yTH = 1
    In("input_dy", 6, 32, (6, 6), 1, 0, 0, "wino6_input_coop_kernel<6,0>"),      # the same in the lane-spread form
    In("input_dy", 6, 96, (7, 13), 2, 0, 0, "wino6_input_coop_kernel<6,0>"),
    In("input_dy", 6, 32, (17, 11), 1, PT, 0, "wino6_input_kernel<6,0>"),
    In("input_dy", 6, 96, (2, 3), 3, 0, 0, "wino6_input_coop_kernel<6,0>"),
    In("input_dy", 6, 32, (4, 4), 2, 0, 0, "wino6_input_coop_kernel<6,0>"),      # a 6 x 6 data gradient: one whole tile
    # Yt alone, over a sentinel halo of 0, 1 and 2
    In("dy", 3, 4, (2, 3), 1, 0, 0, "wino6_dy_kernel<3>"),
    In("dy", 3, 36, (11, 7), 2, 0, 2, "wino6_dy_kernel<3>"),
    In("dy", 4, 32, (5, 9), 3, 0, 1, "wino6_dy_kernel<4>"),
    In("dy", 4, 8, (8, 12), 1, 0, 2, "wino6_dy_kernel<4>"),
    In("dy", 6, 8, (6, 6), 1, 0, 0, "wino6_dy_kernel<6>"),
    In("dy", 6, 100, (12, 18), 2, 0, 1, "wino6_dy_kernel<6>"),                  # 3 blocks
    In("dy", 6, 252, (17, 11), 3, 0, 2, "wino6_dy_kernel<6>"),                  # 9 blocks
    In("dy", 6, 360, (7, 13), 3, 0, 1, "wino6_dy_kernel<6>"),                   # 13 blocks
]
IN_KERNELS = {"wino6_input_kernel<3,0>", "wino6_input_kernel<4,0>", "wino6_input_kernel<6,0>", "wino6_input_kernel<3,1>", "wino6_input_kernel<6,1>",
              "wino6_input_coop_kernel<6,0>", "wino6_input_coop_kernel<4,0>", "wino6_input_coop_kernel<6,1>", "wino6_dy_kernel<3>", "wino6_dy_kernel<4>",
              "wino6_dy_kernel<6>"}            # wino6_input_coop_kernel<6,2> is nirgan_wino6_input_dy_norm's: DYNORM_CASES


IN_STAGE = {"input": L.W6_STAGE_INPUT, "input_dy": L.W6_STAGE_INPUT, "input_norm": L.W6_STAGE_INPUT_NORM}


def ran_on(what, d, stage, kernel):
    """the library's own routing decision for the launch of ``d`` names the table's kernel (the emulator has no kernels)"""
    if not L.is_emulated():
        name = L.backend().nirgan_wino6_transform_kernel_name(C.byref(d), stage).decode()
        assert name == kernel, f"{what}: the launch takes {name!r}"


def in_extent(c):
    """(H, W) of the transform's descriptor: the data gradient of an input_dy case covers dY's extent + r - 1"""
    r = w6_geo(c.v)[0]
    return (c.hw[0] + r - 1, c.hw[1] + r - 1) if c.entry == "input_dy" else c.hw


def in_blocks(c):
    H, W = in_extent(c)
    T = c.B * int(np.prod(tiles_of(H, W, c.v)))
    if "coop" in c.kernel:
        return -(-T * (c.C // 32) // 4)
    return -(-T * (c.C // (4 if c.v == 3 else 2)) // 256)


def in_table_conditions_hold():
    assert {c.kernel for c in IN_CASES} == IN_KERNELS
    for c in IN_CASES:
        assert c.entry != "dy" or c.kernel == f"wino6_dy_kernel<{c.v}>", c        # one kernel per variant: nothing to route
        assert c.C % 4 == 0 and min(c.hw) > 1
    for fam in ("wino6_input_kernel", "wino6_input_coop_kernel", "wino6_dy_kernel"):           # the kernels that remap blockIdx
        counts = {in_blocks(c) for c in IN_CASES if c.kernel.startswith(fam + "<")}
        assert counts >= {1, 3, 9, 13}, (fam, sorted(counts))
    for v, ext in ((6, {(2, 3), (6, 6), (7, 13), (12, 18), (17, 11)}), (3, {(2, 3), (5, 9), (11, 7)}), (4, {(2, 3), (4, 4), (5, 9), (8, 12), (11, 7)})):
        assert {c.hw for c in IN_CASES if c.v == v} >= ext
    assert {c.C for c in IN_CASES} >= {4, 8, 36, 32, 96} and {c.B for c in IN_CASES} == {1, 2, 3}
    assert any(c.entry == "input_dy" and tiles_of(*in_extent(c), c.v)[0] > tiles_of(*c.hw, c.v)[0] and "coop" in c.kernel for c in IN_CASES)
    assert any(c.entry == "input_dy" and tiles_of(*in_extent(c), c.v)[0] > tiles_of(*c.hw, c.v)[0] and "coop" not in c.kernel for c in IN_CASES)
    assert {c.opt for c in IN_CASES if c.entry == "dy"} == {0, 1, 2}
    # a wave takes a (patch, 32 channels) unit, four to a block: some lane-spread case leaves dead waves in its last block
    assert any("coop" in c.kernel and (c.B * int(np.prod(tiles_of(*in_extent(c), c.v))) * (c.C // 32)) % 4 for c in IN_CASES)


@functools.lru_cache(maxsize=4)
def in_data(c, integer):
    """the case's inputs and float64 expectations: dict with the host arrays, V / Yt references and bounds"""
    r, mo, n = w6_geo(c.v)
    B, Cc = c.B, c.C
    seed = 7 * IN_CASES.index(c) + integer
    H, W = in_extent(c)
    o = {"H": H, "W": W}
    if c.entry == "input":
        o["x"] = draw((B, H + r - 1, W + r - 1, Cc), integer, seed)
        x64 = o["x"].astype(np.float64)
        ex = None
    elif c.entry == "input_dy":
        yH, yW = c.hw
        o["x"] = np.zeros((B, yH + 2 * (r - 1), yW + 2 * (r - 1), Cc), dtype=np.float32)          # dY under a zero halo of r - 1
        o["x"][:, r - 1:r - 1 + yH, r - 1:r - 1 + yW] = draw((B, yH, yW, Cc), integer, seed)
        x64 = o["x"].astype(np.float64)
        ex = None
    elif c.entry == "input_norm":
        o["y"] = draw((B, H, W, Cc), integer, seed)
        if integer:
            o["mean"], o["rstd"], o["slope"] = np.zeros((B, Cc), np.float32), np.ones((B, Cc), np.float32), INT_SLOPE
        else:
            o["mean"] = (0.5 * draw((B, Cc), False, seed + 1)).astype(np.float32)
            o["rstd"] = (0.5 + 1.5 * np.random.default_rng(seed).random((B, Cc))).astype(np.float32)
            o["slope"] = f32_slope(SLOPE)
        y, m, s = (a.astype(np.float64) for a in (o["y"], o["mean"], o["rstd"]))
        a = act64((y - m[:, None, None]) * s[:, None, None], c.opt, o["slope"])
        ea = 3 * U * (np.abs(y) + np.abs(m[:, None, None])) * s[:, None, None]
        hh, ww = reflect_idx(H), reflect_idx(W)
        x64, ex = a[:, hh][:, :, ww], ea[:, hh][:, :, ww]
    if c.entry != "dy":
        Vr, A, A1 = v_ref(x64, H, W, c.v)
        o["V"], o["bV"] = Vr, KR_IN[c.v] * U * A
        if ex is not None and not integer:
            o["bV"] = o["bV"] + v_ref(ex, H, W, c.v)[1] * (1 + KR_IN[c.v] * U)
        if integer:
            g = 2 if c.entry == "input_norm" and c.opt == LRELU else 0
            exact_or_die(f"{c} V", [(A1, g), (A, g)])
    if c.entry == "input_dy":
        dy = x64[:, r - 1:r - 1 + c.hw[0], r - 1:r - 1 + c.hw[1]]
    elif c.entry == "dy":
        p = c.opt
        o["dy"] = np.full((B, c.hw[0] + 2 * p, c.hw[1] + 2 * p, Cc), np.nan, dtype=np.float32)      # the halo holds the sentinel NaN
        o["dy"].view(np.uint32)[:] = SENT32 & 0xFFFFFFFF
        o["dy"][:, p:p + c.hw[0], p:p + c.hw[1]] = draw((B, c.hw[0], c.hw[1], Cc), integer, seed)
        dy = o["dy"][:, p:p + c.hw[0], p:p + c.hw[1]].astype(np.float64)
    if c.entry in ("input_dy", "dy"):
        Yr, A, A1 = yt_ref(dy, c.v)
        o["Yt"], o["bYt"] = Yr, KR_YT[c.v] * U * A
        if integer:
            exact_or_die(f"{c} Yt", [(A1, GRAN[c.v]), (A, 2 * GRAN[c.v])])
    return o


def in_desc(c, H, W, x, V, n_v):
    r = w6_geo(c.v)[0]
    d = L.Wino6Desc()
    d.x, d.x_hp, d.x_wp = x, H + r - 1, W + r - 1
    d.B, d.H, d.W, d.C, d.K, d.r, d.algo = c.B, H, W, c.C, c.C, c.v, c.algo
    d.V, d.V_elems = V.ptr, n_v + SLACK
    return d


def dy_desc(c, dy_ptr, pad, Yt, n_yt):
    y = L.WinoDyDesc()
    y.dy, y.dy_pad, y.dy_hp, y.dy_wp = dy_ptr, pad, c.hw[0] + 2 * pad, c.hw[1] + 2 * pad
    y.B, y.H, y.W, y.K, y.r = c.B, c.hw[0], c.hw[1], c.C, c.v
    y.Yt, y.Yt_elems = Yt.ptr, n_yt + SLACK
    return y


def input_against_float64(dev, c):
    """one case of IN_CASES: the integer pass bitwise, the random pass under the bound, every buffer guarded"""
    r, mo, n = w6_geo(c.v)
    st = stream(dev)
    for integer in (True, False):
        o = in_data(c, integer)
        H, W = o["H"], o["W"]
        what = f"{tuple(c)} {'integer' if integer else 'random'}"
        T = c.B * int(np.prod(tiles_of(H, W, c.v)))
        yT = c.B * int(np.prod(tiles_of(*c.hw, c.v)))
        n_v, n_yt = n * n * T * c.C, n * n * yT * c.C
        outs = []
        if c.entry != "dy":
            V = Armed(n_v + SLACK, dev)
            outs.append(V)
        if c.entry in ("input_dy", "dy"):
            Yt = Armed(n_yt + SLACK, dev)
            outs.append(Yt)
        if c.entry in ("input", "input_dy"):
            x = dev_t(o["x"], dev)
            d = in_desc(c, H, W, x.data_ptr(), V, n_v)
            if c.entry == "input":
                launch = lambda: L.call("nirgan_wino6_input", C.byref(d), st)
            else:
                y = dy_desc(c, x.data_ptr(), r - 1, Yt, n_yt)
                launch = lambda: L.call("nirgan_wino6_input_dy", C.byref(d), C.byref(y), st)
            src = x
        elif c.entry == "input_norm":
            yv, mean, rstd = dev_t(o["y"], dev), dev_t(o["mean"], dev), dev_t(o["rstd"], dev)
            d = in_desc(c, H, W, None, V, n_v)
            launch = lambda: L.call("nirgan_wino6_input_norm", C.byref(d), yv.data_ptr(), mean.data_ptr(), rstd.data_ptr(), c.opt, o["slope"], st)
            src = yv
        else:
            dyt = dev_t(o["dy"], dev)
            y = dy_desc(c, dyt.data_ptr(), c.opt, Yt, n_yt)
            launch = lambda: L.call("nirgan_wino6_dy", C.byref(y), st)
            src = dyt
        if c.entry != "dy":
            ran_on(what, d, IN_STAGE[c.entry], c.kernel)
        before = src.cpu().view(torch.int32).clone()
        twice(dev, launch, outs)
        assert torch.equal(src.cpu().view(torch.int32), before), f"{what}: the input buffer was written"
        if c.entry != "dy":
            held(f"wino6_{c.entry} r{c.v} V {c.kernel}", what, owned(what + " V", V, n_v), o["V"].reshape(-1), o["bV"].reshape(-1), integer)
        if c.entry in ("input_dy", "dy"):
            fam = f"wino6_{c.entry} r{c.v} Yt {c.kernel}"
            held(fam, what, owned(what + " Yt", Yt, n_yt), o["Yt"].reshape(-1), o["bYt"].reshape(-1), integer)


# ---------------------------------------------------------------------------------------------------------------- stage 2: plane GEMMs
# (variant, B, H, W) -> T tiles; kernel as nirgan_wino6_gemm_kernel_name reports it; x3: 0 no planes, 1 U and its planes, 2 the planes only
Gemm = namedtuple("Gemm", "v T C K algo x3 kernel")
GEMM_CASES = [
    Gemm(3, 1, 4, 68, 0, 0, "wino6_gemm_kernel"),
    Gemm(4, 129, 20, 128, 0, 0, "wino6_gemm_kernel"),
    Gemm(6, 129, 4, 128, 0, 0, "wino6_gemm_kernel"),
    Gemm(3, 129, 32, 68, L.W6_DIRECT_TILE, 0, "wino6_gemm_kernel"),
    Gemm(6, 1, 32, 128, L.W6_DIRECT_TILE, 0, "wino6_gemm_kernel"),
    Gemm(3, 1, 16, 68, 0, 0, "wino6_gemm16_kernel"),
    Gemm(4, 128, 48, 192, 0, 0, "wino6_gemm16_kernel"),
    Gemm(6, 129, 48, 68, 0, 0, "wino6_gemm16_kernel"),
    Gemm(3, 129, 16, 192, 0, 0, "wino6_gemm16_kernel"),
    Gemm(6, 128, 256, 128, L.W6_ONE_TILE, 0, "wino6_gemm16_kernel"),
    Gemm(3, 129, 256, 192, 0, 0, "wino6_gemm32p_kernel"),       # 36 x 2 x 2 = 144 tiles: fewer than the 512 workgroups
    Gemm(6, 257, 256, 384, 0, 0, "wino6_gemm32p_kernel"),       # 64 x 3 x 3 = 576 tiles: an uneven last round
    Gemm(4, 130, 512, 68, 0, 0, "wino6_gemm32p_kernel"),        # 49 x 2 x 1 = 98 tiles of 16 k-steps each, a 68-column tile
    Gemm(3, 129, 32, 128, 0, 1, "conv_x3_kernel<128> (planes)"),
    Gemm(6, 1, 64, 128, 0, 2, "conv_x3_kernel<128> (planes)"),
    Gemm(4, 129, 64, 192, 0, 1, "conv_x3_kernel<64> (planes)"),
    Gemm(6, 1, 32, 128, L.W6_X3_R4, 2, "conv_x3_kernel<128> (planes)"),         # asked for, but below the register-fed tile's 3 k-tiles
    Gemm(6, 520, 96, 128, L.W6_X3_R4, 2, "conv_x3r_kernel<128> (planes)"),      # the register-fed tile takes C >= 96 and 16 rows
    Gemm(4, 257, 128, 128, L.W6_X3_R4, 2, "conv_x3r_kernel<128> (planes)"),
    Gemm(3, 129, 96, 256, L.W6_X3_R4, 1, "conv_x3r_kernel<128> (planes)"),
]
GEMM_KERNELS = {"wino6_gemm_kernel", "wino6_gemm16_kernel", "wino6_gemm32p_kernel", "conv_x3_kernel<128> (planes)", "conv_x3_kernel<64> (planes)",
                "conv_x3r_kernel<128> (planes)"}


def gemm_table_conditions_hold():
    assert {g.kernel for g in GEMM_CASES} == GEMM_KERNELS
    for g in GEMM_CASES:
        assert g.T <= 520 and g.C <= 512 and g.K > 64 and 4 * g.C < 2 ** 24
        if g.kernel == "wino6_gemm32p_kernel":
            assert g.C in (256, 512)
    p = [w6_geo(g.v)[2] ** 2 * -(-g.T // 128) * -(-g.K // 128) for g in GEMM_CASES if g.kernel == "wino6_gemm32p_kernel"]      # 128 x 128 tiles
    assert any(t < 512 for t in p) and any(t > 512 and t % 512 for t in p)
    assert {g.x3 for g in GEMM_CASES} == {0, 1, 2} and {g.C for g in GEMM_CASES if g.x3} >= {32, 64}


def gemm_geo(g):
    """(B, H, W) with nirgan_wino6_tiles_r(B, H, W, v) == T"""
    mo = w6_geo(g.v)[1]
    return 1, mo, mo * g.T


def bf16_planes(u, dev):
    """the three bf16 planes of fp32 u (nirgan_split3's rule, on the host) as one int16 tensor [3][u.size]"""
    p = np.stack([q.reshape(-1) for q in split3_host(np.ascontiguousarray(u, dtype=np.float32).reshape(-1))])
    return torch.from_numpy(p.view(np.int16).copy()).to(dev)


def gemm_against_float64(dev, g):
    r, mo, n = w6_geo(g.v)
    npl, st = n * n, stream(dev)
    B, H, W = gemm_geo(g)
    zero = torch.zeros(64, device=dev)
    prec = 3 if g.x3 else 0
    for integer in (True, False):
        what = f"{tuple(g)} {'integer' if integer else 'random'}"
        seed = 11 * GEMM_CASES.index(g) + integer
        V = draw((npl, g.T, g.C), integer, seed)
        keep = []
        d = L.Wino6Desc()
        d.B, d.H, d.W, d.C, d.K, d.r, d.algo = B, H, W, g.C, g.K, g.v, g.algo
        Vd = dev_t(V, dev)
        if g.x3 and not integer:
            # the planes as the library writes them: U = G w G^T by nirgan_wino6_weights_x3; the reference reads the U the call wrote
            w = dev_t(draw((g.K, g.C, r, r), False, seed + 5), dev)
            Ud, U3 = torch.zeros(npl * g.K * g.C, device=dev), torch.zeros(3 * npl * g.K * g.C, dtype=torch.int16, device=dev)
            L.call("nirgan_wino6_weights_x3", w.data_ptr(), g.K, g.C, g.v, 0, Ud.data_ptr(), U3.data_ptr(), st)
            if g.x3 == 2:          # the planes only: a second transform without U (the one the launch under test reads)
                U3b = torch.zeros_like(U3)
                L.call("nirgan_wino6_weights_x3", w.data_ptr(), g.K, g.C, g.v, 0, None, U3b.data_ptr(), st)
                sync(dev)
                assert torch.equal(U3b.cpu(), U3.cpu())
                U3 = U3b
            sync(dev)
            Uh = Ud.cpu().numpy().reshape(npl, g.K, g.C)
            keep += [w, Ud, U3]
            d.U, d.U3 = (Ud.data_ptr() if g.x3 == 1 else None), U3.data_ptr()
        else:
            Uh = draw((npl, g.K, g.C), integer, seed + 3)
            Ud = dev_t(Uh, dev)
            d.U = Ud.data_ptr()
            if g.x3:               # integers are exact bf16: h = U, m = l = 0
                U3 = bf16_planes(Uh, dev)
                assert (U3.cpu()[1:] == 0).all()
                d.U3 = U3.data_ptr()
                keep.append(U3)
        n_m = npl * g.T * g.K
        M = Armed(n_m + SLACK, dev)
        d.V, d.V_elems, d.M, d.M_elems, d.zero_page = Vd.data_ptr(), Vd.numel(), M.ptr, n_m + SLACK, zero.data_ptr()
        if not L.is_emulated():
            name = L.backend().nirgan_wino6_gemm_kernel_name(C.byref(d)).decode()
            assert name == g.kernel, f"{what}: the launch takes {name}"
        before = Vd.cpu().clone()
        twice(dev, lambda: L.call("nirgan_wino6_gemm", C.byref(d), st), [M])
        assert torch.equal(Vd.cpu(), before)
        ref = V.astype(np.float64) @ Uh.astype(np.float64).transpose(0, 2, 1)
        A = np.abs(V).astype(np.float64) @ np.abs(Uh).astype(np.float64).transpose(0, 2, 1)
        if integer:
            exact_or_die(what, [(A, 0)])
        held(f"wino6_gemm {g.kernel}", what, owned(what + " M", M, n_m), ref.reshape(-1), ((g.C * PRODUCTS_PER_FP32[prec] + 8) * U * A).reshape(-1), integer)


# ---------------------------------------------------------------------------------------------------------------- stage 3: output transforms
Out = namedtuple("Out", "v K hw B bias stats kernel")
OUT_CASES = [
    Out(3, 4, (2, 3), 1, True, True, "wino6_output_kernel<3>"),
    Out(3, 36, (5, 9), 2, False, True, "wino6_output_kernel<3>"),
    Out(3, 128, (11, 7), 3, True, False, "wino6_output_kernel<3>"),
    Out(3, 4, (4, 4), 2, False, False, "wino6_output_kernel<3>"),
    Out(3, 36, (8, 12), 1, True, True, "wino6_output_kernel<3>"),
    Out(4, 4, (5, 9), 3, False, True, "wino6_output_kernel<4>"),
    Out(4, 36, (2, 3), 2, True, True, "wino6_output_kernel<4>"),
    Out(4, 128, (4, 4), 1, True, False, "wino6_output_kernel<4>"),
    Out(4, 36, (11, 7), 1, False, True, "wino6_output_kernel<4>"),
    Out(4, 4, (8, 12), 2, True, True, "wino6_output_kernel<4>"),
    Out(6, 4, (2, 3), 3, True, True, "wino6_output_kernel<6>"),
    Out(6, 36, (6, 6), 1, False, True, "wino6_output_kernel<6>"),
    Out(6, 128, (7, 13), 2, True, True, "wino6_output_kernel<6>"),
    Out(6, 36, (12, 18), 1, True, False, "wino6_output_kernel<6>"),
    Out(6, 4, (17, 11), 2, False, True, "wino6_output_kernel<6>"),
    Out(6, 128, (17, 11), 1, False, False, "wino6_output_kernel<6>"),
    # the extents the engines' layers leave modulo the tile, with their bias / statistics combinations
    Out(4, 128, (11, 7), 2, True, True, "wino6_output_kernel<4>"),
    Out(4, 128, (6, 10), 2, False, False, "wino6_output_kernel<4>"),
    Out(4, 128, (11, 7), 1, True, False, "wino6_output_kernel<4>"),
    Out(6, 128, (8, 9), 1, True, True, "wino6_output_kernel<6>"),
    Out(6, 128, (9, 10), 2, True, True, "wino6_output_kernel<6>"),
    Out(6, 128, (10, 8), 1, True, True, "wino6_output_kernel<6>"),
    Out(6, 128, (13, 6), 1, True, True, "wino6_output_kernel<6>"),
    Out(6, 128, (6, 6), 2, False, False, "wino6_output_kernel<6>"),
    Out(6, 128, (10, 8), 2, False, False, "wino6_output_kernel<6>"),
    Out(6, 128, (10, 10), 1, True, False, "wino6_output_kernel<6>"),
]


def out_table_conditions_hold():
    for v, ext in ((6, {(2, 3), (6, 6), (7, 13), (12, 18), (17, 11)}), (3, {(2, 3), (4, 4), (5, 9), (8, 12), (11, 7)}), (4, {(2, 3), (4, 4), (5, 9), (8, 12), (11, 7)})):
        cs = [c for c in OUT_CASES if c.v == v]
        assert {c.hw for c in cs} >= ext and {c.K for c in cs} == {4, 36, 128} and {c.B for c in cs} == {1, 2, 3}
        assert {(c.bias, c.stats) for c in cs} == {(True, True), (False, True), (True, False), (False, False)} or v != 3
        assert {(c.bias, c.stats) for c in cs} >= {(True, True), (False, True), (True, False)}
        assert all(c.kernel == f"wino6_output_kernel<{v}>" for c in cs)


def tile_view(a, mo):
    """[B][mo TH][mo TW][K] -> [B][TH][TW][mo mo][K]"""
    B, Hh, Ww, K = a.shape
    return a.reshape(B, Hh // mo, mo, Ww // mo, mo, K).transpose(0, 1, 3, 2, 4, 5).reshape(B, Hh // mo, Ww // mo, mo * mo, K)


def stats_expect(R, E, got_k, H, W, mo, g2):
    """the two sums of a tile against the kernel's own shift: (ref [B][TH][TW][2][K], bound, exact mask), by conv_replay.stats_bound's rule
    with the tile's stored-output count: a stored o is within E of R, o - k rounds once, the sums add count terms in any order, the
    squares round once more.  exact: the record's absolute sum stays below 2^24 in units of 2^-g2 (2^-2 g2 for the squares)"""
    B, Hh, Ww, K = R.shape
    valid = np.zeros((Hh, Ww, 1))
    valid[:H, :W] = 1
    vt = tile_view(np.broadcast_to(valid, (B, Hh, Ww, 1)), mo)                              # [B][TH][TW][mo mo][1]
    cnt = vt.sum(3)                                                                            # [B][TH][TW][1]
    dv = (tile_view(R, mo) - got_k[:, :, :, None, :]) * vt
    de = (tile_view(E, mo) + U * (np.abs(dv) + tile_view(E, mo))) * vt
    a1, a2 = np.abs(dv).sum(3), (dv * dv).sum(3)
    b1 = de.sum(3) + cnt * U * (np.abs(dv) + de).sum(3)
    b2 = (2 * np.abs(dv) * de + de * de).sum(3) + (cnt + 1) * U * ((np.abs(dv) + de) ** 2).sum(3)
    exact = np.stack([a1 * 2.0 ** g2 < 2.0 ** 24, a2 * 4.0 ** g2 < 2.0 ** 24], 3)
    return np.stack([dv.sum(3), a2], 3), np.stack([b1, b2], 3), exact, cnt


@functools.lru_cache(maxsize=4)
def out_data(c, integer):
    """M, the bias, R = A^T M A over the tiled extent, the element bound E of R, y's reference and bound"""
    r, mo, n = w6_geo(c.v)
    H, W = c.hw
    T = c.B * int(np.prod(tiles_of(H, W, c.v)))
    seed = 13 * OUT_CASES.index(c) + integer
    o = {"M": draw((n * n, T, c.K), integer, seed), "bias": draw((c.K,), integer, seed + 1) if c.bias else None}
    R, A, A1 = out_ref(o["M"].astype(np.float64), c.B, H, W, c.v)
    if integer:
        exact_or_die(f"{c} y", [(A1, GRAN[c.v]), (A + 2, 2 * GRAN[c.v])])
    o["R"], o["E"] = R, KR_OUT[c.v] * U * A
    o["y"] = R[:, :H, :W] + (o["bias"].astype(np.float64) if c.bias else 0)
    o["by"] = (KR_OUT[c.v] + 1) * U * (A[:, :H, :W] + (np.abs(o["bias"]) if c.bias else 0))
    return o


def output_checks(c, integer, got, rec):
    """y [B][H][W][K] and (with stats_ws) the records [B][TH][TW][4][K] as written, against out_data"""
    o = out_data(c, integer)
    mo = w6_geo(c.v)[1]
    H, W = c.hw
    what, fam = f"{tuple(c)} {'integer' if integer else 'random'}", f"wino6_output r{c.v}"
    held(fam + " y", what, got, o["y"], o["by"], integer)
    if rec is None:
        return
    held(fam + " stats k", what, rec[:, :, :, 0], o["R"][:, ::mo, ::mo], o["E"][:, ::mo, ::mo], integer)
    if not c.bias:
        assert np.array_equal(rec[:, :, :, 0].view(np.uint32), got[:, ::mo, ::mo].view(np.uint32)), f"{what}: without a bias k is y at the tile origin"
    sums, sb, exact, cnt = stats_expect(o["R"], o["E"] * (0 if integer else 1), rec[:, :, :, 0].astype(np.float64), H, W, mo, 2 * GRAN[c.v])
    assert np.array_equal(rec[:, :, :, 3], np.broadcast_to(cnt, rec[:, :, :, 3].shape).astype(np.float32)), f"{what}: the count record is not the stored outputs'"
    assert cnt.min() >= 1 and cnt.max() <= mo * mo and (cnt.min() < mo * mo or (H % mo == 0 and W % mo == 0))
    held(fam + " stats sums", what, rec[:, :, :, 1:3], sums, sb, integer, exact)


def output_against_float64(dev, c):
    r, mo, n = w6_geo(c.v)
    st = stream(dev)
    H, W = c.hw
    TH, TW = tiles_of(H, W, c.v)
    T = c.B * TH * TW
    n_y, n_s = c.B * H * W * c.K, T * 4 * c.K
    for integer in (True, False):
        o = out_data(c, integer)
        what = f"{tuple(c)} {'integer' if integer else 'random'}"
        Md, bd = dev_t(o["M"], dev), (dev_t(o["bias"], dev) if c.bias else None)
        y, stats = Armed(n_y, dev), Armed(n_s + SLACK, dev)
        d = L.Wino6Desc()
        d.B, d.H, d.W, d.C, d.K, d.r = c.B, H, W, c.K, c.K, c.v
        d.M, d.M_elems, d.y, d.bias = Md.data_ptr(), Md.numel(), y.ptr, (bd.data_ptr() if c.bias else None)
        if c.stats:
            d.stats_ws, d.stats_ws_elems = stats.ptr, n_s + SLACK
        ran_on(what, d, L.W6_STAGE_OUTPUT, c.kernel)
        before = Md.cpu().clone()
        twice(dev, lambda: L.call("nirgan_wino6_output", C.byref(d), st), [y, stats])
        assert torch.equal(Md.cpu(), before)
        got = owned(what + " y", y, n_y).reshape(c.B, H, W, c.K)
        if not c.stats:
            untouched(what + " stats_ws", stats)
        output_checks(c, integer, got, owned(what + " stats_ws", stats, n_s).reshape(c.B, TH, TW, 4, c.K) if c.stats else None)


# the fused mode (F(6x6,3x3) data gradients): (K, hw, B, algo, g2, act, kernel)
Fuse = namedtuple("Fuse", "K hw B algo g2 act kernel")
PAIRK, COOPK = "wino6_output_inbwd_kernel<6>", "wino6_output_inbwd_coop_kernel"
FUSE_CASES = [
    Fuse(4, (6, 6), 1, 0, False, NONE, PAIRK),
    Fuse(36, (6, 9), 2, 0, True, RELU, PAIRK),
    Fuse(4, (9, 6), 3, 0, True, LRELU, PAIRK),
    Fuse(36, (10, 11), 1, 0, False, RELU, PAIRK),
    Fuse(36, (12, 12), 3, 0, True, NONE, PAIRK),            # 12 tiles x 18 pairs: 216 threads; K = 36 B = 3 at (11, 15): two blocks, the last partly filled
    Fuse(36, (11, 15), 3, 0, True, LRELU, PAIRK),
    Fuse(32, (6, 6), 1, 0, True, RELU, COOPK),
    Fuse(96, (6, 6), 1, 0, False, LRELU, COOPK),            # 3 units: a dead wave reaches the barrier and the shuffles
    Fuse(96, (6, 9), 1, 0, True, RELU, COOPK),              # 6 units: two dead waves in the second block
    Fuse(32, (9, 6), 2, 0, True, NONE, COOPK),
    Fuse(96, (10, 11), 2, 0, True, LRELU, COOPK),
    Fuse(32, (12, 12), 3, 0, False, RELU, COOPK),
    Fuse(32, (11, 15), 1, 0, True, LRELU, COOPK),
] + [Fuse(32, hw, 1 + (hw[0] + a) % 2, 0, g2, a, COOPK) for hw in ((9, 9), (10, 10), (11, 11)) for g2, a in ((False, RELU), (True, NONE), (True, RELU))] + [
    Fuse(32, (6, 6), 2, 0, True, NONE, COOPK),
    Fuse(32, (11, 15), 1, PT, True, LRELU, PAIRK),
    Fuse(32, (6, 6), 1, PT, True, RELU, PAIRK),
]


def fuse_table_conditions_hold():
    for k in (PAIRK, COOPK):
        cs = [c for c in FUSE_CASES if c.kernel == k]
        assert {c.hw for c in cs} >= {(6, 6), (6, 9), (9, 6), (10, 11), (12, 12), (11, 15)}
        assert {c.g2 for c in cs} == {True, False} and {c.act for c in cs} == {NONE, RELU, LRELU}
    for c in FUSE_CASES:
        assert all((e - 3) // 6 == (e - 1) // 6 and e >= 6 for e in c.hw)
    assert {(e - 3) % 6 for c in FUSE_CASES for e in c.hw} >= {0, 1, 2, 3}           # the far fold's line at tile offsets 0 .. 3
    assert any(c.kernel == PAIRK and -(-c.B * int(np.prod(tiles_of(*c.hw, 6))) * (c.K // 2) // 256) > 1
               and (c.B * int(np.prod(tiles_of(*c.hw, 6))) * (c.K // 2)) % 256 for c in FUSE_CASES)
    assert any(c.kernel == COOPK and c.K == 96 and c.B * int(np.prod(tiles_of(*c.hw, 6))) in (1, 2) for c in FUSE_CASES)
    assert {(c.K, c.hw, c.B, c.g2, c.act) for c in FUSE_CASES if c.algo == PT} <= {(c.K, c.hw, c.B, c.g2, c.act) for c in FUSE_CASES if c.algo == 0}


@functools.lru_cache(maxsize=4)
def fuse_data(c, integer):
    v, mo, n = 6, 6, 8
    H, W = c.hw
    TH, TW = tiles_of(H, W, v)
    T = c.B * TH * TW
    seed = 17 * [x[:3] + x[4:6] for x in FUSE_CASES].index(c[:3] + c[4:6]) + integer        # the two forms of a shape draw the same inputs
    o = {"M": draw((n * n, T, c.K), integer, seed)}
    Hi, Wi = H - 2, W - 2
    o["g2"] = draw((c.B, Hi, Wi, c.K), integer, seed + 1) if c.g2 else None
    y = draw((c.B, Hi, Wi, c.K), integer, seed + 2)
    if integer:
        mean, rstd, slope = np.zeros((c.B, c.K), np.float32), np.ones((c.B, c.K), np.float32), INT_SLOPE
    else:
        mean = (0.5 * draw((c.B, c.K), False, seed + 3)).astype(np.float32)
        rstd = (0.5 + 1.5 * np.random.default_rng(seed).random((c.B, c.K))).astype(np.float32)
        slope = f32_slope(SLOPE)
    m64, s64 = mean.astype(np.float64)[:, None, None], rstd.astype(np.float64)[:, None, None]
    zs = lambda yy: (np.abs(yy.astype(np.float64)) + np.abs(m64)) * s64
    z = (y.astype(np.float64) - m64) * s64
    close = np.abs(z) <= Z_MARGIN * zs(y)
    y[close] += np.float32(0.5)                                  # as conv_replay.Replay._keep_z_off_zero
    z = (y.astype(np.float64) - m64) * s64
    assert (np.abs(z) > Z_MARGIN * zs(y)).all(), "fuse_y: a z within the margin of 0 is left"
    o.update(y=y, mean=mean, rstd=rstd, slope=slope, z=z, zs=zs(y))
    R, A, A1 = out_ref(o["M"].astype(np.float64), c.B, H, W, v)
    ga, Aa = fold(R, H, W), fold(A, H, W)
    if c.g2:
        ga, Aa = ga + o["g2"], Aa + np.abs(o["g2"])
    if integer:
        exact_or_die(f"{c} g_a", [(A1, GRAN[v]), (Aa, 2 * GRAN[v])])
    o["ga"], o["bga"] = ga, (KR_OUT[v] + 3) * U * Aa
    o["e"] = (0 if integer else 1) * o["bga"]
    # the tile's sums over its interior pixels, by conv_replay.fuse_bound's rule with the tile's pixel count
    f = np.ones_like(z) if c.act == NONE else np.where(z > 0, 1.0, 0.0 if c.act == RELU else slope)
    gz, ez = ga * f, 3 * U * o["zs"]
    egz = o["e"] * f + U * (np.abs(gz) + o["e"] * f)
    t = np.abs(gz) * np.abs(z)
    et = egz * np.abs(z) + np.abs(gz) * ez + egz * ez
    et = et + U * (t + et)

    def per_tile(a):
        grid = np.zeros((c.B, mo * TH, mo * TW, c.K))
        grid[:, 1:H - 1, 1:W - 1] = a
        return tile_view(grid, mo).sum(3)

    cnt = per_tile(np.ones_like(z))
    o["part"] = np.stack([per_tile(gz), per_tile(gz * z)], 3)                                   # [B][TH][TW][2][K]
    o["bpart"] = np.stack([per_tile(egz) + cnt * U * per_tile(np.abs(gz) + egz), per_tile(et) + cnt * U * per_tile(t + et)], 3)
    g2 = 2 * GRAN[v]
    o["exact"] = np.stack([per_tile(np.abs(gz)) * 2.0 ** g2 < 2.0 ** 24, per_tile(t) * 2.0 ** g2 < 2.0 ** 24], 3) & (c.act != LRELU)
    assert 1 <= cnt.min() and cnt.max() <= 36
    return o


def fused_output_run(dev, c, integer):
    """one launch of the fused mode over armed buffers; returns (g_a [B][H-2][W-2][K], fuse_part [B][TH][TW][2][K]) as written"""
    o = fuse_data(c, integer)
    st = stream(dev)
    H, W = c.hw
    TH, TW = tiles_of(H, W, 6)
    T = c.B * TH * TW
    n_g, n_p = c.B * (H - 2) * (W - 2) * c.K, T * 2 * c.K
    what = f"{tuple(c)} {'integer' if integer else 'random'}"
    Md, yd, md, sd = (dev_t(o[k], dev) for k in ("M", "y", "mean", "rstd"))
    g2 = dev_t(o["g2"], dev) if c.g2 else None
    gz, part, y = Armed(n_g, dev), Armed(n_p + SLACK, dev), Armed(c.B * H * W * c.K, dev)
    d = L.Wino6Desc()
    d.B, d.H, d.W, d.C, d.K, d.r, d.algo = c.B, H, W, c.K, c.K, 6, c.algo
    d.M, d.M_elems, d.y = Md.data_ptr(), Md.numel(), y.ptr
    d.fuse_y, d.fuse_mean, d.fuse_rstd, d.fuse_g2 = yd.data_ptr(), md.data_ptr(), sd.data_ptr(), (g2.data_ptr() if c.g2 else None)
    d.fuse_gz, d.fuse_part, d.fuse_part_elems, d.fuse_act, d.fuse_slope = gz.ptr, part.ptr, n_p + SLACK, c.act, o["slope"]
    ran_on(what, d, L.W6_STAGE_OUTPUT, c.kernel)
    twice(dev, lambda: L.call("nirgan_wino6_output", C.byref(d), st), [gz, part, y])
    untouched(what + " y", y)
    return owned(what + " fuse_gz", gz, n_g).reshape(o["ga"].shape), owned(what + " fuse_part", part, n_p).reshape(o["part"].shape)


def fused_checks(c, integer, ga, part):
    o = fuse_data(c, integer)
    what = f"{tuple(c)} {'integer' if integer else 'random'}"
    held(f"wino6_output fused g_a {c.kernel}", what, ga, o["ga"], o["bga"], integer)
    held(f"wino6_output fuse_part {c.kernel}", what, part, o["part"], o["bpart"], integer, o["exact"])


def fused_output_against_float64(dev, c):
    for integer in (True, False):
        o = fuse_data(c, integer)
        what = f"{tuple(c)} {'integer' if integer else 'random'}"
        ga, part = fused_output_run(dev, c, integer)
        fused_checks(c, integer, ga, part)
        twin = next(x for x in FUSE_CASES if x.algo == 0 and x[:3] + x[4:6] == c[:3] + c[4:6])       # the same shape on the default route
        if c.algo == PT and twin.kernel == COOPK:   # the two forms: g_a bitwise equal, as the lane-spread kernel's comment promises
            ga2, part2 = fused_output_run(dev, twin, integer)
            assert np.array_equal(ga.view(np.uint32), ga2.view(np.uint32)), f"{what}: g_a of the two forms differs"


# ---------------------------------------------------------------------------------------------------------------- guards
def _refused(be, dev, what, rc, outs):
    sync(dev)
    assert fails(rc), f"{what}: accepted"
    assert be.nirgan_last_error(), f"{what}: no error message"
    for o in outs:
        assert (o.bits() == SENT32).all(), f"{what}: refused, but a buffer was written"


def _base(dev, v, B, H, W, Cc, K, bufs):
    """a valid descriptor of every stage over the armed buffers ``bufs`` (x, U, V, M, y, zero page are large enough for every guard case)"""
    r, mo, n = w6_geo(v)
    d = L.Wino6Desc()
    d.x, d.x_hp, d.x_wp = bufs["x"].data_ptr(), H + r - 1, W + r - 1
    d.B, d.H, d.W, d.C, d.K, d.r = B, H, W, Cc, K, v
    T = B * int(np.prod(tiles_of(H, W, v)))
    d.U, d.zero_page = bufs["x"].data_ptr(), bufs["zero"].data_ptr()
    d.V, d.V_elems, d.M, d.M_elems, d.y = bufs["V"].ptr, n * n * T * Cc, bufs["M"].ptr, n * n * T * K, bufs["y"].ptr
    return d, T


def query_guards(be, D, stages, unsupported):
    """nirgan_wino6_transform_kernel_name names no kernel for a NULL descriptor, an unknown variant, algo or stage, and for a stage the
    variant does not have (``unsupported``: (descriptor, stage) pairs); the emulator has no kernels to name"""
    if L.is_emulated():
        return
    name = be.nirgan_wino6_transform_kernel_name
    for stage in stages:
        assert name(C.byref(D()), stage), f"stage {stage}: a valid descriptor names no kernel"
        assert name(None, stage) == b"", f"stage {stage}: NULL descriptor"
        assert name(C.byref(D(r=5)), stage) == b"", f"stage {stage}: variant 5"
        assert name(C.byref(D(algo=2)), stage) == b"", f"stage {stage}: retired algo 2"
    for stage in (-1, 4):
        assert name(C.byref(D()), stage) == b"", f"unknown stage {stage}"
    for d, stage in unsupported:
        assert name(C.byref(d), stage) == b"", f"stage {stage} of variant {d.r}, C = {d.C}"


def input_guards(dev):
    be, st = L.backend(), stream(dev)
    bufs = {"x": torch.ones(1 << 16, device=dev), "zero": torch.zeros(64, device=dev), "V": Armed(1 << 16, dev), "M": Armed(1 << 16, dev),
            "y": Armed(1 << 14, dev), "Yt": Armed(1 << 16, dev)}
    outs = [bufs[k] for k in ("V", "M", "y", "Yt")]
    R = lambda what, rc: _refused(be, dev, what, rc, outs)

    def D(v=6, Cc=32, H=7, W=8, **kw):
        d, _ = _base(dev, v, 2, H, W, Cc, 128, bufs)
        for k, val in kw.items():
            setattr(d, k, val)
        return d

    def Y(d, **kw):
        r = w6_geo(d.r)[0]
        y = L.WinoDyDesc()
        y.dy, y.dy_pad, y.dy_hp, y.dy_wp, y.B, y.H, y.W, y.K, y.r = d.x, r - 1, d.x_hp, d.x_wp, d.B, d.H - r + 1, d.W - r + 1, d.C, d.r
        y.Yt, y.Yt_elems = bufs["Yt"].ptr, 1 << 16
        for k, val in kw.items():
            setattr(y, k, val)
        return y

    ok = D()
    for name in ("input", "input_dy"):
        call = (lambda d, y=None: be.nirgan_wino6_input(C.byref(d), st)) if name == "input" else (lambda d, y=None: be.nirgan_wino6_input_dy(C.byref(d), C.byref(y or Y(d)), st))
        R(f"{name}: variant 5", call(D(r=5)))
        R(f"{name}: retired algo 2", call(D(algo=2)))
        R(f"{name}: retired algo 4", call(D(algo=4)))
        R(f"{name}: x_hp", call(D(x_hp=ok.x_hp + 1)))
        R(f"{name}: x_wp", call(D(x_wp=ok.x_wp - 1)))
        R(f"{name}: V one element too small", call(D(V_elems=ok.V_elems - 1)))
        R(f"{name}: C % 4", call(D(Cc=6)))
    d = D()
    for what, kw in (("another buffer", {"dy": d.x + 16}), ("another halo", {"dy_pad": 1}), ("another extent", {"H": 6}), ("another width", {"W": 5}),
                     ("other channels", {"K": 16}), ("another variant", {"r": 3}), ("another batch", {"B": 1})):
        R(f"input_dy: {what}", be.nirgan_wino6_input_dy(C.byref(d), C.byref(Y(d, **kw)), st))
    R("input_dy: Yt one element too small", be.nirgan_wino6_input_dy(C.byref(d), C.byref(Y(d, Yt_elems=64 * 2 * 1 * 1 * 32 - 1)), st))
    p = bufs["x"].data_ptr()
    R("input_norm: variant 4", be.nirgan_wino6_input_norm(C.byref(D(v=4)), p, p, p, RELU, 0.0, st))
    R("input_norm: C % 4", be.nirgan_wino6_input_norm(C.byref(D(Cc=6)), p, p, p, RELU, 0.0, st))
    R("input_norm: V one element too small", be.nirgan_wino6_input_norm(C.byref(D(V_elems=ok.V_elems - 1)), p, p, p, RELU, 0.0, st))
    y = Y(D(H=9, W=10))
    y.dy_pad, y.dy_hp, y.dy_wp = 1, y.H + 2, y.W + 2
    R("dy: variant 5", be.nirgan_wino6_dy(C.byref(Y(D(), r=5)), st))
    y.dy_hp += 1
    R("dy: dy_hp", be.nirgan_wino6_dy(C.byref(y), st))
    y.dy_hp -= 1
    y.Yt_elems = 64 * 2 * 2 * 2 * 32 - 1
    R("dy: Yt one element too small", be.nirgan_wino6_dy(C.byref(y), st))
    # input_dy_norm: the fused dY pass exists for F(6x6,3x3) with C % 32 == 0
    nb = L.InBwdDesc()
    nb.norm, nb.y, nb.mean, nb.rstd, nb.ws, nb.ws_elems, nb.g2 = 1, p, p, p, p, 1 << 16, p
    for what, kw in (("variant 4", {"v": 4, "Cc": 32}), ("C % 32", {"v": 6, "Cc": 36})):
        d = D(**kw)
        y = Y(d)
        nb.B, nb.C, nb.H, nb.W = d.B, d.C, y.H, y.W
        R(f"input_dy_norm: {what}", be.nirgan_wino6_input_dy_norm(C.byref(d), C.byref(y), C.byref(nb), st))
    query_guards(be, D, (L.W6_STAGE_INPUT, L.W6_STAGE_INPUT_NORM, L.W6_STAGE_INPUT_DY_NORM),
                 [(D(v=4), L.W6_STAGE_INPUT_NORM), (D(v=4), L.W6_STAGE_INPUT_DY_NORM), (D(v=3), L.W6_STAGE_INPUT_DY_NORM), (D(Cc=36), L.W6_STAGE_INPUT_DY_NORM)])


def gemm_guards(dev):
    be, st = L.backend(), stream(dev)
    bufs = {"x": torch.ones(1 << 19, device=dev), "zero": torch.zeros(64, device=dev), "V": Armed(1 << 10, dev), "M": Armed(1 << 17, dev), "y": Armed(64, dev)}
    V = torch.ones(1 << 16, device=dev)
    R = lambda what, rc: _refused(be, dev, what, rc, [bufs["M"], bufs["y"]])

    def D(v=6, Cc=32, K=128, **kw):
        d, _ = _base(dev, v, 2, 7, 8, Cc, K, bufs)
        d.V = V.data_ptr()
        for k, val in kw.items():
            setattr(d, k, val)
        return d

    ok = D()
    R("gemm: variant 5", be.nirgan_wino6_gemm(C.byref(D(r=5)), st))
    R("gemm: retired algo 2", be.nirgan_wino6_gemm(C.byref(D(algo=2)), st))
    R("gemm: retired algo 4", be.nirgan_wino6_gemm(C.byref(D(algo=4)), st))
    R("gemm: V one element too small", be.nirgan_wino6_gemm(C.byref(D(V_elems=ok.V_elems - 1)), st))
    R("gemm: M one element too small", be.nirgan_wino6_gemm(C.byref(D(M_elems=ok.M_elems - 1)), st))
    R("gemm: C % 4", be.nirgan_wino6_gemm(C.byref(D(Cc=6)), st))
    R("gemm: K = 64", be.nirgan_wino6_gemm(C.byref(D(K=64)), st))
    R("gemm: K = 32", be.nirgan_wino6_gemm(C.byref(D(K=32)), st))
    R("gemm: K % 4", be.nirgan_wino6_gemm(C.byref(D(K=70)), st))
    R("gemm: neither U nor its planes", be.nirgan_wino6_gemm(C.byref(D(U=None)), st))


def output_guards(dev):
    be, st = L.backend(), stream(dev)
    bufs = {"x": torch.ones(1 << 17, device=dev), "zero": torch.zeros(64, device=dev), "V": Armed(64, dev), "M": Armed(64, dev), "y": Armed(1 << 15, dev),
            "gz": Armed(1 << 15, dev), "part": Armed(1 << 12, dev), "stats": Armed(1 << 13, dev)}
    outs = [bufs[k] for k in ("y", "gz", "part", "stats")]
    R = lambda what, rc: _refused(be, dev, what, rc, outs)
    p = bufs["x"].data_ptr()

    def D(v=6, K=32, H=9, W=10, fused=False, **kw):
        d, T = _base(dev, v, 2, H, W, 32, K, bufs)
        d.M = p
        if fused:
            d.fuse_y, d.fuse_mean, d.fuse_rstd, d.fuse_gz, d.fuse_part, d.fuse_part_elems, d.fuse_act = p, p, p, bufs["gz"].ptr, bufs["part"].ptr, T * 2 * K, RELU
        for k, val in kw.items():
            setattr(d, k, val)
        return d

    ok = D()
    R("output: variant 5", be.nirgan_wino6_output(C.byref(D(r=5)), st))
    R("output: retired algo 2", be.nirgan_wino6_output(C.byref(D(algo=2)), st))
    R("output: M one element too small", be.nirgan_wino6_output(C.byref(D(M_elems=ok.M_elems - 1)), st))
    R("output: K % 4", be.nirgan_wino6_output(C.byref(D(K=6)), st))
    R("output: stats_ws one element too small", be.nirgan_wino6_output(C.byref(D(stats_ws=bufs["stats"].ptr, stats_ws_elems=2 * 2 * 2 * 4 * 32 - 1)), st))
    for H in (7, 8, 13):
        R(f"output: fused mode with H = {H}", be.nirgan_wino6_output(C.byref(D(H=H, fused=True)), st))
        R(f"output: fused mode with W = {H}", be.nirgan_wino6_output(C.byref(D(W=H, fused=True)), st))
    R("output: fused mode with H = 5", be.nirgan_wino6_output(C.byref(D(H=5, fused=True)), st))
    R("output: fused mode with a bias", be.nirgan_wino6_output(C.byref(D(fused=True, bias=p)), st))
    R("output: fused mode with stats_ws", be.nirgan_wino6_output(C.byref(D(fused=True, stats_ws=bufs["stats"].ptr, stats_ws_elems=1 << 13)), st))
    R("output: fused mode of F(4x4,3x3)", be.nirgan_wino6_output(C.byref(D(v=3, fused=True)), st))
    R("output: fuse_part one element too small", be.nirgan_wino6_output(C.byref(D(fused=True, fuse_part_elems=2 * 2 * 2 * 2 * 32 - 1)), st))
    R("output: fused mode without fuse_y", be.nirgan_wino6_output(C.byref(D(fused=True, fuse_y=None)), st))
    R("output: fuse_act 3", be.nirgan_wino6_output(C.byref(D(fused=True, fuse_act=3)), st))
    query_guards(be, D, (L.W6_STAGE_OUTPUT,), [(D(v=3, fused=True), L.W6_STAGE_OUTPUT), (D(v=4, fused=True), L.W6_STAGE_OUTPUT)])


# ---------------------------------------------------------------------------------------------------------------- stage 1: the fused dY pass
# nirgan_wino6_input_dy_norm (wino6_input_coop_kernel<6,2>): dY is the instance-norm backward's second pass evaluated on the fly.  The
# float64 dY and its bound are tests/instnorm_cases.py's (bwd_case over the same case construction); nirgan_instnorm_bwd with dy = NULL
# runs first and leaves the two means in ws, where the kernel reads them.  Random pass only: a normalised gradient has no integer form.
DyNorm = namedtuple("DyNorm", "kind shape")            # shape = (B, H, W, C) of dY
DYNORM_CASES = [DyNorm("fold", (2, 4, 6, 32)), DyNorm("skip", (1, 8, 7, 32)), DyNorm("pre", (2, 7, 8, 64)), DyNorm("fold", (1, 9, 9, 32)),
                DyNorm("skip", (1, 10, 4, 96)), DyNorm("pre", (1, 4, 6, 96))]
DYNORM_KERNEL = "wino6_input_coop_kernel<6,2>"


def dynorm_spec(c):
    kw = {"fold": dict(fold=True, g_pad=1, act=RELU), "skip": dict(fold=True, g_pad=1, g2=True, gsum=True, act=NONE),
          "pre": dict(g=False, pre="gsum", act=RELU)}[c.kind]
    return dict(shape=c.shape, dy=None, **kw)


def dynorm_case(c):
    """instnorm_cases.bwd_case of the block (cached there under a key of its own)"""
    import instnorm_cases as I
    key = f"wino6_input_dy_norm {c.kind} {c.shape}"
    I.BWD[key] = dynorm_spec(c)
    try:
        return key, I.bwd_case(key)
    finally:
        del I.BWD[key]


def dynorm_against_float64(dev, c):
    import instnorm_cases as I
    key, bc = dynorm_case(c)
    B, H, W, Cc = c.shape
    I.kink_free(bc["z"], bc["b_z"], False)
    st, what = stream(dev), f"{tuple(c)} random"
    nd, keep, need = I.bwd_desc(dev, key, None)
    L.call("nirgan_instnorm_bwd", C.byref(nd), st)            # dy = NULL: the two reductions; their means stay in ws
    sync(dev)
    pch = I.PRE_CHUNKS if c.kind == "pre" else I.geometry(c.shape)["nchunk"]
    within("in_bwd means (ws)", what, keep["ws"].cpu()[B * pch * 2 * Cc:need].reshape(B, 2, Cc), bc["m"], bc["b_m"])
    # the buffer the two descriptors describe: neither read nor written -- it holds the sentinel NaN
    hole = Armed(B * (H + 4) * (W + 4) * Cc, dev, extra=0)
    Hd, Wd = H + 2, W + 2
    T, yT = B * int(np.prod(tiles_of(Hd, Wd, 6))), B * int(np.prod(tiles_of(H, W, 6)))
    n_v, n_yt = 64 * T * Cc, 64 * yT * Cc
    V, Yt = Armed(n_v + SLACK, dev), Armed(n_yt + SLACK, dev)
    case = In("input_dy", 6, Cc, (H, W), B, 0, 0, DYNORM_KERNEL)
    d = in_desc(case, Hd, Wd, hole.ptr, V, n_v)
    y = dy_desc(case, hole.ptr, 2, Yt, n_yt)
    ran_on(what, d, L.W6_STAGE_INPUT_DY_NORM, DYNORM_KERNEL)
    ws_before = keep["ws"].cpu().clone()
    twice(dev, lambda: L.call("nirgan_wino6_input_dy_norm", C.byref(d), C.byref(y), C.byref(nd), st), [V, Yt])
    untouched(what + " the buffer behind c->x / y->dy", hole)
    assert torch.equal(keep["ws"].cpu().view(torch.int32), ws_before.view(torch.int32)), f"{what}: ws was written"
    dy, b_dy = bc["dy"].numpy(), bc["b_dy"].numpy()
    x = np.zeros((B, H + 4, W + 4, Cc))
    e = np.zeros_like(x)
    x[:, 2:2 + H, 2:2 + W], e[:, 2:2 + H, 2:2 + W] = dy, b_dy
    Vr, A, _ = v_ref(x, Hd, Wd, 6)
    bV = KR_IN[6] * U * A + v_ref(e, Hd, Wd, 6)[1] * (1 + KR_IN[6] * U)
    held(f"wino6_input_dy_norm V {DYNORM_KERNEL}", what, owned(what + " V", V, n_v), Vr.reshape(-1), bV.reshape(-1), False)
    Yr, A, _ = yt_ref(dy, 6)
    bY = KR_YT[6] * U * A + yt_ref(b_dy, 6)[1] * (1 + KR_YT[6] * U)
    held(f"wino6_input_dy_norm Yt {DYNORM_KERNEL}", what, owned(what + " Yt", Yt, n_yt), Yr.reshape(-1), bY.reshape(-1), False)


# ---------------------------------------------------------------------------------------------------------------- stage 2: the fused pair
# nirgan_wino6_gemm_wgrad_pair: the two descriptors as the engine builds them (emit_wino6 + emit_wino6_backward, B = 1), then the pair op
# alone over armed buffers.  opt: the options the route needs (the split tile runs the pair as two ops of the plan: split3 off here)
Pair = namedtuple("Pair", "v hw cin cout opt kernel")
PAIR_CASES = [
    Pair(6, (18, 13), 128, 128, {}, "wino6_pair_kernel"),
    Pair(4, (9, 11), 128, 96, {}, "wino6_pair_kernel"),
    Pair(6, (18, 18), 128, 256, {}, "wino6_pair16p_kernel"),
    Pair(6, (7, 13), 68, 256, {"wgrad_algo": L.WGRAD_ONE_UNIT}, "wino6_pair16_kernel"),
    Pair(6, (12, 18), 128, 64, {}, ""),                      # a weight gradient of 64 rows: two launches
]


def pair_descs(dev, c):
    """(copies of the data gradient's nirgan_wino6_desc and the weight gradient's nirgan_wgrad_desc of the plan's pair op, what keeps the
    plan's buffers alive)"""
    from nirgan_hip.engine import Ctx, Halo, Plan, SlabPool, _FullExtent, emit_wino6, emit_wino6_backward
    from nirgan_hip.options import OPT
    from wgrad_replay import copy_desc
    r = w6_geo(c.v)[0]
    H, W = c.hw
    OPT.reset()
    try:
        OPT.split3 = False
        if c.v == 3:
            OPT.winograd = "f4"
        for k, val in c.opt.items():
            assert hasattr(OPT, k)
            setattr(OPT, k, val)
        ctx = Ctx(dev, "fp32")
        inp, dy, gx = Halo(ctx, 1, H + r - 3, W + r - 3, c.cin, 1), Halo(ctx, 1, H, W, c.cout, r - 1), Halo(ctx, 1, H + r - 3, W + r - 3, c.cin, 1)
        gw, wd = ctx.zeros(c.cout, c.cin, r, r), ctx.zeros(c.cout, c.cin, r, r)
        plan, pack = Plan(ctx), Plan(ctx)
        wdesc = emit_wino6(None, pack, ctx, dy, wd, None, _FullExtent(gx), H=gx.hp, W=gx.wp, cin=c.cout, cout=c.cin, flip=True, r=r)
        emit_wino6_backward(plan, ctx, dy, inp, gw, OH=H, OW=W, cin=c.cin, cout=c.cout, slabs_pool=SlabPool(ctx), dgrad=wdesc, r=r)
    finally:
        OPT.reset()
    ops = [args for op, args in plan.ops if op == "nirgan_wino6_gemm_wgrad_pair"]
    assert len(ops) == 1, [op for op, _ in plan.ops]
    return copy_desc(ops[0][0]._obj), copy_desc(ops[0][1]._obj), (ctx, plan, pack, inp, dy, gx, gw, wd)


def pair_against_float64(dev, c):
    from wgrad_replay import restate_with_scale, slab_count
    cd, wd, keep = pair_descs(dev, c)
    r, mo, n = w6_geo(c.v)
    npl, st = n * n, stream(dev)
    T = int(L.backend().nirgan_wino6_tiles_r(cd.B, cd.H, cd.W, cd.r))
    assert (cd.C, cd.K, wd.N, max(wd.nplanes, 1), wd.precision, cd.r) == (c.cout, c.cin, c.cout, npl, 0, c.v) and not cd.U3 and not wd.pq_bf16
    zero = torch.zeros(64, device=dev)
    n_m, n_s = npl * T * cd.K, slab_count(wd)
    for integer in (True, False):
        what = f"{tuple(c)} {'integer' if integer else 'random'}"
        seed = 19 * PAIR_CASES.index(c) + integer
        Vh, Uh = draw((npl, T, cd.C), integer, seed), draw((npl, cd.K, cd.C), integer, seed + 1)
        ph, qh = draw((wd.p_elems,), integer, seed + 2), draw((wd.q_elems,), integer, seed + 3)
        Vd, Ud, pd, qd = (dev_t(a, dev) for a in (Vh, Uh, ph, qh))
        M, slabs = Armed(n_m + SLACK, dev), Armed(max(int(wd.slab_elems), n_s) + SLACK, dev)
        cd.V, cd.V_elems, cd.U, cd.M, cd.M_elems, cd.zero_page = Vd.data_ptr(), Vd.numel(), Ud.data_ptr(), M.ptr, n_m + SLACK, zero.data_ptr()
        wd.p, wd.q, wd.slabs, wd.slab_elems, wd.zero_page = pd.data_ptr(), qd.data_ptr(), slabs.ptr, max(int(wd.slab_elems), n_s) + SLACK, zero.data_ptr()
        if not L.is_emulated():
            name = L.backend().nirgan_wino6_pair_kernel_name(C.byref(cd), C.byref(wd)).decode()
            assert name == c.kernel, f"{what}: the launch takes {name!r}"
        twice(dev, lambda: L.call("nirgan_wino6_gemm_wgrad_pair", C.byref(cd), C.byref(wd), st), [M, slabs])
        ref = Vh.astype(np.float64) @ Uh.astype(np.float64).transpose(0, 2, 1)
        A = np.abs(Vh).astype(np.float64) @ np.abs(Uh).astype(np.float64).transpose(0, 2, 1)
        val, scale = (t.numpy() for t in restate_with_scale(wd, torch.from_numpy(ph), torch.from_numpy(qh), 0))
        if integer:
            exact_or_die(what, [(A, 0), (scale, 0)])
        fam = f"wino6_pair {c.kernel or 'two launches'}"
        held(fam + " M", what, owned(what + " M", M, n_m), ref.reshape(-1), ((cd.C + 8) * U * A).reshape(-1), integer)
        held(fam + " slabs", what, owned(what + " slabs", slabs, n_s), val.reshape(-1), ((wd.rows_per_split + wd.nsplit + 8) * U * scale).reshape(-1), integer)
