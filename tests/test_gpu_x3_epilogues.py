"""The three epilogue kinds of the four-wave split tile (csrc/igemm_x3r.h, conv_x3r_kernel<128, KIND>; igemm_conv.hip::conv_x3_route):
0 plain (no stats_ws, no fuse_y), 1 instance-norm statistics records (stats_ws), 2 the fused first pass of the instance-norm backward
(fuse_y, from NG_X3R_GEN_MIN_NK = 24 K-tiles on) -- each against the eight-wave tile conv_x3_kernel<128> (descriptor algo 0) on the same
operands and against float64.

The workspaces the epilogues write into are filled with a sentinel bit pattern before every launch and compared as int32: every record
outside the launch's own chunks [chunk0, chunk0 + chunks) -- a guard sample behind the last one included -- must keep it (records of
waves past M, wrong stats_chunk0 / fuse_chunk0 arithmetic).

The record bounds are the recursive-summation bounds of the sums, not tuned tolerances: a statistics record sums 64 rows (70 u), a
fused-pass record 128 rows (135 u), u = 2^-24, relative to the sum of the magnitudes of the terms.

The launch needs at least 192 tiles of 256 x 128 (three quarters of the CUs) for 128-column tiles (igemm_x3.h::conv_x3_bn), and only
128-column tiles take the four-wave tile: the shapes below keep the geometry each case is about and scale the batch to get there.

Last: outputs of 3 and 4.5 GiB.  The plain and statistics kinds store full tiles with 32-bit byte offsets from the output base
(epilogue_full), so the four-wave tile takes only outputs below 2^32 bytes (conv_x3r_ok); larger ones run on the eight-wave tile."""
import ctypes as C
import gc

import pytest
import torch

from nirgan_hip import geometry as G
from nirgan_hip import lib as L
from nirgan_hip.engine import IN_EPS, Ctx, Halo, Plan, Weights, emit_conv, emit_phase_pairs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R4 = L.CONV_X3_R4
SENT = 0x7FA5A5A5                 # a NaN no kernel computes
U = 2.0 ** -24
STATS_BOUND, FUSED_BOUND = 70 * U, 135 * U


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


class _Eng:
    def __init__(self, ctx):
        self.ctx, self.weights = ctx, Weights(ctx)


def _err(got, ref):
    e = (got.double() - ref).abs()
    s = ref.abs().max().item()
    return e.max().item() / s, e.pow(2).mean().sqrt().item() / s


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sentinel(t):
    t.view(torch.int32).fill_(SENT)


def _split3(ctx, t):
    n = t.numel()
    plane = (n + 7) // 8 * 8
    tw = torch.zeros(3 * plane, dtype=torch.bfloat16, device=DEV)
    L.call("nirgan_split3", t.data_ptr(), tw.data_ptr(), n, plane, None)
    ctx.keep.append(tw)
    return tw, plane


def _packed(ctx, w, k):
    """conv weights [cout][cin][k][k] packed [N][K] with their three bf16 planes"""
    cout, cin = w.shape[:2]
    spec = G.conv_fwd_pack(cout, cin, k)
    wp = ctx.zeros(spec.N, spec.K)
    ctx.keep.append(wp)
    L.call("nirgan_pack_rows", w.data_ptr(), w.numel(), spec.row_stride, ctx.i32(spec.index_map).data_ptr(), wp.data_ptr(), spec.N, spec.K, None)
    return wp, _split3(ctx, wp)


def _conv_desc(ctx, x, w, wp, planes, bias, y, s, **kw):
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    OH, OW = G.conv_out(x.hp, k, s, 0), G.conv_out(x.wp, k, s, 0)
    d = emit_conv(None, ctx, x, G.conv_fwd_taps(k, cin), wp, bias, y, N=cout, OH=OH, OW=OW, in_stride=s, allow_split=False, **kw)
    d.precision, d.w_x3, d.w_x3_plane = 3, planes[0].data_ptr(), planes[1]
    return d


def _launch(descs):
    if len(descs) == 1:
        L.call("nirgan_conv_igemm", C.byref(descs[0]), None)
    else:
        arr = (C.POINTER(L.ConvDesc) * len(descs))(*[C.pointer(d) for d in descs])
        L.call("nirgan_conv_igemm_group", arr, len(descs), None)


def _name(d):
    return L.backend().nirgan_conv_kernel_name(C.byref(d))


def _check_name(descs, algo):
    """the name query of a single-problem launch (a group has none: its kind is stated by the case and seen in a kernel trace)"""
    if len(descs) == 1:
        name = _name(descs[0])
        assert (name.startswith(b"conv_x3r_kernel<128>") if algo else name == b"conv_x3_kernel<128>"), name


def _run(descs, algo, out, ws, bias=None, name=True):
    """two launches of `descs` with algo (and bias pointers, or none), the output NaN-filled and the workspace sentinel-filled before
    each: both launches bitwise alike; returns (output, workspace)"""
    for i, d in enumerate(descs):
        d.algo = algo
        d.bias = None if bias is None else bias[i]
    if name:
        _check_name(descs, algo)
    got = None
    for _ in range(2):
        out.fill_(float("nan"))
        _sentinel(ws)
        _launch(descs)
        torch.cuda.synchronize()
        cur = (out.clone(), ws.clone())
        if got is not None:
            assert torch.equal(_bits(cur[0]), _bits(got[0])) and torch.equal(_bits(cur[1]), _bits(got[1])), "a launch differs from the first one"
        got = cur
    return got


def _view(t, d, oh0, ow0, q, ch):
    """[B][OH][OW][ch] of what GEMM row (oh, ow), pixel q of its out_span, addresses in the halo'd buffer t"""
    s = d.out_stride
    return t[:, oh0:oh0 + (d.OH - 1) * s + 1:s, ow0 + q:ow0 + q + (d.OW - 1) * s + 1:s, :ch]


def _records(ws, B, cps, fields, ch):
    return ws[:B * cps * fields * ch].view(B, cps, fields, ch)


def _untouched_keep_sentinel(ws, B, cps, fields, ch, written):
    rec = _bits(ws[:B * cps * fields * ch]).view(B, cps, fields * ch)
    assert (rec[~written] == SENT).all(), "a record outside the launch's chunks was written"
    assert (_bits(ws[B * cps * fields * ch:]) == SENT).all(), "a record past the last sample was written"


def _check_stats(ws, y0, descs, B, cps):
    """statistics records [B][cps][4][ch] against float64 on the bias-free launch's own stored output y0: k bitwise y0 at the chunk's
    first pixel, count 64, s1 / s2 within the 64-term summation bound"""
    ch = descs[0].N // max(1, descs[0].out_span)
    rec = _records(ws, B, cps, 4, ch)
    written = torch.zeros(B, cps, dtype=torch.bool, device=DEV)
    for d in descs:
        span = max(1, d.out_span)
        nch = d.OH * d.OW // 64
        for q in range(span):
            v = _view(y0, d, d.out_oh, d.out_ow, q, ch).reshape(B, nch, 64, ch)
            idx = d.stats_chunk0 + torch.arange(nch, device=DEV) * span + q
            r = rec[:, idx]
            k = v[:, :, 0]
            assert torch.equal(_bits(r[:, :, 0]), _bits(k)), "k is not the chunk's first pixel"
            assert (r[:, :, 3] == 64.0).all(), "count"
            t = v.double() - k.double()[:, :, None]
            s1, s2 = t.sum(2), t.pow(2).sum(2)
            assert ((r[:, :, 1].double() - s1).abs() <= STATS_BOUND * t.abs().sum(2)).all(), "sum (v - k)"
            assert ((r[:, :, 2].double() - s2).abs() <= STATS_BOUND * s2).all(), "sum (v - k)^2"
            written[:, idx] = True
    _untouched_keep_sentinel(ws, B, cps, 4, ch, written)


def _same_records(a, b, B, cps, ch, what):
    """k, sum (v - k) and the count bitwise; sum (v - k)^2 within the 64-term bound of each other.  Why not bitwise: both tiles take the
    same rows in the same per-lane order (mt, then r) and the same xor-16 / xor-32 shuffles -- k, sum (v - k) and the count agree in every
    record -- but sum (v - k)^2 is formed differently.  The four-wave tile's is exactly the v_fmac chain of stats_acc in that order; the
    eight-wave tile's `s2 += v * v` (conv_x3_persist) reproduces neither that fused chain nor the separately rounded one (checked against
    both, emulated in fp32): measured, ~2 % of its records differ from the four-wave tile's, by at most ~4 u sum (v - k)^2, and both
    stay at ~3.6 u of float64 -- far inside the 70 u bound each is held to against float64 (_check_stats)."""
    ra, rb = _records(a, B, cps, 4, ch), _records(b, B, cps, 4, ch)
    for f in (0, 1, 3):
        assert torch.equal(_bits(ra[:, :, f]), _bits(rb[:, :, f])), f"{what}: field {f}"
    a2, b2 = ra[:, :, 2], rb[:, :, 2]
    near = (a2.double() - b2.double()).abs() <= STATS_BOUND * a2.double().abs()
    assert (near | (_bits(a2) == _bits(b2))).all(), f"{what}: sum (v - k)^2"         # (bits: the sentinel of unwritten chunks)
    assert torch.equal(_bits(a[B * cps * 4 * ch:]), _bits(b[B * cps * 4 * ch:])), f"{what}: guard"


def _in_fwd_stats(y, B, H, W, Cc, ws, cps, shift):
    """nirgan_instnorm_fwd on the producer's records (statistics only): mean, rstd"""
    mean, rstd = torch.zeros(B, Cc, device=DEV), torch.zeros(B, Cc, device=DEV)
    d = L.InFwdDesc()
    d.y, d.B, d.H, d.W, d.C = y.data_ptr(), B, H, W, Cc
    d.norm, d.eps, d.mean, d.rstd = 1, IN_EPS, mean.data_ptr(), rstd.data_ptr()
    d.act = L.ACT_NONE
    d.ws, d.ws_elems, d.stats_chunks, d.stats_shift = ws.data_ptr(), ws.numel(), cps, shift.data_ptr()
    L.call("nirgan_instnorm_fwd", C.byref(d), None)
    torch.cuda.synchronize()
    yd = y.double().reshape(B, H * W, Cc)
    ref_m = yd.mean(1)
    ref_r = 1.0 / torch.sqrt(yd.var(1, unbiased=False) + IN_EPS)
    assert (mean.double() - ref_m).abs().max().item() <= 1e-6 * ref_m.abs().max().item(), "mean"
    assert (rstd.double() - ref_r).abs().max().item() <= 3e-6 * ref_r.abs().max().item(), "rstd"


def _stats_case(descs, y, ref, ref_bias, bias, shift, B, cps, consumer=True):
    """kind 1: both algos bias-free and with the bias; outputs bitwise alike and at float64; records bitwise alike, against float64, and
    with the bias bitwise those without it (the records are of the output without the bias); the consumer on the four-wave records"""
    ch = descs[0].N // max(1, descs[0].out_span)
    ws = torch.zeros((B + 1) * cps * 4 * ch, device=DEV)          # (+ a guard sample)
    for d in descs:
        d.stats_ws, d.stats_ws_elems, d.stats_chunks = ws.data_ptr(), B * cps * 4 * ch, cps
    res = {(a, b): _run(descs, a, y, ws, bias if b else None) for a in (0, R4) for b in (False, True)}
    for b, r in ((False, ref), (True, ref_bias)):
        assert torch.equal(_bits(res[(0, b)][0]), _bits(res[(R4, b)][0])), "output: four-wave tile against eight-wave tile"
        assert _err(res[(R4, b)][0], r)[0] < 2e-6
    for b in (False, True):
        _same_records(res[(0, b)][1], res[(R4, b)][1], B, cps, ch, "records: four-wave tile against eight-wave tile")
    assert torch.equal(_bits(res[(R4, True)][1]), _bits(res[(R4, False)][1])), "records with the bias differ from those without it"
    _check_stats(res[(R4, False)][1], res[(R4, False)][0], descs, B, cps)
    _check_stats(res[(0, False)][1], res[(0, False)][0], descs, B, cps)
    if consumer:
        yb = res[(R4, True)][0]
        _in_fwd_stats(yb, B, yb.shape[1], yb.shape[2], ch, res[(R4, True)][1], cps, shift)


STATS_CONVS = [  # name, B, H, W, cin, cout, k, stride, chunk0 / spare chunks
    ("straddle", 129, 16, 24, 64, 128, 3, 1, 0),      # OH OW = 384: 256-row items straddle samples, the last item half filled
    ("odd_width", 2, 128, 133, 64, 256, 3, 1, 0),     # OW = 133: the row walk wraps inside a slice; two column tiles
    ("ow16", 200, 16, 16, 64, 128, 3, 1, 0),          # OW = 16, the least conv_x3r_ok takes
    ("k1x1_cin96", 13, 64, 64, 96, 128, 1, 1, 0),     # 1 x 1, cin 96: three K-tiles, the cursor's minimum
    ("items512", 16, 128, 128, 128, 256, 3, 2, 0),    # 16 x 64 x 64, stride 2, N = 256: 512 items, stores behind the next item's waits
    ("chunk0", 129, 16, 24, 64, 128, 3, 1, 3),        # stats_chunk0 = 3 inside a workspace of chunks + 5 per sample
]


@pytest.mark.parametrize("case", STATS_CONVS, ids=[c[0] for c in STATS_CONVS])
def test_statistics_kind_is_the_eight_wave_tiles_records_and_float64(case):
    """kind 1 (stats_ws set, no fuse_y): conv_x3r_kernel<128, 1>"""
    _, B, H, W, cin, cout, k, s, chunk0 = case
    g = torch.Generator().manual_seed(51)
    ctx = Ctx(DEV)
    pad = k // 2
    x = Halo(ctx, B, H, W, cin, pad)
    x.interior().copy_(torch.randn(B, H, W, cin, generator=g).to(DEV))
    w = (torch.randn(cout, cin, k, k, generator=g) * 0.05).to(DEV)
    bias = (torch.randn(cout, generator=g) * 3.0).to(DEV)
    wp, planes = _packed(ctx, w, k)
    OH, OW = G.conv_out(H, k, s, pad), G.conv_out(W, k, s, pad)
    assert OH * OW % 128 == 0
    y = Halo(ctx, B, OH, OW, cout, 0)
    d = _conv_desc(ctx, x, w, wp, planes, None, y, s)
    d.stats_chunk0 = chunk0
    cps = OH * OW // 64 + (chunk0 + 2 if chunk0 else 0)
    xd = x.t.double().permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(xd, w.double(), None, stride=s).permute(0, 2, 3, 1)
    ref_b = ref + bias.double()
    _stats_case([d], y.t, ref, ref_b, [bias.data_ptr()], bias, B, cps, consumer=chunk0 == 0)


@pytest.mark.parametrize("shape", [(16, 32, 32), (21, 32, 32)])
def test_statistics_kind_on_the_four_transposed_conv_phases(shape):
    """kind 1 over ConvTranspose2d(256, 128, 3, s2, p1, op1)'s four sub-pixel phases (1 / 2 / 2 / 4 taps) as ONE group launch on the
    spread walk (64 and 84 tiles per phase), the chunks numbered across the phases into one workspace"""
    B, H, W = shape
    gen = torch.Generator().manual_seed(52)
    ctx = Ctx(DEV)
    eng = _Eng(ctx)
    Cin, Cout, k = 256, 128, 3
    x = Halo(ctx, B, H, W, Cin, 1)
    x.interior().copy_(torch.randn(B, H, W, Cin, generator=gen).to(DEV))
    w = (torch.randn(Cin, Cout, k, k, generator=gen) * 0.05).to(DEV)
    bias = (torch.randn(Cout, generator=gen) * 3.0).to(DEV)
    y = Halo(ctx, B, 2 * H, 2 * W, Cout, 0)
    pack = Plan(ctx)
    descs, first = [], 0
    for ph in G.convT_fwd_phases(H, W, k, 1):
        wp = eng.weights.packed(pack, w, G.convT_fwd_pack(Cin, Cout, k, ph.taps_hw))
        d = emit_conv(None, ctx, x, G.Taps(ph.dh, ph.dw, Cin), wp, bias, y, N=Cout, OH=ph.n_h, OW=ph.n_w,
                      in_oh=ph.in_oh, in_ow=ph.in_ow, out_stride=2, out_oh=ph.out_oh, out_ow=ph.out_ow)
        d.stats_chunk0 = first
        first += d.OH * d.OW // 64
        descs.append(d)
    pack.run()
    assert all(d.precision == 3 for d in descs) and sorted(d.ntaps for d in descs) == [1, 2, 2, 4]
    assert sum(-(-(d.B * d.OH * d.OW) // 256) for d in descs) >= 256          # a full grid: the spread walk
    biases = [d.bias for d in descs]
    xd = x.interior().permute(0, 3, 1, 2).double()
    ref = torch.nn.functional.conv_transpose2d(xd, w.double(), None, stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)
    _stats_case(descs, y.t, ref, ref + bias.double(), biases, bias, B, first)


@pytest.mark.parametrize("shape", [(16, 48, 48), (12, 32, 64)])
def test_statistics_kind_on_the_paired_phases(shape):
    """kind 1 on the out_span = 2 problems of engine.emit_phase_pairs (ConvTranspose2d(128, 64, 3, s2) + bias: 128 columns = two
    adjacent output pixels): two records per 64 GEMM rows, pixel parity 0 then 1"""
    B, H, W = shape
    gen = torch.Generator().manual_seed(53)
    ctx = Ctx(DEV)
    eng = _Eng(ctx)
    Cin, Cout, k = 128, 64, 3
    x = Halo(ctx, B, H, W, Cin, 1)
    x.interior().copy_(torch.randn(B, H, W, Cin, generator=gen).to(DEV))
    w = (torch.randn(Cin, Cout, k, k, generator=gen) * 0.05).to(DEV)
    bias = (torch.randn(Cout, generator=gen) * 3.0).to(DEV)
    y = Halo(ctx, B, 2 * H, 2 * W, Cout, 0)
    pack = Plan(ctx)
    descs = emit_phase_pairs(eng, pack, ctx, x, G.convT_fwd_phases(H, W, k, 1), lambda hw: G.convT_fwd_pack(Cin, Cout, k, hw), w, bias, y,
                             N=Cout, in_off=0, out_off=0)
    pack.run()
    assert descs is not None and [d.out_span for d in descs] == [2, 2]
    assert sum(-(-(d.B * d.OH * d.OW) // 256) for d in descs) >= 192
    first = 0
    for d in descs:
        d.stats_chunk0 = first
        first += d.OH * d.OW // 64 * 2
    biases = [d.bias for d in descs]
    xd = x.interior().permute(0, 3, 1, 2).double()
    ref = torch.nn.functional.conv_transpose2d(xd, w.double(), None, stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)
    _stats_case(descs, y.t, ref, ref + bias.double(), biases, bias, B, first)


# ------------------------------------------------------------------------------------------------------------------------------------
# kind 2: the fused first pass of the instance-norm backward


def _fuse(descs, y, mean, rstd, act, part, B, fcps, fo):
    """fuse_* of each descriptor: y [B][fh][fw][ch] dense, the GEMM row's pixel at (oh s + out_oh - fo, ...) of y"""
    ch = descs[0].N // max(1, descs[0].out_span)
    for d in descs:
        d.fuse_y, d.fuse_mean, d.fuse_rstd = y.data_ptr(), mean.data_ptr(), rstd.data_ptr()
        d.fuse_h, d.fuse_w, d.fuse_oh, d.fuse_ow = y.shape[1], y.shape[2], d.out_oh - fo, d.out_ow - fo
        d.fuse_act, d.fuse_slope = act, 0.2
        d.fuse_part, d.fuse_part_elems, d.fuse_chunks = part.data_ptr(), B * fcps * 2 * ch, fcps


def _fused_sums(g, y, mean, rstd, act, B, d, q, ch):
    """float64 sums of g_z and g_z z per 128-row chunk from the STORED g, z = (y - mean) rstd in fp32 as the kernel forms it"""
    nch = d.OH * d.OW // 128
    z = ((y - mean[:, None, None]) * rstd[:, None, None])
    gv = _view(g, d, d.out_oh, d.out_ow, q, ch).reshape(B, nch, 128, ch)
    zv = _view(z, d, d.fuse_oh, d.fuse_ow, q, ch).reshape(B, nch, 128, ch)
    neg = {L.ACT_NONE: 1.0, L.ACT_RELU: 0.0, L.ACT_LRELU: 0.2}[act]
    gz = torch.where(zv > 0, gv, gv * neg).double()
    p2 = gz * zv.double()
    return gz.sum(2), gz.abs().sum(2), p2.sum(2), p2.abs().sum(2)


def _check_fused(part, g, y, mean, rstd, act, descs, B, fcps, other=None):
    ch = descs[0].N // max(1, descs[0].out_span)
    rec = _records(part, B, fcps, 2, ch)
    written = torch.zeros(B, fcps, dtype=torch.bool, device=DEV)
    for d in descs:
        span = max(1, d.out_span)
        nch = d.OH * d.OW // 128
        for q in range(span):
            s1, a1, s2, a2 = _fused_sums(g, y, mean, rstd, act, B, d, q, ch)
            idx = d.fuse_chunk0 + torch.arange(nch, device=DEV) * span + q
            r = rec[:, idx].double()
            assert ((r[:, :, 0] - s1).abs() <= FUSED_BOUND * a1).all(), "sum g_z"
            assert ((r[:, :, 1] - s2).abs() <= FUSED_BOUND * a2).all(), "sum g_z z"
            if other is not None:
                # (not bitwise: the eight-wave tile sums a row over 16 lanes, the four-wave tile over 32 -- another order)
                o = _records(other, B, fcps, 2, ch)[:, idx].double()
                assert ((r[:, :, 0] - o[:, :, 0]).abs() <= FUSED_BOUND * a1).all() and ((r[:, :, 1] - o[:, :, 1]).abs() <= FUSED_BOUND * a2).all()
            written[:, idx] = True
    _untouched_keep_sentinel(part, B, fcps, 2, ch, written)


def _fused_case(descs, gbuf, y, act, B, fcps, ref, fo, chunk0=0):
    mean = y.mean((1, 2)).contiguous()
    rstd = (1.0 / torch.sqrt(y.var((1, 2), unbiased=False) + IN_EPS)).contiguous()
    ch = descs[0].N // max(1, descs[0].out_span)
    part = torch.zeros((B + 1) * fcps * 2 * ch, device=DEV)
    _fuse(descs, y, mean, rstd, act, part, B, fcps, fo)
    first = chunk0
    for d in descs:
        d.fuse_chunk0 = first
        first += d.OH * d.OW // 128 * max(1, d.out_span)
    res = {a: _run(descs, a, gbuf, part) for a in (0, R4)}
    assert torch.equal(_bits(res[0][0]), _bits(res[R4][0])), "g: four-wave tile against eight-wave tile"
    gi = res[R4][0][:, fo:gbuf.shape[1] - fo, fo:gbuf.shape[2] - fo]
    assert _err(gi, ref)[0] < 2e-6
    _check_fused(res[R4][1], res[R4][0], y, mean, rstd, act, descs, B, fcps, other=res[0][1])
    _check_fused(res[0][1], res[0][0], y, mean, rstd, act, descs, B, fcps)


FUSED_CONVS = [  # name, B, H, W, cin, cout, in_stride, act
    ("cin96_relu", 129, 16, 24, 96, 128, 1, L.ACT_RELU),          # 27 K-tiles, OH OW = 384 (items straddle samples, half-filled last)
    ("dgrad_s2_lrelu", 16, 128, 128, 128, 256, 2, L.ACT_LRELU),   # in_stride 2, run 128, N = 256: 512 items
]


@pytest.mark.parametrize("case", FUSED_CONVS, ids=[c[0] for c in FUSED_CONVS])
def test_fused_pass_kind_against_the_eight_wave_tile_and_float64(case):
    """kind 2 (fuse_y set, >= 24 K-tiles): conv_x3r_kernel<128, 2>; g written into the interior of a halo-1 buffer"""
    _, B, H, W, cin, cout, s, act = case
    gen = torch.Generator().manual_seed(54)
    ctx = Ctx(DEV)
    x = Halo(ctx, B, H, W, cin, 1)
    x.interior().copy_(torch.randn(B, H, W, cin, generator=gen).to(DEV))
    w = (torch.randn(cout, cin, 3, 3, generator=gen) * 0.05).to(DEV)
    wp, planes = _packed(ctx, w, 3)
    OH, OW = G.conv_out(H, 3, s, 1), G.conv_out(W, 3, s, 1)
    g = Halo(ctx, B, OH, OW, cout, 1)
    d = _conv_desc(ctx, x, w, wp, planes, None, g, s, out_oh=1, out_ow=1)
    y = (torch.randn(B, OH, OW, cout, generator=gen) * 1.5 + 0.3).to(DEV)
    ref = torch.nn.functional.conv2d(x.t.double().permute(0, 3, 1, 2), w.double(), None, stride=s).permute(0, 2, 3, 1)
    _fused_case([d], g.t, y, act, B, OH * OW // 128, ref, 1)


def test_fused_pass_kind_with_an_output_stride_and_chunk0():
    """kind 2 writing every second pixel of every second row (out_stride 2, out_oh = out_ow = 1: a sub-pixel phase) with y read at the
    same pixels (fuse_oh = fuse_ow = 1), no activation, fuse_chunk0 = 2 inside a workspace of chunks + 5 per sample"""
    B, H, W, cin, cout = 50, 32, 32, 96, 128
    gen = torch.Generator().manual_seed(55)
    ctx = Ctx(DEV)
    x = Halo(ctx, B, H, W, cin, 1)
    x.interior().copy_(torch.randn(B, H, W, cin, generator=gen).to(DEV))
    w = (torch.randn(cout, cin, 3, 3, generator=gen) * 0.05).to(DEV)
    wp, planes = _packed(ctx, w, 3)
    g = Halo(ctx, B, 2 * H, 2 * W, cout, 0)
    d = _conv_desc(ctx, x, w, wp, planes, None, g, 1, out_stride=2, out_oh=1, out_ow=1)
    y = (torch.randn(B, 2 * H, 2 * W, cout, generator=gen) * 1.5 + 0.3).to(DEV)
    conv = torch.nn.functional.conv2d(x.t.double().permute(0, 3, 1, 2), w.double(), None).permute(0, 2, 3, 1)
    # (the launch writes only its own pixels: the others stay NaN in both, compared as bits; float64 on the written ones)
    mean = y.mean((1, 2)).contiguous()
    rstd = (1.0 / torch.sqrt(y.var((1, 2), unbiased=False) + IN_EPS)).contiguous()
    fcps = H * W // 128 + 5
    part = torch.zeros((B + 1) * fcps * 2 * cout, device=DEV)
    _fuse([d], y, mean, rstd, L.ACT_NONE, part, B, fcps, 0)
    d.fuse_chunk0 = 2
    res = {a: _run([d], a, g.t, part) for a in (0, R4)}
    assert torch.equal(_bits(res[0][0]), _bits(res[R4][0]))
    assert _err(res[R4][0][:, 1::2, 1::2], conv)[0] < 2e-6
    assert torch.isnan(res[R4][0][:, 0::2]).all() and torch.isnan(res[R4][0][:, :, 0::2]).all()
    _check_fused(res[R4][1], res[R4][0], y, mean, rstd, L.ACT_NONE, [d], B, fcps, other=res[0][1])
    _check_fused(res[0][1], res[0][0], y, mean, rstd, L.ACT_NONE, [d], B, fcps)


def test_fused_pass_kind_on_paired_phases():
    """kind 2 on the two out_span = 2 problems of the data gradient of Conv2d(64, 384, 3, s2, p1) (emit_phase_pairs; run 384: 24 and 48
    K-tiles), ReLU: two records per 128 GEMM rows, pixel parity 0 then 1"""
    B, H, W, Ci, Co, k = 24, 64, 64, 64, 384, 3
    gen = torch.Generator().manual_seed(56)
    ctx = Ctx(DEV)
    eng = _Eng(ctx)
    dy = Halo(ctx, B, H // 2, W // 2, Co, 1)
    dy.interior().copy_(torch.randn(B, H // 2, W // 2, Co, generator=gen).to(DEV))
    w = (torch.randn(Co, Ci, k, k, generator=gen) * 0.05).to(DEV)
    dx = Halo(ctx, B, H, W, Ci, 0)
    pack = Plan(ctx)
    descs = emit_phase_pairs(eng, pack, ctx, dy, G.conv_dgrad_s2_phases(H, W, k, 1), lambda hw: G.conv_dgrad_pack(Co, Ci, k, hw), w, None, dx,
                             N=Ci, in_off=0, out_off=0)
    pack.run()
    assert descs is not None and [d.out_span for d in descs] == [2, 2]
    assert min(d.ntaps * d.run // 32 for d in descs) >= 24
    assert sum(-(-(d.B * d.OH * d.OW) // 256) for d in descs) >= 192
    y = (torch.randn(B, H, W, Ci, generator=gen) * 1.5 + 0.3).to(DEV)
    ref = torch.nn.grad.conv2d_input((B, Ci, H, W), w.double(), dy.interior().permute(0, 3, 1, 2).double(), stride=2, padding=1).permute(0, 2, 3, 1)
    _fused_case(descs, dx.t, y, L.ACT_RELU, B, H * W // 128, ref, 0)


@pytest.mark.parametrize("run,name", [(736, b"conv_x3_kernel<128>"), (768, b"conv_x3r_kernel<128>")])
def test_fused_pass_takes_the_four_wave_tile_from_24_k_tiles(run, name):
    """1 x 1 with run 736 (23 K-tiles): the eight-wave tile even when the four-wave tile is asked for; run 768 (24): the four-wave
    tile.  g bitwise that of algo 0 in both"""
    B, H, W, cout = 12, 64, 64, 128
    gen = torch.Generator().manual_seed(57)
    ctx = Ctx(DEV)
    x = Halo(ctx, B, H, W, run, 0)
    x.t.copy_(torch.randn(B, H, W, run, generator=gen).to(DEV))
    w = (torch.randn(cout, run, 1, 1, generator=gen) * 0.05).to(DEV)
    wp, planes = _packed(ctx, w, 1)
    g = Halo(ctx, B, H, W, cout, 0)
    d = _conv_desc(ctx, x, w, wp, planes, None, g, 1)
    y = (torch.randn(B, H, W, cout, generator=gen) * 1.5 + 0.3).to(DEV)
    ref = torch.einsum("bhwc,nc->bhwn", x.t.double(), w.double()[:, :, 0, 0])
    d.algo = R4
    assert _name(d) == b"conv_x3r_kernel<128>", "without fuse_y the four-wave tile takes three K-tiles on"
    mean = y.mean((1, 2)).contiguous()
    rstd = (1.0 / torch.sqrt(y.var((1, 2), unbiased=False) + IN_EPS)).contiguous()
    fcps = H * W // 128
    part = torch.zeros((B + 1) * fcps * 2 * cout, device=DEV)
    _fuse([d], y, mean, rstd, L.ACT_LRELU, part, B, fcps, 0)
    d.algo = R4
    assert _name(d) == name
    res = {a: _run([d], a, g.t, part, name=False) for a in (0, R4)}
    assert torch.equal(_bits(res[0][0]), _bits(res[R4][0]))
    assert _err(res[R4][0], ref)[0] < 2e-6
    _check_fused(res[R4][1], res[R4][0], y, mean, rstd, L.ACT_LRELU, [d], B, fcps, other=res[0][1])


# ------------------------------------------------------------------------------------------------------------------------------------
# outputs of 3 and 4.5 GiB: N = 128 channels written into a 1024-channel buffer (little compute, a wide extent)

BIG = [(kind, B) for kind in (0, 1, 2) for B in (12, 17)]          # 256^2 x 1024 floats: 12 -> 3.2 GiB, 17 -> 4.6 GiB


@pytest.mark.parametrize("kind,B", BIG, ids=[f"kind{k}_{'3' if b == 12 else '4.5'}GiB" for k, b in BIG])
def test_outputs_of_3_and_4_5_gib(kind, B):
    """3 x 3, cin 96 (27 K-tiles), N = 128, out_cs = 1024 at 256 x 256.  The four-wave tile's full-tile stores use 32-bit byte offsets
    from the output base: at 3 GiB the launch runs on it (offsets 2^31 .. 2^32 are unsigned), at 4.5 GiB on the eight-wave tile
    (conv_x3r_ok).  Either way bitwise the eight-wave tile's output, channels 128 .. 1023 untouched, float64 on sampled rows -- among
    them the rows whose byte offset first reaches 2^31 and 2^32."""
    H = W = 256
    cin, cout, CS = 96, 128, 1024
    gen = torch.Generator(device=DEV).manual_seed(58)
    ctx = Ctx(DEV)
    x = Halo(ctx, B, H, W, cin, 1)
    x.interior().copy_(torch.randn(B, H, W, cin, generator=gen, device=DEV))
    w = torch.randn(cout, cin, 3, 3, generator=gen, device=DEV) * 0.05
    bias = torch.randn(cout, generator=gen, device=DEV) if kind == 0 else None
    wp, planes = _packed(ctx, w, 3)
    out = Halo(ctx, B, H, W, CS, 0)
    M = B * H * W
    assert out.t.numel() * 4 >= (3 << 30) and (out.t.numel() * 4 >= (1 << 32)) == (B == 17)
    d = _conv_desc(ctx, x, w, wp, planes, bias, out, 1)
    ws = torch.zeros(1, device=DEV)
    cps = H * W // (64 if kind == 1 else 128)
    y = mean = rstd = None
    if kind == 1:
        ws = torch.zeros((B + 1) * cps * 4 * cout, device=DEV)
        d.stats_ws, d.stats_ws_elems, d.stats_chunks = ws.data_ptr(), B * cps * 4 * cout, cps
    elif kind == 2:
        y = torch.randn(B, H, W, cout, generator=gen, device=DEV) * 1.5 + 0.3
        mean = y.mean((1, 2)).contiguous()
        rstd = (1.0 / torch.sqrt(y.var((1, 2), unbiased=False) + IN_EPS)).contiguous()
        ws = torch.zeros((B + 1) * cps * 2 * cout, device=DEV)
        _fuse([d], y, mean, rstd, L.ACT_RELU, ws, B, cps, 0)
    got, recs = {}, {}
    for algo in (0, R4):
        d.algo = algo
        for rep in range(2):
            _sentinel(out.t)
            _sentinel(ws)
            _launch([d])
            torch.cuda.synchronize()
            if rep == 0 and algo == 0:
                got[0], recs[0] = out.t[..., :cout].clone(), ws.clone()
            else:
                for b in range(B):
                    assert torch.equal(_bits(out.t[b, ..., :cout]), _bits(got[0][b])), f"sample {b} differs from the eight-wave tile's output"
                if kind == 1 and algo == 0:
                    assert torch.equal(_bits(ws), _bits(recs[0])), "a launch differs from the first one"
                elif kind == 1:
                    _same_records(recs[0], ws, B, cps, cout, "records: four-wave tile against eight-wave tile")
        recs[algo] = ws.clone()
        for b in range(B):
            assert (out.t[b, ..., cout:].view(torch.int32) == SENT).all(), f"channels {cout} .. {CS - 1} of sample {b} were written"
    # float64 on ~2 K sampled rows, the rows at byte offsets 2^31 and 2^32 (and their neighbours) among them
    row_bytes = CS * 4
    special = [0, M - 1] + [m for c in (1 << 31, 1 << 32) for m in (c // row_bytes - 1, c // row_bytes) if m < M]
    rows = torch.cat([torch.tensor(special), torch.randint(0, M, (2000,), generator=torch.Generator().manual_seed(59))]).to(DEV)
    b_, r_ = rows // (H * W), rows % (H * W)
    oh, ow = r_ // W, r_ % W
    dd = torch.arange(3, device=DEV)
    patch = x.t[b_[:, None, None], (oh[:, None] + dd)[:, :, None], (ow[:, None] + dd)[:, None, :]]          # [R][3][3][cin]
    ref = torch.einsum("rhwc,nchw->rn", patch.double(), w.double())
    if bias is not None:
        ref = ref + bias.double()
    assert _err(got[0][b_, oh, ow], ref)[0] < 2e-6
    if kind == 1:
        # the records of the samples that hold the rows at 2^31 and 2^32 bytes (and the first / last) against float64
        for b in sorted({0, B - 1} | {m // (H * W) for m in special}):
            yb = got[0][b:b + 1].reshape(1, cps, 64, cout)
            r = _records(recs[R4], B, cps, 4, cout)[b:b + 1]
            k = yb[:, :, 0]
            assert torch.equal(_bits(r[:, :, 0]), _bits(k)) and (r[:, :, 3] == 64.0).all()
            t = yb.double() - k.double()[:, :, None]
            assert ((r[:, :, 1].double() - t.sum(2)).abs() <= STATS_BOUND * t.abs().sum(2)).all()
            assert ((r[:, :, 2].double() - t.pow(2).sum(2)).abs() <= STATS_BOUND * t.pow(2).sum(2)).all()
        assert (_bits(recs[R4][B * cps * 4 * cout:]) == SENT).all()
    if kind == 2:
        for b in sorted({0, B - 1} | {m // (H * W) for m in special}):
            s1, a1, s2, a2 = _fused_sums(got[0][b:b + 1], y[b:b + 1], mean[b:b + 1], rstd[b:b + 1], L.ACT_RELU, 1, d, 0, cout)
            for algo in (0, R4):
                rec = _records(recs[algo], B, cps, 2, cout)[b:b + 1]
                assert ((rec[:, :, 0].double() - s1).abs() <= FUSED_BOUND * a1).all()
                assert ((rec[:, :, 1].double() - s2).abs() <= FUSED_BOUND * a2).all()
        for algo in (0, R4):
            assert (_bits(recs[algo][B * cps * 2 * cout:]) == SENT).all()
    d.algo = R4
    assert _name(d) == (b"conv_x3r_kernel<128>" if B == 12 else b"conv_x3_kernel<128>")
