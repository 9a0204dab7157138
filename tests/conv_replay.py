"""Shared by the convolution replay tests: a float64 restatement of one nirgan_conv_desc with its two optional epilogue outputs, copies of
descriptors pointed at fresh buffers, and the census of the convolution launches in the engines' plans.  Test infrastructure: plain torch
and ctypes, it neither calls the emulator nor needs the library.

    out[b][oh * out_stride + out_oh][ow * out_stride + out_ow][n] (+ bias[n]) = sum over taps t and c < run of
        in[b][oh * in_stride + in_oh + tap_dh[t]][ow * in_stride + in_ow + tap_dw[t]] (float c) * w[n][t * run + c]

(include/nirgan_hip.h, nirgan_conv_desc).  The `run` floats of a tap are contiguous from the pixel's first channel on and may run into the
next pixel's channels.  out_span = 2: N = 2 C columns, column n is channel n % C of the pixel n / C to the right -- with out_cs == C
(dense pixels, out_stride >= 2) as with out_cs == N (the caller's pixel pairs) that is element n from the row's first pixel on."""
import ctypes as C

import torch

from wgrad_replay import GUARD, PRODUCTS, SENTINEL_BITS, FreshWgrad, copy_desc, operand_terms

SENTINEL_BF16 = 0x7FDE       # the sentinel's bf16 analogue: a quiet NaN with a payload no kernel computes
PRODUCTS_PER_FP32 = {0: 1, 1: 1, 2: 3, 3: 6}     # bf16 products summed in fp32 per product of the modelled precision
# csrc/igemm_conv.hip: CONV_KERNEL_NAMES, and the register-fed tile's epilogue forms (X3Kernel)
CONV_KERNEL_NAMES = ("conv_x3r_kernel<128>", "conv_x3_kernel<128>", "conv_x3_kernel<64>", "conv_igemm256_kernel", "conv_igemm_kernel<128>",
                     "conv_igemm_kernel<64>")
X3R, X3R_FORMS = CONV_KERNEL_NAMES[0], {"plain": "X3R_PLAIN", "stats": "X3R_STATS", "fused": "X3R_GENERIC"}
X3_ROUTES = CONV_KERNEL_NAMES[:3]


# ------------------------------------------------------------------------------------------------------------ the descriptor's fields
def span_of(d) -> int:
    return d.out_span if d.out_span > 1 else 1


def channels_of(d) -> int:
    """channels per output pixel: N, or N / 2 with out_span = 2"""
    return d.N // span_of(d)


def conv_x3_ok(d) -> bool:
    """the split tile's coverage (csrc/igemm_x3.h::conv_x3_ok, tests/emu_backend.py): anything else of precision 3 runs as exact fp32"""
    K = d.ntaps * d.run
    return bool(d.precision == 3 and d.w_x3 and d.run % 32 == 0 and d.N % 64 == 0 and d.ksplit <= 1
                and not (d.in_bf16 or d.w_bf16 or d.out_bf16 or d.fuse_y_bf16)
                and (d.out_cs | (d.out_oh * d.out_wp * d.out_cs + d.out_ow * d.out_cs) | (d.out_wp * d.out_cs) | (d.out_hp * d.out_wp * d.out_cs)) % 4 == 0
                and d.in_elems * 4 < 2 ** 32 and d.w_elems * 4 < 2 ** 32 and d.N * K * 2 < 2 ** 32)


def modelled_precision(d) -> int:
    """the operand treatment a launch of d applies: its precision, or 0 for a precision-3 descriptor the split tile does not cover"""
    return 0 if d.precision == 3 and not conv_x3_ok(d) else d.precision


def epilogue_form(d) -> str:
    return "fused" if d.fuse_y else ("stats" if d.stats_ws else "plain")


def geometry(d) -> tuple:
    """the descriptor without its addresses (which pointers are set is part of it): launches of equal geometry do the same work"""
    return tuple((n, bool(getattr(d, n)) if t is C.c_void_p else (tuple(getattr(d, n)) if n.startswith("tap_") else getattr(d, n)))
                 for n, t in type(d)._fields_)


def group_route(ds, names, cus: int) -> str:
    """the kernel a launch of the 1..4 problems ds through nirgan_conv_igemm_group runs on (csrc/igemm_conv.hip::conv_route with group =
    true), from the kernel each problem takes alone (`names`, nirgan_conv_kernel_name) and the device's CU count: the split tile where it
    covers every problem of one tile width -- 128 columns when the problems together have 256 x 128 tiles for three quarters of the CUs,
    register-fed when every problem qualifies at that width --, else the 128-row tile of the group's width; never the 256-wide tile."""
    if all(n.startswith("conv_x3") for n in names) and len({d.N % 128 == 0 for d in ds}) == 1:
        tiles = sum(-(-(d.B * d.OH * d.OW) // 256) * (d.N // 128) for d in ds)
        bn = 128 if ds[0].N % 128 == 0 and tiles * 4 >= 3 * cus else 64
        reg_fed = all(bn == 128 and d.algo == 4 and d.OW >= 16 and d.ntaps * (d.run // 32) >= (24 if d.fuse_y else 3)
                      and d.out_elems * 4 <= 2 ** 32 and d.B * d.OH * d.OW < 2 ** 24 for d in ds)
        return X3R if reg_fed else f"conv_x3_kernel<{bn}>"
    return f"conv_igemm_kernel<{128 if ds[0].N > 64 else 64}>"


def launch_form(ds) -> str:
    """the epilogue form of a launch (the register-fed tile's KIND: fused if any problem runs the fused pass, else stats if any leaves them)"""
    forms = {epilogue_form(d) for d in ds}
    return "fused" if "fused" in forms else ("stats" if "stats" in forms else "plain")


# ------------------------------------------------------------------------------------------------------------ restatement
def out_offsets(d, device) -> torch.Tensor:
    """[B][OH * OW][N] flat element offsets into `out` of the values a launch writes, out_span included"""
    dev = device
    b = torch.arange(d.B, dtype=torch.int64, device=dev)[:, None, None, None]
    oh = torch.arange(d.OH, dtype=torch.int64, device=dev)[None, :, None, None]
    ow = torch.arange(d.OW, dtype=torch.int64, device=dev)[None, None, :, None]
    n = torch.arange(d.N, dtype=torch.int64, device=dev)[None, None, None, :]
    ch = channels_of(d)
    row = d.out_wp * d.out_cs
    if span_of(d) == 2 and d.out_cs != d.N:
        assert d.out_cs == ch and d.out_stride >= 2, "out_span = 2 needs out_cs == N / 2 with out_stride >= 2, or out_cs == N"
    # column n = channel n % ch of the pixel n / ch to the right of the row's first
    off = (b * (d.out_hp * row) + (oh * d.out_stride + d.out_oh) * row + (ow * d.out_stride + d.out_ow) * d.out_cs
           + (n // ch) * (d.out_cs if d.out_cs != d.N else ch) + n % ch)
    return off.reshape(d.B, d.OH * d.OW, d.N)


def in_columns(d, device) -> torch.Tensor:
    """offset of GEMM column t * run + c from a pixel's input origin"""
    col = [(d.tap_dh[t] * d.in_wp + d.tap_dw[t]) * d.in_cs + c for t in range(d.ntaps) for c in range(d.run)]
    return torch.tensor(col, dtype=torch.int64, device=device)


def restate_conv(d, inp: torch.Tensor, w: torch.Tensor, bias, precision: int, kinds=("value", "abs"), chunk_elems: int = 1 << 23):
    """(offsets, [one float64 tensor per kind]) of descriptor d over the flat operand tensors inp and w (float32, or bfloat16 where the
    descriptor reads bf16) and bias ([N] or None), all [B][OH * OW][N].  precision: the operand treatment to model (modelled_precision).
    kinds: "value" = the header's equation, "acc" = the same without the bias (what the epilogue's sums are taken from), "abs" = |in| . |w|
    of the modelled terms (+ |bias|), the scale of the rounding bound, "acc_abs" = that scale without the bias.  Runs on inp's device,
    sample by sample in chunks of pixels."""
    dev = inp.device
    K, ohw = d.ntaps * d.run, d.OH * d.OW
    cols = in_columns(d, dev)
    wt = [t.T.contiguous() for t in operand_terms(w[:d.N * K].reshape(d.N, K), precision)]
    wa = [t.abs() for t in wt]
    need = {"acc": any(k in ("value", "acc") for k in kinds), "acc_abs": any(k in ("abs", "acc_abs") for k in kinds)}
    sums = {k: torch.zeros(d.B, ohw, d.N, dtype=torch.float64, device=dev) for k, v in need.items() if v}
    m = torch.arange(ohw, dtype=torch.int64, device=dev)
    base = (m // d.OW * d.in_stride + d.in_oh) * (d.in_wp * d.in_cs) + (m % d.OW * d.in_stride + d.in_ow) * d.in_cs
    step = max(64, chunk_elems // (K + d.N))
    for b in range(d.B):
        for m0 in range(0, ohw, step):
            sl = slice(m0, min(m0 + step, ohw))
            at = operand_terms(inp[b * d.in_hp * d.in_wp * d.in_cs + base[sl, None] + cols[None, :]], precision)
            for x, y in PRODUCTS[precision]:
                if need["acc"]:
                    sums["acc"][b, sl] += at[x] @ wt[y]
                if need["acc_abs"]:
                    sums["acc_abs"][b, sl] += at[x].abs() @ wa[y]
    bv = None if bias is None else bias[:d.N].double()
    outs = []
    for kind in kinds:
        if kind in ("acc", "acc_abs"):
            outs.append(sums[kind])
        elif kind == "value":
            outs.append(sums["acc"] if bv is None else sums["acc"] + bv)
        else:
            outs.append(sums["acc_abs"] if bv is None else sums["acc_abs"] + bv.abs())
    return out_offsets(d, dev), outs


def _chunks(d, x: torch.Tensor, rows: int) -> torch.Tensor:
    """[B][OH * OW][N] -> [B][records][rows][ch]: `rows` GEMM rows per record, with out_span = 2 one record per pixel of the row (the
    first pixel's first)"""
    span, ch = span_of(d), channels_of(d)
    return x.reshape(d.B, -1, rows, span, ch).transpose(2, 3).reshape(d.B, -1, rows, ch)


def restate_stats(d, acc: torch.Tensor) -> torch.Tensor:
    """The instance-norm partial sums of the launch, [B][OH * OW / 64 * span][4][ch] float64: per 64 GEMM rows the shift k (the chunk's first
    row), sum (v - k), sum (v - k)^2 and the count 64, from the values WITHOUT the bias (`acc`).  They belong to the records
    stats_ws[b][stats_chunk0 + chunk]."""
    rows = _chunks(d, acc, 64)
    k = rows[:, :, 0]
    dv = rows - k[:, :, None]
    return torch.stack([k, dv.sum(2), (dv * dv).sum(2), torch.full_like(k, 64.0)], dim=2)


def fuse_index(d, device) -> torch.Tensor:
    """[B][OH][OW][N] flat element offsets into fuse_y of the y the fused pass reads next to every output element: y pixel
    (oh * out_stride + fuse_oh, ow * out_stride + fuse_ow + n / ch), channel n % ch"""
    ch = channels_of(d)
    b = torch.arange(d.B, dtype=torch.int64, device=device)[:, None, None, None]
    oh = torch.arange(d.OH, dtype=torch.int64, device=device)[None, :, None, None]
    ow = torch.arange(d.OW, dtype=torch.int64, device=device)[None, None, :, None]
    n = torch.arange(d.N, dtype=torch.int64, device=device)[None, None, None, :]
    return ((b * d.fuse_h + oh * d.out_stride + d.fuse_oh) * d.fuse_w + ow * d.out_stride + d.fuse_ow + n // ch) * ch + n % ch


def fuse_z(d, y: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor):
    """[B][OH * OW][N] float64: z = (y - mean) * rstd of the fused pass at every output element, and (|y| + |mean|) rstd there (the scale
    of z's rounding)"""
    ch, span = channels_of(d), span_of(d)
    yv = y[fuse_index(d, y.device)].double().reshape(d.B, -1, d.N)
    mv = mean.double().reshape(d.B, 1, ch).repeat(1, 1, span)
    rv = rstd.double().reshape(d.B, 1, ch).repeat(1, 1, span)
    return (yv - mv) * rv, (yv.abs() + mv.abs()) * rv.abs()


def act_factor(d, z: torch.Tensor) -> torch.Tensor:
    """act'(z) of the fused pass: 1 for z > 0, else 0 (ReLU), the slope as the fp32 value the descriptor holds (LeakyReLU) or 1 (none)"""
    neg = 0.0 if d.fuse_act == 1 else (float(d.fuse_slope) if d.fuse_act == 2 else 1.0)
    return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, neg))


def restate_fuse(d, g: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """The fused instance-norm-backward sums, [B][OH * OW / 128 * span][2][ch] float64: per 128 GEMM rows sum g_z and sum g_z * z with
    g_z = g * act'(z), g the launch's output as fp32.  They belong to the records fuse_part[b][fuse_chunk0 + tile]."""
    gz = g * act_factor(d, z)
    return torch.stack([_chunks(d, gz, 128).sum(2), _chunks(d, gz * z, 128).sum(2)], dim=2)


def record_offsets(d, which: str, device) -> torch.Tensor:
    """flat element offsets into stats_ws ([b][chunk0 + chunk][4][ch]) or fuse_part ([b][chunk0 + tile][2][ch]) of the records the launch
    writes, shaped like restate_stats / restate_fuse"""
    ch, span = channels_of(d), span_of(d)
    vals, rows, chunk0, per = (4, 64, d.stats_chunk0, d.stats_chunks) if which == "stats" else (2, 128, d.fuse_chunk0, d.fuse_chunks)
    count = d.OH * d.OW // rows * span
    b = torch.arange(d.B, dtype=torch.int64, device=device)[:, None, None, None]
    c = torch.arange(count, dtype=torch.int64, device=device)[None, :, None, None]
    v = torch.arange(vals, dtype=torch.int64, device=device)[None, None, :, None]
    n = torch.arange(ch, dtype=torch.int64, device=device)[None, None, None, :]
    return ((b * per + chunk0 + c) * vals + v) * ch + n


# ------------------------------------------------------------------------------------------------------------ fresh buffers
def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """one unit in the last place of the bf16 format at |x| (float64)"""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


def split3(w: torch.Tensor):
    """w = h + m + l as three bfloat16 tensors, each the nearest-even bf16 of what the previous ones left (what nirgan_split3 writes)"""
    h = w.float().to(torch.bfloat16)
    m = (w.float() - h.float()).to(torch.bfloat16)
    l = (w.float() - h.float() - m.float()).to(torch.bfloat16)
    return h, m, l


class FreshConv:
    """A byte copy of a convolution descriptor over buffers of its own, of the sizes the descriptor declares; nothing of the original's
    memory is referenced.  `share`: original address -> tensor, filled as buffers are made -- the members of a group handed one dict share
    what the originals share (the output, the statistics and fused-sum workspaces, the input).  Fails on a pointer field it does not
    know, so that a new field cannot keep pointing at freed memory."""

    def __init__(self, d, device, share=None):
        self.orig, self.d, self.device = d, copy_desc(d), device
        share = {} if share is None else share
        ch = channels_of(d)
        bf, f32 = torch.bfloat16, torch.float32
        spec = {   # field -> (elements, dtype, elements past them that a launch must leave alone)
            "inp": (d.in_elems, bf if d.in_bf16 else f32, 0), "w": (d.w_elems, bf if d.w_bf16 else f32, 0), "bias": (d.N, f32, 0),
            "out": (d.out_elems, bf if d.out_bf16 else f32, GUARD), "zero_page": (64, f32, 0), "split_ws": (d.split_ws_elems, f32, 0),
            "stats_ws": (d.stats_ws_elems, f32, GUARD), "fuse_y": (d.B * d.fuse_h * d.fuse_w * ch, bf if d.fuse_y_bf16 else f32, 0),
            "fuse_mean": (d.B * ch, f32, 0), "fuse_rstd": (d.B * ch, f32, 0), "fuse_part": (d.fuse_part_elems, f32, GUARD),
            "w_x3": (3 * d.w_x3_plane, bf, 0),
        }
        self.t = {}
        for name, typ in type(d)._fields_:
            if typ is not C.c_void_p:
                continue
            addr = getattr(d, name)
            if not addr:
                continue
            assert name in spec, f"FreshConv: unknown pointer field {name}"
            n, dtype, guard = spec[name]
            if addr not in share:
                share[addr] = torch.zeros(max(int(n), 1) + guard, dtype=dtype, device=device)
            t = share[addr]
            assert t.dtype == dtype and (t.numel() >= max(int(n), 1) if not guard else t.numel() == max(int(n), 1) + guard), \
                f"FreshConv: {name} shares an address with a buffer of another size or type"
            self.t[name] = t
            setattr(self.d, name, t.data_ptr())
        assert {"inp", "w", "out", "zero_page"} <= set(self.t), "a convolution descriptor needs in, w, out and zero_page"
        self.inp, self.w, self.out, self.bias = self.t["inp"], self.t["w"], self.t["out"], self.t.get("bias")

    def sync_x3(self):
        """the three planes of w_x3, w_x3_plane apart, as the three-term split of the current w (built here, not by nirgan_split3)"""
        if "w_x3" in self.t:
            nk, plane = self.d.N * self.d.ntaps * self.d.run, self.d.w_x3_plane
            for i, term in enumerate(split3(self.w[:nk])):
                self.t["w_x3"][i * plane:i * plane + nk] = term

    def guarded(self):
        """(tensor, its sentinel as an integer view) of every buffer a launch writes and the replay watches"""
        out = []
        for name in ("out", "stats_ws", "fuse_part"):
            t = self.t.get(name)
            if t is not None:
                out.append((name, t.view(torch.int16), SENTINEL_BF16) if t.dtype == torch.bfloat16 else (name, t.view(torch.int32), SENTINEL_BITS))
        return out

    def arm(self):
        """out with its guard, stats_ws and fuse_part to the sentinel"""
        for _, bits, sentinel in self.guarded():
            bits.fill_(sentinel)


    def untouched(self, offsets: torch.Tensor) -> bool:
        """every element of out and its guard outside `offsets` (what restate_conv returned), and every record of stats_ws / fuse_part
        outside [chunk0, chunk0 + count), still holds the sentinel"""
        return not untouched([self], written_sets([self], [offsets]))


def written_sets(members, refs) -> dict:
    """{buffer name: flat offsets} a launch of `members` (a list of FreshConv sharing their outputs) writes: the union of the members'
    sets, which must be disjoint.  refs[i]: the offsets restate_conv returned for member i."""
    sets = {"out": [r.reshape(-1) for r in refs]}
    for f in members:
        if f.d.stats_ws:
            sets.setdefault("stats_ws", []).append(record_offsets(f.d, "stats", f.device).reshape(-1))
        if f.d.fuse_y:
            sets.setdefault("fuse_part", []).append(record_offsets(f.d, "fuse", f.device).reshape(-1))
    out = {}
    for name, parts in sets.items():
        assert len({f.t[name].data_ptr() for f in members if name in f.t}) == 1, f"the members of a group write different {name} buffers"
        allo = torch.cat(parts)
        assert torch.unique(allo).numel() == allo.numel(), f"the members' written sets of {name} overlap"
        out[name] = allo
    return out


def untouched(members, written: dict) -> list:
    """names of the watched buffers in which an element outside the written set no longer holds the sentinel: halo pixels, channels from N
    up to out_cs, the pixels between strided outputs, the guard; the statistics' and fused sums' records outside [chunk0, chunk0 + count)"""
    bad, done = [], set()
    for f in members:
        for name, bits, sentinel in f.guarded():
            if bits.data_ptr() in done:
                continue
            done.add(bits.data_ptr())
            keep = torch.ones(bits.numel(), dtype=torch.bool, device=bits.device)
            if name in written:
                keep[written[name]] = False
            if not bool((bits[keep] == sentinel).all()):
                bad.append(name)
    return bad


# ------------------------------------------------------------------------------------------------------------ rounding bounds
U = 2.0 ** -24               # unit roundoff of fp32
Z_MARGIN = 2.0 ** -16        # random pass: |z| of the fused pass stays above Z_MARGIN * (|y| + |mean|) * rstd, 2^8 times z's fp32 rounding


def stats_bound(d, acc: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """Bound on |record - restate_stats(d, acc)| of a launch whose fp32 values lie within e of acc (both [B][OH * OW][N]): the shift k carries
    its element's e_k; a difference v - k formed in fp32 is off by e_v + e_k plus its own rounding (the first row's is 0 on both sides);
    the two sums add 64 such terms in fp32, in any order: (64 - 1 roundings <) 64 u times the sum of their magnitudes, the square one
    rounding more."""
    rows, er = _chunks(d, acc, 64), _chunks(d, e, 64)
    k, ek = rows[:, :, :1], er[:, :, :1]
    dv = (rows - k).abs()
    de = er + ek + U * (dv + er + ek)
    de[:, :, 0] = 0.0
    b1 = de.sum(2) + 64 * U * (dv + de).sum(2)
    b2 = (2 * dv * de + de * de).sum(2) + 65 * U * ((dv + de) ** 2).sum(2)
    return torch.stack([ek[:, :, 0], b1, b2, torch.zeros_like(b1)], dim=2)


def fuse_bound(d, g: torch.Tensor, z: torch.Tensor, zscale: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """Bound on |record - restate_fuse(d, g, z)| of a launch whose fp32 output lies within e of g and whose z is formed in fp32 from y, mean
    and rstd (a difference and a product, or a product and a fused multiply-add: at most 3 u (|y| + |mean|) rstd = 3 u zscale off), with
    act'(z) the same on both sides (|z| is kept above Z_MARGIN zscale): g_z = g act' rounds once more, g_z z once more, and each sum
    adds 128 terms in fp32 in any order."""
    f = act_factor(d, z)
    ez = 3 * U * zscale
    gz = (g * f).abs()
    egz = e * f + U * (gz + e * f)
    t = gz * z.abs()
    et = egz * z.abs() + gz * ez + egz * ez
    et = et + U * (t + et)
    ba = _chunks(d, egz, 128).sum(2) + 128 * U * _chunks(d, gz + egz, 128).sum(2)
    bb = _chunks(d, et, 128).sum(2) + 128 * U * _chunks(d, t + et, 128).sum(2)
    return torch.stack([ba, bb], dim=2)


# ------------------------------------------------------------------------------------------------------------ one launch over fresh buffers
INTEGERS = (-2.0, -1.0, 1.0, 2.0)


def _fill(t: torch.Tensor, integers: bool, g: torch.Generator):
    if integers:
        v = torch.tensor(INTEGERS, device=t.device)[torch.randint(0, 4, (t.numel(),), generator=g, device=t.device)]
    else:
        v = torch.randn(t.numel(), generator=g, device=t.device)
    t.copy_(v.to(t.dtype))


class Replay:
    """One launch (Launch) over fresh buffers: the members of a group share what the originals share, the weight-gradient half of a pair
    reads and writes scratch of its own (FreshWgrad; the data gradient reads the same dY where the originals do)."""

    def __init__(self, launch, device):
        self.launch, self.device = launch, device
        share = {}
        self.fw = None
        if launch.w is not None:
            c, w = launch.ds[0], launch.w
            same = w.p == c.inp
            self.fw = FreshWgrad(w, device, p_elems_min=c.in_elems if same else 0)
            if same:
                assert bool(w.pq_bf16) == bool(c.in_bf16)
                share[c.inp] = self.fw.p
        self.members = [FreshConv(d, device, share) for d in launch.ds]
        assert len({f.out.data_ptr() for f in self.members}) == 1, "the members of a group write one output"
        self.refs = None

    def _unique(self, name):
        seen, out = set(), []
        for f in self.members:
            t = f.t.get(name)
            if t is not None and t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                out.append(t)
        return out

    def fill(self, integers: bool, g: torch.Generator):
        """every element of in, w and bias (halos and the channels beyond `run` included) from INTEGERS, or N(0, 1) (bf16 values where the
        buffer holds bf16); the fused pass's y, mean and rstd: integers with mean 0 and rstd 1 (z is then exact and never 0), or y ~ N(0, 1),
        mean ~ N(0, 1/4), rstd in [1/2, 2) with every |z| the launch reads above Z_MARGIN (|y| + |mean|) rstd -- a y that is not is moved
        by 1/2"""
        for name in ("inp", "w", "bias"):
            for t in self._unique(name):
                _fill(t, integers, g)
        if self.fw is not None:
            _fill(self.fw.q, integers, g)
            if self.fw.p.data_ptr() != self.members[0].inp.data_ptr():
                _fill(self.fw.p, integers, g)
        for f in self.members:
            f.sync_x3()
        for t in self._unique("fuse_y"):
            _fill(t, integers, g)
        for t in self._unique("fuse_mean"):
            t.zero_() if integers else t.copy_(0.5 * torch.randn(t.numel(), generator=g, device=t.device))
        for t in self._unique("fuse_rstd"):
            t.fill_(1.0) if integers else t.copy_(0.5 + 1.5 * torch.rand(t.numel(), generator=g, device=t.device))
        if not integers:
            for f in self.members:
                if f.d.fuse_y:
                    self._keep_z_off_zero(f)
        self.refs = None

    def _keep_z_off_zero(self, f):
        d = f.d
        idx = fuse_index(d, self.device).reshape(-1)
        y = f.t["fuse_y"]
        z, zs = fuse_z(d, y, f.t["fuse_mean"], f.t["fuse_rstd"])
        close = (z.abs() <= Z_MARGIN * zs).reshape(-1)
        y[idx[close]] = (y[idx[close]].float() + 0.5).to(y.dtype)
        z, zs = fuse_z(d, y, f.t["fuse_mean"], f.t["fuse_rstd"])
        assert bool((z.abs() > Z_MARGIN * zs).all()), "fuse_y: a z within the margin of 0 is left"

    def arm(self):
        for f in self.members:
            f.arm()
        if self.fw is not None:
            self.fw.arm()

    def reference(self):
        """per member the restatement of its output and what the bounds need; the written sets (disjoint between members)"""
        if self.refs is None:
            refs = []
            for f in self.members:
                d = f.d
                prec = modelled_precision(d)
                off, (value, acc) = restate_conv(d, f.inp, f.w, f.bias, prec, kinds=("value", "acc"))
                refs.append(dict(off=off, value=value, acc=acc, prec=prec))
            self.written = written_sets(self.members, [r["off"] for r in refs])
            self.refs = refs
        return self.refs

    def _scales(self, f, r):
        """the scales of the rounding bounds, computed when a bound is first asked for (the bitwise pass mostly does without)"""
        if "scale" not in r:
            _, (r["scale"], r["acc_scale"]) = restate_conv(f.d, f.inp, f.w, f.bias, r["prec"], kinds=("abs", "acc_abs"))
        return r

    def snapshot(self):
        """the bits of every watched buffer (for the comparison of two launches)"""
        return [bits.clone() for f in self.members for _, bits, _ in f.guarded()]

    def verify(self, exact: bool, elem_bound, tag: str) -> dict:
        """The buffers after a launch against the restatement.  exact (the integer pass): `out` bitwise (a bf16 output: the nearest-even
        bf16 of the restatement); the statistics' and the fused sums' records bitwise where every intermediate is an integer below 2^24
        -- the sums of |v - k|, (v - k)^2, |g_z| and |g_z z| of the record are, and no LeakyReLU slope enters --, elsewhere within the
        bounds below.  Otherwise every element within elem_bound(d, ref) (+ one bf16 ulp of |ref| for a bf16 output), the records within
        stats_bound / fuse_bound of it.  Everything outside the written sets still holds the sentinel.  Returns the worst fractions."""
        worst = {"out": 0.0, "stats": 0.0, "fused": 0.0}
        refs = self.reference()
        for f, r in zip(self.members, refs):
            d = f.d
            got = f.out[r["off"]]
            never = int(torch.isnan(got.float()).sum())
            if exact:
                want = r["value"].float().to(got.dtype)
                bad = (got != want) | torch.isnan(got.float())
                assert not bool(bad.any()), (f"integer pass: {int(bad.sum())} of {bad.numel()} output elements differ, {never} never written, "
                                             f"first at [b, m, n] = {bad.nonzero()[0].tolist()}; {tag}")
            else:
                self._scales(f, r)
                e = elem_bound(d, r["value"], r["scale"]) + (bf16_ulp(r["value"]) if d.out_bf16 else 0.0)
                err = (got.double() - r["value"]).abs()
                ok = err <= e                                  # (a NaN -- an element never written -- fails the comparison)
                frac = (err / e.clamp_min(1e-300))
                assert bool(ok.all()), (f"output: {int((~ok).sum())} of {ok.numel()} elements outside the bound ({never} never written), worst "
                                        f"{frac.nan_to_num(float('inf')).max().item():.3g} x, first at [b, m, n] = {(~ok).nonzero()[0].tolist()}; {tag}")
                worst["out"] = max(worst["out"], frac.max().item())
            if d.stats_ws or d.fuse_y:
                self._scales(f, r)
                e_acc = elem_bound(d, r["acc"], r["acc_scale"])
            if d.stats_ws:
                ref = restate_stats(d, r["acc"])
                got = f.t["stats_ws"][record_offsets(d, "stats", self.device)].double()
                bound = stats_bound(d, r["acc"], e_acc)
                rows = _chunks(d, r["acc"], 64)
                dv = rows - rows[:, :, :1]
                small = ((dv.abs().sum(2) < 2 ** 24) & ((dv * dv).sum(2) < 2 ** 24) & (rows[:, :, 0].abs() < 2 ** 24))[:, :, None, :]
                self._records("statistics", got, ref, bound, small.expand_as(ref) if exact else None, worst, "stats", tag)
            if d.fuse_y:
                z, zs = fuse_z(d, f.t["fuse_y"], f.t["fuse_mean"], f.t["fuse_rstd"])
                g = r["acc"].float().double()                  # (no bias with the fused pass: the launch's output as fp32)
                ref = restate_fuse(d, g, z)
                got = f.t["fuse_part"][record_offsets(d, "fuse", self.device)].double()
                bound = fuse_bound(d, g, z, zs, e_acc + U * g.abs())
                gz = (g * act_factor(d, z)).abs()
                small = ((_chunks(d, gz, 128).sum(2) < 2 ** 24) & (_chunks(d, gz * z.abs(), 128).sum(2) < 2 ** 24))[:, :, None, :]
                small = small & (d.fuse_act != 2)
                self._records("fused sums", got, ref, bound, small.expand_as(ref) if exact else None, worst, "fused", tag)
        bad = untouched(self.members, self.written)
        assert not bad, f"a store outside the written set of {bad}; {tag}"
        return worst

    @staticmethod
    def _records(what, got, ref, bound, bitwise, worst, key, tag):
        err = (got - ref).abs()
        ok = err <= bound
        if bitwise is not None:
            ok = torch.where(bitwise, got == ref, ok)
        assert bool(ok.all()), (f"{what}: {int((~ok).sum())} of {ok.numel()} values wrong ({int(torch.isnan(got).sum())} never written), first at "
                                f"[b, record, value, channel] = {(~ok).nonzero()[0].tolist()}: {got[~ok][0].item()!r} for {ref[~ok][0].item()!r}; {tag}")
        if bitwise is None:
            worst[key] = max(worst[key], (err / bound.clamp_min(1e-300))[bound > 0].max().item() if bool((bound > 0).any()) else 0.0)


# ------------------------------------------------------------------------------------------------------------ census
class Launch:
    """one convolution launch of a plan: kind = single | group | pair, `ds` copies of its descriptors (still holding the originals'
    addresses, which say what the members share), `w` the copy of the weight-gradient half of a pair"""

    def __init__(self, kind, plan, ds, w=None):
        self.kind, self.plan, self.ds, self.w = kind, plan, [copy_desc(d) for d in ds], (copy_desc(w) if w is not None else None)

    def geometry(self):
        addr = []
        for name in ("inp", "w", "out", "stats_ws", "fuse_part"):       # which members share which buffer
            vals = [getattr(d, name) for d in self.ds]
            addr.append(tuple(vals.index(v) for v in vals))
        wkey = None if self.w is None else tuple((n, tuple(getattr(self.w, n)) if n.startswith("tap_") else getattr(self.w, n))
                                                 for n, t in type(self.w)._fields_ if t is not C.c_void_p)
        return self.kind, tuple(geometry(d) for d in self.ds), tuple(addr), wkey

    def line(self):
        out = []
        for d in self.ds:
            out.append(f"B {d.B} OH {d.OH} OW {d.OW} N {d.N} K {d.ntaps}x{d.run} s{d.in_stride}/{d.out_stride} prec {d.precision}"
                       + (f" ksplit {d.ksplit}" if d.ksplit > 1 else "") + (" in16" if d.in_bf16 else "") + (" w16" if d.w_bf16 else "")
                       + (" out16" if d.out_bf16 else "") + (" stats" if d.stats_ws else "") + (" fused" if d.fuse_y else "")
                       + (f" span {d.out_span}" if d.out_span > 1 else "") + ("" if d.bias else " nobias"))
        return f"{self.plan} {self.kind}: " + " | ".join(out)


def launches_of(engines: dict, plan_names) -> list:
    """every convolution launch in the named plans of the engines {name: engine}: each ConvDesc behind nirgan_conv_igemm, the members of
    each nirgan_conv_igemm_group, the first argument of each nirgan_conv_wgrad_pair"""
    out = []
    for ename, eng in engines.items():
        for pname in plan_names:
            plan = getattr(eng, pname, None)
            if plan is None:
                continue
            for op, args in plan.ops:
                if op == "nirgan_conv_igemm":
                    out.append(Launch("single", f"{ename}.{pname}", [args[0]._obj]))
                elif op == "nirgan_conv_igemm_group":
                    out.append(Launch("group", f"{ename}.{pname}", [args[0][i].contents for i in range(args[1])]))
                elif op == "nirgan_conv_wgrad_pair":
                    out.append(Launch("pair", f"{ename}.{pname}", [args[0]._obj], args[1]._obj))
    return out


def build_engines(P, cfg: dict, device="cpu") -> tuple:
    """({engine name: engine}, what keeps their buffers alive) of one configuration of scripts/plan_signature.py (module P) with its plans built and nothing launched:
    Pix2PixTrainer._prepare, or a lone GeneratorEngine(need_backward=False) for an inference configuration.  Sets the configuration's
    options and leaves them set: the caller resets them (OPT.reset()) when it is done with the descriptors."""
    from nirgan_hip.nets import GeneratorEngine
    from nirgan_hip.options import OPT
    from nirgan_hip.trainer import Pix2PixTrainer
    OPT.reset()
    for k, v in cfg["opt"].items():
        assert hasattr(OPT, k), k
        setattr(OPT, k, v)
    if str(device) == "cpu":
        netG, netD = P._nets(cfg)
    else:
        torch.manual_seed(0)
        netG, netD = (n.to(device) for n in P._make_nets(cfg))
    B, H, W = cfg["shape"]
    if cfg["infer"]:
        flat = netG._flat()
        flat.ensure()
        return {"G": GeneratorEngine(flat.param_views(), None, cfg["blocks"], B, H, W, data_pad=cfg["padding"], inject=cfg["inject"],
                                     need_backward=False, precision=cfg["precision"])}, flat
    tr = Pix2PixTrainer(netG, netD, n_blocks=cfg["blocks"], padding=cfg["padding"], inject=cfg["inject"], precision=cfg["precision"],
                        micro_batches=cfg["micro_batches"])
    tr._prepare(B, H, W)
    out = {}
    for i, m in enumerate(tr._state.micros):
        tag = f"m{i}." if tr._state.n > 1 else ""
        out.update({tag + "G": m.G, tag + "D2": m.D2, tag + "D1": m.D1})
    return out, tr
