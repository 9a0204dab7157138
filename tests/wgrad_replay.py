"""Shared by the weight-gradient replay tests: a float64 restatement of one nirgan_wgrad_desc, and copies of descriptors pointed at fresh
buffers.  Test infrastructure: plain torch and ctypes, it neither calls the emulator nor needs the library.

    slab[plane][s][n][t * run + c] = sum over the pixels m of split s of
        p[plane][b][oh + p_oh][ow + p_ow][n] * q[plane][b][oh * q_stride + q_oh + tap_dh[t]][ow * q_stride + q_ow + tap_dw[t]] (float c)

with m = (b, oh, ow) over B * OH * OW, split s = pixels [s * rows_per_split, (s + 1) * rows_per_split) (include/nirgan_hip.h,
nirgan_wgrad_desc).  The `run` floats of a tap are contiguous from the pixel's first channel on and may run into the next pixel's channels
(the row-packed first layer).  Plane i reads p + i * p_plane and q + i * q_plane; pq_bf16 operands are bf16 elements."""
import ctypes as C

import torch

GUARD = 4096                 # floats past slab_elems that a launch must leave alone
SENTINEL_BITS = 0x7FC0DEAD   # a quiet NaN no kernel computes: slab elements still holding it were never written


def pixel_bases(d, m0: int, m1: int, device):
    """Element offsets (without the plane) of P's and Q's window origin for pixels m0 .. m1 - 1."""
    m = torch.arange(m0, m1, dtype=torch.int64, device=device)
    ohw = d.OH * d.OW
    b, r = m // ohw, m % ohw
    oh, ow = r // d.OW, r % d.OW
    pb = b * (d.p_hp * d.p_wp * d.p_cs) + (oh + d.p_oh) * (d.p_wp * d.p_cs) + (ow + d.p_ow) * d.p_cs
    qb = b * (d.q_hp * d.q_wp * d.q_cs) + (oh * d.q_stride + d.q_oh) * (d.q_wp * d.q_cs) + (ow * d.q_stride + d.q_ow) * d.q_cs
    return pb, qb


def q_columns(d, device):
    """Offset of GEMM column J = t * run + c from a pixel's Q origin."""
    col = [d.tap_dh[t] * d.q_wp * d.q_cs + d.tap_dw[t] * d.q_cs + c for t in range(d.ntaps) for c in range(d.run)]
    return torch.tensor(col, dtype=torch.int64, device=device)


def operand_terms(x: torch.Tensor, precision: int):
    """The bf16 terms an operand enters the matrix pipe as (include/nirgan_hip.h, nirgan_conv_desc.precision): 0 = the fp32 value,
    1 = its nearest-even bf16, 2 = two terms, 3 = three terms (each the nearest-even bf16 of what the previous ones left)."""
    x = x.float()
    if precision == 0:
        return [x.double()]
    terms, rest = [], x
    for _ in range({1: 1, 2: 2, 3: 3}[precision]):
        t = rest.to(torch.bfloat16).float()
        terms.append(t.double())
        rest = rest - t
    return terms


# the products each precision forms from those terms (h = 0, m = 1, l = 2): the bf16x3 mode drops m * m, the three-term split everything
# below 2^-16 of h * h
PRODUCTS = {0: [(0, 0)], 1: [(0, 0)], 2: [(0, 0), (0, 1), (1, 0)], 3: [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]}


def restate(d, p: torch.Tensor, q: torch.Tensor, precision: int = 0, absolute: bool = False, chunk_elems: int = 1 << 24) -> torch.Tensor:
    """float64 slabs [nplanes][nsplit][N][ntaps * run] of descriptor d over the operand buffers p and q (flat tensors holding what the
    descriptor's p and q point to: float32, or bfloat16 when pq_bf16).  precision: the operand treatment to model (0 = exact products).
    absolute: |P|^T |Q| (of the modelled terms) instead -- the scale of a rigorous rounding bound."""
    return restate_with_scale(d, p, q, precision, chunk_elems, kinds=("abs",) if absolute else ("value",))[0]


def restate_with_scale(d, p: torch.Tensor, q: torch.Tensor, precision: int = 0, chunk_elems: int = 1 << 24, kinds=("value", "abs")):
    """restate() for several kinds ("value", "abs") over one gather of the operands.  Runs on p's device, split by split and in chunks of
    pixels, so that the biggest layers fit."""
    dev = p.device
    K = d.ntaps * d.run
    M = d.B * d.OH * d.OW
    nplanes = max(d.nplanes, 1)
    cols = q_columns(d, dev)
    rows_n = torch.arange(d.N, dtype=torch.int64, device=dev)
    outs = [torch.zeros(nplanes, d.nsplit, d.N, K, dtype=torch.float64, device=dev) for _ in kinds]
    step = max(32, chunk_elems // (d.N + K))
    for i in range(nplanes):
        po, qo = i * d.p_plane, i * d.q_plane
        for s in range(d.nsplit):
            a, e = s * d.rows_per_split, min((s + 1) * d.rows_per_split, M)
            for m0 in range(a, e, step):
                m1 = min(m0 + step, e)
                pb, qb = pixel_bases(d, m0, m1, dev)
                pt = operand_terms(p[po + pb[:, None] + rows_n[None, :]], precision)
                qt = operand_terms(q[qo + qb[:, None] + cols[None, :]], precision)
                for out, kind in zip(outs, kinds):
                    for x, y in PRODUCTS[precision]:
                        out[i, s] += (pt[x].abs().T @ qt[y].abs()) if kind == "abs" else (pt[x].T @ qt[y])
    return outs


def _buffer(n: int, bf16: bool, device) -> torch.Tensor:
    return torch.zeros(max(int(n), 1), dtype=torch.bfloat16 if bf16 else torch.float32, device=device)


def copy_desc(d):
    """A byte copy of a ctypes descriptor (what the emulator does for planes): it still points where d points."""
    c = type(d)()
    C.memmove(C.byref(c), C.byref(d), C.sizeof(d))
    return c


def slab_count(d) -> int:
    """floats of the slabs the launch owns: [nplanes][nsplit][N][K]"""
    return max(d.nplanes, 1) * d.nsplit * d.N * d.ntaps * d.run


class FreshWgrad:
    """A copy of a weight-gradient descriptor over buffers of its own, of the sizes the descriptor declares: p and q (bf16 when pq_bf16),
    the slabs plus GUARD floats, a zero page.  Nothing of the original's memory is referenced.  p_elems_min: a larger p (the replay of a
    fused pair hands the same buffer to the data gradient's input)."""

    def __init__(self, d, device, p_elems_min: int = 0):
        self.d = copy_desc(d)
        bf = bool(d.pq_bf16)
        self.p = _buffer(max(d.p_elems, p_elems_min), bf, device)
        self.q = _buffer(d.q_elems, bf, device)
        self.slabs = torch.empty(d.slab_elems + GUARD, dtype=torch.float32, device=device)
        self.zero = torch.zeros(64, dtype=torch.float32, device=device)
        self.d.p, self.d.q = self.p.data_ptr(), self.q.data_ptr()
        self.d.slabs, self.d.zero_page = self.slabs.data_ptr(), self.zero.data_ptr()

    def arm(self):
        """every slab element and the guard to the sentinel"""
        self.slabs.view(torch.int32).fill_(SENTINEL_BITS)

    def written(self) -> torch.Tensor:
        """the slabs the launch owns, [nplanes][nsplit][N][K]"""
        d = self.d
        return self.slabs[:slab_count(d)].view(max(d.nplanes, 1), d.nsplit, d.N, d.ntaps * d.run)

    def untouched_tail(self) -> bool:
        """the rest of the declared slabs and the guard still hold the sentinel"""
        return bool((self.slabs[slab_count(self.d):].view(torch.int32) == SENTINEL_BITS).all())


def fresh_conv(c, inp: torch.Tensor, device):
    """A copy of the data-gradient half of a fused pair (nirgan_conv_desc) that reads `inp` (the replay's P buffer: the same dY) and
    reads or writes nothing of the original's memory: weights, bias, split-K workspace, statistics, fused-backward operands and output
    all point at scratch of the declared sizes.  Returns (copy, the scratch tensors to keep alive).  Fails on a pointer field it does
    not know, so that a new field cannot keep pointing at freed memory."""
    cc = copy_desc(c)
    keep = [inp]
    ch = c.N
    sizes = {   # field -> floats (bf16 buffers get as many floats: twice the bytes they need)
        "w": c.w_elems, "bias": c.N, "out": c.out_elems, "split_ws": c.split_ws_elems, "stats_ws": c.stats_ws_elems,
        "fuse_y": c.B * c.fuse_h * c.fuse_w * ch, "fuse_mean": c.B * ch, "fuse_rstd": c.B * ch, "fuse_part": c.fuse_part_elems,
        "w_x3": (3 * c.w_x3_plane + 1) // 2 + 8, "zero_page": 64,
    }
    for name, typ in type(c)._fields_:
        if typ is not C.c_void_p or name == "inp":
            continue
        if not getattr(c, name):
            continue
        assert name in sizes, f"fresh_conv: unknown pointer field {name}"
        t = torch.zeros(max(int(sizes[name]), 64), dtype=torch.float32, device=device)
        keep.append(t)
        setattr(cc, name, t.data_ptr())
    cc.inp = inp.data_ptr()
    return cc, keep
