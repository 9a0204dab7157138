"""Case bodies of the blended tiled inference (predict_tiled(blend="blend"), nirgan_tile_count_ov / _gather_ov / nirgan_tile_blend),
shared by tests/test_tile_blend_emulated.py (numpy emulator, CPU) and tests/test_gpu_tile_blend.py (MI355X).

The float64 numpy restatement below is written from the geometry alone, per SCENE axis and for all tiles at once:
    core = tile - 2 margin, stride = core - overlap, 0 <= overlap <= core / 2;
    tile i reads scene rows i stride - margin .. + tile - 1, reflected (one reflection is the gather's rule; rows further out
    continue it with period 2 (H - 1)); its usable region is scene rows [i stride, i stride + core);
    tiles per axis: 1 if H <= core, else ceil((H - core) / stride) + 1; numbering b-major, then ti, then tj;
    band position t counts from the later tile's first usable row: later tile r(t), earlier tile 1 - r(t),
    linear r = (t + 0.5) / overlap, cosine r = 0.5 - 0.5 cos(pi (t + 0.5) / overlap); weight 1 outside the bands; a pixel's weight for
    a tile is row weight x column weight.

Bounds.  The gather copies: exact.  The blend sums at most 4 terms, each one fp32 weight product plus one fma rounding on top of the
fp32 weights themselves: <= 4 * 3 * 2^-24 ~ 7e-7 of max|v|, and the weights sum to 1 (no cancellation) -> TOL = 1e-6 of max|v|.  The
blend is compared on the per-tile predictions the model under test actually produced (recorded), so the bound is the blend's alone.
"""
import ctypes as C
import math

import numpy as np
import torch

from nirgan_hip import lib as L
from nirgan_hip.inference import predict_tiled

TOL = 1e-6
GUARD = 64
TILINGS = [(16, 2, 4), (16, 2, 6), (16, 2, 1), (16, 0, 8), (12, 3, 3)]             # (tile, margin, overlap)
SCENES = [(1, 3, 5, 7), (1, 3, 12, 12), (1, 3, 13, 29), (2, 3, 37, 50), (1, 1, 64, 23)]
WINDOWS = ("linear", "cosine")
WINDOW_ID = {"linear": 0, "cosine": 1}


# ------------------------------------------------------------------------------------------------ models (cheap torch callables)
def take0(x):
    return x[:, :1]


def tile_offset(x):
    """the instance-norm effect in miniature: every tile loses its own mean"""
    return x[:, :1] - x[:, :1].mean(dim=(2, 3), keepdim=True)


def tile_ramp(x):
    """elementwise (bitwise the same whatever the batch size) and position dependent: two tiles disagree where they overlap"""
    t = x.shape[-1]
    ramp = torch.arange(t * t, dtype=torch.float32, device=x.device).reshape(1, 1, t, t) / float(t * t)
    return x[:, :1] * (0.5 + ramp)


class Recorder:
    """wraps a model: keeps the tiles it was given and what it answered (CPU copies, in tile order)"""

    def __init__(self, model):
        self.model, self.inputs, self.outputs = model, [], []

    def __call__(self, x, *extra):
        y = self.model(x, *extra)
        self.inputs.append(x.detach().cpu().clone())
        self.outputs.append(y.detach().to(torch.float32).cpu().clone())
        return y

    def tiles(self):
        return torch.cat(self.inputs).numpy(), torch.cat(self.outputs).numpy()


def scene_of(shape, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * shape[2] + shape[3])
    return 0.05 + 0.9 * torch.rand(*shape, generator=g)


# ------------------------------------------------------------------------------------------------ float64 restatement
def reflect(i, n):
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def tiles_per_axis(extent, tile, margin, overlap):
    core = tile - 2 * margin
    return 1 if extent <= core else math.ceil((extent - core) / (core - overlap)) + 1


def count(B, H, W, tile, margin, overlap):
    return B * tiles_per_axis(H, tile, margin, overlap) * tiles_per_axis(W, tile, margin, overlap)


def later(t, overlap, window):
    t = np.asarray(t, dtype=np.float64)
    return (t + 0.5) / overlap if window == "linear" else 0.5 - 0.5 * np.cos(np.pi * (t + 0.5) / overlap)


def axis_table(extent, tile, margin, overlap, window):
    """[tiles per axis][extent] float64: the weight of every tile of the axis at every scene position (0 outside its usable region)"""
    core = tile - 2 * margin
    stride = core - overlap
    nt = tiles_per_axis(extent, tile, margin, overlap)
    table = np.zeros((nt, extent))
    for i in range(nt):
        for h in range(i * stride, min(i * stride + core, extent)):
            w = 1.0
            if i >= 1 and h - i * stride < overlap:                             # band with the earlier tile: this one is the later
                w = later(h - i * stride, overlap, window)
            if i + 1 < nt and h >= (i + 1) * stride:                            # band with the later tile
                w = 1.0 - later(h - (i + 1) * stride, overlap, window)
            table[i, h] = w
    assert np.abs(table.sum(0) - 1).max() < 1e-12 and (np.count_nonzero(table, axis=0) <= 2).all()
    return table


def gather64(scene, tile, margin, overlap):
    """scene [B][C][H][W] -> every tile [count][C][tile][tile] (same dtype: a gather copies)"""
    B, _, H, W = scene.shape
    stride = tile - 2 * margin - overlap
    out = []
    for b in range(B):
        for ti in range(tiles_per_axis(H, tile, margin, overlap)):
            hh = reflect(ti * stride - margin + np.arange(tile), H)
            for tj in range(tiles_per_axis(W, tile, margin, overlap)):
                ww = reflect(tj * stride - margin + np.arange(tile), W)
                out.append(scene[b][:, hh][:, :, ww])
    return np.stack(out)


def blend64(preds, B, H, W, tile, margin, overlap, window):
    """preds [count][C][tile][tile] -> float64 scene [B][C][H][W]: the weighted sum of the usable regions"""
    core = tile - 2 * margin
    stride = core - overlap
    ty, tx = axis_table(H, tile, margin, overlap, window), axis_table(W, tile, margin, overlap, window)
    out = np.zeros((B, preds.shape[1], H, W))
    k = 0
    for b in range(B):
        for ti in range(ty.shape[0]):
            for tj in range(tx.shape[0]):
                h0, w0 = ti * stride, tj * stride
                nh, nw = min(core, H - h0), min(core, W - w0)
                w = ty[ti, h0:h0 + nh, None] * tx[tj, None, w0:w0 + nw]
                out[b, :, h0:h0 + nh, w0:w0 + nw] += w * preds[k, :, margin:margin + nh, margin:margin + nw].astype(np.float64)
                k += 1
    assert k == len(preds)
    return out


# ------------------------------------------------------------------------------------------------ raw entries
def desc(scene, tiles, shape, tiling, window, first, n, channels=None):
    B, Cc, H, W = shape
    d = L.TileBlendDesc()
    d.B, d.C, d.H, d.W = B, Cc if channels is None else channels, H, W
    d.tile, d.margin, d.overlap = tiling
    d.window, d.first, d.n = WINDOW_ID[window], first, n
    d.scene, d.tiles = scene.data_ptr(), tiles.data_ptr()
    return d


def stream_of(dev):
    return torch.cuda.current_stream(dev).cuda_stream if torch.device(dev).type == "cuda" else None


def guarded(n, fill, guard_fill, dev, shift=0):
    """a buffer of n floats filled with ``fill`` between two guard bands of GUARD floats (+ shift: an address that is not 16-byte aligned)"""
    buf = torch.full((GUARD + shift + n + GUARD,), float(guard_fill), device=dev)
    view = buf[GUARD + shift:GUARD + shift + n]
    view.fill_(float(fill))
    return buf, view


def guards_intact(buf, n, guard_fill, shift=0):
    lo, hi = buf[:GUARD + shift], buf[GUARD + shift + n:]
    return bool((lo == guard_fill).all()) and bool((hi == guard_fill).all()) and hi.numel() == GUARD


# ------------------------------------------------------------------------------------------------ case bodies
def partition_of_unity(dev, shape, tiling):
    """take0: the blended scene is the scene's first channel, whatever the weights (they sum to 1), reflected reads included"""
    tile, margin, overlap = tiling
    scene = scene_of(shape)
    for window in WINDOWS:
        got = predict_tiled(take0, scene.to(dev), tile=tile, margin=margin, batch=5, blend="blend", overlap=overlap, window=window)
        assert got.shape == (shape[0], 1, shape[2], shape[3]) and got.dtype == scene.dtype
        err = (got.cpu().double() - scene[:, :1].double()).abs().max().item() / scene.abs().max().item()
        print(f"partition of unity {shape} {tiling} {window}: {err:.3e}")
        assert err <= TOL, (window, err)


def against_float64(dev, shape, tiling):
    """tile_offset: the tiles the model saw are the float64 gather (exact), the result is the float64 blend of its answers"""
    tile, margin, overlap = tiling
    B, _, H, W = shape
    scene = scene_of(shape)
    for window in WINDOWS:
        rec = Recorder(tile_offset)
        got = predict_tiled(rec, scene.to(dev), tile=tile, margin=margin, batch=4, blend="blend", overlap=overlap, window=window)
        seen, preds = rec.tiles()
        assert len(seen) == count(B, H, W, *tiling)
        assert np.array_equal(seen, gather64(scene.numpy(), *tiling))
        ref = blend64(preds, B, H, W, tile, margin, overlap, window)
        err = np.abs(got.cpu().double().numpy() - ref).max() / np.abs(preds).max()
        print(f"float64 restatement {shape} {tiling} {window}: {err:.3e} of max|v|")
        assert np.isfinite(got.cpu().numpy()).all() and err <= TOL, (window, err)


def split_independence(dev, shape, tiling):
    """batch = 1, 3, 7, all: bitwise the same scene; two runs bitwise equal"""
    tile, margin, overlap = tiling
    scene = scene_of(shape).to(dev)
    total = count(shape[0], shape[2], shape[3], *tiling)
    for window in WINDOWS:
        runs = [predict_tiled(tile_ramp, scene, tile=tile, margin=margin, batch=b, blend="blend", overlap=overlap, window=window)
                for b in (total, 1, 3, 7, total)]
        for r in runs[1:]:
            assert torch.equal(r, runs[0]), window


def raw_entries_need_no_initialisation(dev, shape, tiling, shift=0):
    """the entries on guarded buffers: the gather is the float64 gather, the blend of a NaN-filled scene is finite and independent of
    the split into launches, pixels past H x W are dropped and nothing outside the buffers is touched"""
    tile, margin, overlap = tiling
    B, Cc, H, W = shape
    be, st = L.backend(), stream_of(dev)
    total = int(be.nirgan_tile_count_ov(B, H, W, tile, margin, overlap))
    assert total == count(B, H, W, *tiling)
    scene = scene_of(shape).to(dev).contiguous()
    n_t = total * Cc * tile * tile
    tbuf, tiles = guarded(n_t, -3.0, -7.0, dev, shift)
    for first in range(0, total, 3):
        n = min(3, total - first)
        L.check(be.nirgan_tile_gather_ov(C.byref(desc(scene, tiles[first * Cc * tile * tile:], shape, tiling, "linear", first, n)), st), "tile_gather_ov")
    assert guards_intact(tbuf, n_t, -7.0, shift)
    assert np.array_equal(tiles.view(total, Cc, tile, tile).cpu().numpy(), gather64(scene.cpu().numpy(), *tiling))
    preds = tile_offset(tiles.view(total, Cc, tile, tile)).contiguous()
    for window in WINDOWS:
        results = []
        for split in (total, 2):
            obuf, out = guarded(B * H * W, float("nan"), -5.0, dev, shift)
            for first in range(0, total, split):
                n = min(split, total - first)
                L.check(be.nirgan_tile_blend(C.byref(desc(out, preds[first:], shape, tiling, window, first, n, channels=1)), st), "tile_blend")
            assert guards_intact(obuf, B * H * W, -5.0, shift)
            assert bool(torch.isfinite(out).all())
            results.append(out.clone())
        assert torch.equal(results[0], results[1])
        ref = blend64(preds.cpu().numpy(), B, H, W, tile, margin, overlap, window)
        err = np.abs(results[0].view(B, 1, H, W).cpu().double().numpy() - ref).max() / np.abs(preds.cpu().numpy()).max()
        assert err <= TOL, (window, err)


def overlap_zero_is_todays_path(dev, shape, tiling):
    tile, margin, _ = tiling
    B, _, H, W = shape
    scene = scene_of(shape).to(dev)
    be = L.backend()
    assert int(be.nirgan_tile_count_ov(B, H, W, tile, margin, 0)) == int(be.nirgan_tile_count(B, H, W, tile, margin))
    for model in (tile_offset, tile_ramp):
        old = predict_tiled(model, scene, tile=tile, margin=margin, batch=3)
        for window in WINDOWS:
            new = predict_tiled(model, scene, tile=tile, margin=margin, batch=3, blend="blend", overlap=0, window=window)
            assert torch.equal(new, old)
        assert torch.equal(predict_tiled(model, scene, tile=tile, margin=margin, batch=3, blend="none"), old)


def embeds_follow_the_scene(dev):
    """a B = 2 batch: every tile gets the embedding of the scene it was cut from (the new per-image tile count)"""
    shape, (tile, margin, overlap) = (2, 3, 37, 50), (16, 2, 4)
    scene = scene_of(shape)
    embeds = torch.tensor([[0.25, 9.0], [-0.5, 9.0]])

    def model(x, e):
        return x[:, :1] + e[:, :1, None, None]
    got = predict_tiled(model, scene.to(dev), tile=tile, margin=margin, batch=5, embeds=embeds.to(dev), blend="blend", overlap=overlap)
    ref = scene[:, :1].double() + embeds[:, 0].double()[:, None, None, None]
    assert (got.cpu().double() - ref).abs().max().item() <= TOL * ref.abs().max().item()


def seam_moves_as_designed(dev, tiling):
    """A scene whose left and right halves are two constants, tile_offset.  out - scene is minus the (blended) tile means: with
    blend="none" it steps by exactly the difference of two neighbours' means on their stride line and nowhere else; blended, no
    horizontal step exceeds the largest such difference times the largest increment of r (1 / overlap for linear)."""
    tile, margin, overlap = tiling
    B, Cc, H, W = 1, 3, 12, 50
    core = tile - 2 * margin
    scene = torch.empty(B, Cc, H, W)
    scene[..., :23], scene[..., 23:] = 0.2, 0.8
    s64 = scene[:, :1].double().numpy()

    def means_step(rec, ntw):
        seen, _ = rec.tiles()
        m = seen[:, 0].astype(np.float64).mean(axis=(1, 2)).reshape(-1, ntw)       # [ti][tj]; the scene is constant along y
        return np.abs(np.diff(m, axis=1)).max()

    rec = Recorder(tile_offset)
    none = predict_tiled(rec, scene.to(dev), tile=tile, margin=margin, batch=4, blend="none").cpu().double().numpy() - s64
    step = np.abs(np.diff(none, axis=-1))                                         # step[..., x - 1] = |d[x] - d[x - 1]|
    on_line = np.zeros(W - 1, dtype=bool)
    on_line[np.arange(core, W, core) - 1] = True
    d_none = means_step(rec, -(-W // core))
    assert d_none > 0.01
    assert abs(step[..., on_line].max() - d_none) <= TOL and step[..., ~on_line].max() <= TOL
    for window in WINDOWS:
        rec = Recorder(tile_offset)
        got = predict_tiled(rec, scene.to(dev), tile=tile, margin=margin, batch=4, blend="blend", overlap=overlap, window=window)
        d_tiles = means_step(rec, tiles_per_axis(W, *tiling))
        r = np.concatenate(([0.0], later(np.arange(overlap), overlap, window), [1.0]))          # 0 before the band, 1 after it
        factor = 1.0 / overlap if window == "linear" else np.diff(r).max()
        assert np.diff(r).max() <= factor + 1e-12
        _, preds = rec.tiles()
        for name, res in (("float64", blend64(preds, B, H, W, tile, margin, overlap, window)), ("device", got.cpu().double().numpy())):
            worst = np.abs(np.diff(res - s64, axis=-1)).max()
            print(f"seam {tiling} {window} {name}: none {d_none:.6f}, blended {worst:.6f} <= {d_tiles:.6f} * {factor:.4f}")
            assert worst <= d_tiles * factor + TOL, (window, name)
