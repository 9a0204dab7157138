"""Inference helpers around the generator forward.

The reference's create_synthetic_dataset.py (:100-118) runs ``model(hr)`` under no_grad on whole tiles,
then post-processes on the CPU and stores fp16 ``.npz`` files (:49-52, :117).  ``predict_tiled`` adds
what large scenes need on the GPU side: the scene is cut into tiles that overlap by twice the model's
reflect padding trick (model/pix2pix.py:91-93,107-108 hides tile-edge artefacts with pad-10 / crop); the
overlap is discarded, so every output pixel comes from a tile interior.
"""
from __future__ import annotations

import os

import numpy as np
import torch


@torch.no_grad()
def predict_tiled(model, rgb: torch.Tensor, tile: int = 512, margin: int = 16, batch: int = 8, embeds=None,
                  blend: str = "none", overlap=None, window: str = "linear", tta: str = "none") -> torch.Tensor:
    """rgb: B x 3 x H x W (any H, W >= 4) -> B x 1 x H x W.  ``tile`` is the network input size (multiple of 4);
    ``margin`` pixels on every side of a tile are context only.

    On the device the reflect-padded scene is never materialised: one gather launch cuts a batch of overlapping tiles straight out
    of the scene (nirgan_tile_gather reflects at the borders like ``F.pad(mode='reflect')``), the model runs on the batch, one
    scatter launch writes the tiles' cores back (nirgan_tile_scatter) -- no per-tile Python.  Device tensors only (no CPU path; the
    plain-torch statement of the same tiling lives with the oracle: oracle/nirgan_oracle.py::predict_tiled).

    ``blend="blend"`` lets the tiles' usable regions overlap by ``overlap`` pixels (default ``core // 4``, at most ``core // 2``) and
    cross-fades them with a ``"linear"`` or ``"cosine"`` ``window``: the generator's instance norms give every tile its own statistics,
    so neighbouring tiles differ by an offset that ``blend="none"`` leaves as a step on one pixel line.

    ``tta`` = ``"flip"``, ``"flips"`` or ``"d4"`` averages the predictions of the 2, 4 or 8 mirrored / transposed views of every tile
    (dihedral test-time augmentation): one nirgan_tile_views_expand launch after the gather, one model call on the
    ``n * k`` views, one nirgan_tile_views_merge launch before the scatter or blend.  ``batch`` stays the bound on the model's batch,
    so a step takes ``max(1, batch // k)`` tiles.  ``"none"`` runs exactly the launches described above."""
    assert tile % 4 == 0 and 0 <= margin < tile // 2
    if tta != "none":
        return _predict_tta_tiled(model, rgb, tile, margin, batch, embeds, blend, overlap, window, tta)
    if blend != "none":
        return _predict_blended(model, rgb, tile, margin, batch, embeds, blend, overlap, window)
    B, C3, H, W = rgb.shape
    core = tile - 2 * margin
    from . import lib as L
    if rgb.device.type != "cuda" and not L.is_emulated():
        raise RuntimeError("predict_tiled runs on MI355X (cuda tensors) only; there is no CPU path")
    be = L.backend()
    scene = rgb.detach().to(torch.float32).contiguous()
    total = int(be.nirgan_tile_count(B, H, W, tile, margin))
    if total <= 0:
        raise ValueError(f"predict_tiled: bad tiling (scene {H}x{W}, tile {tile}, margin {margin})")
    per_image = total // B
    out = torch.empty(B, 1, H, W, dtype=torch.float32, device=rgb.device)
    st = torch.cuda.current_stream(rgb.device).cuda_stream if rgb.device.type == "cuda" else None
    tiles = torch.empty(min(batch, total), C3, tile, tile, dtype=torch.float32, device=rgb.device)
    for first in range(0, total, batch):
        n = min(batch, total - first)
        L.check(be.nirgan_tile_gather(scene.data_ptr(), B, C3, H, W, tile, margin, first, n, tiles.data_ptr(), st), "tile_gather")
        x = tiles[:n]
        if embeds is None:
            pred = model(x)
        else:
            idx = torch.arange(first, first + n, device=embeds.device) // per_image      # tile -> scene it was cut from
            pred = model(x, embeds.index_select(0, idx))
        pred = pred.detach().to(torch.float32).contiguous()
        L.check(be.nirgan_tile_scatter(pred.data_ptr(), B, 1, H, W, tile, margin, first, n, out.data_ptr(), st), "tile_scatter")
    return out.to(rgb.dtype)


def _predict_blended(model, rgb, tile, margin, batch, embeds, blend, overlap, window):
    """predict_tiled(blend="blend"): nirgan_tile_gather_ov / model / nirgan_tile_blend per batch of tiles, in ascending tile number on
    one stream -- the blend entry needs no zeroed output and its result does not depend on ``batch``."""
    import ctypes as C
    from . import lib as L
    if blend != "blend":
        raise ValueError(f"predict_tiled: blend must be 'none' or 'blend', got {blend!r}")
    windows = {"linear": L.BLEND_LINEAR, "cosine": L.BLEND_COSINE}
    if window not in windows:
        raise ValueError(f"predict_tiled: window must be one of {sorted(windows)}, got {window!r}")
    B, C3, H, W = rgb.shape
    core = tile - 2 * margin
    overlap = core // 4 if overlap is None else int(overlap)
    if not 0 <= overlap <= core // 2:
        raise ValueError(f"predict_tiled: overlap {overlap} outside 0 .. core // 2 = {core // 2} (tile {tile}, margin {margin})")
    if rgb.device.type != "cuda" and not L.is_emulated():
        raise RuntimeError("predict_tiled runs on MI355X (cuda tensors) only; there is no CPU path")
    be = L.backend()
    scene = rgb.detach().to(torch.float32).contiguous()
    total = int(be.nirgan_tile_count_ov(B, H, W, tile, margin, overlap))
    if total <= 0:
        raise ValueError(f"predict_tiled: bad tiling (scene {H}x{W}, tile {tile}, margin {margin}, overlap {overlap})")
    per_image = total // B
    out = torch.empty(B, 1, H, W, dtype=torch.float32, device=rgb.device)
    st = torch.cuda.current_stream(rgb.device).cuda_stream if rgb.device.type == "cuda" else None
    tiles = torch.empty(min(batch, total), C3, tile, tile, dtype=torch.float32, device=rgb.device)
    d = L.TileBlendDesc()
    d.B, d.H, d.W, d.tile, d.margin, d.overlap, d.window = B, H, W, tile, margin, overlap, windows[window]
    for first in range(0, total, batch):
        d.first = first
        d.n = n = min(batch, total - first)
        d.C, d.scene, d.tiles = C3, scene.data_ptr(), tiles.data_ptr()
        L.check(be.nirgan_tile_gather_ov(C.byref(d), st), "tile_gather_ov")
        x = tiles[:n]
        if embeds is None:
            pred = model(x)
        else:
            idx = torch.arange(first, first + n, device=embeds.device) // per_image      # tile -> scene it was cut from
            pred = model(x, embeds.index_select(0, idx))
        pred = pred.detach().to(torch.float32).contiguous()
        d.C, d.scene, d.tiles = 1, out.data_ptr(), pred.data_ptr()
        L.check(be.nirgan_tile_blend(C.byref(d), st), "tile_blend")
    return out.to(rgb.dtype)


def _tta_views(tta, who):
    from . import lib as L
    if tta not in L.TTA_VIEWS:
        raise ValueError(f"{who}: tta must be one of {sorted(L.TTA_VIEWS)}, got {tta!r}")
    return L.TTA_VIEWS[tta]


class _ViewsRunner:
    """expand / model / merge on a batch of whole tiles: the buffers for the views and the merged prediction are allocated once"""

    def __init__(self, k, cap, C3, H, W, device):
        from . import lib as L
        self.L, self.be, self.k = L, L.backend(), k
        self.st = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else None
        self.views = torch.empty(cap * k, C3, H, W, dtype=torch.float32, device=device)
        self.merged = torch.empty(cap, 1, H, W, dtype=torch.float32, device=device)
        self.d = L.TileViewsDesc()
        self.d.H, self.d.W, self.d.views = H, W, k

    def __call__(self, model, x, embeds):
        """x: n x C3 x H x W fp32 contiguous, embeds: None or one row per tile -> n x 1 x H x W (a view of the runner's buffer)"""
        import ctypes as C
        L, d, n = self.L, self.d, x.shape[0]
        v = self.views[:n * self.k]
        d.n, d.C, d.src, d.dst = n, x.shape[1], x.data_ptr(), v.data_ptr()
        L.check(self.be.nirgan_tile_views_expand(C.byref(d), self.st), "tile_views_expand")
        pred = model(v) if embeds is None else model(v, embeds.repeat_interleave(self.k, dim=0))       # every view gets its tile's row
        pred = pred.detach().to(torch.float32).contiguous()
        if pred.shape != (n * self.k, 1, d.H, d.W):
            raise ValueError(f"test-time augmentation needs a model that maps n x C x H x W to n x 1 x H x W, got {tuple(pred.shape)}")
        out = self.merged[:n]
        d.C, d.src, d.dst = 1, pred.data_ptr(), out.data_ptr()
        L.check(self.be.nirgan_tile_views_merge(C.byref(d), self.st), "tile_views_merge")
        return out


def _predict_tta_tiled(model, rgb, tile, margin, batch, embeds, blend, overlap, window, tta):
    """predict_tiled(tta != "none"): gather / expand / model / merge / scatter-or-blend per step of max(1, batch // k) tiles, in
    ascending tile number on one stream.  The merge has a fixed summation order and both the scatter and the blend are independent
    of the split into launches, so the scene does not depend on ``batch``."""
    import ctypes as C
    from . import lib as L
    k = _tta_views(tta, "predict_tiled")
    if blend not in ("none", "blend"):
        raise ValueError(f"predict_tiled: blend must be 'none' or 'blend', got {blend!r}")
    windows = {"linear": L.BLEND_LINEAR, "cosine": L.BLEND_COSINE}
    B, C3, H, W = rgb.shape
    core = tile - 2 * margin
    if blend == "blend":
        if window not in windows:
            raise ValueError(f"predict_tiled: window must be one of {sorted(windows)}, got {window!r}")
        overlap = core // 4 if overlap is None else int(overlap)
        if not 0 <= overlap <= core // 2:
            raise ValueError(f"predict_tiled: overlap {overlap} outside 0 .. core // 2 = {core // 2} (tile {tile}, margin {margin})")
    if rgb.device.type != "cuda" and not L.is_emulated():
        raise RuntimeError("predict_tiled runs on MI355X (cuda tensors) only; there is no CPU path")
    be = L.backend()
    scene = rgb.detach().to(torch.float32).contiguous()
    total = int(be.nirgan_tile_count_ov(B, H, W, tile, margin, overlap) if blend == "blend" else be.nirgan_tile_count(B, H, W, tile, margin))
    if total <= 0:
        raise ValueError(f"predict_tiled: bad tiling (scene {H}x{W}, tile {tile}, margin {margin})")
    per_image = total // B
    step = max(1, batch // k)
    out = torch.empty(B, 1, H, W, dtype=torch.float32, device=rgb.device)
    st = torch.cuda.current_stream(rgb.device).cuda_stream if rgb.device.type == "cuda" else None
    tiles = torch.empty(min(step, total), C3, tile, tile, dtype=torch.float32, device=rgb.device)
    run = _ViewsRunner(k, min(step, total), C3, tile, tile, rgb.device)
    d = L.TileBlendDesc()
    if blend == "blend":
        d.B, d.H, d.W, d.tile, d.margin, d.overlap, d.window = B, H, W, tile, margin, overlap, windows[window]
    for first in range(0, total, step):
        n = min(step, total - first)
        if blend == "blend":
            d.first, d.n = first, n
            d.C, d.scene, d.tiles = C3, scene.data_ptr(), tiles.data_ptr()
            L.check(be.nirgan_tile_gather_ov(C.byref(d), st), "tile_gather_ov")
        else:
            L.check(be.nirgan_tile_gather(scene.data_ptr(), B, C3, H, W, tile, margin, first, n, tiles.data_ptr(), st), "tile_gather")
        idx = None if embeds is None else torch.arange(first, first + n, device=embeds.device) // per_image   # tile -> scene it was cut from
        pred = run(model, tiles[:n], None if embeds is None else embeds.index_select(0, idx))
        if blend == "blend":
            d.C, d.scene, d.tiles = 1, out.data_ptr(), pred.data_ptr()
            L.check(be.nirgan_tile_blend(C.byref(d), st), "tile_blend")
        else:
            L.check(be.nirgan_tile_scatter(pred.data_ptr(), B, 1, H, W, tile, margin, first, n, out.data_ptr(), st), "tile_scatter")
    return out.to(rgb.dtype)


@torch.no_grad()
def predict_tta(model, x: torch.Tensor, tta: str = "d4", embeds=None) -> torch.Tensor:
    """Whole tiles x: B x 3 x H x W -> B x 1 x H x W, the average over the ``tta`` views (``"flip"`` 2, ``"flips"`` 4, ``"d4"`` 8;
    ``"none"`` is one plain model call): one expand launch, ONE model call on the B * k views, one merge launch.  ``"d4"`` transposes,
    so it needs H == W; the flips work on any extent.  ``embeds``: one row per tile, repeated for its views.  Device tensors only."""
    from . import lib as L
    k = _tta_views(tta, "predict_tta")
    if x.dim() != 4:
        raise ValueError(f"predict_tta: x must be [B, C, H, W], got {tuple(x.shape)}")
    B, C3, H, W = x.shape
    if k == 8 and H != W:
        raise ValueError(f"predict_tta: tta='d4' transposes and needs square tiles, got {H} x {W}")
    if x.device.type != "cuda" and not L.is_emulated():
        raise RuntimeError("predict_tta runs on MI355X (cuda tensors) only; there is no CPU path")
    if k == 1:
        return (model(x) if embeds is None else model(x, embeds)).detach()
    run = _ViewsRunner(k, B, C3, H, W, x.device)
    return run(model, x.detach().to(torch.float32).contiguous(), embeds).to(x.dtype)


def save_nir_npz(pred_nir: torch.Tensor, out_path: str, name: str) -> str:
    """fp16 compressed .npz with key 'nir', as create_synthetic_dataset.py:49-52,115-118 writes it."""
    fn = os.path.join(out_path, f"{name}")
    np.savez_compressed(fn, nir=pred_nir.detach().to(torch.float16).cpu().numpy())
    return fn if fn.endswith(".npz") else fn + ".npz"


@torch.no_grad()
def resize_bilinear(x: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """F.interpolate(x, size=(H, W), mode='bilinear', align_corners=False) for [B, 1, h, w] on the device."""
    from . import lib as L
    dev = x.device
    st = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    x = x.detach().to(torch.float32).contiguous()
    up = torch.empty(x.shape[0], 1, H, W, dtype=torch.float32, device=dev)
    L.check(L.backend().nirgan_bilinear_fwd(x.data_ptr(), x.shape[0], x.shape[-2], x.shape[-1], up.data_ptr(), H, W, st), "bilinear")
    return up


@torch.no_grad()
def histogram_match(image: torch.Tensor, reference: torch.Tensor) -> torch.Tensor:
    """create_synthetic_dataset.py:34-47 on the device: ``reference`` ([B, 1, h, w], e.g. the Sentinel-2 NIR band) is
    resized to the tile with F.interpolate(mode='bilinear', align_corners=False) semantics (nirgan_bilinear_fwd), then
    every tile of ``image`` ([B, 1, H, W]) is matched to its reference plane (skimage.exposure.match_histograms,
    channel_axis=None -> nirgan_hist_match).  Returns [B, 1, H, W] like the reference's helper; stays on the GPU."""
    import ctypes as C
    from . import lib as L
    if image.dim() != 4 or reference.dim() != 4 or image.shape[:2] != reference.shape[:2] or image.shape[1] != 1:
        raise ValueError(f"image/reference must be [B, 1, H, W] / [B, 1, h, w], got {tuple(image.shape)} and {tuple(reference.shape)}")
    if image.device != reference.device or (image.device.type != "cuda" and not L.is_emulated()):
        raise RuntimeError("nirgan_hip runs on MI355X (cuda device) only; there is no CPU path")
    dev = image.device
    be = L.backend()
    st = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    img = image.detach().to(torch.float32).contiguous()
    ref = reference.detach().to(torch.float32).contiguous()
    B, _, H, W = img.shape
    if ref.shape[-2:] != (H, W):
        ref = resize_bilinear(ref, H, W)
    N = H * W
    ws = torch.empty(int(be.nirgan_hist_match_ws_bytes(B, N)) // 8, dtype=torch.int64, device=dev)
    out = torch.empty_like(img)
    d = L.HistMatchDesc()
    d.image, d.reference, d.B, d.N = img.data_ptr(), ref.data_ptr(), B, N
    d.ws, d.ws_bytes, d.out = ws.data_ptr(), ws.numel() * 8, out.data_ptr()
    L.check(be.nirgan_hist_match(C.byref(d), st), "hist_match")
    return out
