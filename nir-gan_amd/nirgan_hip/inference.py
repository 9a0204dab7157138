"""Inference helpers around the generator forward.

The reference's create_synthetic_dataset.py (:100-118) runs ``model(hr)`` under no_grad on whole tiles,
then post-processes on the CPU and stores fp16 ``.npz`` files (:49-52, :117).  ``predict_tiled`` adds
what large scenes need on the GPU side: the scene is cut into tiles that overlap by twice the model's
reflect padding trick (model/pix2pix.py:91-93,107-108 hides tile-edge artefacts with pad-10 / crop); the
overlap is discarded, so every output pixel comes from a tile interior.  ``predict_scene`` is the same flow for ONE scene as it is
stored (uint16 reflectance or float32, resident on the device): cut and normalised by the gather, tiles of nothing but nodata
skipped, the blended result written back as uint16 / float16 / float32.
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


_OUT_DTYPES = {"uint16": torch.int16, "float16": torch.float16, "float32": torch.float32}


def _usable_areas(H, W, core, stride, nth, ntw):
    """pixels of every tile's usable region clipped to the scene, row-major [nth * ntw]"""
    hy = np.minimum(core, H - np.arange(nth, dtype=np.int64) * stride)
    wx = np.minimum(core, W - np.arange(ntw, dtype=np.int64) * stride)
    return (hy[:, None] * wx[None, :]).reshape(-1)


@torch.no_grad()
def predict_scene(model, scene, *, bands=(0, 1, 2), divisor=10000.0, nodata=None, geotransform=None, tile: int = 512, margin: int = 16,
                  overlap=None, window: str = "linear", batch: int = 8, tta: str = "none", embeds=None, out: str = "uint16", scale=None,
                  nodata_out=None, match=None, match_nodata=None) -> torch.Tensor:
    """The NIR band of one device-resident scene, predicted in place -> [H, W] device tensor.

    ``scene``: a device tensor [C, H, W], C >= 3, contiguous: uint16 reflectance as the int16 bit patterns ``ScenePool`` stores (or
    torch.uint16), or float32.  A numpy uint16 / float32 array is uploaded once as it is.  ``bands`` name the planes of R, G, B; every
    value is divided by ``divisor`` on the way into a tile (one float32 division, as ``a[bands].astype(float32) / float32(divisor)``).
    ``tile``, ``margin``, ``overlap``, ``window``, ``batch`` and ``tta`` mean what they mean in ``predict_tiled(blend="blend")``;
    ``overlap=0`` is the plain tiling.

    ``nodata``: a pixel is invalid where any of the three bands equals it (uint16) or is NaN (float32; the value is not used); with
    None no pixel is.  A tile whose usable region holds only invalid pixels is skipped -- the generator never sees it; no valid pixel
    changes, since every tile covering a valid pixel still runs on exactly the input it would read otherwise (nodata pixels enter as
    ``nodata / divisor``).  Which tiles run costs ONE copy of a count per tile to the host, the only synchronisation.

    ``out``: ``"uint16"`` (int16 bit patterns: ``rint(v * scale)`` clamped to 0 .. 65535, ``scale`` defaults to ``divisor``; a valid
    pixel that lands on ``nodata_out`` moves to the next code), ``"float16"`` (what ``save_nir_npz`` stores) or ``"float32"`` (bitwise
    ``predict_tiled`` on the converted scene).  Invalid pixels get ``nodata_out``: by default ``nodata`` (0 without) for uint16, NaN for
    the float kinds.

    ``embeds``: None calls ``model(x)``; a [1, 256] tensor gives every tile that row; ``"coords"`` (needs ``geotransform`` = (lon0,
    dlon, lat0, dlat), a sequence or a float64 device tensor) has the gather write the lon / lat of every tile's own centre and calls
    ``model(x, model.satclip_get_inject(coords))``: each tile of a large scene gets the prior of its own location.

    ``match`` (``out="uint16"`` only): a reference band -- a uint16 plane of ANY size, as ``scene_histogram`` takes it, whose
    nodata code is ``match_nodata`` (default: ``nodata``) -- or an int64 [65536] histogram, e.g. ``ScenePool.band_histogram``.  The
    finished plane's histogram is matched to it in place (``histogram_match_scene``) before it is returned.  With ``nodata`` given,
    ``nodata_out`` is the reserved code: invalid pixels keep it and are not counted, valid ones never get it; without, every pixel counts
    and no code is reserved."""
    import ctypes as C
    from . import lib as L
    k = _tta_views(tta, "predict_scene")
    windows = {"linear": L.BLEND_LINEAR, "cosine": L.BLEND_COSINE}
    if window not in windows:
        raise ValueError(f"predict_scene: window must be one of {sorted(windows)}, got {window!r}")
    if out not in L.SCENE_OUT_KINDS:
        raise ValueError(f"predict_scene: out must be one of {sorted(L.SCENE_OUT_KINDS)}, got {out!r}")
    if match is not None and out != "uint16":
        raise ValueError(f"predict_scene: match needs out='uint16', got {out!r}")
    if isinstance(scene, np.ndarray):
        if scene.dtype not in (np.uint16, np.float32):
            raise ValueError(f"predict_scene: a numpy scene must be uint16 or float32, got {scene.dtype}")
        a = np.ascontiguousarray(scene)
        scene = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to("cpu" if L.is_emulated() else "cuda")
    if scene.dim() != 3 or scene.dtype not in (torch.int16, torch.uint16, torch.float32) or not scene.is_contiguous():
        raise ValueError(f"predict_scene: the scene must be a contiguous [C, H, W] tensor of int16 (uint16 bit patterns), uint16 or float32, "
                         f"got {tuple(scene.shape)} {scene.dtype}")
    dev = scene.device
    if dev.type != "cuda" and not L.is_emulated():
        raise RuntimeError("predict_scene runs on MI355X (cuda tensors) only; there is no CPU path")
    if match is not None and not _is_histogram(match):
        match = _code_plane(match, "predict_scene: match", dev)                  # a bad reference is refused before the model runs
    Cs, H, W = (int(v) for v in scene.shape)
    is_u16 = scene.dtype != torch.float32
    bands = tuple(int(b) for b in bands)
    if Cs < 3 or len(bands) != 3 or any(not 0 <= b < Cs for b in bands):
        raise ValueError(f"predict_scene: the scene needs at least 3 bands and bands must name three planes in 0 .. C-1, got C {Cs}, bands {bands}")
    if tile <= 0 or tile % 4 or not 0 <= margin < tile // 2:
        raise ValueError(f"predict_scene: tile must be a positive multiple of 4 and 0 <= margin < tile // 2 (tile {tile}, margin {margin})")
    core = tile - 2 * margin
    overlap = core // 4 if overlap is None else int(overlap)
    if not 0 <= overlap <= core // 2:
        raise ValueError(f"predict_scene: overlap {overlap} outside 0 .. core // 2 = {core // 2} (tile {tile}, margin {margin})")
    if is_u16 and nodata is not None and not 0 <= int(nodata) <= 65535:
        raise ValueError(f"predict_scene: nodata {nodata} outside 0 .. 65535")
    kind = L.SCENE_OUT_KINDS[out]
    if nodata_out is None:
        nodata_out = (int(nodata) if is_u16 and nodata is not None else 0) if kind == L.SCENE_OUT_U16 else float("nan")
    be = L.backend()
    nt = int(be.nirgan_tile_count_ov(1, H, W, tile, margin, overlap))
    if nt <= 0:
        raise ValueError(f"predict_scene: bad tiling (scene {H}x{W}, tile {tile}, margin {margin}, overlap {overlap})")
    stride = core - overlap
    ntw = 1 if W <= core else -(-(W - core) // stride) + 1
    st = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    geo = None
    if geotransform is not None:
        geo = geotransform if torch.is_tensor(geotransform) else torch.tensor([float(v) for v in geotransform], dtype=torch.float64)
        geo = geo.detach().to(device=dev, dtype=torch.float64).reshape(4).contiguous()
    if isinstance(embeds, str):
        if embeds != "coords":
            raise ValueError(f"predict_scene: embeds must be None, a [1, E] tensor or 'coords', got {embeds!r}")
        if geo is None:
            raise ValueError("predict_scene: embeds='coords' needs a geotransform")
    elif embeds is not None and (embeds.dim() != 2 or embeds.shape[0] != 1):
        raise ValueError(f"predict_scene: an embeds tensor is one row [1, E] for the whole scene, got {tuple(embeds.shape)}")
    d = L.ScenePredictDesc()
    d.scene, d.dtype, d.C, d.H, d.W = scene.data_ptr(), L.SCENE_U16 if is_u16 else L.SCENE_F32, Cs, H, W
    d.band = (C.c_int * 3)(*bands)
    d.has_nodata, d.nodata = int(nodata is not None), int(nodata) if is_u16 and nodata is not None else 0
    d.divisor, d.tile, d.margin, d.overlap = float(divisor), tile, margin, overlap
    if nodata is not None:
        counts = torch.empty(nt, dtype=torch.int32, device=dev)
        d.counts = counts.data_ptr()
        L.check(be.nirgan_scene_tile_invalid(C.byref(d), st), "scene_tile_invalid")
        full = counts.cpu().numpy().astype(np.int64) >= _usable_areas(H, W, core, stride, nt // ntw, ntw)     # the one copy to the host
        ids_host = np.ascontiguousarray(np.flatnonzero(~full).astype(np.int32))
    else:
        ids_host = np.arange(nt, dtype=np.int32)
    ids = torch.from_numpy(ids_host.copy()).to(dev)
    total = len(ids_host)
    acc = torch.zeros(1, 1, H, W, dtype=torch.float32, device=dev)
    step = max(1, batch // k)
    if total:
        tiles = torch.empty(min(step, total), 3, tile, tile, dtype=torch.float32, device=dev)
        coords = torch.empty(min(step, total), 2, dtype=torch.float32, device=dev) if isinstance(embeds, str) else None
        run = _ViewsRunner(k, min(step, total), 3, tile, tile, dev) if k > 1 else None
        b = L.TileBlendDesc()
        b.B, b.C, b.H, b.W, b.tile, b.margin, b.overlap, b.window = 1, 1, H, W, tile, margin, overlap, windows[window]
        b.scene = acc.data_ptr()
        d.tiles, d.geo, d.coords = tiles.data_ptr(), None if coords is None else geo.data_ptr(), None if coords is None else coords.data_ptr()
    for i0 in range(0, total, step):
        n = min(step, total - i0)
        d.ids, d.ids_host, d.n = ids.data_ptr() + 4 * i0, ids_host.ctypes.data + 4 * i0, n
        L.check(be.nirgan_scene_tile_gather(C.byref(d), st), "scene_tile_gather")
        x = tiles[:n]
        e = None if embeds is None else (model.satclip_get_inject(coords[:n]) if coords is not None else embeds.expand(n, -1))
        if run is not None:
            pred = run(model, x, e)
        else:
            pred = (model(x) if e is None else model(x, e)).detach().to(torch.float32).contiguous()
            if pred.shape != (n, 1, tile, tile):
                raise ValueError(f"predict_scene needs a model that maps n x 3 x T x T to n x 1 x T x T, got {tuple(pred.shape)}")
        chunk = ids_host[i0:i0 + n]
        starts = np.concatenate(([0], np.flatnonzero(np.diff(chunk) != 1) + 1, [n]))          # maximal runs of consecutive tile numbers
        for a0, a1 in zip(starts[:-1], starts[1:]):
            b.first, b.n, b.tiles = int(chunk[a0]), int(a1 - a0), pred.data_ptr() + 4 * int(a0) * tile * tile
            L.check(be.nirgan_tile_blend(C.byref(b), st), "tile_blend")
    res = torch.empty(H, W, dtype=_OUT_DTYPES[out], device=dev)
    d.blended, d.out_kind, d.out = acc.data_ptr(), kind, res.data_ptr()
    d.scale, d.nodata_out = float(divisor if scale is None else scale), float(nodata_out)
    L.check(be.nirgan_scene_finish(C.byref(d), st), "scene_finish")
    if match is not None:
        ref_nodata = nodata if match_nodata is None else match_nodata
        histogram_match_scene(res, match, nodata=None if nodata is None else int(nodata_out), reference_nodata=ref_nodata, out=res)
    return res


def _is_histogram(t) -> bool:
    return torch.is_tensor(t) and t.dtype == torch.int64 and tuple(t.shape) == (65536,)


def _code_plane(plane, who, dev=None) -> torch.Tensor:
    """a uint16 plane ([H, W] or flat; int16 bit patterns, torch.uint16 or a numpy uint16 array) -> the same memory as a flat tensor"""
    from . import lib as L
    if isinstance(plane, np.ndarray):
        if plane.dtype != np.uint16 or plane.ndim not in (1, 2):
            raise ValueError(f"{who}: a numpy plane must be a uint16 [H, W] or flat array, got {plane.dtype} {plane.shape}")
        plane = torch.from_numpy(np.ascontiguousarray(plane).view(np.int16)).to(dev if dev is not None else ("cpu" if L.is_emulated() else "cuda"))
    if not torch.is_tensor(plane) or plane.dim() not in (1, 2) or plane.dtype not in (torch.int16, torch.uint16) or not plane.is_contiguous():
        raise ValueError(f"{who}: the plane must be a contiguous [H, W] or flat tensor of int16 (uint16 bit patterns) or uint16")
    if plane.numel() < 1:
        raise ValueError(f"{who}: the plane is empty")
    if plane.device.type != "cuda" and not L.is_emulated():
        raise RuntimeError(f"{who} runs on MI355X (cuda tensors) only; there is no CPU path")
    return plane.view(-1)


def _match_desc(dev, nodata, who):
    from . import lib as L
    if nodata is not None and not 0 <= int(nodata) <= 65535:
        raise ValueError(f"{who}: nodata {nodata} outside 0 .. 65535")
    d = L.SceneMatchDesc()
    d.has_nodata, d.nodata = int(nodata is not None), 0 if nodata is None else int(nodata)
    return d, (torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None)


def _check_histogram(h, dev, who):
    if not _is_histogram(h) or not h.is_contiguous() or h.device != dev:
        raise ValueError(f"{who}: a histogram is a contiguous int64 [65536] tensor on {dev}")
    return h


@torch.no_grad()
def scene_histogram(plane, nodata=None, into=None) -> torch.Tensor:
    """int64 [65536]: how often every uint16 code occurs in ``plane`` (an [H, W] or flat tensor of int16 bit patterns or uint16,
    contiguous, possibly a view such as one band of a scene; or a numpy uint16 array, uploaded once), codes equal to ``nodata`` left
    out (nirgan_scene_hist).  ``into``: a histogram to ADD to -- the planes of many calls pool into one -- which is
    also what is returned."""
    import ctypes as C
    from . import lib as L
    flat = _code_plane(plane, "scene_histogram", None if into is None else into.device)
    dev = flat.device
    hist = torch.zeros(65536, dtype=torch.int64, device=dev) if into is None else _check_histogram(into, dev, "scene_histogram: into")
    d, st = _match_desc(dev, nodata, "scene_histogram")
    d.plane, d.n, d.hist = flat.data_ptr(), flat.numel(), hist.data_ptr()
    L.check(L.backend().nirgan_scene_hist(C.byref(d), st), "scene_hist")
    return hist


@torch.no_grad()
def scene_match_lut(src_hist: torch.Tensor, ref_hist: torch.Tensor, nodata=None) -> torch.Tensor:
    """The transfer table [65536] (int16 bit patterns of uint16 codes, as the pool stores them) that matches the histogram ``src_hist``
    to ``ref_hist`` as skimage.exposure.match_histograms does, rounded to the nearest code (ties to even); a result equal to ``nodata``
    moves to the next code.  An empty histogram on either side gives the identity (nirgan_scene_match_lut)."""
    import ctypes as C
    from . import lib as L
    dev = src_hist.device if torch.is_tensor(src_hist) else None
    _check_histogram(src_hist, dev, "scene_match_lut: src_hist")
    _check_histogram(ref_hist, dev, "scene_match_lut: ref_hist")
    if dev.type != "cuda" and not L.is_emulated():
        raise RuntimeError("scene_match_lut runs on MI355X (cuda tensors) only; there is no CPU path")
    lut = torch.empty(65536, dtype=torch.int16, device=dev)
    d, st = _match_desc(dev, nodata, "scene_match_lut")
    d.src_hist, d.ref_hist, d.lut = src_hist.data_ptr(), ref_hist.data_ptr(), lut.data_ptr()
    L.check(L.backend().nirgan_scene_match_lut(C.byref(d), st), "scene_match_lut")
    return lut


_SAME = object()


@torch.no_grad()
def histogram_match_scene(plane, reference, nodata=None, reference_nodata=_SAME, out=None) -> torch.Tensor:
    """``plane`` (as ``scene_histogram`` takes it) with its histogram matched to ``reference``: a uint16 plane of ANY size -- its own
    pixels are counted, nothing is resampled -- or an int64 [65536] histogram.  Pixels equal to ``nodata`` are not counted and pass
    through unchanged, no other pixel becomes ``nodata``; ``reference_nodata`` (default: ``nodata``) is the code left out of a reference
    plane.  ``out``: where the result goes, ``out=plane`` works in place; by default a new tensor shaped like ``plane``.  Two counts, one
    table, one lookup pass; nothing is copied to the host."""
    import ctypes as C
    from . import lib as L
    flat = _code_plane(plane, "histogram_match_scene")
    dev = flat.device
    if torch.is_tensor(plane):
        shaped = plane
    else:
        shaped = flat.view(plane.shape)
    if _is_histogram(reference):
        ref_hist = _check_histogram(reference, dev, "histogram_match_scene: reference")
    else:
        ref_hist = scene_histogram(_code_plane(reference, "histogram_match_scene: reference", dev), nodata if reference_nodata is _SAME else reference_nodata,
                                   torch.zeros(65536, dtype=torch.int64, device=dev))
    lut = scene_match_lut(scene_histogram(flat, nodata), ref_hist, nodata)
    if out is None:
        out = torch.empty_like(shaped)
    elif not torch.is_tensor(out) or out.dtype != shaped.dtype or out.shape != shaped.shape or out.device != dev or not out.is_contiguous():
        raise ValueError(f"histogram_match_scene: out must be a contiguous {shaped.dtype} tensor of shape {tuple(shaped.shape)} on {dev}")
    d, st = _match_desc(dev, nodata, "histogram_match_scene")
    d.plane, d.n, d.lut, d.out = flat.data_ptr(), flat.numel(), lut.data_ptr(), out.data_ptr()
    L.check(L.backend().nirgan_scene_lut_apply(C.byref(d), st), "scene_lut_apply")
    return out


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
