"""MI355X-native counterpart of the reference's ``utils/calculate_metrics.py``.

``calculate_metrics(pred, target, phase)`` keeps the reference's signature and result
(utils/calculate_metrics.py:5-36): a dict ``{phase/L1, phase/L2, phase/PSNR, phase/SSIM}`` of Python floats
(F.l1_loss, F.mse_loss, kornia.metrics.psnr(.., 1.0), kornia.metrics.ssim(window_size=5, max_val=1.).mean()).
The reference moves both tensors to the CPU every 10th batch for this (model/pix2pix.py:183-186); here it is ONE
fused pass on the device (nirgan_image_metrics).  ``image_metrics_device`` returns the three means as a device
tensor without synchronising, for callers that log asynchronously.

``tile_metrics_device(rgb, nir, pred, crop, ..)`` is the per-tile form behind the validation table
(validation_utils/): one row of ``TILE_METRIC_COLUMNS`` per tile of the batch in ONE fused pass (nirgan_tile_metrics),
the centre crop applied by indexing.

``tile_metrics_masked_device(rgb, nir, pred, valid, crop, ..)`` is that table over the VALID pixels of each tile
(nirgan_tile_metrics_masked): ``TILE_METRIC_MASKED_COLUMNS`` adds the counts ``n_valid`` and ``n_ssim``; SSIM is averaged over the
pixels whose whole filter support is valid.  ``calculate_metrics(.., valid=mask)`` pools its rows over a batch by those counts: the
validation scalars of a run that trains on partly valid windows (``grid_loader(.., return_valid=True)``).

``window_stats_device(rgb, nir, pred, y0, x0, wh, ww)`` gives the mean and the median of nir, pred and their NDVI over one window
of every tile of a date stack (nirgan_window_stats): the numbers behind validation_utils/time_series_validation.py.

``class_metrics_device(rgb, nir, pred, mask, classes, crop, ..)`` splits the per-tile rows by the class id of a land-cover mask
(nirgan_class_metrics): one row of ``CLASS_METRIC_COLUMNS`` per (tile, class) in ONE fused pass, behind validation_utils/land_cover.py.
"""
import ctypes as C
import math

import torch

from nirgan_hip import lib as L


def _stream(device):
    """the current stream's handle on a cuda device; None under the emulator"""
    return torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else None


def _prepare(rgb, nir, pred, lead="B", between=None, also=()):
    """``(rgb, nir, pred)`` checked and as fp32 contiguous tensors (rgb cut to its first three bands, or None), then ``B, H, W``.
    ``lead`` names the leading axis in the messages; ``between(B, H, W)`` runs the caller's own checks after the shape checks and
    before the device check; ``also``: further tensors that must lie on nir's device."""
    if nir.shape != pred.shape or nir.dim() != 4 or nir.shape[1] != 1:
        raise ValueError(f"nir/pred must be equal-shaped [{lead}, 1, H, W] tensors, got {tuple(nir.shape)} and {tuple(pred.shape)}")
    B, _, H, W = nir.shape
    if rgb is not None and (rgb.dim() != 4 or rgb.shape[0] != B or rgb.shape[1] < 3 or tuple(rgb.shape[2:]) != (H, W)):
        raise ValueError(f"rgb must be [{lead}, >=3, H, W] matching nir, got {tuple(rgb.shape)}")
    if between is not None:
        between(B, H, W)
    if (any(t.device != nir.device for t in (pred, *also, *(() if rgb is None else (rgb,))))
            or (nir.device.type != "cuda" and not L.is_emulated())):
        raise RuntimeError("nirgan_hip runs on MI355X (cuda device) only; there is no CPU path")
    n = nir.detach().to(torch.float32).contiguous()
    p = pred.detach().to(torch.float32).contiguous()
    c = None if rgb is None else rgb.detach()[:, :3].to(torch.float32).contiguous()
    return c, n, p, B, H, W


def _centre_window(crop, H, W, clip=False):
    """(y0, x0, ch, cw) of the centred ``crop`` x ``crop`` window (None: the whole image).  Not clipped unless ``clip``: a window
    larger than the image is the entry's error to raise."""
    ch, cw = (H, W) if crop is None else (int(crop), int(crop))
    if clip:
        ch, cw = min(ch, H), min(cw, W)
    return (H - ch) // 2, (W - cw) // 2, ch, cw


def image_metrics_device(pred: torch.Tensor, target: torch.Tensor, window_size: int = 5, max_val: float = 1.0,
                         sigma: float = 1.5, eps: float = 1e-12) -> torch.Tensor:
    """[mean |d|, mean d^2, mean SSIM map] as a 3-element fp32 tensor on the inputs' device (no host sync)."""
    if pred.shape != target.shape or pred.dim() != 4:
        raise ValueError(f"pred/target must be equal-shaped [B, C, H, W] tensors, got {tuple(pred.shape)} and {tuple(target.shape)}")
    if pred.device != target.device or (pred.device.type != "cuda" and not L.is_emulated()):
        raise RuntimeError("nirgan_hip runs on MI355X (cuda device) only; there is no CPU path")
    p = pred.detach().to(torch.float32).contiguous()
    t = target.detach().to(torch.float32).contiguous()
    B, Cc, H, W = p.shape
    be = L.backend()
    ws = torch.empty(int(be.nirgan_image_metrics_ws_elems(B * Cc, H, W)), dtype=torch.float32, device=p.device)
    means = torch.empty(3, dtype=torch.float32, device=p.device)
    d = L.MetricsDesc()
    d.pred, d.target, d.planes, d.H, d.W = p.data_ptr(), t.data_ptr(), B * Cc, H, W
    d.window, d.sigma, d.max_val, d.eps = int(window_size), float(sigma), float(max_val), float(eps)
    d.ws, d.ws_elems, d.means = ws.data_ptr(), ws.numel(), means.data_ptr()
    L.check(be.nirgan_image_metrics(C.byref(d), _stream(p.device)), "image_metrics")
    return means


def _pooled_masked_metrics(pred, target, valid, phase):
    """the four scalars over the valid pixels of the batch: per-tile rows of tile_metrics_masked_device pooled by their counts in
    float64 (tiles with a zero count drop out of their sum; a scalar whose total count is 0 is NaN)"""
    if pred.dim() != 4 or pred.shape[1] != 1 or pred.shape != target.shape:
        raise ValueError(f"calculate_metrics(valid=..) takes equal-shaped [B, 1, H, W] tensors, got {tuple(pred.shape)} and {tuple(target.shape)}")
    rows = tile_metrics_masked_device(None, target, pred, valid, crop=None, window_size=5, patch=0).double()
    col = {k: rows[:, j] for j, k in enumerate(TILE_METRIC_MASKED_COLUMNS)}

    def pooled(name, count):
        keep = count > 0
        total = count[keep].sum()
        return ((col[name][keep] * count[keep]).sum() / total) if bool(total > 0) else rows.new_tensor(float("nan"))
    l1, l2, ssim = (float(v) for v in torch.stack([pooled("l1", col["n_valid"]), pooled("l2", col["n_valid"]),
                                                    pooled("ssim", col["n_ssim"])]).tolist())
    psnr = float("nan") if math.isnan(l2) else (10.0 * math.log10(1.0 / l2) if l2 > 0.0 else float("inf"))
    return {phase + '/L1': l1, phase + '/L2': l2, phase + '/PSNR': psnr, phase + '/SSIM': ssim}


def calculate_metrics(pred, target, phase="train", valid=None):
    """
    Calculate PSNR, SSIM, L1 loss, and L2 loss between pred and target ([B, C, H, W]); dict of floats.
    ``valid`` ([B, 1, H, W] or [B, H, W], != 0 is valid; pred / target [B, 1, H, W] then): the four scalars over the valid pixels
    of the batch -- L1, L2 pooled over the tiles by ``n_valid``, SSIM (window 5) over the support-clean pixels pooled by ``n_ssim``,
    PSNR from the pooled L2; NaN where the batch holds no such pixel.
    """
    if valid is not None:
        return _pooled_masked_metrics(pred, target, valid, phase)
    l1, l2, ssim = image_metrics_device(pred, target, window_size=5, max_val=1.0).tolist()
    psnr = 10.0 * math.log10(1.0 / l2) if l2 > 0.0 else float("inf")
    return {
        phase + '/L1': l1,
        phase + '/L2': l2,
        phase + '/PSNR': psnr,
        phase + '/SSIM': ssim,
    }


# column order of nirgan_tile_metrics rows (include/nirgan_hip.h)
TILE_METRIC_COLUMNS = ("l1", "l2", "ssim", "psnr", "l1_ndvi", "l1_ndwi", "l1_evi", "patch_mean_nir", "patch_mean_pred")
assert len(TILE_METRIC_COLUMNS) == L.TILE_METRIC_COLS


def tile_metrics_device(rgb, nir: torch.Tensor, pred: torch.Tensor, crop=None, window_size: int = 11, patch: int = 32,
                        max_val: float = 1.0, sigma: float = 1.5, eps: float = 1e-12) -> torch.Tensor:
    """One row of ``TILE_METRIC_COLUMNS`` per tile: a ``B x 9`` fp32 tensor on the inputs' device, no host sync.

    ``nir`` / ``pred`` are [B, 1, H, W], ``rgb`` [B, 3, H, W] (more bands are cut to the first three) or ``None``: the three
    index columns are then NaN.  ``crop`` is the side of the centred evaluation window (the reference's
    ``crop_center(.., 240)``; ``None`` = the whole image): SSIM reflects at the window's border, exactly as on a cropped copy,
    but nothing is copied.  ``patch`` is the side of the centred square whose nir / pred means are the last two columns
    (0: NaN); it must fit into the window."""
    c, n, p, B, H, W = _prepare(rgb, nir, pred)
    y0, x0, ch, cw = _centre_window(crop, H, W)
    be = L.backend()
    ws = torch.empty(int(be.nirgan_tile_metrics_ws_elems(B, ch, cw)), dtype=torch.float32, device=n.device)
    rows = torch.full((B, L.TILE_METRIC_COLS), float("nan"), dtype=torch.float32, device=n.device)
    d = L.TileMetricsDesc()
    d.rgb = None if c is None else c.data_ptr()
    d.nir, d.pred, d.B, d.H, d.W = n.data_ptr(), p.data_ptr(), B, H, W
    d.y0, d.x0, d.ch, d.cw = y0, x0, ch, cw
    d.window, d.sigma, d.max_val, d.eps, d.patch = int(window_size), float(sigma), float(max_val), float(eps), int(patch)
    d.ws, d.ws_elems, d.rows = ws.data_ptr(), ws.numel(), rows.data_ptr()
    L.check(be.nirgan_tile_metrics(C.byref(d), _stream(n.device)), "tile_metrics")
    return rows


# column order of nirgan_tile_metrics_masked rows (include/nirgan_hip.h)
TILE_METRIC_MASKED_COLUMNS = TILE_METRIC_COLUMNS + ("n_valid", "n_ssim")
assert len(TILE_METRIC_MASKED_COLUMNS) == L.TILE_METRIC_MASKED_COLS


def tile_metrics_masked_device(rgb, nir: torch.Tensor, pred: torch.Tensor, valid: torch.Tensor, crop=None, window_size: int = 11,
                               patch: int = 32, max_val: float = 1.0, sigma: float = 1.5, eps: float = 1e-12) -> torch.Tensor:
    """One row of ``TILE_METRIC_MASKED_COLUMNS`` per tile over its VALID pixels: a ``B x 11`` fp32 tensor on the inputs' device, no
    host sync (nirgan_tile_metrics_masked).

    ``rgb`` / ``nir`` / ``pred`` / ``crop`` / ``patch`` as in ``tile_metrics_device``.  ``valid`` is [B, 1, H, W] or [B, H, W] of any
    dtype on nir's device: an element ``!= 0`` is valid.  l1, l2, psnr, the index errors and the patch means are means over the valid
    pixels of the window (``n_valid`` of them; NaN with none); ssim is the mean of the SSIM map over the ``n_ssim`` support-clean
    pixels, those whose whole reflected filter support is valid (NaN with none).  Whatever lies in the images at an invalid pixel
    (NaN, Inf, nodata) reaches no output."""
    def own_checks(B, H, W):
        if not torch.is_tensor(valid) or tuple(valid.shape) not in ((B, H, W), (B, 1, H, W)) or valid.is_complex():
            raise ValueError(f"valid must be a [B, 1, H, W] or [B, H, W] tensor matching nir, got {tuple(getattr(valid, 'shape', ()))}")
    c, n, p, B, H, W = _prepare(rgb, nir, pred, between=own_checks, also=(valid,))
    v = valid.detach()
    v = (v if v.dtype == torch.float32 else (v != 0).to(torch.float32)).reshape(B, 1, H, W).contiguous()
    y0, x0, ch, cw = _centre_window(crop, H, W)
    be = L.backend()
    ws = torch.empty(int(be.nirgan_tile_metrics_masked_ws_elems(B, ch, cw)), dtype=torch.float32, device=n.device)
    rows = torch.full((B, L.TILE_METRIC_MASKED_COLS), float("nan"), dtype=torch.float32, device=n.device)
    d = L.TileMetricsMaskedDesc()
    d.rgb = None if c is None else c.data_ptr()
    d.nir, d.pred, d.valid, d.B, d.H, d.W = n.data_ptr(), p.data_ptr(), v.data_ptr(), B, H, W
    d.y0, d.x0, d.ch, d.cw = y0, x0, ch, cw
    d.window, d.sigma, d.max_val, d.eps, d.patch = int(window_size), float(sigma), float(max_val), float(eps), int(patch)
    d.ws, d.ws_elems, d.rows = ws.data_ptr(), ws.numel(), rows.data_ptr()
    L.check(be.nirgan_tile_metrics_masked(C.byref(d), _stream(n.device)), "tile_metrics_masked")
    return rows


# column order of nirgan_window_stats rows (include/nirgan_hip.h)
WINDOW_STAT_COLUMNS = ("mean_nir", "median_nir", "mean_pred", "median_pred",
                       "mean_ndvi_nir", "median_ndvi_nir", "mean_ndvi_pred", "median_ndvi_pred")
assert len(WINDOW_STAT_COLUMNS) == L.WINDOW_STAT_COLS


def window_stats_device(rgb, nir: torch.Tensor, pred: torch.Tensor, y0: int, x0: int, wh: int, ww: int) -> torch.Tensor:
    """One row of ``WINDOW_STAT_COLUMNS`` per tile: a ``T x 8`` fp32 tensor on the inputs' device, no host sync.

    ``nir`` / ``pred`` are [T, 1, H, W], ``rgb`` [T, 3, H, W] (more bands are cut to the first three) or ``None``: the four NDVI
    columns are then NaN.  The window is rows ``y0 .. y0 + wh``, columns ``x0 .. x0 + ww`` of every tile, applied by indexing.
    The medians are ``torch.median`` of the flattened window (the lower middle value of an even count, NaN with any NaN)."""
    c, n, p, T, H, W = _prepare(rgb, nir, pred, lead="T")
    rows = torch.full((T, L.WINDOW_STAT_COLS), float("nan"), dtype=torch.float32, device=n.device)
    d = L.WindowStatsDesc()
    d.rgb = None if c is None else c.data_ptr()
    d.nir, d.pred, d.T, d.H, d.W = n.data_ptr(), p.data_ptr(), T, H, W
    d.y0, d.x0, d.wh, d.ww, d.rows = int(y0), int(x0), int(wh), int(ww), rows.data_ptr()
    L.check(L.backend().nirgan_window_stats(C.byref(d), _stream(n.device)), "window_stats")
    return rows


# column order of nirgan_class_metrics rows (include/nirgan_hip.h)
CLASS_METRIC_COLUMNS = ("count", "l1", "l2", "ssim", "psnr", "l1_ndvi", "l1_ndwi", "l1_evi")
assert len(CLASS_METRIC_COLUMNS) == L.CLASS_METRIC_COLS


def _mask_uint8(mask: torch.Tensor, y0: int, x0: int, ch: int, cw: int) -> torch.Tensor:
    """[B, H, W] class ids of any integer or float dtype as uint8 on the same device.  Only the evaluation window is looked at (and
    converted): ids there must be integral and lie in 0..255.  The check reads one flag back, so a uint8 mask skips it."""
    if mask.dtype == torch.uint8:
        return mask.contiguous()
    if mask.dtype == torch.bool:
        return mask.to(torch.uint8).contiguous()
    B, H, W = mask.shape
    out = torch.zeros((B, H, W), dtype=torch.uint8, device=mask.device)
    if y0 < 0 or x0 < 0 or ch <= 0 or cw <= 0 or y0 + ch > H or x0 + cw > W:
        return out                                          # a bad window is the entry's error to raise
    w = mask[:, y0:y0 + ch, x0:x0 + cw]
    bad = ~((w >= 0) & (w <= 255))                          # a NaN fails both comparisons
    if w.is_floating_point():
        bad |= w != w.floor()
    if bool(bad.any()):
        raise ValueError("mask values inside the evaluation window must be integral class ids in 0..255")
    out[:, y0:y0 + ch, x0:x0 + cw] = w.to(torch.uint8)
    return out


def class_metrics_device(rgb, nir: torch.Tensor, pred: torch.Tensor, mask: torch.Tensor, classes: int = 5, crop=None,
                         window_size: int = 11, max_val: float = 1.0, sigma: float = 1.5, eps: float = 1e-12) -> torch.Tensor:
    """One row of ``CLASS_METRIC_COLUMNS`` per (tile, class): a ``B x classes x 8`` fp32 tensor on the inputs' device.

    ``nir`` / ``pred`` are [B, 1, H, W], ``rgb`` [B, 3, H, W] (more bands are cut to the first three) or ``None``: the three index
    columns are then NaN.  ``mask`` is [B, H, W] or [B, 1, H, W] class ids: uint8 goes to the device entry as it is (no host sync);
    any other integer or float dtype (the reference hands its masks through ``torch.Tensor(..)``) is converted on the device after
    a check that every id inside the evaluation window is integral and in 0..255 (``ValueError`` otherwise; the check reads one
    flag back).  Ids ``>= classes`` belong to no class.  ``crop`` as in ``tile_metrics_device``: the SSIM map is that of the whole
    window, each class takes the mean over its own pixels; a class without pixels has count 0 and NaN elsewhere."""
    def own_checks(B, H, W):
        if not torch.is_tensor(mask) or tuple(mask.shape) not in ((B, H, W), (B, 1, H, W)) or mask.is_complex():
            raise ValueError(f"mask must be a [B, H, W] or [B, 1, H, W] tensor of class ids matching nir, got {tuple(getattr(mask, 'shape', ()))}")
        if not 1 <= int(classes) <= L.CLASS_MAX:
            raise ValueError(f"classes must lie in 1..{L.CLASS_MAX}, got {classes}")
    c, n, p, B, H, W = _prepare(rgb, nir, pred, between=own_checks, also=(mask,))
    y0, x0, ch, cw = _centre_window(crop, H, W)
    m = _mask_uint8(mask.detach().reshape(B, H, W), y0, x0, ch, cw)
    be = L.backend()
    ws = torch.empty(int(be.nirgan_class_metrics_ws_elems(B, ch, cw, int(classes))), dtype=torch.float32, device=n.device)
    rows = torch.full((B, int(classes), L.CLASS_METRIC_COLS), float("nan"), dtype=torch.float32, device=n.device)
    d = L.ClassMetricsDesc()
    d.rgb = None if c is None else c.data_ptr()
    d.nir, d.pred, d.mask, d.B, d.H, d.W = n.data_ptr(), p.data_ptr(), m.data_ptr(), B, H, W
    d.y0, d.x0, d.ch, d.cw = y0, x0, ch, cw
    d.window, d.sigma, d.max_val, d.eps, d.classes = int(window_size), float(sigma), float(max_val), float(eps), int(classes)
    d.ws, d.ws_elems, d.rows = ws.data_ptr(), ws.numel(), rows.data_ptr()
    L.check(be.nirgan_class_metrics(C.byref(d), _stream(n.device)), "class_metrics")
    return rows
