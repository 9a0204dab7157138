"""MI355X-native counterpart of the reference's ``utils/logging_helpers.py``: the validation figures.

The reference computes, per image on CPU copies inside its plot functions, a 100-bin ``np.histogram`` of the stretched centre crop,
a 2 % / 98 % percentile stretch of the rgb, NDVI maps, and (model/pix2pix.py:301-309) six min / max / mean scalars.  Here ONE
``nirgan_val_panel`` call per figure leaves all of it on the device for the whole batch (``panel_device``), the plot functions
keep the reference's signatures and titles, draw on the Agg backend from ONE host copy per figure and return the image through
the helper of validation_utils/time_series_validation.py.  The layout follows the reference but is not pixel-exact.

``minmax_percentile`` is this project's reading of the reference's ``data/normalise_s2.py`` (which it does not ship): PER IMAGE,
``clamp((x - lo) / (hi - lo), 0, 1)`` with lo / hi the ``perc``-th and ``(100 - perc)``-th percentile of all of the image's values
(``torch.quantile`` with linear interpolation), 0 where hi == lo.
"""
import ctypes as C

import numpy as np
import torch

from nirgan_hip import lib as L
from utils.calculate_metrics import _centre_window, _prepare, _stream

PANEL_OUTPUTS = ("hist", "stats", "nir_disp", "pred_disp", "ndvi_nir_disp", "ndvi_pred_disp", "rgb_disp")
# column order of nirgan_val_panel stats (include/nirgan_hip.h)
PANEL_STAT_COLUMNS = ("min_nir", "max_nir", "mean_nir", "min_pred", "max_pred", "mean_pred", "rgb_lo", "rgb_hi")
assert len(PANEL_STAT_COLUMNS) == L.PANEL_STAT_COLS
VAL_STATS_KEYS = ("val_stats/min_pred", "val_stats/max_pred", "val_stats/mean_pred",
                  "val_stats/min_input", "val_stats/max_input", "val_stats/mean_input")     # model/pix2pix.py:301-309
MAX_IMAGES = 5


def figure_crop(H, W):
    """(y0, x0, ch, cw) of plot_tensors_hist's centre crop (:79-91): 240 below width 350, else 500; clipped to the image"""
    size = 240 if W < 350 else 500
    ch, cw = min(size, H), min(size, W)
    return (H - ch) // 2, (W - cw) // 2, ch, cw


def _window(crop, H, W):
    if isinstance(crop, (tuple, list)):
        y0, x0, ch, cw = (int(v) for v in crop)
        return y0, x0, ch, cw
    return _centre_window(crop, H, W, clip=True)


def panel_device(rgb, nir: torch.Tensor, pred: torch.Tensor, crop=None, gain: float = 1.5, perc: float = 2.0,
                 clamp_rgb: bool = True, want=PANEL_OUTPUTS) -> dict:
    """The outputs of ONE nirgan_val_panel call named in ``want`` as a dict of tensors on the inputs' device, no host sync.

    ``nir`` / ``pred`` are [B, 1, H, W], ``rgb`` [B, 3, H, W] (more bands are cut to the first three) or ``None``: the outputs
    that need it are then left out and columns 6, 7 of ``stats`` are NaN.  ``crop``: ``None`` = the whole image, an int = the side
    of the centred window (clipped to the image), or ``(y0, x0, ch, cw)``.  ``hist`` [B, 2, 100] int32, ``stats`` [B, 8]
    (``PANEL_STAT_COLUMNS``), ``*_disp`` [B, ch, cw], ``rgb_disp`` [B, ch, cw, 3]."""
    def known_outputs(*_):
        unknown = set(want) - set(PANEL_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown panel outputs {sorted(unknown)}; choose from {PANEL_OUTPUTS}")
    c, n, p, B, H, W = _prepare(rgb, nir, pred, between=known_outputs)
    y0, x0, ch, cw = _window(crop, H, W)
    dev = n.device
    be = L.backend()
    ws = torch.empty(max(int(be.nirgan_val_panel_ws_bytes(B, H, W)), 16) // 4, dtype=torch.int32, device=dev)
    out = {}
    if ch > 0 and cw > 0:                                   # a bad window is the entry's error to raise, not an allocation's
        shapes = {"hist": ((B, 2, L.PANEL_BINS), torch.int32), "stats": ((B, L.PANEL_STAT_COLS), torch.float32),
                  "rgb_disp": ((B, ch, cw, 3), torch.float32)}
        for name in PANEL_OUTPUTS:
            if name in want and (c is not None or name in ("hist", "stats", "nir_disp", "pred_disp")):
                shape, dtype = shapes.get(name, ((B, ch, cw), torch.float32))
                out[name] = torch.full(shape, float("nan"), dtype=dtype, device=dev) if name == "stats" else torch.empty(shape, dtype=dtype, device=dev)
    d = L.ValPanelDesc()
    d.rgb = None if c is None else c.data_ptr()
    d.nir, d.pred, d.B, d.H, d.W = n.data_ptr(), p.data_ptr(), B, H, W
    d.y0, d.x0, d.ch, d.cw = y0, x0, ch, cw
    d.gain, d.perc, d.clamp_rgb = float(gain), float(perc), int(bool(clamp_rgb))
    d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
    for name, t in out.items():
        setattr(d, name, t.data_ptr())
    L.check(be.nirgan_val_panel(C.byref(d), _stream(dev)), "val_panel")
    return out


def minmax_percentile(x: torch.Tensor, perc: float = 2) -> torch.Tensor:
    """Per-image percentile stretch on the device (see the module docstring).  ``x``: [B, 3, H, W], [3, H, W] or, as plot_index
    passes it, [H, W, 3]; the result has ``x``'s layout."""
    if x.dim() == 4:
        c, back = x, lambda t: t.permute(0, 3, 1, 2)
    elif x.dim() == 3 and x.shape[0] == 3:
        c, back = x[None], lambda t: t[0].permute(2, 0, 1)
    elif x.dim() == 3 and x.shape[-1] == 3:
        c, back = x.permute(2, 0, 1)[None], lambda t: t[0]
    else:
        raise ValueError(f"minmax_percentile takes [B, 3, H, W], [3, H, W] or [H, W, 3], got {tuple(x.shape)}")
    if c.shape[1] != 3:
        raise ValueError(f"minmax_percentile takes three channels, got {tuple(x.shape)}")
    plane = c[:, :1]                                        # the entry wants a nir / pred pair; their outputs are not asked for
    return back(panel_device(c, plane, plane, perc=perc, clamp_rgb=False, want=("rgb_disp",))["rgb_disp"])


def val_stats_device(nir: torch.Tensor, pred: torch.Tensor) -> torch.Tensor:
    """The six ``VAL_STATS_KEYS`` values as one fp32 device tensor, no host sync: batch min / max = min / max of the tile values,
    batch mean = mean of the (equal-sized) tiles' means."""
    s = panel_device(None, nir, pred, want=("stats",))["stats"]
    return torch.stack([s[:, 3].min(), s[:, 4].max(), s[:, 5].mean(), s[:, 0].min(), s[:, 1].max(), s[:, 2].mean()])


def _draw():
    from validation_utils.time_series_validation import _image, _plt
    return _plt(), _image


def _host(panel, names, count):
    """ONE host copy: the first ``count`` tiles of the named outputs, flattened into one tensor and cut apart as numpy views"""
    parts = [panel[k][:count] for k in names]
    flat = torch.cat([t.reshape(-1).view(torch.float32) if t.dtype == torch.int32 else t.reshape(-1) for t in parts]).cpu().numpy()
    out, at = {}, 0
    for k, t in zip(names, parts):
        a = flat[at:at + t.numel()].reshape(tuple(t.shape))
        out[k] = a.view(np.int32) if t.dtype == torch.int32 else a
        at += t.numel()
    return out


def _axes(plt, rows, cols, figsize):
    fig, axes = plt.subplots(rows, cols, figsize=figsize)
    return np.expand_dims(axes, 0) if rows == 1 else axes


def plot_tensors(rgb, nir, pred_nir, title="Train"):
    """RGB (clamped, percentile-stretched), NIR and predicted NIR (clamped, RdYlGn), at most 5 images (:9-64)."""
    plt, image = _draw()
    k = min(pred_nir.shape[0], MAX_IMAGES)
    h = _host(panel_device(rgb[:k], nir[:k], pred_nir[:k], gain=1.0, want=("rgb_disp", "nir_disp", "pred_disp")),
              ("rgb_disp", "nir_disp", "pred_disp"), k)
    axes = _axes(plt, k, 3, (15, 5 * k))
    for i in range(k):
        axes[i, 0].imshow(h["rgb_disp"][i])
        axes[i, 1].imshow(h["nir_disp"][i], cmap="RdYlGn")
        axes[i, 2].imshow(h["pred_disp"][i], cmap="RdYlGn")
        if i == 0:
            for ax, name in zip(axes[i], ("RGB Image", "NIR Image", "Predicted NIR Image")):
                ax.set_title(name)
    plt.tight_layout()
    return image(plt)


def plot_tensors_hist(rgb, nir, pred_nir, title="Train"):
    """RGB, NIR, predicted NIR (x 1.5, clamped, viridis) and the 100-bin histogram of both as counts / pixels over the bin centres,
    on the centre crop, at most 5 images (:68-136)."""
    plt, image = _draw()
    k = min(pred_nir.shape[0], MAX_IMAGES)
    names = ("rgb_disp", "nir_disp", "pred_disp", "hist")
    H, W = nir.shape[-2:]
    h = _host(panel_device(rgb[:k], nir[:k], pred_nir[:k], crop=figure_crop(H, W), gain=1.5, perc=2.0, clamp_rgb=True, want=names), names, k)
    axes = _axes(plt, k, 4, (20, 5 * k))
    bins = np.linspace(0, 1, L.PANEL_BINS + 1)
    centers = (bins[:-1] + bins[1:]) / 2
    for i in range(k):
        axes[i, 0].imshow(h["rgb_disp"][i])
        axes[i, 1].imshow(h["nir_disp"][i], cmap="viridis")
        axes[i, 2].imshow(h["pred_disp"][i], cmap="viridis")
        pixels = h["nir_disp"][i].size
        axes[i, 3].plot(centers, h["hist"][i, 0] / pixels, color="blue")
        axes[i, 3].plot(centers, h["hist"][i, 1] / pixels, color="red")
        axes[i, 3].legend(["Real NIR", "Predicted NIR"])
        axes[i, 3].set_xlabel("Pixel Intensity")
        axes[i, 3].set_ylabel("Value Frequency")
        if i == 0:
            for ax, name in zip(axes[i], ("RGB Image", "NIR Image", "Predicted NIR Image", "NIR/ predNIR Histogram")):
                ax.set_title(name)
    plt.tight_layout()
    return image(plt)


def plot_index(rgb, nir, pred_nir, title="Train", index_name="NDVI"):
    """RGB (raw, percentile-stretched), NDVI of the actual and of the predicted NIR (clipped to [-1, 1], stretched to [0, 1], RdYlGn),
    at most 5 images (:139-193).  As in the reference the formula is the NDVI whatever ``index_name`` says: the name titles the panels."""
    plt, image = _draw()
    k = min(pred_nir.shape[0], MAX_IMAGES)
    names = ("rgb_disp", "ndvi_nir_disp", "ndvi_pred_disp")
    h = _host(panel_device(rgb[:k], nir[:k], pred_nir[:k], perc=2.0, clamp_rgb=False, want=names), names, k)
    axes = _axes(plt, k, 3, (15, 5 * k))
    for i in range(k):
        axes[i, 0].imshow(h["rgb_disp"][i])
        axes[i, 0].set_title("RGB Image")
        axes[i, 1].imshow(h["ndvi_nir_disp"][i], cmap="RdYlGn")
        axes[i, 1].set_title(f"{index_name} (Actual)")
        axes[i, 2].imshow(h["ndvi_pred_disp"][i], cmap="RdYlGn")
        axes[i, 2].set_title(f"{index_name} (Predicted)")
    plt.tight_layout()
    return image(plt)


def validation_figures(model, rgb, nir, nir_pred) -> dict:
    """The figures the reference logs from a validation step (model/pix2pix.py:286-298, model/baseline_models.py:43-55):
    ``Images/Val NIR`` always, ``Images/Val NDVI`` with ``custom_configs.Logging.log_ndvi``."""
    out = {"Images/Val NIR": plot_tensors_hist(rgb, nir, nir_pred, title="Val")}
    node = getattr(model, "config", None)
    for name in ("custom_configs", "Logging", "log_ndvi"):
        node = node.get(name) if isinstance(node, dict) else getattr(node, name, None)
    if node:
        out["Images/Val NDVI"] = plot_index(rgb, nir, nir_pred, title="Val")
    return out
