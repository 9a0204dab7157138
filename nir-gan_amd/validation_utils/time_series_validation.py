"""The reference's NDVI time series (validation_utils/time_series_validation.py) on the device.

The reference predicts one date per ``predict_step`` call at batch size 1, copies every tensor to the CPU and computes, inside
its plot functions, per date the mean of the centroid patch (:120-132) and the median NDVI of a small shifted window (:249-266)
in a Python loop.  Here the dates go through ``predict_step`` in batches, the stack stays on the device, and
``ndvi_timeline`` returns those numbers from TWO ``utils.calculate_metrics.window_stats_device`` calls (nirgan_window_stats: the
windows by indexing, the medians by exact radix selection) and ONE host copy.  The plot functions keep the reference's
signatures and draw the numbers of ``ndvi_timeline``; their layout follows the reference but is not pixel-exact.

Raster input: ``root_dir`` may match ``.npy`` files (a ``[4+][H][W]`` array) and ``.npz`` files (``img``: that array, optional
``lonlat``: the centroid as (lon, lat)).  ``.tif`` files are read with rasterio where it imports and raise ImportError where it
does not; the ``.tif`` branch is untested in this repository (rasterio is not among its test dependencies).
"""
import glob
import io
import os

import numpy as np
import torch

from utils.calculate_metrics import window_stats_device

from .tile_metrics import _eval_mode, _predict

PLOT_PATCH_SIZE = 64            # the centre crop every plot and the NDVI window refer to (:169, :225)


def _read_raster(path):
    """(img [bands][H][W] as numpy, (lon, lat) or None)"""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        return np.load(path), None
    if ext == ".npz":
        with np.load(path) as z:
            return z["img"], (tuple(float(v) for v in z["lonlat"]) if "lonlat" in z.files else None)
    if ext in (".tif", ".tiff"):
        try:
            import rasterio
            from rasterio.warp import transform
        except ImportError as e:
            raise ImportError(f"{path}: reading .tif needs rasterio, which is not installed; "
                              "store the bands as .npy / .npz ([4+][H][W], optional lonlat) instead") from e
        with rasterio.open(path) as src:                       # :47-57
            img = src.read()
            h, w = img.shape[1], img.shape[2]
            lon, lat = src.transform * (w // 2, h // 2)
            if src.crs and src.crs.to_epsg() != 4326:
                lon, lat = transform(src.crs, "EPSG:4326", [lon], [lat])
                lon, lat = lon[0], lat[0]
            return img, (float(lon), float(lat))
    raise ValueError(f"{path}: unsupported raster format {ext!r} (.npy, .npz, .tif)")


def predict_stack(model, rgbs, coords=None, batch_size=16):
    """``model.predict_step`` over a [T, 3, H, W] stack in batches of ``batch_size``, eval mode under no_grad, the model's
    train / eval mode restored; the result stays on ``rgbs``' device."""
    with _eval_mode(model):
        out = [_predict(model, rgbs[i:i + batch_size], None if coords is None else coords[i:i + batch_size]).float()
               for i in range(0, rgbs.shape[0], int(batch_size))]
    return torch.cat(out)


def get_pred_nirs_and_info(model=None, device=None, root_dir="validation_utils/time_series_bavaria/*.tif", size_input=256,
                           batch_size=16):
    """(rgbs [T,3,h,w], nirs [T,1,h,w], nir_preds [T,1,h,w], timestamps) of the files ``root_dir`` matches (:20-110).

    Files in sorted order, names containing ``SKIP`` dropped, date = ``stem.split("_")[1].split("T")[0]``; the centre crop of
    ``size_input`` clipped to the image, NaN and +-inf set to 0, values / 10000; bands 0-2 are rgb, band 3 is nir.
    ``model is None`` gives ``nir * 1.15`` (the reference's stand-in).  Unlike the reference, the dates go through
    ``predict_step`` in batches of ``batch_size`` and the tensors stay on the device (``device``, else the model's)."""
    if model is not None and device is None:
        device = next(model.parameters()).device
    rgbs, nirs, lonlats, timestamps = [], [], [], []
    for file in sorted(glob.glob(root_dir)):
        stem = file.split("/")[-1].split(".")[0]
        if "SKIP" in stem:
            continue
        timestamps.append(stem.split("_")[1].split("T")[0])
        img, lonlat = _read_raster(file)
        h, w = img.shape[1], img.shape[2]
        half = size_input // 2                                  # :61-65
        cx, cy = w // 2, h // 2
        x1, y1 = max(cx - half, 0), max(cy - half, 0)
        x2, y2 = min(cx + half, w), min(cy + half, h)
        crop = np.nan_to_num(img[:, y1:y2, x1:x2].astype(np.float32), nan=0.0, posinf=0.0, neginf=0.0)
        t = torch.from_numpy(np.ascontiguousarray(crop)) / 10000.0
        rgbs.append(t[:3])
        nirs.append(t[3:4])
        lonlats.append(lonlat)
    if not timestamps:
        raise FileNotFoundError(f"no time-series rasters match {root_dir!r}")
    rgbs, nirs = torch.stack(rgbs), torch.stack(nirs)
    if device is not None:
        rgbs, nirs = rgbs.to(device), nirs.to(device)
    if model is None:
        return rgbs, nirs, nirs * 1.15, timestamps
    model = model.to(device)
    coords = None if any(c is None for c in lonlats) else torch.tensor(lonlats, dtype=torch.float32, device=device)
    return rgbs, nirs, predict_stack(model, rgbs, coords, batch_size), timestamps


def timeline_windows(H, W, mean_patch_size=32, plot_patch_size=PLOT_PATCH_SIZE, shift_x=3, shift_y=10):
    """((y0, x0, wh, ww) of the centroid patch, (y0, x0, wh, ww) of the NDVI window), in coordinates of the full H x W tile."""
    half = mean_patch_size // 2
    cx, cy = W // 2, H // 2                                      # :123-128
    centroid = (cy - half, cx - half, 2 * half, 2 * half)
    # :223-232 -- the reference reads h from the LAST axis and w from the one before; kept (it matters for non-square tiles only)
    h, w = W, H
    cx, cy = w // 2, h // 2
    pp = plot_patch_size // 2
    x1, y1 = max(cx - pp, 0), max(cy - pp, 0)
    x2, y2 = min(cx + pp, w), min(cy + pp, h)
    x2, y2 = min(x2, W), min(y2, H)                              # what slicing does with a bound past the axis
    # :235-236, :250-254 inside the crop
    h, w = y2 - y1, x2 - x1
    cx, cy = w // 2, h // 2
    wx1, wy1 = max(cx - half - shift_x, 0), max(cy - half - shift_y, 0)
    wx2, wy2 = min(cx + half - shift_x, w), min(cy + half - shift_y, h)
    window = (y1 + wy1, x1 + wx1, wy2 - wy1, wx2 - wx1)
    for name, (y0, x0, wh, ww) in (("centroid patch", centroid), ("NDVI window", window)):
        if wh <= 0 or ww <= 0 or y0 < 0 or x0 < 0 or y0 + wh > H or x0 + ww > W:
            raise ValueError(f"{name} y0={y0} x0={x0} {wh}x{ww} is empty or outside the {H}x{W} tile (mean_patch_size={mean_patch_size})")
    return centroid, window


def ndvi_timeline(rgbs, nirs, nir_preds, mean_patch_size=32, plot_patch_size=PLOT_PATCH_SIZE, shift_x=3, shift_y=10):
    """The numbers the reference computes inside its plot functions, per date, as a dict of lists:
    ``centroid_nir`` / ``centroid_pred`` -- means of nir / prediction over the centred ``mean_patch_size`` square of the full
    tile (plot_timeline, :120-132); ``ndvi_true`` / ``ndvi_pred`` -- medians of the NDVI over the shifted window of the centre
    ``plot_patch_size`` crop (plot_ndvi_timeline, :223-266).  The crop is an index offset; two device calls, one host copy."""
    H, W = nirs.shape[-2:]
    centroid, window = timeline_windows(H, W, mean_patch_size, plot_patch_size, shift_x, shift_y)
    a = window_stats_device(None, nirs, nir_preds, *centroid)
    b = window_stats_device(rgbs, nirs, nir_preds, *window)
    rows = torch.cat([a[:, [0, 2]], b[:, [5, 7]]], dim=1).cpu()
    keys = ("centroid_nir", "centroid_pred", "ndvi_true", "ndvi_pred")
    return {k: [float(v) for v in rows[:, j]] for j, k in enumerate(keys)}


def _plt():
    import logging
    import matplotlib
    matplotlib.use("Agg")
    logging.getLogger("matplotlib").setLevel(logging.ERROR)
    import matplotlib.pyplot as plt
    return plt


def _image(plt):
    """the current figure as a PIL image where Pillow imports, else as an H x W x 4 uint8 array"""
    try:
        from PIL import Image
    except ImportError:
        fig = plt.gcf()
        fig.set_dpi(100)
        fig.canvas.draw()
        out = np.asarray(fig.canvas.buffer_rgba()).copy()
        plt.close()
        return out
    buf = io.BytesIO()
    plt.savefig(buf, format="png", dpi=100)
    buf.seek(0)
    out = Image.open(buf).copy()
    plt.close()
    buf.close()
    return out


def _label(t):
    return t[:4] + "-" + t[4:6] + "-" + t[6:]


def _plot_crop(t, plot_patch_size=PLOT_PATCH_SIZE):
    """centre crop of the last two axes for display (:166-173), as a CPU float tensor"""
    h, w = t.shape[-2], t.shape[-1]
    cx, cy, pp = w // 2, h // 2, plot_patch_size // 2
    return t[..., max(cy - pp, 0):min(cy + pp, h), max(cx - pp, 0):min(cx + pp, w)].detach().float().cpu()


def plot_timeline(rgbs, nirs, nir_preds, timestamps, mean_patch_size=32):
    """Timeline of the centroid patch means of NIR and predicted NIR over a row of up to 6 RGB crops (:114-213)."""
    import matplotlib.patches as patches
    plt = _plt()
    tl = ndvi_timeline(rgbs, nirs, nir_preds, mean_patch_size=mean_patch_size)
    n = len(timestamps)
    fig, axs = plt.subplots(2, 1, figsize=(12, 6), gridspec_kw={"height_ratios": [2, 1]})
    axs[0].plot(timestamps, tl["centroid_nir"], marker="o", label="NIR (centroid)", linestyle="-", color="blue")
    axs[0].plot(timestamps, tl["centroid_pred"], marker="s", label="Predicted NIR (centroid)", linestyle="--", color="red")
    axs[0].set_ylabel("NIR Value")
    axs[0].set_xticks(range(n))
    axs[0].set_xticklabels([_label(t) for t in timestamps], rotation=25)
    axs[0].legend()
    axs[0].set_title("NIR vs. Predicted NIR")
    axs[1].axis("off")
    num_images = min(6, n)
    for i, idx in enumerate(np.linspace(0, n - 1, num_images, dtype=int)):
        ax = fig.add_subplot(2, num_images, num_images + i + 1)
        img = np.clip(_plot_crop(rgbs[idx]).permute(1, 2, 0).numpy() * 3.5, 0, 1)
        ax.imshow(img)
        box = PLOT_PATCH_SIZE // 2 - mean_patch_size // 2
        ax.add_patch(patches.Rectangle((box, box), mean_patch_size, mean_patch_size, linewidth=1, edgecolor="red", facecolor="none"))
        ax.set_xticks([])
        ax.set_yticks([])
        ax.set_xlabel(_label(timestamps[idx]), fontsize=10, labelpad=5)
    plt.tight_layout()
    plt.subplots_adjust(hspace=0.5)
    return _image(plt)


def plot_ndvi_timeline(rgbs, nirs, nir_preds, timestamps, mean_patch_size=32):
    """Timeline of the window medians of the true and the predicted NDVI over rows of RGB, NDVI (true) and NDVI (predicted)
    crops (:217-358)."""
    import matplotlib.patches as patches
    from matplotlib.gridspec import GridSpec
    plt = _plt()
    shift_x, shift_y = 3, 10
    tl = ndvi_timeline(rgbs, nirs, nir_preds, mean_patch_size=mean_patch_size, shift_x=shift_x, shift_y=shift_y)
    n = len(timestamps)
    c, t, p = _plot_crop(rgbs), _plot_crop(nirs), _plot_crop(nir_preds)
    red = c[:, 0]
    ndvi = [((v[:, 0] - red) / (v[:, 0] + red + 1e-6) + 1) / 2 for v in (t, p)]      # display stretch (:290-291)
    datasets = [(c * 5).clamp(0, 1), np.clip(ndvi[0].numpy(), 0, 1), ndvi[1].numpy()]
    num_images = min(6, n)
    selected = np.linspace(0, n - 1, num_images, dtype=int)
    fig = plt.figure(figsize=(12, 10))
    gs = GridSpec(4, num_images, height_ratios=[1.8, 1, 1, 1])
    ax = fig.add_subplot(gs[0, :])
    ax.plot(timestamps, tl["ndvi_true"], marker="o", label="NDVI (true)", linestyle="-", color="blue")
    ax.plot(timestamps, tl["ndvi_pred"], marker="s", label="NDVI (pred.)", linestyle="--", color="red")
    ax.set_ylabel("NDVI", fontweight="bold", fontsize=12)
    ax.set_ylim(-1, 1)
    ax.set_xticks(range(n))
    ax.set_xticklabels([_label(s) for s in timestamps], rotation=25)
    ax.legend()
    ax.set_title("NDVI vs. Predicted NDVI over Time")
    ax.tick_params(axis="x", pad=-36, direction="in")
    half = mean_patch_size // 2
    for row, (data, cmap, title) in enumerate(zip(datasets, (None, "viridis", "viridis"), ("RGB", "NDVI (True)", "NDVI (Pred.)"))):
        for col, idx in enumerate(selected):
            ax = fig.add_subplot(gs[row + 1, col])
            img = data[idx]
            if row == 0:
                img = img.permute(1, 2, 0).numpy()
            else:
                span = img.max() - img.min()
                img = (img - img.min()) / (span if span > 0 else 1.0)
            ax.imshow(img, cmap=cmap)
            ax.set_xticks([])
            ax.set_yticks([])
            ax.set_xlabel(_label(timestamps[idx]) if row == 2 else "", fontsize=10)
            ax.add_patch(patches.Rectangle((PLOT_PATCH_SIZE // 2 - half - shift_x, PLOT_PATCH_SIZE // 2 - half - shift_y),
                                           mean_patch_size, mean_patch_size, linewidth=2, edgecolor="red", facecolor="none"))
            if col == 0:
                ax.set_ylabel(title, fontsize=12, rotation=90, labelpad=15, fontweight="bold")
    plt.tight_layout()
    plt.subplots_adjust(hspace=0.05)
    return _image(plt)


def calculate_and_plot_timeline(model=None, device=None, root_dir="validation_utils/time_series_bavaria/*.tif", size_input=256,
                                mean_patch_size=4):
    r, n, p, t = get_pred_nirs_and_info(model, device, root_dir, size_input=size_input)
    return plot_ndvi_timeline(r, n, p, t, mean_patch_size=mean_patch_size)
