"""Validation against a land-cover mask: how good is the synthetic NIR on water, on vegetation, on built-up land?

The reference ships two figures over a five-class CLC (Corine Land Cover) mask (utils/plot_clc_utils.py, utils/plot_clc_pred.py;
here under the same names in ``utils/``) and no numbers.  ``evaluate_land_cover`` is the table behind that question: the loop of
``evaluate_tiles`` (batched ``predict_step``, the centre crop as an index window) with the metrics split by class id in ONE fused
device pass (utils.calculate_metrics.class_metrics_device) and ONE host copy per batch, one entry per (tile, class) that has pixels.
``summarize_land_cover`` pools the table per class over all tiles, weighting each entry by its pixel count.
"""
import contextlib
import math

import numpy as np

from utils.calculate_metrics import CLASS_METRIC_COLUMNS, _centre_window, _mask_uint8, class_metrics_device

from .tile_metrics import _predicted_batches, _write_table

# the legend of the reference's two figures, ids 0..4
CLC_CLASSES = ("none", "agricultural", "natural vegetation", "water", "artificial")
CLC_COLORS = ("#ffffff", "#90ee90", "#006400", "#1e90ff", "#ff0000")       # white, light green, dark green, blue, red

METRIC_KEYS = ("ssim", "psnr", "l1", "l2", "l1_ndvi", "l1_ndwi", "l1_evi")
LAND_COVER_KEYS = ("id", "x", "y", "class_id", "class_name", "count") + METRIC_KEYS
SUMMARY_KEYS = ("class_id", "class_name", "count") + METRIC_KEYS


def evaluate_land_cover(model, data, classes=CLC_CLASSES, crop=240, batch_size=16, device=None, csv_path=None, mask_key="mask"):
    """The land-cover table of ``data`` under ``model``: a dict of lists with the keys ``LAND_COVER_KEYS``, one entry per
    (tile, class) with ``count > 0``, tiles in order, classes in id order.

    ``data`` as for ``evaluate_tiles``, every sample (or batch) with a class-id mask ([H, W] or [1, H, W]; batches with a leading
    axis) under ``mask_key``.  ``classes``: the class names, id = position (at most 8); ids past the last name are counted nowhere.
    ``model.predict_step(rgb, coords)`` (or a baseline's ``predict_step(rgb)``) runs in eval mode under no_grad and the model's
    mode is restored.  ``crop``: side of the centred evaluation window (None: the whole tile).  ``csv_path``: also write the table
    there, row index first."""
    names = tuple(classes)
    table = {k: [] for k in LAND_COVER_KEYS}
    tile = 0
    with contextlib.closing(_predicted_batches(model, data, batch_size, device, (mask_key,), "evaluate_land_cover")) as batches:
        for rgb, nir, coords, pred, mask in batches:
            mask = _mask_uint8(mask, *_centre_window(crop, *nir.shape[-2:]))      # checked where it lies: no device read-back
            rows = class_metrics_device(rgb, nir, pred, mask.to(rgb.device), classes=len(names), crop=crop, window_size=11).cpu()
            for i in range(rows.shape[0]):
                for c, name in enumerate(names):
                    if rows[i, c, 0] > 0:
                        table["id"].append(tile)
                        table["x"].append(float("nan") if coords is None else float(coords[i][0]))
                        table["y"].append(float("nan") if coords is None else float(coords[i][1]))
                        table["class_id"].append(c)
                        table["class_name"].append(name)
                        table["count"].append(int(rows[i, c, 0]))
                        for j, key in enumerate(CLASS_METRIC_COLUMNS[1:], start=1):
                            table[key].append(float(rows[i, c, j]))
                tile += 1
    if csv_path is not None:
        write_land_cover_csv(table, csv_path)
    return table


def write_land_cover_csv(table, path):
    """the layout of tile_metrics.write_csv"""
    _write_table(table, LAND_COVER_KEYS, path)


def summarize_land_cover(table, max_val=1.0):
    """Per class over all tiles, in float64: a dict of lists with the keys ``SUMMARY_KEYS``, one entry per class id present in
    ``table`` in id order.  ``count`` is the class's pixel count, every mean is sum(count * value) / sum(count) -- the mean over all
    of the class's pixels -- and psnr is recomputed from the pooled l2 (+inf at 0)."""
    ids = np.asarray(table["class_id"], dtype=np.int64)
    count = np.asarray(table["count"], dtype=np.float64)
    out = {k: [] for k in SUMMARY_KEYS}
    for c in sorted(set(ids.tolist())):
        sel = ids == c
        n = count[sel].sum()
        out["class_id"].append(int(c))
        out["class_name"].append(table["class_name"][int(np.flatnonzero(sel)[0])])
        out["count"].append(int(n))
        pooled = {k: float((count[sel] * np.asarray(table[k], dtype=np.float64)[sel]).sum() / n) for k in METRIC_KEYS if k != "psnr"}
        pooled["psnr"] = 10.0 * math.log10(max_val * max_val / pooled["l2"]) if pooled["l2"] > 0 else float("inf")
        for k in METRIC_KEYS:
            out[k].append(pooled[k])
    return out
