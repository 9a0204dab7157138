"""The reference's validation table on the device: one row of metrics per validation tile.

``evaluate_tiles`` restates the loop of validation_utils/get_results_table.py:59-94 and
validation_utils/spider_validation_callback.py:28-64 -- ``pred = model.predict_step(rgb, coords)``, centre crop to 240 x 240,
SSIM (window 11) / PSNR / L1 / L2 and the NDVI / NDWI / EVI L1 errors per tile.  The reference runs it at batch size 1 on CPU
copies; here tiles are batched, the crop is an index window and every batch is ONE fused pass (utils.calculate_metrics.
tile_metrics_device) and ONE host copy.  Two more columns, the nir / pred means of a centred patch, restate the centroid values of
validation_utils/time_series_validation.py:120-132.

Out of scope: the geo-context join of the table (geopandas: geo_ablation.append_info_to_df / clean_economy), the PNG plots,
and data-parallel sharding of the table (every process that calls this evaluates all of ``data``).
"""
import csv
import inspect
import os

import torch

from utils.calculate_metrics import TILE_METRIC_COLUMNS, tile_metrics_device

# the reference's metrics_dict keys in its order, then the two patch means
TABLE_KEYS = ("id", "x", "y", "ssim", "psnr", "l1", "l2", "l1_ndvi", "l1_ndwi", "l1_evi", "patch_mean_nir", "patch_mean_pred")


def _items(data):
    if hasattr(data, "__getitem__") and hasattr(data, "__len__"):
        return (data[i] for i in range(len(data)))
    return iter(data)


def _chunks(data):
    """every item of ``data`` as a batch (rgb [b,C,H,W], nir [b,1,H,W], coords [b,2] or None): samples get a leading axis"""
    for item in _items(data):
        rgb, nir, coords = torch.as_tensor(item["rgb"]), torch.as_tensor(item["nir"]), item.get("coords")
        if coords is not None:
            coords = torch.as_tensor(coords)
        if rgb.dim() == 3:
            rgb, nir = rgb.unsqueeze(0), nir.unsqueeze(0)
            coords = None if coords is None else coords.reshape(1, -1)
        yield rgb, nir, coords


def _batches(data, batch_size):
    """consecutive equal-shaped tiles regrouped into batches of at most ``batch_size``"""
    pend, count = [], 0

    def key(c):
        return (tuple(c[0].shape[1:]), tuple(c[1].shape[1:]), c[2] is None)

    def take(n):
        nonlocal pend, count
        rgb, nir = torch.cat([c[0] for c in pend]), torch.cat([c[1] for c in pend])
        coords = None if pend[0][2] is None else torch.cat([c[2] for c in pend])
        out = (rgb[:n], nir[:n], None if coords is None else coords[:n])
        pend = [(rgb[n:], nir[n:], None if coords is None else coords[n:])] if count > n else []
        count -= n
        return out

    for c in _chunks(data):
        if pend and key(c) != key(pend[0]):
            while count:
                yield take(min(count, batch_size))
        pend.append(c)
        count += c[0].shape[0]
        while count >= batch_size:
            yield take(batch_size)
    while count:
        yield take(min(count, batch_size))


def evaluate_tiles(model, data, crop=240, batch_size=16, device=None, csv_path=None, patch=32):
    """The validation table of ``data`` under ``model``: a dict of lists with the keys ``TABLE_KEYS``, one entry per tile.

    ``data``: a dataset of samples or an iterable of batches, dicts with ``rgb``, ``nir`` and optionally ``coords``
    (x = coords[0], y = coords[1]; NaN without).  ``model.predict_step(rgb, coords)`` is called in eval mode under no_grad
    (a baseline's ``predict_step(rgb)`` is accepted too) and the model's train / eval mode is restored.  ``crop``: side of the
    centred evaluation window (None: the whole tile); ``patch``: side of the centred square of the patch means, cut to the
    window.  ``csv_path``: also write the table there in the layout of the reference's ``DataFrame.to_csv`` (row index first)."""
    device = device or next(model.parameters()).device
    takes_coords = len(inspect.signature(model.predict_step).parameters) >= 2
    table = {k: [] for k in TABLE_KEYS}
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for rgb, nir, coords in _batches(data, int(batch_size)):
                rgb, nir = rgb.to(device), nir.to(device)
                if takes_coords:
                    pred = model.predict_step(rgb, None if coords is None else coords.to(device))
                else:
                    pred = model.predict_step(rgb)
                H, W = nir.shape[-2:]
                side = min(H, W) if crop is None else int(crop)
                rows = tile_metrics_device(rgb, nir, pred, crop=crop, window_size=11, patch=min(int(patch), side)).cpu()
                for i in range(rows.shape[0]):
                    table["id"].append(len(table["id"]))
                    table["x"].append(float("nan") if coords is None else float(coords[i][0]))
                    table["y"].append(float("nan") if coords is None else float(coords[i][1]))
                    for j, name in enumerate(TILE_METRIC_COLUMNS):
                        table[name].append(float(rows[i, j]))
    finally:
        model.train(was_training)
    if csv_path is not None:
        write_csv(table, csv_path)
    return table


def write_csv(table, path):
    folder = os.path.dirname(os.path.abspath(path))
    os.makedirs(folder, exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow([""] + list(TABLE_KEYS))
        for i in range(len(table["id"])):
            w.writerow([i] + [repr(table[k][i]) if isinstance(table[k][i], float) else table[k][i] for k in TABLE_KEYS])


def spider_validation_callback(model, ds, satclip, folder="validation_utils/automated_spiders/", epoch_no=0):
    """The reference's callback (validation_utils/spider_validation_callback.py:13) up to its table: evaluates ``ds`` and writes
    ``<folder>/validation_metrics.csv``; returns the table.  ``satclip`` and ``epoch_no`` only name the reference's GeoJSON,
    which needs the geo-context join and is not written here."""
    return evaluate_tiles(model, ds, crop=240, csv_path=os.path.join(folder, "validation_metrics.csv"))
