"""The reference's validation table on the device: one row of metrics per validation tile.

``evaluate_tiles`` restates the loop of validation_utils/get_results_table.py:59-94 and
validation_utils/spider_validation_callback.py:28-64 -- ``pred = model.predict_step(rgb, coords)``, centre crop to 240 x 240,
SSIM (window 11) / PSNR / L1 / L2 and the NDVI / NDWI / EVI L1 errors per tile.  The reference runs it at batch size 1 on CPU
copies; here tiles are batched, the crop is an index window and every batch is ONE fused pass (utils.calculate_metrics.
tile_metrics_device) and ONE host copy.  Two more columns, the nir / pred means of a centred patch, restate the centroid values of
validation_utils/time_series_validation.py:120-132.

The geo-context join of the table (countries, continents, economies, Koeppen classes) is validation_utils/geo_ablation.py, the
radar charts drawn from it validation_utils/plot_val_spiders.py; ``spider_validation_callback`` runs the join and writes the
reference's GeoJSON when it is given the layers.

Out of scope: data-parallel sharding of the table (every process that calls this evaluates all of ``data``).
"""
import contextlib
import csv
import inspect
import os

import torch

from utils.calculate_metrics import TILE_METRIC_COLUMNS, TILE_METRIC_MASKED_COLUMNS, tile_metrics_device, tile_metrics_masked_device

# the reference's metrics_dict keys in its order, then the two patch means
TABLE_KEYS = ("id", "x", "y", "ssim", "psnr", "l1", "l2", "l1_ndvi", "l1_ndwi", "l1_evi", "patch_mean_nir", "patch_mean_pred")
# the masked table (evaluate_tiles(masked=True)): the same columns over the valid pixels of each tile, then the two counts
MASKED_TABLE_KEYS = TABLE_KEYS + ("n_valid", "n_ssim")


def _items(data):
    if hasattr(data, "__getitem__") and hasattr(data, "__len__"):
        return (data[i] for i in range(len(data)))
    return iter(data)


def _chunks(data, extras=(), who="evaluate_tiles"):
    """every item of ``data`` as a batch (rgb [b,C,H,W], nir [b,1,H,W], coords [b,2] or None, then the per-tile planes under the
    keys ``extras`` as [b,H,W]): samples get a leading axis"""
    for item in _items(data):
        rgb, nir, coords = torch.as_tensor(item["rgb"]), torch.as_tensor(item["nir"]), item.get("coords")
        if coords is not None:
            coords = torch.as_tensor(coords)
        if rgb.dim() == 3:
            rgb, nir = rgb.unsqueeze(0), nir.unsqueeze(0)
            coords = None if coords is None else coords.reshape(1, -1)
        more = []
        for key in extras:
            if key not in item:
                raise KeyError(f"{who}: a sample without '{key}'")
            t = torch.as_tensor(item[key])
            more.append(t.reshape(rgb.shape[0], *t.shape[-2:]))
        yield (rgb, nir, coords, *more)


def _batches(data, batch_size, extras=(), who="evaluate_tiles"):
    """consecutive equal-shaped tiles regrouped into batches of at most ``batch_size``; every column of a chunk is cut with its tile"""
    pend, count = [], 0

    def key(c):
        return (tuple(c[0].shape[1:]), tuple(c[1].shape[1:]), c[2] is None)

    def take(n):
        nonlocal pend, count
        cols = [None if col[0] is None else torch.cat(col) for col in zip(*pend)]
        pend = [tuple(None if t is None else t[n:] for t in cols)] if count > n else []
        count -= n
        return tuple(None if t is None else t[:n] for t in cols)

    for c in _chunks(data, extras, who):
        if pend and key(c) != key(pend[0]):
            while count:
                yield take(min(count, batch_size))
        pend.append(c)
        count += c[0].shape[0]
        while count >= batch_size:
            yield take(batch_size)
    while count:
        yield take(min(count, batch_size))


def _predict(model, rgb, coords):
    if len(inspect.signature(model.predict_step).parameters) >= 2:
        return model.predict_step(rgb, coords)
    return model.predict_step(rgb)                              # the baselines' signature


@contextlib.contextmanager
def _eval_mode(model):
    """eval mode under no_grad; the model's train / eval mode is restored"""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        model.train(was_training)


def _predicted_batches(model, data, batch_size, device=None, extras=(), who="evaluate_tiles"):
    """The frame of the evaluation loops: ``data`` regrouped into batches, rgb / nir on ``device`` (default: the model's) and
    ``pred = model.predict_step(rgb, coords)`` (or a baseline's ``predict_step(rgb)``) in eval mode under no_grad.  Yields
    ``(rgb, nir, coords, pred, *extras)`` with coords and the extras as they came (on the host).  Close it (``contextlib.closing``)
    so that the model's mode is restored when the loop ends, however it ends."""
    device = device or next(model.parameters()).device
    with _eval_mode(model):
        for rgb, nir, coords, *more in _batches(data, int(batch_size), extras, who):
            rgb, nir = rgb.to(device), nir.to(device)
            yield (rgb, nir, coords, _predict(model, rgb, None if coords is None else coords.to(device)), *more)


def evaluate_tiles(model, data, crop=240, batch_size=16, device=None, csv_path=None, patch=32, masked=False):
    """The validation table of ``data`` under ``model``: a dict of lists with the keys ``TABLE_KEYS``, one entry per tile.

    ``data``: a dataset of samples or an iterable of batches, dicts with ``rgb``, ``nir`` and optionally ``coords``
    (x = coords[0], y = coords[1]; NaN without).  ``model.predict_step(rgb, coords)`` is called in eval mode under no_grad
    (a baseline's ``predict_step(rgb)`` is accepted too) and the model's train / eval mode is restored.  ``crop``: side of the
    centred evaluation window (None: the whole tile); ``patch``: side of the centred square of the patch means, cut to the
    window.  ``csv_path``: also write the table there in the layout of the reference's ``DataFrame.to_csv`` (row index first).
    ``masked=True``: every sample or batch must carry ``valid`` ([1, H, W] / [b, 1, H, W], != 0 is valid; ``KeyError`` without) and
    the table has the keys ``MASKED_TABLE_KEYS``: every metric over the valid pixels of its tile (tile_metrics_masked_device), SSIM
    over the pixels whose whole filter support is valid, then the counts ``n_valid`` and ``n_ssim``; a metric without pixels is NaN."""
    if masked:
        return _evaluate_tiles_masked(model, data, crop, batch_size, device, csv_path, patch)
    table = {k: [] for k in TABLE_KEYS}
    with contextlib.closing(_predicted_batches(model, data, batch_size, device)) as batches:
        for rgb, nir, coords, pred in batches:
            H, W = nir.shape[-2:]
            side = min(H, W) if crop is None else int(crop)
            rows = tile_metrics_device(rgb, nir, pred, crop=crop, window_size=11, patch=min(int(patch), side)).cpu()
            for i in range(rows.shape[0]):
                table["id"].append(len(table["id"]))
                table["x"].append(float("nan") if coords is None else float(coords[i][0]))
                table["y"].append(float("nan") if coords is None else float(coords[i][1]))
                for j, name in enumerate(TILE_METRIC_COLUMNS):
                    table[name].append(float(rows[i, j]))
    if csv_path is not None:
        write_csv(table, csv_path)
    return table


def _evaluate_tiles_masked(model, data, crop, batch_size, device, csv_path, patch):
    table = {k: [] for k in MASKED_TABLE_KEYS}
    with contextlib.closing(_predicted_batches(model, data, batch_size, device, extras=("valid",))) as batches:
        for rgb, nir, coords, pred, valid in batches:
            H, W = nir.shape[-2:]
            side = min(H, W) if crop is None else int(crop)
            rows = tile_metrics_masked_device(rgb, nir, pred, valid.to(nir.device), crop=crop, window_size=11,
                                              patch=min(int(patch), side)).cpu()
            for i in range(rows.shape[0]):
                table["id"].append(len(table["id"]))
                table["x"].append(float("nan") if coords is None else float(coords[i][0]))
                table["y"].append(float("nan") if coords is None else float(coords[i][1]))
                for j, name in enumerate(TILE_METRIC_MASKED_COLUMNS):
                    table[name].append(float(rows[i, j]))
    if csv_path is not None:
        _write_table(table, MASKED_TABLE_KEYS, csv_path)
    return table


def _write_table(table, keys, path):
    """row index first, floats by repr (they read back exactly)"""
    folder = os.path.dirname(os.path.abspath(path))
    os.makedirs(folder, exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow([""] + list(keys))
        for i in range(len(table["id"])):
            w.writerow([i] + [repr(table[k][i]) if isinstance(table[k][i], float) else table[k][i] for k in keys])


def write_csv(table, path):
    _write_table(table, TABLE_KEYS, path)


def spider_validation_callback(model, ds, satclip, folder="validation_utils/automated_spiders/", epoch_no=0, world=None, koppen=None,
                               legend=None, masked=False):
    """The reference's callback (validation_utils/spider_validation_callback.py:13): evaluates ``ds`` and writes
    ``<folder>/validation_metrics.csv``.  Without ``world`` that is all, and the table is returned.  With ``world`` (a
    ``geo_ablation.PolygonLayer``; ``koppen``: a ``RasterLayer``, ``legend``: its id -> code legend) the table is joined to the
    layers (``append_info_to_df``), its economy column cleaned (``clean_economy``) and written as
    ``<folder>/validation_metrics_ablation_satclip_<satclip>_e<epoch_no>.geojson``, the reference's name; the joined table is
    returned.  ``masked`` is ``evaluate_tiles``'s: the metrics over the valid pixels of each tile of a ``ds`` that carries ``valid``."""
    table = evaluate_tiles(model, ds, crop=240, csv_path=os.path.join(folder, "validation_metrics.csv"), masked=masked)
    if world is None:
        return table
    from .geo_ablation import append_info_to_df, clean_economy, write_geojson
    joined = clean_economy(append_info_to_df(table, world, koppen, legend))
    write_geojson(joined, os.path.join(folder, "validation_metrics_ablation_satclip_" + str(satclip) + "_e" + str(epoch_no) + ".geojson"))
    return joined
