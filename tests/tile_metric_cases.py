"""Bodies shared by tests/test_tile_metrics_emulated.py (numpy emulator, CPU) and tests/test_gpu_tile_metrics.py (MI355X): the per-tile
metrics table (nirgan_tile_metrics, utils.calculate_metrics.tile_metrics_device, validation_utils.evaluate_tiles) against float64.

Expected values, per tile, on the CROPPED float64 tensors (what the reference's table computes, validation_utils/
spider_validation_callback.py:28-64): oracle ``ssim_map(nir, pred, 11).mean()`` (kornia is not installed: SSIM parity is unpinned
against kornia itself and pinned by the oracle's restatement, as for the batch metrics), ``rs_logging_dict`` for the three index
errors, plain torch for l1 / l2 / psnr / patch means.

Bounds (max-norm relative per column over the tiles, the ``close`` of the existing suites), all taken from existing tests:
  l1 / l2 / ssim      2e-5   what test_gpu_kernels.py::test_image_metrics_kernel holds the batch entry to
  index errors        2e-5   the f3 'logging_dict' check of test_gpu_kernels.py
  psnr                absolute 10 / ln 10 * 2e-5, the error a 2e-5 relative error of l2 implies
  patch means         2e-5   an fp32 mean of <= 1024 values in [0, 1], the same kind of quantity as l1
"""
import math

import torch

import nirgan_oracle as O
from utils.calculate_metrics import TILE_METRIC_COLUMNS, tile_metrics_device

TOL = 2e-5
PSNR_ABS = 10.0 / math.log(10.0) * TOL
INDEX_COLS = ("l1_ndvi", "l1_ndwi", "l1_evi")
# patch side per evaluation-window side: the default 32 where it fits; an odd patch in the odd window; a strict sub-square of 12 x 12
PATCH = {240: 32, 256: 32, 48: 32, 40: 32, 41: 9, 12: 8, 24: 8}


def inputs(shape, seed=11):
    """the bench's ranges: rgb 0.02 + 0.58 U, nir 0.05 + 0.75 U, pred clamp(nir + 0.1 N(0, 1), 0.01, 1)"""
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    rgb = 0.02 + 0.58 * torch.rand(B, 3, H, W, generator=g)
    nir = 0.05 + 0.75 * torch.rand(B, 1, H, W, generator=g)
    pred = (nir + 0.1 * torch.randn(B, 1, H, W, generator=g)).clamp(0.01, 1.0)
    return rgb, nir, pred


def window(t, crop):
    if crop is None:
        return t
    H, W = t.shape[-2:]
    y0, x0 = (H - crop) // 2, (W - crop) // 2
    return t[..., y0:y0 + crop, x0:x0 + crop]


def expected(rgb, nir, pred, crop, patch):
    """float64 rows [B][9] in TILE_METRIC_COLUMNS order, each tile on its own cropped tensors"""
    rows = []
    for b in range(nir.shape[0]):
        c, n, p = (window(t[b:b + 1].double(), crop) for t in (rgb, nir, pred))
        d = n - p
        l2 = (d * d).mean().item()
        rs = O.rs_logging_dict(c, n, p, "l1")
        ch, cw = n.shape[-2:]
        py, px = ch // 2 - patch // 2, cw // 2 - patch // 2
        sq = (slice(None), slice(None), slice(py, py + patch), slice(px, px + patch))
        rows.append([d.abs().mean().item(), l2, O.ssim_map(n, p, 11).mean().item(),
                     10.0 * math.log10(1.0 / l2) if l2 > 0 else float("inf"),
                     rs["indices_loss/ndvi_error"].item(), rs["indices_loss/ndwi_error"].item(), rs["indices_loss/evi_error"].item(),
                     n[sq].mean().item(), p[sq].mean().item()])
    return torch.tensor(rows, dtype=torch.float64)


def close_columns(got, ref, what="", skip=()):
    """every column of ``got`` [B][9] (but those named in ``skip``) against float64 ``ref`` under the bounds of the module docstring;
    prints each figure first"""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for j, name in enumerate(TILE_METRIC_COLUMNS):
        if name in skip:
            continue
        a, b = got[:, j], ref[:, j]
        assert torch.isfinite(a).all(), f"{what} {name}: non-finite"
        err, scale = (a - b).abs().max().item(), b.abs().max().item()
        bound = PSNR_ABS if name == "psnr" else TOL * max(scale, 1e-20)
        print(f"{what} {name}: err {err:.3e} bound {bound:.3e} (scale {scale:.3e})")
        assert err <= bound, f"{what} {name}: err {err:.3e} > {bound:.3e} (scale {scale:.3e})"


def denominators_stay_away_from_zero(shape=(4, 64, 64)):
    """with the ranges of ``inputs`` no index denominator comes near zero, so fp32 against float64 is a fair comparison"""
    rgb, nir, pred = inputs(shape)
    R, G, Bl = rgb[:, 0:1], rgb[:, 1:2], rgb[:, 2:3]
    for v in (nir, pred):
        assert (v + R + 1e-6).min() > 0.03 and (v + G + 1e-6).min() > 0.03
        assert ((v + 6.0) * (R - 7.5) * (Bl + 1.0) + 1e-6).max() < -40.0


def columns_against_float64(dev, shape, crop):
    rgb, nir, pred = inputs(shape)
    side = crop if crop is not None else min(shape[1:])
    patch = PATCH[side]
    got = tile_metrics_device(rgb.to(dev), nir.to(dev), pred.to(dev), crop=crop, window_size=11, patch=patch)
    assert got.shape == (shape[0], len(TILE_METRIC_COLUMNS)) and got.dtype == torch.float32 and got.device.type == torch.device(dev).type
    close_columns(got, expected(rgb, nir, pred, crop, patch), f"{shape} crop {crop}")
    return got


class ScaleModel(torch.nn.Module):
    """a stand-in with the reference's predict_step(rgb, coords): records what it was given"""

    def __init__(self, with_coords=True):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.5, 0.3, 0.4]))
        self.seen, self.with_coords = [], with_coords

    def _pred(self, rgb):
        return (rgb[:, :3] * self.w.view(1, 3, 1, 1)).sum(1, keepdim=True) + 0.05

    def predict_step(self, rgb, coords=None):
        assert not self.training
        self.seen.append((tuple(rgb.shape), None if coords is None else coords.detach().cpu().clone()))
        return self._pred(rgb)


class RgbOnlyModel(ScaleModel):
    def predict_step(self, rgb):                      # the baselines' signature
        assert not self.training
        self.seen.append((tuple(rgb.shape), None))
        return self._pred(rgb)


def samples(shapes, seed=3):
    """a dataset (list of samples): rgb [3,H,W], nir [1,H,W], coords [2]"""
    out = []
    for i, (H, W) in enumerate(shapes):
        rgb, nir, _ = inputs((1, H, W), seed + i)
        out.append({"rgb": rgb[0], "nir": nir[0], "coords": torch.tensor([10.0 + i, -5.0 - i])})
    return out


def table_rows_equal_single_tile_metrics(dev, model, data, table, crop, patch):
    """row i of the table against float64 metrics of predict_step on tile i ALONE"""
    from validation_utils.tile_metrics import TABLE_KEYS
    assert tuple(table) == TABLE_KEYS and table["id"] == list(range(len(data)))
    model.eval()
    got, ref = [], []
    for i, s in enumerate(data):
        rgb, nir = s["rgb"][None], s["nir"][None]
        with torch.no_grad():
            args = (rgb.to(dev), s["coords"][None].to(dev)) if getattr(model, "with_coords", True) else (rgb.to(dev),)
            pred = model.predict_step(*args).float().cpu()
        side = min(crop, *nir.shape[-2:]) if crop is not None else min(nir.shape[-2:])
        ref.append(expected(rgb, nir, pred, crop, min(patch, side))[0])
        got.append([table[k][i] for k in TILE_METRIC_COLUMNS])
        assert table["x"][i] == float(s["coords"][0]) and table["y"][i] == float(s["coords"][1])
    close_columns(torch.tensor(got, dtype=torch.float64), torch.stack(ref), "table")
