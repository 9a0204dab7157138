"""Bodies shared by tests/test_time_series_emulated.py (numpy emulator, CPU) and tests/test_gpu_time_series.py (MI355X): the
window-statistics entry (nirgan_window_stats, utils.calculate_metrics.window_stats_device) and the NDVI time series built on it
(validation_utils.time_series_validation).

Expected values come from ``restatement``: a float64 restatement of what the reference's validation_utils/
time_series_validation.py computes inside its plot functions -- its slicing, line by line, on float64 copies of the same
tensors (the reference module itself cannot be imported: it imports rasterio at the top, and these numbers never leave its plot
functions).

Bounds:
  raw medians (columns 1, 3)   EQUAL, as values, to torch.median of the same fp32 window (an order statistic is one of the inputs)
  means (columns 0, 2, 4, 6)   2e-5 relative, max-norm per column over the tiles: the bound of tests/tile_metric_cases.py
  NDVI medians (columns 5, 7)  2^-21 * max(1, |median|) against the float64 median.  An order statistic moves by at most the
                               largest perturbation of a value; an fp32 NDVI carries four roundings (n - R, n + R, + 1e-6, the
                               division), each <= 2^-24 relative, and with the bench's ranges (rgb in [0.02, 0.6], nir in
                               [0.05, 0.8]) |ndvi| < 1 and no denominator is near zero: 4 * 2^-24 <= 2^-21 with room.
"""
import numpy as np
import torch

from tile_metric_cases import TOL, inputs            # the bench's ranges; 2e-5
from utils.calculate_metrics import WINDOW_STAT_COLUMNS, window_stats_device

MEDIAN_TOL = 2.0 ** -21
MEAN_COLS, RAW_MEDIAN_COLS, NDVI_MEDIAN_COLS = (0, 2, 4, 6), (1, 3), (5, 7)


def restatement(rgbs, nirs, nir_preds, mean_patch_size=32):
    """float64: {centroid_nir, centroid_pred, ndvi_true, ndvi_pred}, lists per date.  Reference line numbers in comments."""
    rgbs, nirs, nir_preds = (t.detach().double().cpu() for t in (rgbs, nirs, nir_preds))
    num_samples = nirs.shape[0]
    # plot_timeline, :120-132
    _, h, w = nirs.shape[1:]
    cx, cy = w // 2, h // 2
    patch_size = mean_patch_size // 2
    centroid_nirs = [nirs[i, 0, cy - patch_size: cy + patch_size, cx - patch_size: cx + patch_size].mean().item()
                     for i in range(num_samples)]
    centroid_preds = [nir_preds[i, 0, cy - patch_size: cy + patch_size, cx - patch_size: cx + patch_size].mean().item()
                      for i in range(num_samples)]
    # plot_ndvi_timeline, :223-232 (h and w read swapped, as there)
    h, w = rgbs.shape[-1], rgbs.shape[-2]
    cx, cy = w // 2, h // 2
    plot_patch_size = 64
    plot_patch_size_half = plot_patch_size // 2
    x1, y1 = max(cx - plot_patch_size_half, 0), max(cy - plot_patch_size_half, 0)
    x2, y2 = min(cx + plot_patch_size_half, w), min(cy + plot_patch_size_half, h)
    rgbs = rgbs[:, :, y1:y2, x1:x2]
    nirs = nirs[:, :, y1:y2, x1:x2]
    nir_preds = nir_preds[:, :, y1:y2, x1:x2]
    # :235-247
    _, h, w = nirs.shape[1:]
    cx, cy = w // 2, h // 2
    reds = rgbs[:, 0, :, :]

    def compute_ndvi(nir, red):
        return (nir - red) / (nir + red + 1e-6)
    ndvi_true = compute_ndvi(nirs[:, 0, :, :], reds)
    ndvi_pred = compute_ndvi(nir_preds[:, 0, :, :], reds)
    # :250-254, :265-266
    mean_patch_half = mean_patch_size // 2
    shift_x = 3
    shift_y = 10
    x1, y1 = max(cx - mean_patch_half - shift_x, 0), max(cy - mean_patch_half - shift_y, 0)
    x2, y2 = min(cx + mean_patch_half - shift_x, w), min(cy + mean_patch_half - shift_y, h)
    centroid_ndvi_true = [ndvi_true[i, y1:y2, x1:x2].median().item() for i in range(num_samples)]
    centroid_ndvi_pred = [ndvi_pred[i, y1:y2, x1:x2].median().item() for i in range(num_samples)]
    return {"centroid_nir": centroid_nirs, "centroid_pred": centroid_preds, "ndvi_true": centroid_ndvi_true, "ndvi_pred": centroid_ndvi_pred}


def timeline_close(got, ref, what=""):
    """ndvi_timeline's dict against ``restatement``'s under the bounds of the module docstring; prints each figure first"""
    assert tuple(got) == ("centroid_nir", "centroid_pred", "ndvi_true", "ndvi_pred")
    for k in got:
        a, b = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        assert a.shape == b.shape and np.isfinite(a).all(), (what, k)
        err = np.abs(a - b)
        if k.startswith("centroid"):
            bound = np.full_like(b, TOL * max(np.abs(b).max(), 1e-20))
        else:
            bound = MEDIAN_TOL * np.maximum(1.0, np.abs(b))
        print(f"{what} {k}: err {err.max():.3e} bound {bound.min():.3e}")
        assert (err <= bound).all(), f"{what} {k}: err {err.max():.3e} > {bound.min():.3e}"


def expected_rows(rgb, nir, pred, y0, x0, wh, ww):
    """float64 rows [T][8]; the raw medians (columns 1, 3) are torch.median of the fp32 window itself"""
    win = (slice(None), slice(y0, y0 + wh), slice(x0, x0 + ww))
    n32, p32 = nir[:, 0][win].reshape(nir.shape[0], -1), pred[:, 0][win].reshape(nir.shape[0], -1)
    n, p = n32.double(), p32.double()
    cols = [n.mean(1), n32.median(1).values.double(), p.mean(1), p32.median(1).values.double()]
    if rgb is not None:
        R = rgb[:, 0][win].reshape(nir.shape[0], -1).double()
        for v in (n, p):
            idx = (v - R) / (v + R + 1e-6)
            cols += [idx.mean(1), idx.median(1).values]
    else:
        cols += [torch.full_like(cols[0], float("nan"))] * 4
    return torch.stack(cols, dim=1)


def rows_close(got, ref, what=""):
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape == (ref.shape[0], len(WINDOW_STAT_COLUMNS)), (what, got.shape, ref.shape)
    for j in RAW_MEDIAN_COLS:
        same = (got[:, j] == ref[:, j]) | (torch.isnan(got[:, j]) & torch.isnan(ref[:, j]))
        assert same.all(), f"{what} {WINDOW_STAT_COLUMNS[j]}: {got[:, j].tolist()} != torch.median {ref[:, j].tolist()}"
    if torch.isnan(ref[:, 4]).all():
        assert torch.isnan(got[:, 4:]).all(), f"{what}: NDVI columns without rgb"
        mean_cols, median_cols = (0, 2), ()
    else:
        mean_cols, median_cols = MEAN_COLS, NDVI_MEDIAN_COLS
    for j in mean_cols:
        err, scale = (got[:, j] - ref[:, j]).abs().max().item(), ref[:, j].abs().max().item()
        print(f"{what} {WINDOW_STAT_COLUMNS[j]}: err {err:.3e} bound {TOL * max(scale, 1e-20):.3e}")
        assert err <= TOL * max(scale, 1e-20), f"{what} {WINDOW_STAT_COLUMNS[j]}: err {err:.3e} (scale {scale:.3e})"
    for j in median_cols:
        err = (got[:, j] - ref[:, j]).abs()
        bound = MEDIAN_TOL * ref[:, j].abs().clamp(min=1.0)
        print(f"{what} {WINDOW_STAT_COLUMNS[j]}: err {err.max().item():.3e} bound {bound.min().item():.3e}")
        assert (err <= bound).all(), f"{what} {WINDOW_STAT_COLUMNS[j]}: err {err.max().item():.3e}"


# (T, H, W, y0, x0, wh, ww): 1x1, 2x2 (even count: the lower median), 3x3, 4x4, 32x32, 48x48 (more values than a workgroup has
# threads), 64x64 (the largest window staged in LDS) and 65x67 on a 70x93 image (the path that re-reads memory)
WINDOW_CASES = [(T, H, W, y0, x0, wh, ww) for T in (1, 5) for (H, W, y0, x0, wh, ww) in
                [(7, 9, 3, 5, 1, 1), (7, 9, 2, 4, 2, 2), (7, 9, 4, 0, 3, 3), (7, 9, 0, 5, 4, 4), (40, 41, 6, 9, 32, 32),
                 (50, 61, 1, 12, 48, 48), (70, 93, 6, 0, 64, 64), (70, 93, 3, 21, 65, 67)]]


def window_case(dev, case):
    T, H, W, y0, x0, wh, ww = case
    rgb, nir, pred = inputs((T, H, W), seed=5 + wh)
    got = window_stats_device(rgb.to(dev), nir.to(dev), pred.to(dev), y0, x0, wh, ww)
    assert got.dtype == torch.float32 and got.device.type == torch.device(dev).type
    rows_close(got, expected_rows(rgb, nir, pred, y0, x0, wh, ww), str(case))
    return got


def adversarial_planes(H=12, W=11):
    """name -> fp32 plane [H][W] for the selection; the window used on them is rows 1 .. H-1, columns 2 .. W-1"""
    g = torch.Generator().manual_seed(21)
    n = H * W
    out = {"all equal": torch.full((n,), 0.375)}
    out["two values, half each"] = torch.tensor([0.25, 0.75]).repeat(n // 2)[torch.randperm(n, generator=g)]
    base = torch.tensor(0.6).view(torch.int32)
    out["lowest mantissa byte only"] = ((base & ~0xFF) | torch.randint(0, 256, (n,), generator=g, dtype=torch.int32)).view(torch.float32)
    mixed = torch.randn(n, generator=g)
    mixed[::5], mixed[1::7] = -0.0, 0.0
    out["mixed signs with both zeros"] = mixed
    out["zeros of both signs only"] = torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0))
    den = torch.rand(n, generator=g) * 1e-3
    den[::3] = 1e-41                                        # denormal
    den[1::3] = -3e-42
    out["denormals"] = den
    inf = torch.randn(n, generator=g)
    inf[::4], inf[1::4] = float("inf"), float("-inf")
    out["infinities"] = inf
    out["mostly +inf"] = torch.where(torch.rand(n, generator=g) < 0.7, torch.tensor(float("inf")), torch.randn(n, generator=g))
    assert n % 2 == 0
    return {k: v.reshape(H, W).contiguous() for k, v in out.items()}


def adversarial_medians(dev):
    """each plane as its own tile of ONE stack (nir = the plane, pred = its negative), plus one tile with a single NaN: the raw
    medians equal torch.median as values and only the NaN tile gives NaN"""
    planes = adversarial_planes()
    names = list(planes) + ["one NaN"]
    nan = torch.rand(12, 11, generator=torch.Generator().manual_seed(2))
    nan[5, 6] = float("nan")
    nir = torch.stack(list(planes.values()) + [nan])[:, None].contiguous()
    pred = (-nir).contiguous()
    y0, x0, wh, ww = 1, 2, 10, 8
    assert torch.isnan(nir[-1, 0, y0:y0 + wh, x0:x0 + ww]).sum() == 1
    got = window_stats_device(None, nir.to(dev), pred.to(dev), y0, x0, wh, ww).cpu()
    ref = expected_rows(None, nir, pred, y0, x0, wh, ww)
    for i, name in enumerate(names):
        for j in RAW_MEDIAN_COLS:
            a, b = got[i, j].item(), ref[i, j].item()
            print(f"{name} col {j}: {a!r} torch.median {b!r}")
            assert a == b or (a != a and b != b), (name, j, a, b)
        assert (got[i, 1] != got[i, 1]).item() == (name == "one NaN"), name
    return got


def date_stack(T=6, size=64, seed=9):
    rgb, nir, _ = inputs((T, size, size), seed)
    return rgb, nir


class NirModel(torch.nn.Module):
    """a stand-in with the reference's predict_step(rgb, coords): records what it was given"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.5, 0.3, 0.4]))
        self.seen = []

    def predict_step(self, rgb, coords=None):
        assert not self.training
        self.seen.append((tuple(rgb.shape), None if coords is None else coords.detach().cpu().clone()))
        return (rgb[:, :3] * self.w.view(1, 3, 1, 1)).sum(1, keepdim=True) + 0.05
