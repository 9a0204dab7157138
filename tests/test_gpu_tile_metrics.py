"""nirgan_tile_metrics on the MI355X: every column against float64 per tile (bodies and bounds: tests/tile_metric_cases.py), bitwise
repeatability and batch independence, the untouched-column and guard contracts, agreement with the existing batch entries, and
validation_utils.evaluate_tiles on a small-width Px2Px_PL."""
import ctypes as C

import pytest
import torch

import tile_metric_cases as Tc
from nirgan_hip import lib as L
from utils.calculate_metrics import TILE_METRIC_COLUMNS, image_metrics_device, tile_metrics_device

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


@pytest.mark.parametrize("shape,crop", [((16, 256, 256), 240), ((64, 256, 256), 240), ((3, 67, 93), 41), ((1, 12, 12), None),
                                        ((5, 276, 276), 256)], ids=str)
def test_columns_against_float64(shape, crop):
    Tc.columns_against_float64(DEV, shape, crop)


def test_bitwise_repeatable_and_a_tile_alone_equals_its_row_in_the_batch():
    rgb, nir, pred = (t.to(DEV) for t in Tc.inputs((64, 256, 256)))
    a = tile_metrics_device(rgb, nir, pred, crop=240)
    b = tile_metrics_device(rgb, nir, pred, crop=240)
    assert torch.equal(a, b)
    for i in (0, 17, 63):
        alone = tile_metrics_device(rgb[i:i + 1], nir[i:i + 1], pred[i:i + 1], crop=240)
        assert torch.equal(alone[0], a[i]), i
    part = tile_metrics_device(rgb[5:21], nir[5:21], pred[5:21], crop=240)
    assert torch.equal(part, a[5:21])
    # odd window with partial blocks
    rgb, nir, pred = (t.to(DEV) for t in Tc.inputs((3, 67, 93)))
    a = tile_metrics_device(rgb, nir, pred, crop=41, patch=9)
    assert torch.equal(tile_metrics_device(rgb[2:3], nir[2:3], pred[2:3], crop=41, patch=9)[0], a[2])


def _desc(rgb, nir, pred, crop, patch, ws, rows):
    B, _, H, W = nir.shape
    d = L.TileMetricsDesc()
    d.rgb = None if rgb is None else rgb.data_ptr()
    d.nir, d.pred, d.B, d.H, d.W = nir.data_ptr(), pred.data_ptr(), B, H, W
    d.y0, d.x0, d.ch, d.cw = (H - crop) // 2, (W - crop) // 2, crop, crop
    d.window, d.sigma, d.max_val, d.eps, d.patch = 11, 1.5, 1.0, 1e-12, patch
    d.ws, d.ws_elems, d.rows = ws.data_ptr(), ws.numel(), rows.data_ptr()
    return d


def test_null_rgb_leaves_the_index_columns_and_guards_around_rows_and_ws_stay_intact():
    rgb, nir, pred = (t.to(DEV).contiguous() for t in Tc.inputs((3, 67, 93)))
    be = L.backend()
    n_ws = int(be.nirgan_tile_metrics_ws_elems(3, 41, 41))
    assert n_ws == 3 * 2 * 2 * 8
    ws_buf = torch.full((GUARD + n_ws + GUARD,), -3.0, device=DEV)
    rows_buf = torch.full((GUARD + 3 * 9 + GUARD,), -5.0, device=DEV)
    ws, rows = ws_buf[GUARD:GUARD + n_ws], rows_buf[GUARD:GUARD + 27]
    st = torch.cuda.current_stream().cuda_stream
    L.check(be.nirgan_tile_metrics(C.byref(_desc(rgb, nir, pred, 41, 9, ws, rows)), st), "tile_metrics")
    full = rows.view(3, 9).clone()
    Tc.close_columns(full, Tc.expected(rgb.cpu(), nir.cpu(), pred.cpu(), 41, 9), "raw entry")
    rows.fill_(-5.0)
    L.check(be.nirgan_tile_metrics(C.byref(_desc(None, nir, pred, 41, 0, ws, rows)), st), "tile_metrics")
    got = rows.view(3, 9)
    assert torch.equal(got[:, :4], full[:, :4]) and (got[:, 4:] == -5.0).all()          # index and patch columns untouched
    for buf, n in ((ws_buf, n_ws), (rows_buf, 27)):
        fill = buf[0].item()
        assert (buf[:GUARD] == fill).all() and (buf[GUARD + n:] == fill).all()


def test_identical_images_give_exact_zeros_infinite_psnr_and_ssim_one():
    rgb, nir, _ = (t.to(DEV) for t in Tc.inputs((4, 256, 256)))
    rows = tile_metrics_device(rgb, nir, nir.clone(), crop=240).cpu()
    col = {k: rows[:, j] for j, k in enumerate(TILE_METRIC_COLUMNS)}
    for k in ("l1", "l2", "l1_ndvi", "l1_ndwi", "l1_evi"):
        assert (col[k] == 0).all(), k
    assert (col["psnr"] == float("inf")).all()
    assert (col["ssim"] - 1).abs().max().item() <= Tc.TOL
    assert torch.equal(col["patch_mean_nir"], col["patch_mean_pred"])


@pytest.mark.parametrize("shape,crop", [((16, 256, 256), 240), ((3, 67, 93), 41)], ids=str)
def test_mean_of_the_rows_equals_the_existing_batch_entries(shape, crop):
    """The batch means the parent's entries give on crop COPIES (image_metrics_device with window 11; the 'logging_dict' of
    RemoteSensingIndices) against the mean of the new entry's rows: the same quantities in another summation order, held to the
    2e-5 the batch entries themselves are held to against float64 (fp32 summation-order noise, no new tolerance)."""
    from utils.remote_sensing_indices import RemoteSensingIndices
    rgb, nir, pred = (t.to(DEV) for t in Tc.inputs(shape))
    rows = tile_metrics_device(rgb, nir, pred, crop=crop, patch=Tc.PATCH[crop]).double().mean(0).cpu()
    c, n, p = (Tc.window(t, crop).contiguous() for t in (rgb, nir, pred))
    batch = image_metrics_device(p, n, window_size=11).double().cpu()
    log = RemoteSensingIndices("loss", "l1").get_and_weight_losses(c, n, p, mode="logging_dict")
    pairs = [("l1", batch[0]), ("l2", batch[1]), ("ssim", batch[2])] + [(f"l1_{k}", log[f"indices_loss/{k}_error"]) for k in ("ndvi", "ndwi", "evi")]
    for name, ref in pairs:
        got, ref = rows[TILE_METRIC_COLUMNS.index(name)].item(), float(ref)
        print(f"{name}: rows mean {got:.9e} batch entry {ref:.9e} rel {abs(got - ref) / abs(ref):.3e}")
        assert abs(got - ref) <= Tc.TOL * abs(ref), name


def test_evaluate_tiles_on_a_small_px2px_pl_equals_single_tile_metrics(tmp_path):
    import api_cases as A
    from model.pix2pix import Px2Px_PL
    from validation_utils import evaluate_tiles
    torch.manual_seed(0)
    m = Px2Px_PL(A.px_config(6, 8)).to(DEV)
    # an untrained generator's output crosses -rgb, where the indices are singular: lift the output layer's bias so that the
    # prediction stays positive (tanh(~1.5) ~ 0.9) and fp32 against float64 is a fair comparison for every column
    sd = m.state_dict()
    last = [k for k in sd if k.startswith("netG.") and k.endswith(".bias") and sd[k].numel() == 1][-1]
    sd[last] = torch.full_like(sd[last], 1.5)
    m.load_state_dict(sd)
    data = Tc.samples([(64, 64)] * 5 + [(48, 80)] * 2)
    m.train()
    table = evaluate_tiles(m, data, crop=40, batch_size=4, device=DEV, csv_path=str(tmp_path / "t.csv"), patch=16)
    assert m.training and (tmp_path / "t.csv").exists()
    m.with_coords = False                       # Px2Px_PL without SatCLIP: predict_step(rgb) on each tile alone
    Tc.table_rows_equal_single_tile_metrics(DEV, m, data, table, 40, 16)
