"""nirgan_window_stats on the MI355X: the raw medians equal to torch.median as values, means and NDVI medians against float64
(bodies and bounds: tests/time_series_cases.py), adversarial planes for the radix selection, bitwise repeatability and stack
independence, the untouched-column and guard contracts, and validation_utils.ndvi_timeline / fit(time_series=..) on a
small-width Px2Px_PL."""
import ctypes as C

import pytest
import torch

import time_series_cases as Sc
from nirgan_hip import lib as L
from utils.calculate_metrics import window_stats_device

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


@pytest.mark.parametrize("case", Sc.WINDOW_CASES, ids=str)
def test_window_columns_against_torch_median_and_float64(case):
    Sc.window_case(DEV, case)


def test_adversarial_planes_select_what_torch_median_selects():
    Sc.adversarial_medians(DEV)


@pytest.mark.parametrize("shape,win", [((5, 40, 41), (6, 9, 32, 32)), ((5, 70, 93), (3, 21, 65, 67)), ((5, 9, 7), (2, 1, 3, 2))], ids=str)
def test_bitwise_repeatable_and_a_tile_alone_equals_its_row_in_the_stack(shape, win):
    rgb, nir, pred = (t.to(DEV) for t in Sc.inputs(shape))
    a = window_stats_device(rgb, nir, pred, *win)
    b = window_stats_device(rgb, nir, pred, *win)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    for i in range(shape[0]):
        alone = window_stats_device(rgb[i:i + 1], nir[i:i + 1], pred[i:i + 1], *win)
        assert torch.equal(alone[0], a[i]), i
    assert torch.equal(window_stats_device(rgb[1:4], nir[1:4], pred[1:4], *win), a[1:4])


@pytest.mark.parametrize("win", [(6, 0, 64, 64), (3, 21, 65, 67)], ids=str)
def test_null_rgb_leaves_the_ndvi_columns_and_the_guards_around_rows_stay_intact(win):
    rgb, nir, pred = (t.to(DEV).contiguous() for t in Sc.inputs((3, 70, 93)))
    be = L.backend()
    rows_buf = torch.full((GUARD + 3 * 8 + GUARD,), -5.0, device=DEV)
    rows = rows_buf[GUARD:GUARD + 24]
    st = torch.cuda.current_stream().cuda_stream

    def desc(c):
        d = L.WindowStatsDesc()
        d.rgb = None if c is None else c.data_ptr()
        d.nir, d.pred, d.T, d.H, d.W = nir.data_ptr(), pred.data_ptr(), 3, 70, 93
        d.y0, d.x0, d.wh, d.ww, d.rows = *win, rows.data_ptr()
        return d
    L.check(be.nirgan_window_stats(C.byref(desc(rgb)), st), "window_stats")
    full = rows.view(3, 8).clone()
    Sc.rows_close(full, Sc.expected_rows(rgb.cpu(), nir.cpu(), pred.cpu(), *win), "raw entry")
    rows.fill_(-5.0)
    L.check(be.nirgan_window_stats(C.byref(desc(None)), st), "window_stats")
    got = rows.view(3, 8)
    assert torch.equal(got[:, :4], full[:, :4]) and (got[:, 4:] == -5.0).all()
    assert (rows_buf[:GUARD] == -5.0).all() and (rows_buf[GUARD + 24:] == -5.0).all()


@pytest.mark.parametrize("size,patch", [(256, 4), (256, 32), (40, 32)], ids=str)
def test_ndvi_timeline_against_the_restatement(size, patch):
    from validation_utils import ndvi_timeline
    rgb, nir, pred = Sc.inputs((6, size, size), seed=size + patch)
    got = ndvi_timeline(rgb.to(DEV), nir.to(DEV), pred.to(DEV), mean_patch_size=patch)
    Sc.timeline_close(got, Sc.restatement(rgb, nir, pred, patch), f"{size} patch {patch}")


def _small_px2px():
    import api_cases as A
    from model.pix2pix import Px2Px_PL
    torch.manual_seed(0)
    m = Px2Px_PL(A.px_config(6, 8)).to(DEV)
    # an untrained generator's output crosses -red, where the NDVI is singular: lift the output layer's bias so that the
    # prediction stays positive (tanh(~1.5) ~ 0.9) and fp32 against float64 is a fair comparison
    sd = m.state_dict()
    last = [k for k in sd if k.startswith("netG.") and k.endswith(".bias") and sd[k].numel() == 1][-1]
    sd[last] = torch.full_like(sd[last], 1.5)
    m.load_state_dict(sd)
    return m


def test_ndvi_timeline_of_a_small_generators_predictions(tmp_path):
    """six dates written as rasters, read back, predicted in batches by a small define_G generator (ngf 8) and summarised on the
    device, against the restatement applied to the SAME predictions"""
    import numpy as np
    from validation_utils import get_pred_nirs_and_info, ndvi_timeline
    rgb, nir = Sc.date_stack(T=6, size=64)
    for i in range(6):
        np.save(tmp_path / f"S2_2021{i + 1:02d}15T101031_x.npy", (torch.cat([rgb[i], nir[i]]) * 10000.0).numpy())
    m = _small_px2px().train()
    rgbs, nirs, preds, stamps = get_pred_nirs_and_info(m, DEV, str(tmp_path / "*.npy"), size_input=64, batch_size=4)
    assert m.training and stamps == [f"2021{i + 1:02d}15" for i in range(6)]
    assert preds.shape == (6, 1, 64, 64) and preds.device.type == "cuda"
    assert preds.min().item() > 0.3                     # with red >= 0.02 every NDVI denominator is then > 0.32: fp32 against float64 is fair
    assert (rgbs.cpu() - rgb).abs().max().item() < 1e-6
    for patch in (4, 32):
        Sc.timeline_close(ndvi_timeline(rgbs, nirs, preds, mean_patch_size=patch), Sc.restatement(rgbs, nirs, preds, patch), f"generator patch {patch}")


def test_fit_appends_the_timeline_of_the_current_model():
    import api_cases as A
    from nirgan_hip.fit import fit
    from validation_utils.time_series_validation import predict_stack
    m = _small_px2px()
    train, val = A._loaders(DEV, n_train=1, n_val=1)
    rgbs, nirs = Sc.date_stack(T=6, size=64)
    hist = fit(m, train, val, max_epochs=1, log_every=1, device=DEV, time_series=(rgbs, nirs))
    assert len(hist["time_series"]) == 1 and hist["time_series"][0]["epoch"] == 0
    got = {k: v for k, v in hist["time_series"][0].items() if k != "epoch"}
    preds = predict_stack(m, rgbs.to(DEV))
    assert preds.min().item() > 0.3                                                    # one step does not undo the lifted bias
    Sc.timeline_close(got, Sc.restatement(rgbs, nirs, preds), "fit")
