"""nirgan_val_panel on the MI355X: histograms equal to np.histogram, exact order statistics and percentiles against float64
torch.quantile, min / max / mean, the display planes (bodies and bounds: tests/val_panel_cases.py), NaN isolation, bitwise
repeatability and batch independence, the guard and NULL-output contracts, and the figures end to end on device tensors."""
import ctypes as C

import pytest
import torch

import val_panel_cases as Vc
from nirgan_hip import lib as L
from utils.logging_helpers import PANEL_OUTPUTS, panel_device

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64


@pytest.mark.parametrize("case", Vc.CASES, ids=str)
def test_every_output_against_numpy_and_torch(case):
    Vc.panel_case(DEV, case)


@pytest.mark.parametrize("perc,clamp", [(0.0, False), (0.0, True), (25.0, True), (25.0, False), (2.0, False)], ids=str)
def test_percentiles_and_raw_mode(perc, clamp):
    Vc.panel_case(DEV, ((3, 67, 93), (3, 5, 41, 57)), perc=perc, clamp_rgb=clamp)
    Vc.panel_case(DEV, ((2, 64, 64), (1, 3, 33, 21)), perc=perc, clamp_rgb=clamp)


def test_selection_spread_over_many_workgroups_on_tied_data():
    """256^2 tiles quantised to 1/16: the ranks sit inside long runs of ties and every block of the selection counts them"""
    shape, win = (5, 256, 256), (8, 8, 240, 240)
    rgb, nir, pred = Vc.inputs(shape, seed=11)
    rgb = torch.round(rgb * 16) / 16
    for perc, clamp in ((2.0, False), (25.0, True)):
        got = panel_device(rgb.to(DEV), nir.to(DEV), pred.to(DEV), crop=win, perc=perc, clamp_rgb=clamp)
        Vc.check_panel(got, rgb, nir, pred, win, 1.5, perc, clamp, f"sixteenths perc {perc}")


def test_histogram_on_the_bin_edges():
    Vc.histogram_edges(DEV)


def test_adversarial_order_statistics():
    Vc.adversarial_quantiles(DEV)


def test_a_nan_stays_in_its_tile():
    Vc.nan_isolation(DEV)


@pytest.mark.parametrize("shape,win", [((5, 67, 93), (3, 5, 41, 57)), ((5, 256, 256), (8, 8, 240, 240)), ((5, 5, 5), (1, 1, 3, 3))], ids=str)
def test_bitwise_repeatable_and_a_tile_alone_equals_its_share_of_the_batch(shape, win):
    rgb, nir, pred = (t.to(DEV) for t in Vc.inputs(shape, seed=7))
    a = panel_device(rgb, nir, pred, crop=win, clamp_rgb=False)
    b = panel_device(rgb, nir, pred, crop=win, clamp_rgb=False)
    for k in PANEL_OUTPUTS:
        assert torch.equal(a[k], b[k]) and (k == "hist" or torch.isfinite(a[k]).all()), k
    for i in range(shape[0]):
        alone = panel_device(rgb[i:i + 1], nir[i:i + 1], pred[i:i + 1], crop=win, clamp_rgb=False)
        for k in PANEL_OUTPUTS:
            assert torch.equal(alone[k][0], a[k][i]), (k, i)
    part = panel_device(rgb[1:4], nir[1:4], pred[1:4], crop=win, clamp_rgb=False)
    assert all(torch.equal(part[k], a[k][1:4]) for k in PANEL_OUTPUTS)


@pytest.mark.parametrize("shape,win", [((3, 67, 93), (3, 5, 41, 57)), ((2, 64, 64), (0, 0, 64, 64))], ids=str)
def test_guards_stay_intact_and_null_outputs_are_not_written(shape, win):
    B, H, W = shape
    _, _, ch, cw = win
    rgb, nir, pred = (t.to(DEV).contiguous() for t in Vc.inputs(shape, seed=9))
    be = L.backend()
    st = torch.cuda.current_stream().cuda_stream
    sizes = {"hist": B * 200, "stats": B * 8, "nir_disp": B * ch * cw, "pred_disp": B * ch * cw, "ndvi_nir_disp": B * ch * cw,
             "ndvi_pred_disp": B * ch * cw, "rgb_disp": B * ch * cw * 3}
    bufs = {k: (torch.full((GUARD + n + GUARD,), -5, dtype=torch.int32, device=DEV) if k == "hist" else
                torch.full((GUARD + n + GUARD,), -5.0, device=DEV)) for k, n in sizes.items()}
    ws_bytes = int(be.nirgan_val_panel_ws_bytes(B, H, W))
    ws = torch.full((GUARD + ws_bytes // 4 + GUARD,), -5, dtype=torch.int32, device=DEV)

    def run(names, with_rgb=True):
        d = L.ValPanelDesc()
        d.rgb = rgb.data_ptr() if with_rgb else None
        d.nir, d.pred, d.B, d.H, d.W = nir.data_ptr(), pred.data_ptr(), B, H, W
        d.y0, d.x0, d.ch, d.cw = win
        d.gain, d.perc, d.clamp_rgb = 1.5, 2.0, 1
        d.ws, d.ws_bytes = ws[GUARD:].data_ptr(), ws_bytes
        for k in names:
            setattr(d, k, bufs[k][GUARD:].data_ptr())
        L.check(be.nirgan_val_panel(C.byref(d), st), "val_panel")

    def guards_ok():
        return all((t[:GUARD] == -5).all() and (t[GUARD + sizes[k]:] == -5).all() for k, t in bufs.items()) and \
            (ws[:GUARD] == -5).all() and (ws[GUARD + ws_bytes // 4:] == -5).all()
    run(PANEL_OUTPUTS)
    assert guards_ok()
    shapes = {"hist": (B, 2, 100), "stats": (B, 8), "rgb_disp": (B, ch, cw, 3)}
    full = {k: bufs[k][GUARD:GUARD + sizes[k]].view(shapes.get(k, (B, ch, cw))).clone() for k in PANEL_OUTPUTS}
    Vc.check_panel(full, rgb.cpu(), nir.cpu(), pred.cpu(), win, what="raw entry")
    for names, with_rgb in ((("stats",), True), (("hist", "nir_disp"), False), (("rgb_disp",), True), (("stats", "pred_disp"), False)):
        for t in bufs.values():
            t.fill_(-5)
        run(names, with_rgb)
        assert guards_ok()
        for k in PANEL_OUTPUTS:
            body = bufs[k][GUARD:GUARD + sizes[k]]
            if k not in names:
                assert (body == -5).all(), (names, k)                                  # a NULL output is not written
            elif k == "stats" and not with_rgb:
                got = body.view(B, 8)
                assert torch.equal(got[:, :6], full["stats"][:, :6]) and (got[:, 6:] == -5).all()     # columns 6, 7 untouched without rgb
            else:
                assert torch.equal(body.view(full[k].shape), full[k]), (names, k)


def test_val_stats_device_equals_the_six_torch_reductions():
    Vc.val_stats_case(DEV)
    Vc.val_stats_case(DEV, shape=(2, 256, 256))


def test_plot_functions_return_images_from_device_tensors():
    Vc.figures_case(DEV, size=256, B=2)


def test_validation_figures_of_a_small_generator_and_a_baseline():
    import api_cases as A
    import baseline_cases as Bc
    from types import SimpleNamespace as NS
    from model.pix2pix import Px2Px_PL
    cfg = A.px_config(6, 8)
    cfg.custom_configs = NS(Logging=NS(log_ndvi=True, num_val_images=1, log_input_stats=False))
    torch.manual_seed(0)
    m = Px2Px_PL(cfg).to(DEV).eval()
    _, val = A._loaders(DEV, n_train=1, n_val=1)
    batch = {k: v.to(DEV) for k, v in val[0].items()}
    figs = m.validation_figures(batch)
    assert list(figs) == ["Images/Val NIR", "Images/Val NDVI"]
    for im in figs.values():
        Vc.image_ok(im, 200, 700)
    b = Bc.make("mlp", 0, DEV).eval()
    assert list(b.validation_figures(batch)) == ["Images/Val NIR"]
