"""The validation figure panels without a GPU: the host logic (utils.logging_helpers, validation_figures, fit(figures_dir=..)) on the
numpy statement of nirgan_val_panel (tests/emu_val_panel.py) against stock numpy / torch (tests/val_panel_cases.py), the argument
checks, workspace size and struct layout of the real library, and the resource usage of the shipped kernels (hipcc cross-compiles).
Bodies shared with tests/test_gpu_val_panel.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import val_panel_cases as Vc
from emu_val_panel import EmuValPanel
from nirgan_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def emu():
    be = EmuValPanel()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.mark.parametrize("case", Vc.CASES, ids=str)
def test_every_output_against_numpy_and_torch(emu, case):
    Vc.panel_case("cpu", case)
    assert emu.calls == ["val_panel"]


@pytest.mark.parametrize("perc,clamp", [(0.0, False), (25.0, True), (2.0, False)], ids=str)
def test_percentiles_and_raw_mode(emu, perc, clamp):
    Vc.panel_case("cpu", ((3, 67, 93), (3, 5, 41, 57)), perc=perc, clamp_rgb=clamp)


def test_histogram_on_the_bin_edges(emu):
    Vc.histogram_edges("cpu")


def test_adversarial_order_statistics(emu):
    Vc.adversarial_quantiles("cpu")


def test_a_nan_stays_in_its_tile(emu):
    Vc.nan_isolation("cpu")


def test_val_stats_device_equals_the_six_torch_reductions(emu):
    Vc.val_stats_case("cpu")
    assert emu.calls == ["val_panel"]


def test_panel_device_host_logic(emu):
    from utils.logging_helpers import PANEL_OUTPUTS, PANEL_STAT_COLUMNS, figure_crop, minmax_percentile, panel_device
    assert L.PANEL_BINS == 100 and len(PANEL_STAT_COLUMNS) == 8
    assert figure_crop(256, 256) == (8, 8, 240, 240) and figure_crop(532, 532) == (16, 16, 500, 500)
    assert figure_crop(64, 72) == (0, 0, 64, 72) and figure_crop(300, 349) == (30, 54, 240, 240) and figure_crop(400, 350) == (0, 0, 400, 350)
    rgb, nir, pred = Vc.inputs((2, 20, 24))
    full = panel_device(rgb, nir, pred, crop=(3, 5, 8, 6))
    assert tuple(full) == PANEL_OUTPUTS and full["rgb_disp"].shape == (2, 8, 6, 3) and full["hist"].dtype == torch.int32
    some = panel_device(rgb, nir, pred, crop=(3, 5, 8, 6), want=("stats", "ndvi_pred_disp"))
    assert tuple(some) == ("stats", "ndvi_pred_disp") and torch.equal(some["stats"], full["stats"])
    no_rgb = panel_device(None, nir, pred, crop=12)                                    # an int: the centred window
    Vc.check_panel(no_rgb, None, nir, pred, (4, 6, 12, 12), what="no rgb")
    five = torch.cat([rgb, nir, pred], dim=1)                                          # more bands are cut to the first three
    assert torch.equal(panel_device(five, nir, pred, want=("rgb_disp",))["rgb_disp"], panel_device(rgb, nir, pred, want=("rgb_disp",))["rgb_disp"])
    with pytest.raises(ValueError):
        panel_device(rgb, nir, pred[:, :, :10])
    with pytest.raises(ValueError):
        panel_device(rgb[:1], nir, pred)
    with pytest.raises(ValueError):
        panel_device(rgb, nir, pred, want=("histogram",))
    for bad in [dict(crop=(13, 0, 8, 4)), dict(crop=(0, 19, 4, 6)), dict(crop=(-1, 0, 4, 4)), dict(crop=(0, 0, 0, 4)), dict(perc=50.0), dict(perc=-1.0)]:
        with pytest.raises(RuntimeError, match="val_panel"):
            panel_device(rgb, nir, pred, **bad)
    # minmax_percentile: per image, every layout the reference passes
    out = minmax_percentile(rgb, perc=2)
    assert out.shape == rgb.shape
    for b in range(2):
        (lo, _), (hi, _) = Vc.quantile_ref(rgb[b].flatten(), 2.0)
        assert (out[b].double() - ((rgb[b].double() - lo) / (hi - lo)).clamp(0, 1)).abs().max().item() < 1e-6
        assert torch.equal(minmax_percentile(rgb[b]), out[b]) and torch.equal(minmax_percentile(rgb[b].permute(1, 2, 0)), out[b].permute(1, 2, 0))
    with pytest.raises(ValueError):
        minmax_percentile(nir)
    L.set_backend(None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        panel_device(rgb, nir, pred)


def _desc(bufs, B=2, H=20, W=24, win=(3, 5, 8, 6), ws=None):
    d = L.ValPanelDesc()
    d.rgb, d.nir, d.pred, d.B, d.H, d.W = bufs["rgb"].data_ptr(), bufs["nir"].data_ptr(), bufs["pred"].data_ptr(), B, H, W
    d.y0, d.x0, d.ch, d.cw = win
    d.gain, d.perc, d.clamp_rgb = 1.5, 2.0, 1
    if ws is not None:
        d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
    return d


def test_emulator_overwrites_skips_null_outputs_and_checks_arguments(emu):
    from utils.logging_helpers import PANEL_OUTPUTS
    rgb, nir, pred = Vc.inputs((2, 20, 24))
    ws = torch.zeros(emu.nirgan_val_panel_ws_bytes(2, 20, 24) // 4, dtype=torch.int32)
    d = _desc({"rgb": rgb, "nir": nir, "pred": pred}, ws=ws)
    outs = {"hist": torch.full((2, 2, 100), 7, dtype=torch.int32), "stats": torch.full((2, 8), 7.0)}
    outs.update({k: torch.full((2, 8, 6), 7.0) for k in ("nir_disp", "pred_disp", "ndvi_nir_disp", "ndvi_pred_disp")})
    outs["rgb_disp"] = torch.full((2, 8, 6, 3), 7.0)
    for k, t in outs.items():
        setattr(d, k, t.data_ptr())
    assert emu.nirgan_val_panel(C.byref(d)) == 0 and all((t != 7).any() for t in outs.values())
    first = {k: t.clone() for k, t in outs.items()}
    assert emu.nirgan_val_panel(C.byref(d)) == 0 and all(torch.equal(outs[k], first[k]) for k in outs)      # OVERWRITTEN, not accumulated
    for t in outs.values():
        t.fill_(7)
    d.rgb = d.ndvi_nir_disp = d.ndvi_pred_disp = d.rgb_disp = d.hist = None
    assert emu.nirgan_val_panel(C.byref(d)) == 0
    assert torch.equal(outs["stats"][:, :6], first["stats"][:, :6]) and (outs["stats"][:, 6:] == 7).all()     # columns 6, 7 untouched without rgb
    assert torch.equal(outs["nir_disp"], first["nir_disp"]) and all((outs[k] == 7).all() for k in ("hist", "rgb_disp", "ndvi_nir_disp"))
    d.rgb_disp = outs["rgb_disp"].data_ptr()
    assert emu.nirgan_val_panel(C.byref(d)) == -1 and b"need rgb" in emu.nirgan_last_error()
    d.rgb_disp, d.rgb = None, rgb.data_ptr()
    for field, value in (("y0", 13), ("x0", -1), ("ch", 0), ("cw", 25), ("nir", None), ("pred", None), ("perc", 50.0), ("perc", -0.5),
                         ("ws", None), ("ws_bytes", ws.numel() * 4 - 4), ("B", 0), ("H", -1)):
        keep = getattr(d, field)
        setattr(d, field, value)
        assert emu.nirgan_val_panel(C.byref(d)) == -1 and b"val_panel" in emu.nirgan_last_error(), field
        setattr(d, field, keep)
    assert emu.nirgan_val_panel(C.byref(d)) == 0 and set(PANEL_OUTPUTS) == set(outs)


def test_real_library_rejects_bad_arguments_before_any_launch_and_sizes_the_workspace_like_the_emulator():
    be, emu = L.backend(), EmuValPanel()
    assert not L.is_emulated()
    for shape in [(1, 5, 5), (3, 67, 93), (5, 256, 256), (1, 532, 532), (2, 2047, 1), (2, 2049, 1), (0, 4, 4), (4, -1, 4), (1, 26755, 26755)]:
        assert be.nirgan_val_panel_ws_bytes(*shape) == emu.nirgan_val_panel_ws_bytes(*shape), shape
    assert be.nirgan_val_panel_ws_bytes(5, 256, 256) == 5 * (9 * 2048 + 32) * 4 + 5 * 32 * 8 * 4 and be.nirgan_val_panel_ws_bytes(1, 26755, 26755) == 0
    assert be.nirgan_val_panel(L.ValPanelDesc(), None) == -1 and b"val_panel" in be.nirgan_last_error()
    buf = torch.zeros(2 * 3 * 20 * 24 + 64)
    ws = torch.zeros(be.nirgan_val_panel_ws_bytes(2, 20, 24) // 4, dtype=torch.int32)
    d = _desc({"rgb": buf, "nir": buf, "pred": buf}, ws=ws)
    d.stats = buf.data_ptr()
    bad = [("y0", 13, b"outside"), ("y0", -1, b"outside"), ("x0", 19, b"outside"), ("x0", -1, b"outside"), ("ch", 18, b"outside"),
           ("cw", 20, b"outside"), ("ch", 0, b"positive"), ("cw", -3, b"positive"), ("nir", None, b"null"), ("pred", None, b"null"),
           ("B", 0, b"empty"), ("H", 0, b"empty"), ("W", -2, b"empty"), ("perc", 50.0, b"perc"), ("perc", -1.0, b"perc"),
           ("perc", float("nan"), b"perc"), ("ws", None, b"workspace"), ("ws_bytes", ws.numel() * 4 - 1, b"workspace"), ("B", 70000, b"65535")]
    for field, value, word in bad:
        keep = getattr(d, field)
        setattr(d, field, value)
        assert be.nirgan_val_panel(d, None) == -1, field
        msg = be.nirgan_last_error()
        assert b"val_panel" in msg and word in msg, (field, msg)
        setattr(d, field, keep)
    d.rgb = None
    for field in ("ndvi_nir_disp", "ndvi_pred_disp", "rgb_disp"):
        setattr(d, field, buf.data_ptr())
        assert be.nirgan_val_panel(d, None) == -1 and b"need rgb" in be.nirgan_last_error(), field
        setattr(d, field, None)


def test_struct_layout_matches_the_header(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
           'printf("%zu %d %d", sizeof(nirgan_val_panel_desc), NIRGAN_PANEL_BINS, NIRGAN_PANEL_STAT_COLS);\n')
    for name, _ in L.ValPanelDesc._fields_:
        src += f'printf(" %zu", offsetof(nirgan_val_panel_desc, {name}));\n'
    src += "return 0;}\n"
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert nums[0] == C.sizeof(L.ValPanelDesc) and nums[1] == L.PANEL_BINS == 100 and nums[2] == L.PANEL_STAT_COLS == 8
    assert nums[3:] == [getattr(L.ValPanelDesc, name).offset for name, _ in L.ValPanelDesc._fields_]


def test_shipped_kernels_use_no_scratch_no_spills_and_fit_the_lds(tmp_path):
    """csrc/valpanel.hip compiled to gfx950 assembly: every kernel in it has zero scratch, zero spilled registers and LDS below a
    CU's 160 KB (read from the kernel descriptors and the metadata; nothing else in the assembly is looked at)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = tmp_path / "valpanel.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-result", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "nir-gan_amd", "csrc", "valpanel.hip"), "-o", str(asm)], check=True, timeout=600)
    text = asm.read_text()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    assert len(names) == 4 and {k for n in names for k in ("first_pass", "select", "finish") if k in n} == {"first_pass", "select", "finish"}
    for name in names:
        desc = text[text.index(".amdhsa_kernel " + name):text.index(".end_amdhsa_kernel", text.index(".amdhsa_kernel " + name))]
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1))
        md = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?.*\.vgpr_spill_count:\s+(\d+)", text)
        sg = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?.*\.sgpr_spill_count:\s+(\d+)", text)
        print(f"{name}: LDS {lds} B, scratch {scratch} B")
        assert scratch == 0 and 0 < lds < 160 * 1024, name
        assert md and int(md.group(1)) == 0 and sg and int(sg.group(1)) == 0, name


def test_plot_functions_return_images(emu):
    Vc.figures_case("cpu")
    assert emu.calls == ["val_panel"] * 3                                             # one entry call per figure
    try:
        from PIL import Image
        from utils.logging_helpers import plot_index
        rgb, nir, pred = Vc.inputs((1, 40, 40))
        assert isinstance(plot_index(rgb, nir, pred, index_name="GNDVI"), Image.Image)
    except ImportError:
        pass


def _px(log_ndvi, num_val_images=1):
    import api_cases as A
    from model.pix2pix import Px2Px_PL
    cfg = A.px_config(6, 8)
    from types import SimpleNamespace as NS
    cfg.custom_configs = NS(Logging=NS(log_ndvi=log_ndvi, num_val_images=num_val_images, log_input_stats=False))
    torch.manual_seed(0)
    return Px2Px_PL(cfg).to("cpu")


def test_validation_figures_asserts_eval_mode_and_returns_the_reference_keys(emu):
    import api_cases as A
    _, val = A._loaders("cpu", n_train=1, n_val=1)
    batch = next(iter(val))
    m = _px(True)
    with pytest.raises(AssertionError, match="eval"):
        m.train().validation_figures(batch)
    figs = m.eval().validation_figures(batch)
    assert list(figs) == ["Images/Val NIR", "Images/Val NDVI"] and emu.calls.count("val_panel") == 2
    for im in figs.values():
        Vc.image_ok(im, 200, 700)
    assert list(_px(False).eval().validation_figures(batch)) == ["Images/Val NIR"]


def test_fit_writes_the_figures_and_is_unchanged_without(emu, tmp_path):
    import api_cases as A
    from nirgan_hip.fit import fit
    train, val = A._loaders("cpu", n_train=1, n_val=2)
    plain = fit(_px(True), train, val, max_epochs=3, log_every=1, device="cpu")
    assert "figures" not in plain and emu.calls.count("val_panel") == 0
    hist = fit(_px(True), train, val, max_epochs=3, log_every=1, device="cpu", figures_dir=str(tmp_path / "figs"), figures_every=2)
    paths = hist.pop("figures")
    assert hist == plain                                                             # the hook changes nothing the loop computes
    want = [f"val_{kind}_e{e}_b0.png" for e in (0, 2) for kind in ("nir", "ndvi")]          # num_val_images = 1 of 2 batches, every 2nd epoch
    assert [os.path.basename(p) for p in paths] == want and sorted(os.listdir(tmp_path / "figs")) == sorted(want)
    assert all(os.path.getsize(p) > 1000 for p in paths)
    only = fit(_px(False, 1), train, val, max_epochs=1, log_every=1, device="cpu", figures_dir=str(tmp_path / "one"))
    assert [os.path.basename(p) for p in only["figures"]] == ["val_nir_e0_b0.png"]


def test_fit_writes_the_figures_of_a_pixel_baseline(emu, tmp_path):
    import api_cases as A
    import baseline_cases as Bc
    from nirgan_hip.fit import fit
    m = Bc.make("linear", 0, "cpu")
    m.config.custom_configs.Logging.num_val_images, m.config.custom_configs.Logging.log_ndvi = 1, True
    train, val = A._loaders("cpu", n_train=1, n_val=2)
    hist = fit(m, train, val, max_epochs=1, log_every=1, device="cpu", figures_dir=str(tmp_path))
    assert [os.path.basename(p) for p in hist["figures"]] == ["val_nir_e0_b0.png", "val_ndvi_e0_b0.png"]
    with pytest.raises(AssertionError, match="eval"):
        m.train().validation_figures(next(iter(val)))
