"""The NDVI time series without a GPU: the host logic (utils.calculate_metrics.window_stats_device, validation_utils.
time_series_validation, fit(time_series=..)) on the numpy statement of nirgan_window_stats (tests/emu_time_series.py) against the
float64 restatement of the reference's script (tests/time_series_cases.py), the argument checks and struct layout of the real
library, and the resource usage of the shipped kernel (hipcc cross-compiles).  Bodies shared with tests/test_gpu_time_series.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import time_series_cases as Sc
from emu_time_series import EmuTimeSeries
from nirgan_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def emu():
    be = EmuTimeSeries()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.mark.parametrize("case", Sc.WINDOW_CASES, ids=str)
def test_window_columns_against_torch_median_and_float64(emu, case):
    Sc.window_case("cpu", case)
    assert emu.calls == ["window_stats"]


def test_adversarial_planes_select_what_torch_median_selects(emu):
    Sc.adversarial_medians("cpu")


def test_columns_without_rgb_are_nan_and_bad_arguments_raise(emu):
    from utils.calculate_metrics import WINDOW_STAT_COLUMNS, window_stats_device
    assert WINDOW_STAT_COLUMNS == ("mean_nir", "median_nir", "mean_pred", "median_pred",
                                   "mean_ndvi_nir", "median_ndvi_nir", "mean_ndvi_pred", "median_ndvi_pred")
    rgb, nir, pred = Sc.inputs((2, 20, 24))
    full = window_stats_device(rgb, nir, pred, 3, 5, 8, 6)
    rows = window_stats_device(None, nir, pred, 3, 5, 8, 6)
    assert torch.equal(rows[:, :4], full[:, :4]) and torch.isnan(rows[:, 4:]).all() and torch.isfinite(full).all()
    with pytest.raises(ValueError):
        window_stats_device(rgb, nir, pred[:, :, :10], 0, 0, 4, 4)
    with pytest.raises(ValueError):
        window_stats_device(rgb[:1], nir, pred, 0, 0, 4, 4)
    for bad in [(13, 0, 8, 4), (0, 19, 4, 6), (-1, 0, 4, 4), (0, 0, 0, 4), (0, 0, 4, -2), (0, 0, 21, 4)]:
        with pytest.raises(RuntimeError, match="window_stats"):
            window_stats_device(rgb, nir, pred, *bad)
    L.set_backend(None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        window_stats_device(rgb, nir, pred, 3, 5, 8, 6)


def test_emulator_overwrites_and_leaves_the_ndvi_columns_without_rgb(emu):
    rgb, nir, pred = Sc.inputs((2, 20, 24))
    rows = torch.full((2, 8), 7.0)
    d = L.WindowStatsDesc()
    d.rgb, d.nir, d.pred, d.T, d.H, d.W = rgb.data_ptr(), nir.data_ptr(), pred.data_ptr(), 2, 20, 24
    d.y0, d.x0, d.wh, d.ww, d.rows = 3, 5, 8, 6, rows.data_ptr()
    assert emu.nirgan_window_stats(C.byref(d)) == 0 and (rows != 7).all()
    first = rows.clone()
    assert emu.nirgan_window_stats(C.byref(d)) == 0 and torch.equal(rows, first)         # OVERWRITTEN, not accumulated
    rows.fill_(7.0)
    d.rgb = None
    assert emu.nirgan_window_stats(C.byref(d)) == 0 and torch.equal(rows[:, :4], first[:, :4]) and (rows[:, 4:] == 7).all()
    for field, value in (("y0", 13), ("x0", -1), ("wh", 0), ("ww", 25), ("nir", None), ("pred", None), ("rows", None)):
        keep = getattr(d, field)
        setattr(d, field, value)
        assert emu.nirgan_window_stats(C.byref(d)) == -1 and b"window_stats" in emu.nirgan_last_error(), field
        setattr(d, field, keep)


def test_real_library_rejects_bad_arguments_before_any_launch():
    be = L.backend()
    assert not L.is_emulated()
    assert be.nirgan_window_stats(L.WindowStatsDesc(), None) == -1 and b"window_stats" in be.nirgan_last_error()
    buf = torch.zeros(3 * 20 * 24 + 64)
    d = L.WindowStatsDesc()
    d.rgb = d.nir = d.pred = d.rows = buf.data_ptr()
    d.T, d.H, d.W, d.y0, d.x0, d.wh, d.ww = 1, 20, 24, 3, 5, 8, 6
    bad = [("y0", 13, b"outside"), ("y0", -1, b"outside"), ("x0", 19, b"outside"), ("x0", -1, b"outside"), ("wh", 18, b"outside"),
           ("ww", 20, b"outside"), ("wh", 0, b"positive"), ("ww", -3, b"positive"), ("nir", None, b"null"), ("pred", None, b"null"),
           ("rows", None, b"null"), ("T", 0, b"empty"), ("H", 0, b"empty")]
    for field, value, word in bad:
        keep = getattr(d, field)
        setattr(d, field, value)
        assert be.nirgan_window_stats(d, None) == -1, field
        msg = be.nirgan_last_error()
        assert b"window_stats" in msg and word in msg, (field, msg)
        setattr(d, field, keep)


def test_struct_layout_matches_the_header(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
           'printf("%zu %d", sizeof(nirgan_window_stats_desc), NIRGAN_WINDOW_STAT_COLS);\n')
    for name, _ in L.WindowStatsDesc._fields_:
        src += f'printf(" %zu", offsetof(nirgan_window_stats_desc, {name}));\n'
    src += "return 0;}\n"
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert nums[0] == C.sizeof(L.WindowStatsDesc) and nums[1] == L.WINDOW_STAT_COLS == 8
    assert nums[2:] == [getattr(L.WindowStatsDesc, name).offset for name, _ in L.WindowStatsDesc._fields_]


def test_shipped_kernel_uses_no_scratch_no_spills_and_fits_the_lds(tmp_path):
    """csrc/windowstats.hip compiled to gfx950 assembly: the kernel spills nothing, uses no scratch, counts with integer LDS
    atomics and no global atomics, and its LDS (4096 staged keys + the histogram) stays under a CU's 160 KB."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = tmp_path / "windowstats.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-result", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "nir-gan_amd", "csrc", "windowstats.hip"), "-o", str(asm)], check=True, timeout=600)
    text = asm.read_text()
    name = next(n for n in re.findall(r"^(_Z\w+):", text, re.M) if "window_stats_kernel" in n)
    body = text.split("\n" + name + ":", 1)[1].split(".Lfunc_end", 1)[0]
    assert not re.search(r"^\s*scratch_", body, re.M)
    assert not re.search(r"^\s*(global|flat)_atomic", body, re.M)
    assert re.search(r"^\s*ds_add_u32", body, re.M)
    desc = text[text.index(".amdhsa_kernel " + name):text.index(".end_amdhsa_kernel", text.index(".amdhsa_kernel " + name))]
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1))
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1))
    print(f"window_stats kernel: LDS {lds} B, scratch {scratch} B")
    assert scratch == 0 and 4096 * 4 < lds < 160 * 1024
    md = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?.*\.vgpr_spill_count:\s+(\d+)", text)
    assert md and int(md.group(1)) == 0


def test_window_arithmetic_of_the_reference():
    from validation_utils.time_series_validation import timeline_windows
    assert timeline_windows(256, 256, 32) == ((112, 112, 32, 32), (102, 109, 32, 32))
    assert timeline_windows(256, 256, 4) == ((126, 126, 4, 4), (116, 123, 4, 4))
    assert timeline_windows(40, 40, 32) == ((4, 4, 32, 32), (0, 1, 26, 32))           # the shifted window clips at row 0
    assert timeline_windows(40, 40, 4) == ((18, 18, 4, 4), (8, 15, 4, 4))
    with pytest.raises(ValueError, match="centroid patch"):
        timeline_windows(20, 20, 32)


@pytest.mark.parametrize("size,patch", [(256, 4), (256, 32), (40, 32), (40, 4)], ids=str)
def test_ndvi_timeline_against_the_restatement(emu, size, patch):
    from validation_utils import ndvi_timeline
    rgb, nir, pred = Sc.inputs((3, size, size), seed=size + patch)
    got = ndvi_timeline(rgb, nir, pred, mean_patch_size=patch)
    assert emu.calls == ["window_stats", "window_stats"]                               # two device calls
    Sc.timeline_close(got, Sc.restatement(rgb, nir, pred, patch), f"{size} patch {patch}")
    assert all(isinstance(v, float) for k in got for v in got[k]) and all(len(got[k]) == 3 for k in got)


def _write_stack(folder, with_lonlat=False, width=52):
    """five dates written out of order, one of them marked SKIP; returns the kept (date, array) pairs in sorted order"""
    g = np.random.default_rng(4)
    kept = []
    for i, (stem, size) in enumerate([("S2_20210703T101031_x", 48), ("S2_20210105T101031_x", 48), ("S2_20210410T101031_SKIP", 48),
                                      ("S2_20210922T101031_x", 48), ("S2_20210301T101031_x", 48)]):
        img = g.uniform(200.0, 6000.0, size=(5, size, width)).astype(np.float32)       # a fifth band that is ignored
        img[0, 10, 11], img[3, 20, 21], img[1, 30, 31] = np.nan, np.inf, -np.inf
        if with_lonlat:
            np.savez(folder / f"{stem}.npz", img=img, lonlat=np.array([11.0 + i, 48.0 - i]))
        else:
            np.save(folder / f"{stem}.npy", img)
        if "SKIP" not in stem:
            kept.append((stem.split("_")[1][:8], img, (11.0 + i, 48.0 - i)))
    return sorted(kept, key=lambda t: t[0])


def test_get_pred_nirs_and_info_reads_sorts_skips_crops_and_scales(tmp_path):
    from validation_utils import get_pred_nirs_and_info
    kept = _write_stack(tmp_path)
    rgbs, nirs, preds, stamps = get_pred_nirs_and_info(None, None, str(tmp_path / "*.npy"), size_input=32)
    assert stamps == ["20210105", "20210301", "20210703", "20210922"] == [k[0] for k in kept]
    assert rgbs.shape == (4, 3, 32, 32) and nirs.shape == preds.shape == (4, 1, 32, 32) and rgbs.dtype == torch.float32
    for i, (_, img, _) in enumerate(kept):                                           # centre crop 32 of 48 x 52: rows 8.., columns 10..
        ref = torch.from_numpy(np.nan_to_num(img[:, 8:40, 10:42], nan=0.0, posinf=0.0, neginf=0.0)) / 10000.0
        assert torch.equal(rgbs[i], ref[:3]) and torch.equal(nirs[i], ref[3:4])
    assert nirs[0, 0, 12, 11] == 0 and rgbs[0, 0, 2, 1] == 0 and rgbs[0, 1, 22, 21] == 0        # inf, NaN, -inf -> 0
    assert torch.equal(preds, nirs * 1.15)                                           # model=None
    whole = get_pred_nirs_and_info(None, None, str(tmp_path / "*.npy"), size_input=256)[0]
    assert whole.shape == (4, 3, 48, 52)                                             # the crop is clipped to the image
    with pytest.raises(FileNotFoundError):
        get_pred_nirs_and_info(None, None, str(tmp_path / "*.nothing"))
    (tmp_path / "S2_20210101T000000_x.tif").write_bytes(b"II*\0")
    with pytest.raises(ImportError, match="rasterio"):
        get_pred_nirs_and_info(None, None, str(tmp_path / "*.tif"))


def test_get_pred_nirs_and_info_predicts_in_batches_and_restores_the_mode(tmp_path):
    from validation_utils import get_pred_nirs_and_info
    kept = _write_stack(tmp_path, with_lonlat=True)
    m = Sc.NirModel().train()
    rgbs, nirs, preds, stamps = get_pred_nirs_and_info(m, "cpu", str(tmp_path / "*.npz"), size_input=32, batch_size=3)
    assert m.training and len(stamps) == 4
    assert [s for s, _ in m.seen] == [(3, 3, 32, 32), (1, 3, 32, 32)]
    assert torch.equal(torch.cat([c for _, c in m.seen]), torch.tensor([k[2] for k in kept], dtype=torch.float32))
    m.eval()
    assert torch.equal(preds, torch.cat([m.predict_step(rgbs[i:i + 1]) for i in range(4)]).detach())
    get_pred_nirs_and_info(m, None, str(tmp_path / "*.npz"), size_input=32)
    assert not m.training and m.seen[-1][0] == (4, 3, 32, 32)                        # default batch size 16: one call


def test_plot_functions_return_an_image(emu, tmp_path):
    from validation_utils import calculate_and_plot_timeline, plot_ndvi_timeline, plot_timeline
    rgb, nir, pred = Sc.inputs((7, 72, 72))
    stamps = [f"202101{d:02d}" for d in range(1, 8)]
    _write_stack(tmp_path)
    images = [plot_timeline(rgb, nir, pred, stamps, mean_patch_size=32), plot_ndvi_timeline(rgb, nir, pred, stamps, mean_patch_size=4),
              calculate_and_plot_timeline(None, None, str(tmp_path / "*.npy"), size_input=48)]
    assert emu.calls.count("window_stats") == 6
    for im in images:
        a = np.asarray(im)
        assert a.ndim == 3 and a.shape[2] == 4 and a.dtype == np.uint8 and a.shape[0] >= 400 and a.shape[1] >= 800
        assert a[..., :3].std() > 0                                                   # something was drawn
    try:
        from PIL import Image
        assert all(isinstance(im, Image.Image) for im in images)
    except ImportError:
        pass


def test_fit_appends_the_timeline_and_is_unchanged_without(emu, tmp_path):
    import api_cases as A
    from model.pix2pix import Px2Px_PL
    from nirgan_hip.fit import fit
    from validation_utils.time_series_validation import predict_stack
    cfg = A.px_config(6, 8)

    def fresh():
        torch.manual_seed(0)
        return Px2Px_PL(cfg).to("cpu")
    train, val = A._loaders("cpu", n_train=1, n_val=1)
    plain = fit(fresh(), train, val, max_epochs=3, log_every=1, device="cpu")
    assert "time_series" not in plain and emu.calls.count("window_stats") == 0
    rgbs, nirs = Sc.date_stack(T=5, size=40)
    m = fresh()
    hist = fit(m, train, val, max_epochs=3, log_every=1, device="cpu", time_series=(rgbs, nirs), time_series_every=2)
    ts = hist.pop("time_series")
    assert hist == plain                                                             # the hook changes nothing the loop computes
    assert [e["epoch"] for e in ts] == [0, 2] and emu.calls.count("window_stats") == 4
    assert sorted(ts[0]) == ["centroid_nir", "centroid_pred", "epoch", "ndvi_pred", "ndvi_true"] and len(ts[0]["ndvi_true"]) == 5
    # the last entry describes the model as it is now; an untrained generator's output crosses -red, where the NDVI is singular,
    # so the prediction-side medians are compared on conditioned data (above, and on the GPU)
    last = {k: v for k, v in ts[-1].items() if k != "epoch"}
    ref = Sc.restatement(rgbs, nirs, predict_stack(m, rgbs))
    for k in ("centroid_nir", "centroid_pred", "ndvi_true"):
        Sc.timeline_close({kk: (last[kk] if kk == k else ref[kk]) for kk in last}, ref, f"fit {k}")
    # a glob works the same way
    _write_stack(tmp_path, width=48)
    g = fit(fresh(), train, val, max_epochs=1, log_every=1, device="cpu", time_series=str(tmp_path / "*.npy"))
    assert len(g["time_series"]) == 1 and len(g["time_series"][0]["ndvi_true"]) == 4
