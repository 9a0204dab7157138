"""Land-cover-stratified validation without a GPU: the host logic (utils.calculate_metrics.class_metrics_device, validation_utils.
evaluate_land_cover / summarize_land_cover, fit(land_cover_table_path=..), the two CLC figures) on the numpy statement of
nirgan_class_metrics (tests/emu_class_metrics.py) against float64, the argument checks and struct layout of the real library, and the
resource usage of the shipped kernels (hipcc cross-compiles).  Bodies shared with tests/test_gpu_class_metrics.py."""
import csv
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import class_metric_cases as Cc
import tile_metric_cases as Tc
from emu_class_metrics import EmuClassMetrics
from nirgan_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def emu():
    be = EmuClassMetrics()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.mark.parametrize("shape,crop", Cc.CASES, ids=str)
def test_masks_hold_their_conditions_and_the_float64_expectation_is_finite(shape, crop):
    for drop in ((True, False) if shape[0] == 1 else (True,)):
        Cc.mask_conditions_hold(shape, crop, drop)
        Cc.expectation_is_finite(shape, crop, drop)


@pytest.mark.parametrize("shape,crop", Cc.CASES, ids=str)
def test_rows_against_float64(emu, shape, crop):
    Cc.rows_against_float64("cpu", shape, crop)
    assert set(emu.calls) == {"class_metrics"}


def test_one_class_equals_the_per_tile_entry(emu):
    Cc.one_class_equals_tile_metrics("cpu")


def test_count_weighted_classes_reproduce_the_per_tile_entry(emu):
    Cc.weighted_classes_reproduce_tile_metrics("cpu")


def test_nan_outside_the_window_changes_nothing(emu):
    Cc.poison_outside_the_window_changes_nothing("cpu")


def test_no_rgb_gives_nan_index_columns(emu):
    Cc.no_rgb_gives_nan_index_columns("cpu")


def test_bitwise_repeatable_and_a_tile_alone_equals_its_rows_in_a_batch_of_64(emu):
    Cc.bitwise_repeatable_and_batch_independent("cpu")


def test_raw_entry_overwrites_and_keeps_its_guards(emu):
    Cc.raw_entry_overwrites_and_keeps_its_guards("cpu")


def test_mask_layouts_dtypes_and_bad_arguments(emu):
    from utils.calculate_metrics import CLASS_METRIC_COLUMNS, class_metrics_device
    assert CLASS_METRIC_COLUMNS == ("count", "l1", "l2", "ssim", "psnr", "l1_ndvi", "l1_ndwi", "l1_evi")
    assert L.CLASS_MAX == 8 and L.CLASS_METRIC_COLS == 8
    rgb, nir, pred, mask, _ = Cc.case((2, 41, 41), 41)
    base = class_metrics_device(rgb, nir, pred, mask, classes=5, crop=41)
    for m in (mask.long(), mask.to(torch.int16)[:, None], mask.double(), mask.float()[:, None]):
        assert Cc.same(class_metrics_device(rgb, nir, pred, m, classes=5, crop=41), base)
    eight = class_metrics_device(rgb, nir, pred, mask, classes=8, crop=41)
    assert Cc.same(eight[:, :5], base) and (eight[:, 5:7, 0] == 0).all() and (eight[:, 7, 0] > 0).all()      # id 7 is a class now
    for bad in (mask.float() + 0.5, mask.long() - 1, mask.long() + 300, torch.where(mask == 4, float("nan"), mask.float())):
        with pytest.raises(ValueError, match="mask"):
            class_metrics_device(rgb, nir, pred, bad, classes=5, crop=41)
    with pytest.raises(ValueError):
        class_metrics_device(rgb, nir, pred, mask[:, :40], classes=5, crop=41)
    with pytest.raises(ValueError):
        class_metrics_device(rgb, nir, pred[:, :, :10], mask, classes=5, crop=8)
    with pytest.raises(ValueError):
        class_metrics_device(rgb[:, :2], nir, pred, mask, classes=5, crop=41)
    for k in (0, 9):
        with pytest.raises(ValueError, match="classes"):
            class_metrics_device(rgb, nir, pred, mask, classes=k, crop=41)
    with pytest.raises(RuntimeError, match="class_metrics"):
        class_metrics_device(rgb, nir, pred, mask, classes=5, crop=48)                  # window outside the image
    with pytest.raises(RuntimeError, match="class_metrics"):
        class_metrics_device(rgb, nir, pred, mask.float(), classes=5, crop=48)
    with pytest.raises(RuntimeError, match="class_metrics"):
        class_metrics_device(rgb, nir, pred, mask, classes=5, crop=41, window_size=4)
    L.set_backend(None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        class_metrics_device(rgb, nir, pred, mask, classes=5, crop=41)


def _valid_desc(buf):
    d = L.ClassMetricsDesc()
    d.rgb = d.nir = d.pred = d.mask = d.ws = d.rows = buf.data_ptr()
    d.B, d.H, d.W, d.y0, d.x0, d.ch, d.cw = 1, 20, 20, 2, 2, 16, 16
    d.window, d.sigma, d.max_val, d.eps, d.classes, d.ws_elems = 11, 1.5, 1.0, 1e-12, 5, 1 << 20
    return d


BAD_ARGUMENTS = [("window", 4, b"window"), ("window", 13, b"window"), ("y0", 5, b"outside"), ("x0", -1, b"outside"), ("cw", 19, b"outside"),
                 ("ch", 5, b"radius"), ("sigma", 0.0, b"sigma"), ("max_val", 0.0, b"max_val"), ("ws_elems", 39, b"workspace"),
                 ("nir", None, b"null"), ("pred", None, b"null"), ("mask", None, b"null"), ("ws", None, b"null"), ("rows", None, b"null"),
                 ("B", 0, b"empty"), ("classes", 0, b"classes"), ("classes", 9, b"classes")]


@pytest.mark.parametrize("which", ["library", "emulator"])
def test_bad_arguments_are_rejected_before_any_launch(which):
    """the real library without a GPU (an argument error returns before any launch), and the emulator's restatement of the same checks"""
    be = L.backend() if which == "library" else EmuClassMetrics()
    assert (which == "library") == (not getattr(be, "is_emulator", True) and not L.is_emulated())
    assert be.nirgan_class_metrics(C.byref(L.ClassMetricsDesc()), None) == -1 and b"class_metrics" in be.nirgan_last_error()
    buf = torch.zeros(3 * 20 * 20 + 64)
    d = _valid_desc(buf)
    for field, value, word in BAD_ARGUMENTS:
        keep = getattr(d, field)
        setattr(d, field, value)
        assert be.nirgan_class_metrics(C.byref(d), None) == -1, field
        msg = be.nirgan_last_error()
        assert b"class_metrics" in msg and word in msg, (field, msg)
        setattr(d, field, keep)
    d.H = d.W = d.ch = d.cw = 4096                                          # 2^24 pixels: the count would not be exact as a float
    d.y0 = d.x0 = 0
    assert be.nirgan_class_metrics(C.byref(d), None) == -1 and b"class_metrics" in be.nirgan_last_error() and b"2^24" in be.nirgan_last_error()


def test_workspace_sizes_of_the_library_and_the_emulator_agree():
    be, emu = L.backend(), EmuClassMetrics()
    assert not L.is_emulated()
    assert be.nirgan_class_metrics_ws_elems(16, 240, 240, 5) == 16 * 64 * 5 * 8
    for args in [(16, 240, 240, 5), (64, 240, 240, 5), (3, 41, 41, 1), (1, 12, 12, 8), (2, 33, 64, 3), (0, 4, 4, 5), (1, 4, 4, 0), (1, 4, 4, 9)]:
        assert emu.nirgan_class_metrics_ws_elems(*args) == be.nirgan_class_metrics_ws_elems(*args), args


def test_struct_layout_matches_the_header(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
           'printf("%zu %zu %d %d", sizeof(nirgan_class_metrics_desc), offsetof(nirgan_class_metrics_desc, rows), '
           'NIRGAN_CLASS_MAX, NIRGAN_CLASS_METRIC_COLS);\n')
    for name, _ in L.ClassMetricsDesc._fields_:
        src += f'printf(" %zu", offsetof(nirgan_class_metrics_desc, {name}));\n'
    src += "return 0;}\n"
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert nums[0] == C.sizeof(L.ClassMetricsDesc) and nums[1] == L.ClassMetricsDesc.rows.offset
    assert nums[2] == L.CLASS_MAX and nums[3] == L.CLASS_METRIC_COLS
    assert nums[4:] == [getattr(L.ClassMetricsDesc, name).offset for name, _ in L.ClassMetricsDesc._fields_]


def test_shipped_kernels_use_no_scratch_spill_nothing_and_fit_the_lds(tmp_path):
    """csrc/classmetrics.hip compiled for gfx950; only the kernel descriptors and the metadata are read: no private segment, no
    spilled register, and an LDS footprint within the CU's 160 KB (the staging kernel's must be above 0)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = tmp_path / "classmetrics.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-result", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "nir-gan_amd", "csrc", "classmetrics.hip"), "-o", str(asm)], check=True, timeout=600)
    text = asm.read_text()
    names = re.findall(r"\.amdhsa_kernel\s+(\S+)", text)
    assert len(names) == 2 and any("class_metrics_kernel" in n for n in names) and any("class_metrics_fold_kernel" in n for n in names)
    for name in names:
        start = text.index(".amdhsa_kernel " + name)
        desc = text[start:text.index(".end_amdhsa_kernel", start)]
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1))
        md = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?.*\.vgpr_spill_count:\s+(\d+)", text)
        print(f"{name}: LDS {lds} B, private segment {scratch} B, vgpr_spill_count {md and md.group(1)}")
        assert scratch == 0 and 0 < lds <= 160 * 1024
        assert md and int(md.group(1)) == 0


def test_land_cover_table_csv_and_summary(emu, tmp_path):
    Cc.land_cover_table_and_summary("cpu", tmp_path)
    assert emu.calls.count("class_metrics") == 3                           # ONE fused call per batch: 2 + 2 + 1 tiles


def test_land_cover_accepts_batches_and_baseline_signatures_and_needs_a_mask(emu):
    from validation_utils import evaluate_land_cover
    data = Cc.land_cover_samples()
    one = evaluate_land_cover(Cc.MeanModel().eval(), data, crop=40, batch_size=16)
    batches = [{"rgb": torch.stack([s["rgb"] for s in data[:3]]), "nir": torch.stack([s["nir"] for s in data[:3]]),
                "mask": torch.stack([s["mask"].reshape(48, 48).float() for s in data[:3]])},
               {"rgb": torch.stack([s["rgb"] for s in data[3:]]), "nir": torch.stack([s["nir"] for s in data[3:]]),
                "mask": torch.stack([s["mask"].reshape(1, 48, 48).to(torch.uint8) for s in data[3:]])}]

    class RgbOnly(Cc.MeanModel):
        def predict_step(self, rgb):
            return super().predict_step(rgb)
    two = evaluate_land_cover(RgbOnly().eval(), iter(batches), crop=40, batch_size=4)
    assert emu.calls.count("class_metrics") == 1 + 2
    assert all(np.isnan(v) for v in two["x"])
    for k in one:
        if k not in ("x", "y"):
            assert one[k] == two[k], k
    names = evaluate_land_cover(Cc.MeanModel().eval(), data[:1], classes=("a", "b"), crop=40)
    assert names["class_name"] == ["a", "b"] and names["count"] == one["count"][:2]
    with pytest.raises(KeyError, match="mask"):
        evaluate_land_cover(Cc.MeanModel().eval(), [{k: v for k, v in data[0].items() if k != "mask"}], crop=40)
    with pytest.raises(ValueError, match="mask"):
        evaluate_land_cover(Cc.MeanModel().eval(), [dict(data[0], mask=data[0]["mask"].float() + 0.25)], crop=40)


def test_fit_writes_one_land_cover_table_per_validation_epoch_and_is_unchanged_without(emu, tmp_path):
    import api_cases as A
    from model.pix2pix import Px2Px_PL
    from nirgan_hip.fit import fit
    from validation_utils.land_cover import LAND_COVER_KEYS
    cfg = A.px_config(6, 8)

    def fresh():
        torch.manual_seed(0)
        return Px2Px_PL(cfg).to("cpu")
    train, val = A._loaders("cpu", n_train=1, n_val=2)
    val = [dict(b, mask=Cc.masks((2, 32, 32), 24, seed=40 + i)) for i, b in enumerate(val)]
    plain = fit(fresh(), train, val, max_epochs=2, log_every=1, device="cpu")
    assert emu.calls.count("class_metrics") == 0
    path = tmp_path / "tables" / "val_land_cover.csv"
    hist = fit(fresh(), train, val, max_epochs=2, log_every=1, device="cpu", land_cover_table_path=str(path), land_cover_crop=24)
    assert hist == plain                                                   # the table changes nothing the loop computes
    assert emu.calls.count("class_metrics") == 2                           # 2 epochs x (2 batches of 2 regrouped into one of 4)
    assert sorted(os.listdir(tmp_path / "tables")) == ["val_land_cover_e0.csv", "val_land_cover_e1.csv"]
    for epoch in (0, 1):
        rows = list(csv.reader(open(tmp_path / "tables" / f"val_land_cover_e{epoch}.csv")))
        assert rows[0] == [""] + list(LAND_COVER_KEYS)
        pairs = [(int(r[1]), int(r[4])) for r in rows[1:]]
        # tiles 0..3 in order, classes in id order; class 3 is absent from the last tile of each batch of masks
        assert pairs == [(t, c) for t in range(4) for c in range(5) if not (c == 3 and t in (1, 3))]
        assert sum(int(r[6]) for r in rows[1:] if int(r[1]) == 0) == 24 * 24 - int((val[0]["mask"][0, 4:28, 4:28] == 7).sum())


def _panel_centre(image, col, cols):
    """the pixel at the centre of panel ``col`` of a one-row figure drawn with matplotlib's default subplot spacing"""
    import matplotlib
    a = np.asarray(image.convert("RGB")) if hasattr(image, "convert") else np.asarray(image)[..., :3]
    rc = matplotlib.rcParams
    left, right, wspace = rc["figure.subplot.left"], rc["figure.subplot.right"], rc["figure.subplot.wspace"]
    bottom, top = rc["figure.subplot.bottom"], rc["figure.subplot.top"]
    w = (right - left) / (cols + wspace * (cols - 1))
    cx = left + col * w * (1 + wspace) + w / 2
    return a, a[int(round((1 - (bottom + top) / 2) * a.shape[0])), int(round(cx * a.shape[1]))]


def test_clc_figures_show_the_legend_colours():
    from matplotlib.colors import to_rgb
    from utils.plot_clc_pred import plot_rgb_nir_and_mask
    from utils.plot_clc_utils import plot_rgb_and_mask
    from validation_utils import CLC_CLASSES, CLC_COLORS
    assert CLC_CLASSES == ("none", "agricultural", "natural vegetation", "water", "artificial")
    assert CLC_COLORS == ("#ffffff", "#90ee90", "#006400", "#1e90ff", "#ff0000")
    rgb, nir, pred = (t[0] for t in Tc.inputs((1, 48, 48)))
    for cls in (1, 2, 3, 4):
        want = [round(255 * v) for v in to_rgb(CLC_COLORS[cls])]
        for mask in (torch.full((48, 48), cls, dtype=torch.uint8), torch.full((1, 48, 48), float(cls))):
            a, px = _panel_centre(plot_rgb_and_mask(rgb, mask, it=3, title="tile"), 1, 2)
            assert a.shape[0] > 0 and a.shape[1] > 0 and px.tolist() == want, (cls, px)
            a, px = _panel_centre(plot_rgb_nir_and_mask(rgb, nir, pred[0], mask, title="tile"), 3, 4)
            assert a.shape[0] > 0 and a.shape[1] > 0 and px.tolist() == want, (cls, px)
    # the rgb panel: x 5, clipped -- a tile of 0.3 is white there
    a, px = _panel_centre(plot_rgb_and_mask(torch.full((3, 48, 48), 0.3), torch.zeros(48, 48)), 0, 2)
    assert px.tolist() == [255, 255, 255]
    with pytest.raises(ValueError):
        plot_rgb_and_mask(rgb, torch.zeros(40, 48))
