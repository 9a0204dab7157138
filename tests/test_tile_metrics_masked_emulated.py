"""The masked validation metrics without a GPU: the host logic (utils.calculate_metrics.tile_metrics_masked_device /
calculate_metrics(valid=), validation_utils.evaluate_tiles(masked=True), fit(masked_validation=True)) on the numpy statement of
nirgan_tile_metrics_masked (tests/emu_tile_metrics_masked.py) against float64, the argument checks and struct layout of the real
library, and the resource usage of the shipped kernel (hipcc cross-compiles).  Bodies shared with
tests/test_gpu_tile_metrics_masked.py (tests/tile_metrics_masked_cases.py)."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest
import torch

import tile_metric_cases as Tc
import tile_metrics_masked_cases as Mc
from emu_tile_metrics_masked import EmuPoolTileMetricsMasked, EmuTileMetricsMasked
from nirgan_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(4)


@pytest.fixture()
def emu():
    be = EmuTileMetricsMasked()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.fixture()
def pool_emu():
    be = EmuPoolTileMetricsMasked()
    L.set_backend(be)
    yield be
    L.set_backend(None)


COLUMNS = [(shape, crop, kind, w) for shape, crop, kind, windows in Mc.COLUMN_CASES for w in windows]


@pytest.mark.parametrize("shape,crop,kind,window", COLUMNS, ids=lambda v: getattr(v, "__name__", str(v)))
def test_columns_against_float64(emu, shape, crop, kind, window):
    Mc.columns_against_float64("cpu", shape, crop, kind, window)
    assert emu.calls == ["tile_metrics_masked"]


@pytest.mark.parametrize("window", [11, 5])
def test_raw_window_with_nan_everywhere_outside_it(emu, window):
    Mc.raw_window_with_nan_outside("cpu", window)


@pytest.mark.parametrize("shape,crop", [((3, 67, 93), 41), ((1, 12, 12), None)], ids=str)
def test_mask_of_ones_equals_the_unmasked_entry(emu, shape, crop):
    assert Mc.ones_equal_the_unmasked_entry("cpu", shape, crop)                    # the emulator's own ssim: bitwise too
    assert emu.calls == ["tile_metrics", "tile_metrics_masked"]


def test_poison_at_dropped_pixels_reaches_no_output(emu):
    Mc.poison_at_dropped_pixels("cpu")


def test_all_invalid_tile_between_two_ordinary_ones(emu):
    Mc.all_invalid_tile_between_two("cpu")


def test_no_clean_support_gives_nan_ssim_and_finite_rest(emu):
    Mc.no_clean_support_but_valid_pixels("cpu")


def test_patch_without_a_valid_pixel_gives_nan_patch_means(emu):
    Mc.patch_without_a_valid_pixel("cpu")


def test_identical_images(emu):
    Mc.identical_images("cpu")


def test_negative_zero_is_invalid_and_any_other_value_valid(emu):
    Mc.values_of_valid("cpu")


def test_repeatable_and_a_tile_alone_equals_its_row_in_the_batch(emu):
    Mc.repeatable_and_batch_independent("cpu")


def test_null_rgb_and_patch_zero_leave_their_columns_and_guards_stay_intact(emu):
    Mc.null_rgb_and_no_patch_leave_their_columns("cpu")


def test_python_entry_rejects_bad_shapes_and_devices(emu):
    from utils.calculate_metrics import TILE_METRIC_COLUMNS, TILE_METRIC_MASKED_COLUMNS, calculate_metrics, tile_metrics_masked_device
    assert TILE_METRIC_MASKED_COLUMNS == TILE_METRIC_COLUMNS + ("n_valid", "n_ssim") and L.TILE_METRIC_MASKED_COLS == 11
    rgb, nir, pred = Tc.inputs((2, 20, 20))
    valid = torch.ones(2, 1, 20, 20)
    rows = tile_metrics_masked_device(None, nir, pred, valid, crop=16, patch=0)
    assert torch.isnan(rows[:, 4:9]).all() and torch.isfinite(rows[:, :4]).all() and (rows[:, 9:] == 256).all()
    with pytest.raises(ValueError, match="valid"):
        tile_metrics_masked_device(rgb, nir, pred, valid[:, :, :10], crop=16)
    with pytest.raises(ValueError, match="valid"):
        tile_metrics_masked_device(rgb, nir, pred, None, crop=16)
    with pytest.raises(RuntimeError, match="tile_metrics_masked"):
        tile_metrics_masked_device(rgb, nir, pred, valid, crop=24)                # window outside the image
    with pytest.raises(RuntimeError, match="tile_metrics_masked"):
        tile_metrics_masked_device(rgb, nir, pred, valid, crop=16, patch=17)
    with pytest.raises(ValueError, match=r"\[B, 1, H, W\]"):
        calculate_metrics(rgb, rgb, valid=valid)                                  # three channels
    with pytest.raises(RuntimeError, match="no CPU path"):
        tile_metrics_masked_device(rgb, nir, pred, valid.to("meta"), crop=16)
    L.set_backend(None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tile_metrics_masked_device(rgb, nir, pred, valid, crop=16, patch=4)


def test_emulator_rejects_bad_arguments(emu):
    Mc.refusals(emu)


def test_real_library_rejects_bad_arguments_before_any_launch():
    be = L.backend()
    assert not L.is_emulated()
    Mc.refusals(be)
    emu = EmuTileMetricsMasked()
    assert be.nirgan_tile_metrics_masked_ws_elems(16, 240, 240) == 16 * 64 * 11
    for args in Mc.WS_ARGS:
        assert emu.nirgan_tile_metrics_masked_ws_elems(*args) == be.nirgan_tile_metrics_masked_ws_elems(*args), args


def test_struct_layout_matches_the_header(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
           'printf("%zu %d", sizeof(nirgan_tile_metrics_masked_desc), NIRGAN_TILE_METRIC_MASKED_COLS);\n')
    for name, _ in L.TileMetricsMaskedDesc._fields_:
        src += f'printf(" %zu", offsetof(nirgan_tile_metrics_masked_desc, {name}));\n'
    src += "return 0;}\n"
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    nums = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert nums[0] == C.sizeof(L.TileMetricsMaskedDesc) and nums[1] == L.TILE_METRIC_MASKED_COLS
    assert nums[2:] == [getattr(L.TileMetricsMaskedDesc, name).offset for name, _ in L.TileMetricsMaskedDesc._fields_]
    assert L.TileMetricsMaskedDesc._fields_[-1][0] == "valid"


def test_shipped_kernel_uses_no_scratch_and_under_64k_of_lds(tmp_path):
    """csrc/tilemetrics_masked.hip compiled to gfx950 assembly; from the kernel descriptor and the metadata only: nothing spilled, no
    scratch, less than 64 KB of static LDS"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = tmp_path / "tilemetrics_masked.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-result", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "nir-gan_amd", "csrc", "tilemetrics_masked.hip"), "-o", str(asm)], check=True, timeout=600)
    text = asm.read_text()
    names = [n for n in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M) if "tile_metrics_masked" in n]
    assert len(names) == 2, names
    for name in names:
        start = text.index(".amdhsa_kernel " + name)
        desc = text[start:text.index(".end_amdhsa_kernel", start)]
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1))
        md = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?.*\.vgpr_spill_count:\s+(\d+)", text)
        print(f"{name}: LDS {lds} B, scratch {scratch} B, vgpr spills {md and md.group(1)}")
        assert scratch == 0 and 0 < lds < 64 * 1024
        assert md and int(md.group(1)) == 0


def test_calculate_metrics_over_valid_and_unchanged_without(emu):
    from utils.calculate_metrics import calculate_metrics
    Mc.calculate_metrics_over_valid("cpu")
    assert set(emu.calls) == {"tile_metrics_masked"}
    del emu.calls[:]
    _, nir, pred = Tc.inputs((3, 33, 47))
    out = calculate_metrics(pred, nir, phase="val")
    assert emu.calls == ["metrics"] and sorted(out) == ["val/L1", "val/L2", "val/PSNR", "val/SSIM"]


def test_evaluate_tiles_masked_from_the_pool(pool_emu, tmp_path):
    Mc.table_from_the_pool("cpu", tmp_path, pool_emu.calls)


def test_spider_validation_callback_passes_masked_through(emu, tmp_path):
    from validation_utils import MASKED_TABLE_KEYS, spider_validation_callback
    rgb, nir, _ = Tc.inputs((2, 244, 244))
    valid = Mc.mask_planes(2, 244, 244, Mc.centre(244, 244, 240))
    ds = [{"rgb": rgb[i], "nir": nir[i], "valid": valid[i], "coords": torch.tensor([1.0 * i, 2.0])} for i in range(2)]
    table = spider_validation_callback(Tc.ScaleModel().eval(), ds, satclip=False, folder=str(tmp_path / "spiders"), masked=True)
    assert tuple(table) == MASKED_TABLE_KEYS and emu.calls == ["tile_metrics_masked"]
    assert all(0 < s < v < 240 * 240 for s, v in zip(table["n_ssim"], table["n_valid"]))
    with pytest.raises(KeyError, match="valid"):
        spider_validation_callback(Tc.ScaleModel().eval(), [{k: v for k, v in s.items() if k != "valid"} for s in ds], satclip=False,
                                   folder=str(tmp_path / "spiders"), masked=True)


# ------------------------------------------------------------------------------------------------ fit(masked_validation=True)
def _fit_pieces(all_invalid_batch=False):
    import api_cases as A
    from model.pix2pix import Px2Px_PL
    cfg = A.px_config(6, 8)

    def fresh():
        torch.manual_seed(0)
        return Px2Px_PL(cfg).to("cpu")
    train, val = A._loaders("cpu", n_train=1, n_val=3)
    for i, batch in enumerate(val):
        batch["valid"] = Mc.mask_planes(2, 32, 32, (0, 0, 32, 32)).roll(i, 0)
    if all_invalid_batch:
        val[1]["valid"] = torch.zeros(2, 1, 32, 32)
    return fresh, train, val


def _masked_l1(model, val):
    """float64: the mean over the batches with a valid pixel of the masked mean of |predict_step - nir|"""
    model.eval()
    per_batch = []
    for batch in val:
        keep = batch["valid"] != 0
        if bool(keep.any()):
            with torch.no_grad():
                pred = model.predict_step(batch["rgb"]).double()
            per_batch.append(float((pred - batch["nir"].double()).abs()[keep].mean()))
    return sum(per_batch) / len(per_batch)


@pytest.mark.parametrize("all_invalid_batch", [False, True])
def test_fit_with_masked_validation(emu, tmp_path, all_invalid_batch):
    import csv
    from nirgan_hip.fit import fit
    fresh, train, val = _fit_pieces(all_invalid_batch)
    m = fresh()
    assert m.masked_validation is False
    path = tmp_path / "val_tiles.csv"
    hist = fit(m, train, val, max_epochs=2, log_every=1, device="cpu", masked_validation=True, tile_table_path=str(path), tile_table_crop=24)
    assert m.masked_validation is False                                                    # restored
    assert "metrics" not in emu.calls and "tile_metrics" not in emu.calls
    assert emu.calls.count("tile_metrics_masked") == 2 * (3 + 1)                            # per epoch: three batches, one table of six tiles
    last = hist["val"][-1]
    assert all(math.isfinite(last[k]) for k in ("val/L1", "val/L2", "val/PSNR", "val/SSIM")) and "val_not_finite" not in hist
    want = _masked_l1(m, val)
    print(f"val/L1 {last['val/L1']:.9g} vs float64 masked {want:.9g}")
    assert abs(last["val/L1"] - want) <= 1e-5 * want
    rows = list(csv.reader(open(tmp_path / "val_tiles_e1.csv")))
    assert rows[0][-2:] == ["n_valid", "n_ssim"] and len(rows) == 1 + 6
    if all_invalid_batch:
        assert [r[-2:] for r in rows[3:5]] == [["0.0", "0.0"]] * 2 and rows[3][4:7] == ["nan"] * 3


def test_fit_restores_the_attribute_when_the_run_fails(emu):
    from nirgan_hip.fit import fit
    fresh, train, val = _fit_pieces()
    m = fresh()
    m.masked_validation = True                                                    # the caller's own setting survives a run without
    fit(m, train, val, max_epochs=1, log_every=0, device="cpu")
    assert m.masked_validation is True and "tile_metrics_masked" in emu.calls
    m.masked_validation = False
    bad = [dict(val[0], valid=torch.ones(2, 1, 8, 8))]
    with pytest.raises(ValueError, match="valid"):
        fit(m, train, bad, max_epochs=1, log_every=0, device="cpu", masked_validation=True)
    assert m.masked_validation is False


def test_fit_without_masked_validation_ignores_valid(emu):
    """batches that carry "valid" validate as ever: the history of a run whose batches have it stripped, exactly"""
    from nirgan_hip.fit import fit
    fresh, train, val = _fit_pieces()
    with_valid = fit(fresh(), train, val, max_epochs=2, log_every=1, device="cpu")
    assert "tile_metrics_masked" not in emu.calls and emu.calls.count("metrics") == 6
    stripped = [{k: v for k, v in b.items() if k != "valid"} for b in val]
    assert with_valid == fit(fresh(), train, stripped, max_epochs=2, log_every=1, device="cpu")
    masked = fit(fresh(), train, val, max_epochs=2, log_every=1, device="cpu", masked_validation=True)
    assert masked["train"] == with_valid["train"] and masked["val"][0]["val/L1"] != with_valid["val"][0]["val/L1"]


def test_a_key_without_a_finite_batch_is_nan_and_not_handed_to_the_scheduler(emu):
    import api_cases as A
    from model.pix2pix import Px2Px_PL
    from nirgan_hip.fit import fit
    _, train, val = _fit_pieces()
    for batch in val:
        batch["valid"] = torch.zeros(2, 1, 32, 32)
    torch.manual_seed(0)
    m = Px2Px_PL(A.px_config(6, 8, patience_g=0, patience_d=0)).to("cpu")          # patience 0: any epoch the scheduler sees may cut the lr
    hist = fit(m, train, val, max_epochs=3, log_every=0, device="cpu", masked_validation=True)
    assert all(math.isnan(v[k]) for v in hist["val"] for k in ("val/L1", "val/L2", "val/PSNR", "val/SSIM"))
    assert hist["val_not_finite"] == [{"epoch": e, "keys": ["val/L1", "val/L2", "val/PSNR", "val/SSIM"]} for e in range(3)]
    rates = [{k: v for k, v in rec.items() if k != "epoch"} for rec in hist["lr"]]
    assert rates == [rates[0]] * 3                                                 # no step of ReduceLROnPlateau on a NaN
