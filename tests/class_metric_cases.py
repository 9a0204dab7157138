"""Bodies shared by tests/test_class_metrics_emulated.py (numpy emulator, CPU) and tests/test_gpu_class_metrics.py (MI355X): the
land-cover-stratified metrics (nirgan_class_metrics, utils.calculate_metrics.class_metrics_device, validation_utils.
evaluate_land_cover / summarize_land_cover) against float64.

Inputs: the generators of tile_metric_cases.inputs; masks from a seeded generator (``masks``) so that inside the evaluation window
every case holds all five classes, one class (3) absent from the last tile, a class (4) of exactly one pixel per tile, class borders
that run through a 32 x 32 block and through the two rows a wave owns, and a few pixels with id 7, which ``classes=5`` must ignore.
A batch of ONE tile cannot both hold and lack class 3: such a case is run with both masks.  Outside the window the mask holds other
random ids, so a read past the window moves the counts.

Expected values, per (tile, class), in float64 on the CROPPED tensors: ``O.ssim_map(n, p, 11)[m == c].mean()`` (the SSIM map of the
whole crop), the per-pixel index errors behind ``O.rs_logging_dict`` (``O.rs_index_pairs(.., "loss")``) masked, plain torch for
count / l1 / l2 / psnr.

Bounds, all from tile_metric_cases (nothing new): per column max-norm relative 2e-5 over all (tile, class) rows with count > 0;
count exact; psnr per row absolute 10 / ln 10 * 2e-5 * max(l2 column) / l2[row], the error a 2e-5-of-column-scale error of l2
implies; rows with count == 0 are NaN in columns 1-7 and have count 0.
"""
import csv
import ctypes as C
import functools
import math

import torch

import nirgan_oracle as O
import tile_metric_cases as Tc
from nirgan_hip import lib as L
from utils.calculate_metrics import CLASS_METRIC_COLUMNS, TILE_METRIC_COLUMNS, class_metrics_device, tile_metrics_device

TOL = Tc.TOL
CASES = [((1, 12, 12), None), ((2, 41, 41), 41), ((3, 48, 56), None), ((2, 64, 64), 40), ((2, 256, 256), 240)]
GUARD = 64


def geometry(shape, crop):
    _, H, W = shape
    ch, cw = (H, W) if crop is None else (crop, crop)
    return (H - ch) // 2, (W - cw) // 2, ch, cw


def masks(shape, crop, seed=5, drop=True):
    """uint8 [B, H, W]; see the module docstring.  ``drop``: class 3 is absent from the last tile"""
    B, H, W = shape
    y0, x0, ch, cw = geometry(shape, crop)
    g = torch.Generator().manual_seed(seed)
    out = torch.randint(0, 5, (B, H, W), generator=g, dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(ch), torch.arange(cw), indexing="ij")
    for b in range(B):
        # a slanted vertical border near the middle column and a horizontal one at three quarters of the height
        m = torch.where(xx + (yy // 2) % 5 < cw // 2 - b, 1, 2)
        low = yy >= ch - ch // 4 - b
        m = torch.where(low, 3 - m, m)
        m[torch.rand(ch, cw, generator=g) < 0.15] = 0
        if not (drop and b == B - 1):
            s = max(2, ch // 5)
            ry, rx = (int(torch.randint(0, n - s + 1, (1,), generator=g)) for n in (ch, cw))
            m[ry:ry + s, rx:rx + s] = 3
        at = torch.randperm(ch * cw, generator=g)[:4]
        m.view(-1)[at[:3]] = 7
        m.view(-1)[at[3]] = 4
        out[b, y0:y0 + ch, x0:x0 + cw] = m.to(torch.uint8)
    return out


def mask_conditions_hold(shape, crop, drop=True):
    y0, x0, ch, cw = geometry(shape, crop)
    w = masks(shape, crop, drop=drop)[:, y0:y0 + ch, x0:x0 + cw]
    B = shape[0]
    assert set(w.unique().tolist()) == ({0, 1, 2, 3, 4, 7} if (B > 1 or not drop) else {0, 1, 2, 4, 7})
    assert all((w[b] == 4).sum() == 1 and 1 <= (w[b] == 7).sum() <= 3 for b in range(B))
    assert ((w[B - 1] == 3).sum() == 0) == drop and all((w[b] == 3).sum() > 0 for b in range(B - 1))
    # the 1 | 2 border crosses the inside of a 32 x 32 block in both rows of a wave's row pair, the horizontal one a block's inside
    at = (cw // 2) // 32 * 32
    assert all({1, 2} <= set(row[at:at + 32].tolist()) for row in w[0, 0:2])
    assert (ch - ch // 4) % 32 != 0


def expected(rgb, nir, pred, mask, crop, classes=5):
    """float64 rows [B][classes][8] in CLASS_METRIC_COLUMNS order, each tile on its own cropped tensors; NaN where count == 0"""
    rows = torch.full((nir.shape[0], classes, len(CLASS_METRIC_COLUMNS)), float("nan"), dtype=torch.float64)
    for b in range(nir.shape[0]):
        n, p = (Tc.window(t[b:b + 1].double(), crop) for t in (nir, pred))
        m = Tc.window(mask[b:b + 1].reshape(1, 1, *mask.shape[-2:]), crop)
        terms = {"l1": (n - p).abs(), "l2": (n - p) ** 2, "ssim": O.ssim_map(n, p, 11)}
        if rgb is not None:
            idx = O.rs_index_pairs(Tc.window(rgb[b:b + 1].double(), crop), n, p, "loss")
            terms.update({f"l1_{k}": (idx[k][0] - idx[k][1]).abs() for k in ("ndvi", "ndwi", "evi")})
        for c in range(classes):
            sel = m == c
            rows[b, c, 0] = int(sel.sum())
            if rows[b, c, 0] == 0:
                continue
            for k, t in terms.items():
                rows[b, c, CLASS_METRIC_COLUMNS.index(k)] = t[sel].mean()
            l2 = rows[b, c, 2].item()
            rows[b, c, 4] = 10.0 * math.log10(1.0 / l2) if l2 > 0 else float("inf")
    return rows


@functools.lru_cache(maxsize=None)
def case(shape, crop, drop=True):
    """(rgb, nir, pred, mask, float64 expectation) of a case, computed once and shared; nobody writes to them"""
    rgb, nir, pred = Tc.inputs(shape)
    mask = masks(shape, crop, drop=drop)
    return rgb, nir, pred, mask, expected(rgb, nir, pred, mask, crop)


def expectation_is_finite(shape, crop, drop=True):
    """every row with pixels has a finite float64 expectation, the others are NaN, and the counts add up to the window less the 7s"""
    _, _, _, mask, ref = case(shape, crop, drop)
    y0, x0, ch, cw = geometry(shape, crop)
    has = ref[:, :, 0] > 0
    assert torch.isfinite(ref[has]).all() and torch.isnan(ref[~has][:, 1:]).all()
    sevens = (mask[:, y0:y0 + ch, x0:x0 + cw] == 7).sum((1, 2))
    assert ref[:, :, 0].sum(1).tolist() == (ch * cw - sevens).tolist()


def close_rows(got, ref, what="", skip=()):
    """``got`` [B][classes][8] against float64 ``ref`` under the bounds of the module docstring; prints each figure first"""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(got[:, :, 0], ref[:, :, 0]), f"{what} count"
    has = ref[:, :, 0] > 0
    empty = got[~has]
    for j, name in enumerate(CLASS_METRIC_COLUMNS[1:], start=1):
        if name in skip:
            continue
        assert torch.isnan(empty[:, j]).all(), f"{what} {name}: a class without pixels must be NaN"
        a, b = got[:, :, j][has], ref[:, :, j][has]
        assert torch.isfinite(a).all(), f"{what} {name}: non-finite"
        if name == "psnr":
            l2 = ref[:, :, 2][has]
            err, bound = (a - b).abs(), Tc.PSNR_ABS * l2.max() / l2
            worst = (err / bound).argmax()
            print(f"{what} psnr: worst err {err[worst].item():.3e} bound {bound[worst].item():.3e}")
            assert (err <= bound).all(), f"{what} psnr: err {err[worst].item():.3e} > {bound[worst].item():.3e}"
            continue
        err, scale = (a - b).abs().max().item(), b.abs().max().item()
        bound = TOL * max(scale, 1e-20)
        print(f"{what} {name}: err {err:.3e} bound {bound:.3e} (scale {scale:.3e})")
        assert err <= bound, f"{what} {name}: err {err:.3e} > {bound:.3e} (scale {scale:.3e})"


def rows_against_float64(dev, shape, crop):
    for drop in ((True, False) if shape[0] == 1 else (True,)):
        rgb, nir, pred, mask, ref = case(shape, crop, drop)
        got = class_metrics_device(rgb.to(dev), nir.to(dev), pred.to(dev), mask.to(dev), classes=5, crop=crop)
        assert got.shape == (shape[0], 5, 8) and got.dtype == torch.float32 and got.device.type == torch.device(dev).type
        close_rows(got, ref, f"{shape} crop {crop}")
        # the reference's route: the mask as a float tensor with a channel axis
        again = class_metrics_device(rgb.to(dev), nir.to(dev), pred.to(dev), mask[:, None].float().to(dev), classes=5, crop=crop)
        assert same(again, got)


def same(a, b):
    """bitwise, NaN equal to NaN"""
    return a.shape == b.shape and torch.equal(a.detach().cpu().view(torch.int32), b.detach().cpu().view(torch.int32))


def one_class_equals_tile_metrics(dev, shape=(2, 64, 64), crop=40):
    rgb, nir, pred = (t.to(dev) for t in Tc.inputs(shape))
    rows = class_metrics_device(rgb, nir, pred, torch.zeros(shape, dtype=torch.uint8, device=dev), classes=1, crop=crop).double().cpu()
    tile = tile_metrics_device(rgb, nir, pred, crop=crop, patch=0).double().cpu()
    assert rows.shape == (shape[0], 1, 8) and (rows[:, 0, 0] == crop * crop).all()
    for j, name in enumerate(TILE_METRIC_COLUMNS[:7]):
        a, b = rows[:, 0, 1 + j], tile[:, j]
        rel = ((a - b).abs() / b.abs()).max().item()
        print(f"one class {name}: rel {rel:.3e}")
        assert rel <= 1e-6, name


def weighted_classes_reproduce_tile_metrics(dev, shape=(2, 64, 64), crop=40):
    rgb, nir, pred = (t.to(dev) for t in Tc.inputs(shape))
    g = torch.Generator().manual_seed(9)
    mask = torch.randint(0, 5, shape, generator=g, dtype=torch.uint8).to(dev)
    rows = class_metrics_device(rgb, nir, pred, mask, classes=5, crop=crop).double().cpu()
    tile = tile_metrics_device(rgb, nir, pred, crop=crop, patch=0).double().cpu()
    assert (rows[:, :, 0].sum(1) == crop * crop).all()
    for name in ("l1", "l2", "ssim", "l1_ndvi", "l1_ndwi", "l1_evi"):
        a = (rows[:, :, 0] * rows[:, :, CLASS_METRIC_COLUMNS.index(name)]).sum(1) / (crop * crop)
        b = tile[:, TILE_METRIC_COLUMNS.index(name)]
        rel = ((a - b).abs() / b.abs()).max().item()
        print(f"count-weighted {name}: rel {rel:.3e}")
        assert rel <= TOL, name


def poison_outside_the_window_changes_nothing(dev, shape=(2, 64, 64), crop=40):
    rgb, nir, pred, mask, _ = case(shape, crop)
    y0, x0, ch, cw = geometry(shape, crop)
    src = mask.float()
    clean = class_metrics_device(rgb.to(dev), nir.to(dev), pred.to(dev), src.to(dev), classes=5, crop=crop)
    assert same(clean, class_metrics_device(rgb.to(dev), nir.to(dev), pred.to(dev), mask.to(dev), classes=5, crop=crop))
    inside = torch.zeros(shape[1:], dtype=torch.bool)
    inside[y0:y0 + ch, x0:x0 + cw] = True
    bad = [torch.where(inside, t, torch.full_like(t, float("nan"))) for t in (rgb, nir, pred, src)]
    assert all(torch.isnan(t).any() for t in bad)
    got = class_metrics_device(*(t.to(dev) for t in bad), classes=5, crop=crop)
    assert same(got, clean)
    wild = mask.clone()                                     # a uint8 mask goes to the entry as it is: other ids outside the window
    wild[:, ~inside] = 4 - wild[:, ~inside].clamp(max=4)
    assert same(class_metrics_device(bad[0].to(dev), bad[1].to(dev), bad[2].to(dev), wild.to(dev), classes=5, crop=crop), clean)


def no_rgb_gives_nan_index_columns(dev, shape=(2, 41, 41), crop=41):
    rgb, nir, pred, mask, _ = case(shape, crop)
    full = class_metrics_device(rgb.to(dev), nir.to(dev), pred.to(dev), mask.to(dev), classes=5, crop=crop)
    bare = class_metrics_device(None, nir.to(dev), pred.to(dev), mask.to(dev), classes=5, crop=crop)
    assert same(bare[:, :, :5], full[:, :, :5]) and torch.isnan(bare[:, :, 5:]).all()


def bitwise_repeatable_and_batch_independent(dev, shape=(64, 40, 40)):
    rgb, nir, pred = (t.to(dev) for t in Tc.inputs(shape))
    mask = masks(shape, None).to(dev)
    a = class_metrics_device(rgb, nir, pred, mask, classes=5)
    assert same(a, class_metrics_device(rgb, nir, pred, mask, classes=5))
    for k in (0, 17, 63):
        alone = class_metrics_device(rgb[k:k + 1], nir[k:k + 1], pred[k:k + 1], mask[k:k + 1], classes=5)
        assert same(alone[0], a[k]), k
    assert same(class_metrics_device(rgb[5:21], nir[5:21], pred[5:21], mask[5:21], classes=5), a[5:21])


def desc(rgb, nir, pred, mask, crop, classes, ws, rows):
    B, _, H, W = nir.shape
    y0, x0, ch, cw = geometry((B, H, W), crop)
    d = L.ClassMetricsDesc()
    d.rgb = None if rgb is None else rgb.data_ptr()
    d.nir, d.pred, d.mask, d.B, d.H, d.W = nir.data_ptr(), pred.data_ptr(), mask.data_ptr(), B, H, W
    d.y0, d.x0, d.ch, d.cw = y0, x0, ch, cw
    d.window, d.sigma, d.max_val, d.eps, d.classes = 11, 1.5, 1.0, 1e-12, classes
    d.ws, d.ws_elems, d.rows = ws.data_ptr(), ws.numel(), rows.data_ptr()
    return d


def raw_entry_overwrites_and_keeps_its_guards(dev, shape=(2, 41, 41), crop=41):
    """the entry itself: rows OVERWRITTEN (not accumulated), index columns untouched without rgb, guard values around rows and ws"""
    rgb, nir, pred, mask, ref = (t.to(dev).contiguous() if i < 4 else t for i, t in enumerate(case(shape, crop)))
    be = L.backend()
    B = shape[0]
    n_ws, n_rows = int(be.nirgan_class_metrics_ws_elems(B, crop, crop, 5)), B * 5 * 8
    assert n_ws == B * 2 * 2 * 5 * 8
    ws_buf = torch.full((GUARD + n_ws + GUARD,), -3.0, device=dev)
    rows_buf = torch.full((GUARD + n_rows + GUARD,), -5.0, device=dev)
    ws, rows = ws_buf[GUARD:GUARD + n_ws], rows_buf[GUARD:GUARD + n_rows]
    st = torch.cuda.current_stream().cuda_stream if torch.device(dev).type == "cuda" else None
    L.check(be.nirgan_class_metrics(C.byref(desc(rgb, nir, pred, mask, crop, 5, ws, rows)), st), "class_metrics")
    full = rows.view(B, 5, 8).clone()
    close_rows(full, ref, "raw entry")
    L.check(be.nirgan_class_metrics(C.byref(desc(rgb, nir, pred, mask, crop, 5, ws, rows)), st), "class_metrics")
    assert same(rows.view(B, 5, 8), full)
    rows.fill_(-5.0)
    L.check(be.nirgan_class_metrics(C.byref(desc(None, nir, pred, mask, crop, 5, ws, rows)), st), "class_metrics")
    got = rows.view(B, 5, 8)
    assert same(got[:, :, :5], full[:, :, :5]) and (got[:, :, 5:] == -5.0).all()
    for buf, n in ((ws_buf, n_ws), (rows_buf, n_rows)):
        fill = buf[0].item()
        assert (buf[:GUARD] == fill).all() and (buf[GUARD + n:] == fill).all()


class MeanModel(torch.nn.Module):
    """a stand-in with the reference's predict_step(rgb, coords): a fixed perturbation of the rgb mean"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.9, 0.07]))
        self.seen = []

    def predict_step(self, rgb, coords=None):
        assert not self.training
        self.seen.append(tuple(rgb.shape))
        return rgb[:, :3].mean(1, keepdim=True) * self.w[0] + self.w[1]


def land_cover_samples(n=5, side=48, crop=40):
    out = []
    for i in range(n):
        rgb, nir, _ = Tc.inputs((1, side, side), 3 + i)
        mask = masks((1, side, side), crop, seed=20 + i, drop=(i == 1))[0]
        out.append({"rgb": rgb[0], "nir": nir[0], "coords": torch.tensor([10.0 + i, -5.0 - i]),
                    "mask": mask if i % 2 else mask[None].float()})       # both layouts and dtypes the reference hands over
    return out


def land_cover_table_and_summary(dev, tmp_path, crop=40):
    """evaluate_land_cover on 5 samples in batches of 2 (a tail of 1): keys and order, count > 0 rows only, every row against float64
    of its tile alone, the CSV round trip, and summarize_land_cover against float64 pooled over ALL pixels of a class"""
    from validation_utils import CLC_CLASSES, evaluate_land_cover, summarize_land_cover
    from validation_utils.land_cover import LAND_COVER_KEYS, SUMMARY_KEYS
    data = land_cover_samples(crop=crop)
    model = MeanModel().to(dev).train()
    path = tmp_path / "sub" / "land_cover.csv"
    table = evaluate_land_cover(model, data, crop=crop, batch_size=2, device=dev, csv_path=str(path))
    assert model.training and model.seen == [(2, 3, 48, 48), (2, 3, 48, 48), (1, 3, 48, 48)]
    assert tuple(table) == LAND_COVER_KEYS == ("id", "x", "y", "class_id", "class_name", "count", "ssim", "psnr", "l1", "l2",
                                               "l1_ndvi", "l1_ndwi", "l1_evi")
    refs, pooled = [], {}
    model.eval()
    for i, s in enumerate(data):
        rgb, nir, mask = s["rgb"][None], s["nir"][None], s["mask"].reshape(1, 48, 48).to(torch.uint8)
        with torch.no_grad():
            pred = model.predict_step(rgb.to(dev)).float().cpu()
        ref = expected(rgb, nir, pred, mask, crop)[0]
        refs.append(ref)
        for c in range(5):
            if ref[c, 0] > 0:
                pooled.setdefault(c, []).append(ref[c])
    model.train()
    want = [(i, c) for i, ref in enumerate(refs) for c in range(5) if ref[c, 0] > 0]
    assert list(zip(table["id"], table["class_id"])) == want and (1, 3) not in want       # the class absent from tile 1 has no row
    assert table["class_name"] == [CLC_CLASSES[c] for _, c in want] and all(isinstance(n, int) and n > 0 for n in table["count"])
    assert table["x"] == [10.0 + i for i, _ in want] and table["y"] == [-5.0 - i for i, _ in want]
    got = torch.tensor([[table[k][r] for k in CLASS_METRIC_COLUMNS] for r in range(len(want))], dtype=torch.float64)
    close_rows(got[None], torch.stack([refs[i][c] for i, c in want])[None], "table")
    rows = list(csv.reader(open(path)))
    assert rows[0] == [""] + list(LAND_COVER_KEYS) and len(rows) == 1 + len(want)
    for r, row in enumerate(rows[1:]):
        assert int(row[0]) == r and int(row[1]) == table["id"][r] and int(row[4]) == table["class_id"][r] and row[5] == table["class_name"][r]
        assert int(row[6]) == table["count"][r]
        assert [float(v) for v in row[2:4] + row[7:]] == [table[k][r] for k in ("x", "y") + LAND_COVER_KEYS[6:]]      # repr round trip: exact
    summary = summarize_land_cover(table)
    assert tuple(summary) == SUMMARY_KEYS and summary["class_id"] == sorted(pooled) == [0, 1, 2, 3, 4]
    assert summary["class_name"] == list(CLC_CLASSES)
    for at, c in enumerate(summary["class_id"]):
        parts = torch.stack(pooled[c])
        n = parts[:, 0].sum()
        assert summary["count"][at] == int(n)
        for k in ("l1", "l2", "ssim", "l1_ndvi", "l1_ndwi", "l1_evi", "psnr"):
            # the mean over all of the class's pixels: per-tile float64 means weighted by their exact counts
            ref = 10.0 * math.log10(1.0 / ((parts[:, 0] * parts[:, 2]).sum() / n).item()) if k == "psnr" else \
                ((parts[:, 0] * parts[:, CLASS_METRIC_COLUMNS.index(k)]).sum() / n).item()
            val = summary[k][at]
            assert isinstance(val, float)
            print(f"summary class {c} {k}: {val:.9e} float64 {ref:.9e} rel {abs(val - ref) / abs(ref):.3e}")
            assert abs(val - ref) <= TOL * abs(ref), (c, k)
    return table
