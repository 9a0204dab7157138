"""Bodies shared by tests/test_tile_metrics_masked_emulated.py (numpy emulator, CPU) and tests/test_gpu_tile_metrics_masked.py
(MI355X): the masked per-tile metrics (nirgan_tile_metrics_masked, utils.calculate_metrics.tile_metrics_masked_device /
calculate_metrics(valid=), validation_utils.evaluate_tiles(masked=True)) against float64.

Expected values, per tile, on the CROPPED float64 tensors (the way of tests/tile_metric_cases.py ``expected``): the means of |d|, d^2
and the three index errors (oracle ``rs_index_pairs``) over ``valid``; ``ssim_map(n, p, window)[clean].mean()`` with ``clean`` from
numpy -- the boolean mask reflect-padded by r, the logical AND over its (2r+1)^2 shifts; the patch means over the valid patch pixels.
An empty selection gives NaN.  Counts are compared exactly.

Bounds: those of tests/tile_metric_cases.py, imported (TOL max-norm relative per column over the tiles, PSNR_ABS for psnr): the same
kinds of quantity, fp32 means of fewer values.  No new tolerance.

Masks.  "wedge": invalid where y/ch + x/cw < 0.6 (flipped to another corner for tile b of a batch), plus three isolated invalid
pixels at (ch-2, cw-2), (ch-1, cw/2) and (min(31, ch-1), cw-1) -- the last on the last row of the first 32-block, reflecting across
the right border.  "corner": the single pixel (0, 0).  Every case asserts from the float64 restatement, before looking at the device,
that 0.25 <= n_ssim / (ch cw) <= 0.8 and n_ssim < n_valid < ch cw for every tile.
"""
import ctypes as C
import math

import numpy as np
import torch

import nirgan_oracle as O
import tile_metric_cases as Tc
from nirgan_hip import lib as L
from tile_metric_cases import PSNR_ABS, TOL
from utils.calculate_metrics import (TILE_METRIC_COLUMNS, TILE_METRIC_MASKED_COLUMNS, calculate_metrics, tile_metrics_device,
                                     tile_metrics_masked_device)

GUARD = 64
NAN = float("nan")
PATCH = {**Tc.PATCH, 33: 9, 64: 32}                 # by the smaller side of the evaluation window


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream if torch.device(dev).type == "cuda" else None


# ------------------------------------------------------------------------------------------------ masks
def wedge(ch, cw, flip=0):
    """bool [ch][cw], True = valid; ``flip`` & 1 mirrors the wedge left-right, & 2 up-down; the three isolated pixels stay put"""
    yy, xx = np.meshgrid(np.arange(ch), np.arange(cw), indexing="ij")
    if flip & 1:
        xx = cw - 1 - xx
    if flip & 2:
        yy = ch - 1 - yy
    keep = ~(yy / ch + xx / cw < 0.6)
    for y, x in ((ch - 2, cw - 2), (ch - 1, cw // 2), (min(31, ch - 1), cw - 1)):
        keep[y, x] = False
    return keep


def corner(ch, cw, flip=0):
    keep = np.ones((ch, cw), bool)
    keep[0, 0] = False
    return keep


def mask_planes(B, H, W, rect, kind=wedge):
    """float32 [B][1][H][W]: the mask of ``kind`` inside the window ``rect`` = (y0, x0, ch, cw), tile b flipped by b % 4; ones outside"""
    y0, x0, ch, cw = rect
    v = torch.ones(B, 1, H, W)
    for b in range(B):
        v[b, 0, y0:y0 + ch, x0:x0 + cw] = torch.from_numpy(kind(ch, cw, b % 4).astype(np.float32))
    return v


def centre(H, W, crop):
    ch, cw = (H, W) if crop is None else (crop, crop)
    return (H - ch) // 2, (W - cw) // 2, ch, cw


def clean_of(keep, r):
    """bool [ch][cw]: all (2r+1)^2 taps of the support, reflected at the window's border, are valid"""
    ch, cw = keep.shape
    t = np.pad(keep, r, mode="reflect")
    out = np.ones_like(keep)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out &= t[dy:dy + ch, dx:dx + cw]
    return out


# ------------------------------------------------------------------------------------------------ float64
def _mean(t, sel):
    return t[sel].mean().item() if bool(sel.any()) else NAN


def expected(rgb, nir, pred, valid, rect, patch, window=11):
    """float64 rows [B][11] in TILE_METRIC_MASKED_COLUMNS order, each tile on its own cropped tensors; rgb None / patch 0: NaN there"""
    y0, x0, ch, cw = rect
    cut = (Ellipsis, slice(y0, y0 + ch), slice(x0, x0 + cw))
    rows = []
    for b in range(nir.shape[0]):
        n, p = nir[b:b + 1][cut].double(), pred[b:b + 1][cut].double()
        keep_np = valid[b].reshape(valid.shape[-2:])[cut[1:]].cpu().numpy() != 0
        keep, clean = torch.from_numpy(keep_np)[None, None], torch.from_numpy(clean_of(keep_np, window // 2))[None, None]
        d = n - p
        l2 = _mean(d * d, keep)
        psnr = NAN if math.isnan(l2) else (10.0 * math.log10(1.0 / l2) if l2 > 0 else float("inf"))
        idx = [NAN] * 3
        if rgb is not None:
            pairs = O.rs_index_pairs(rgb[b:b + 1, :3][cut].double(), n, p, "loss")
            idx = [_mean((pairs[k][0] - pairs[k][1]).abs(), keep) for k in ("ndvi", "ndwi", "evi")]
        pm = [NAN, NAN]
        if patch > 0:
            py, px = ch // 2 - patch // 2, cw // 2 - patch // 2
            sq = (slice(None), slice(None), slice(py, py + patch), slice(px, px + patch))
            pm = [_mean(n[sq], keep[sq]), _mean(p[sq], keep[sq])]
        rows.append([_mean(d.abs(), keep), l2, _mean(O.ssim_map(n, p, window), clean), psnr, *idx, *pm,
                     float(keep.sum()), float(clean.sum())])
    return torch.tensor(rows, dtype=torch.float64)


def cap(ref, rect, what=""):
    """the masks bite: from the float64 restatement alone"""
    area = rect[2] * rect[3]
    for b, row in enumerate(ref.tolist()):
        n_valid, n_ssim = row[9], row[10]
        print(f"{what} tile {b}: n_ssim share {n_ssim / area:.3f}, n_valid share {n_valid / area:.3f}")
        assert 0.25 <= n_ssim / area <= 0.8 and n_ssim < n_valid < area, (what, b, n_ssim, n_valid, area)


def close_rows(got, ref, what="", cols=None):
    """``got`` [B][11] against float64 ``ref``: the counts exactly; NaN and +-inf where and only where expected; every other figure of a
    column under the bounds of tests/tile_metric_cases.py (max-norm relative per column over the tiles).  Prints each figure first."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(got[:, 9:], ref[:, 9:]), f"{what} counts: {got[:, 9:].tolist()} != {ref[:, 9:].tolist()}"
    for j, name in enumerate(TILE_METRIC_COLUMNS):
        if cols is not None and name not in cols:
            continue
        a, b = got[:, j], ref[:, j]
        fin = torch.isfinite(b)
        assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{what} {name}: NaN at {torch.isnan(a).tolist()}, expected {torch.isnan(b).tolist()}"
        assert torch.equal(a[~fin & ~torch.isnan(b)], b[~fin & ~torch.isnan(b)]), f"{what} {name}: infinities differ"
        if not bool(fin.any()):
            continue
        assert torch.isfinite(a[fin]).all(), f"{what} {name}: non-finite"
        err, scale = (a[fin] - b[fin]).abs().max().item(), b[fin].abs().max().item()
        bound = PSNR_ABS if name == "psnr" else TOL * max(scale, 1e-20)
        print(f"{what} {name}: err {err:.3e} bound {bound:.3e} (scale {scale:.3e})")
        assert err <= bound, f"{what} {name}: err {err:.3e} > {bound:.3e} (scale {scale:.3e})"


# ------------------------------------------------------------------------------------------------ the raw entry
def raw_rows(dev, rgb, nir, pred, valid, rect, window=11, patch=0, rows_fill=NAN, check=True):
    """nirgan_tile_metrics_masked itself on planes as they are, guards of 64 floats around rows and ws; returns rows [B][11] (clone)
    after checking the guards"""
    be = L.backend()
    B, _, H, W = nir.shape
    y0, x0, ch, cw = rect
    n_ws, n_rows = int(be.nirgan_tile_metrics_masked_ws_elems(B, ch, cw)), B * L.TILE_METRIC_MASKED_COLS
    assert n_ws == B * (-(-ch // 32)) * (-(-cw // 32)) * 11
    ws_buf = torch.full((GUARD + n_ws + GUARD,), -3.0, device=dev)
    rows_buf = torch.full((GUARD + n_rows + GUARD,), -5.0, device=dev)
    ws, rows = ws_buf[GUARD:GUARD + n_ws], rows_buf[GUARD:GUARD + n_rows]
    rows.fill_(rows_fill)
    keep = [None if t is None else t.to(dev).float().contiguous() for t in (rgb, nir, pred, valid)]
    d = L.TileMetricsMaskedDesc()
    d.rgb = None if keep[0] is None else keep[0].data_ptr()
    d.nir, d.pred, d.valid, d.B, d.H, d.W = keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), B, H, W
    d.y0, d.x0, d.ch, d.cw = y0, x0, ch, cw
    d.window, d.sigma, d.max_val, d.eps, d.patch = window, 1.5, 1.0, 1e-12, patch
    d.ws, d.ws_elems, d.rows = ws.data_ptr(), ws.numel(), rows.data_ptr()
    rc = be.nirgan_tile_metrics_masked(C.byref(d), stream(dev))
    if check:
        L.check(rc, "tile_metrics_masked")
    out = rows.view(B, L.TILE_METRIC_MASKED_COLS).clone().cpu()
    for buf, n, fill in ((ws_buf, n_ws, -3.0), (rows_buf, n_rows, -5.0)):
        assert (buf[:GUARD] == fill).all() and (buf[GUARD + n:] == fill).all(), "guard overwritten"
    return out


# ------------------------------------------------------------------------------------------------ 1. columns against float64
# (stored shape, crop or None, mask kind, SSIM windows)
COLUMN_CASES = [((3, 67, 93), 41, wedge, (11, 5)), ((2, 64, 64), None, wedge, (11, 5)), ((1, 12, 12), None, corner, (11,)),
                ((2, 40, 70), None, wedge, (11, 5)), ((1, 24, 24), None, wedge, (11, 5))]


def columns_against_float64(dev, shape, crop, kind, window):
    B, H, W = shape
    rgb, nir, pred = Tc.inputs(shape)
    rect = centre(H, W, crop)
    valid = mask_planes(B, H, W, rect, kind)
    patch = PATCH[min(rect[2:])]
    ref = expected(rgb, nir, pred, valid, rect, patch, window)
    cap(ref, rect, f"{shape} crop {crop} window {window}")
    got = tile_metrics_masked_device(rgb.to(dev), nir.to(dev), pred.to(dev), valid.to(dev), crop=crop, window_size=window, patch=patch)
    assert got.shape == (B, len(TILE_METRIC_MASKED_COLUMNS)) and got.dtype == torch.float32 and got.device.type == torch.device(dev).type
    close_rows(got, ref, f"{shape} crop {crop} window {window}")
    return got


def raw_window_with_nan_outside(dev, window):
    """(3, 67, 93) cut by the raw entry to the 33 x 47 window at (17, 23): partial blocks, two 32-blocks per axis; NaN everywhere
    OUTSIDE the window in all six planes, the mask included"""
    shape, rect = (3, 67, 93), (17, 23, 33, 47)
    rgb, nir, pred = Tc.inputs(shape)
    valid = mask_planes(3, 67, 93, rect, wedge)
    ref = expected(rgb, nir, pred, valid, rect, PATCH[33], window)
    cap(ref, rect, f"raw 33x47 window {window}")
    inside = torch.zeros(67, 93, dtype=torch.bool)
    inside[17:17 + 33, 23:23 + 47] = True
    rgb, nir, pred, valid = (torch.where(inside, t, torch.tensor(NAN)) for t in (rgb, nir, pred, valid))
    got = raw_rows(dev, rgb, nir, pred, valid, rect, window, PATCH[33])
    close_rows(got, ref, f"raw 33x47 window {window}")


# ------------------------------------------------------------------------------------------------ 2. mask of ones
def ones_equal_the_unmasked_entry(dev, shape, crop):
    """n_valid == n_ssim == ch cw; l1, l2, psnr, the three indices and the patch means BITWISE those of nirgan_tile_metrics; ssim within
    the float64 bound of the module docstring of each other (printed: whether it is bitwise too)"""
    B, H, W = shape
    rgb, nir, pred = (t.to(dev) for t in Tc.inputs(shape))
    _, _, ch, cw = centre(H, W, crop)
    patch = PATCH[min(ch, cw)]
    plain = tile_metrics_device(rgb, nir, pred, crop=crop, patch=patch)
    got = tile_metrics_masked_device(rgb, nir, pred, torch.ones_like(nir), crop=crop, patch=patch)
    assert (got[:, 9:] == float(ch * cw)).all()
    for j, name in enumerate(TILE_METRIC_COLUMNS):
        if name != "ssim":
            assert torch.equal(bits(got[:, j]), bits(plain[:, j])), name
    a, b = got[:, 2].double().cpu(), plain[:, 2].double().cpu()
    same = torch.equal(bits(got[:, 2]), bits(plain[:, 2]))
    err = (a - b).abs().max().item()
    print(f"{shape} crop {crop}: ssim under a mask of ones is {'bitwise' if same else 'NOT bitwise'} the unmasked entry's, max diff {err:.3e}")
    assert err <= TOL * b.abs().max().item()
    return same


# ------------------------------------------------------------------------------------------------ 3. poison
def poison_at_dropped_pixels(dev):
    """(3, 67, 93) crop 41, wedge: NaN, +Inf and 1e30 at the invalid pixels of nir, pred and rgb against benign values there"""
    shape, crop = (3, 67, 93), 41
    rgb, nir, pred = Tc.inputs(shape)
    rect = centre(67, 93, crop)
    valid = mask_planes(3, 67, 93, rect, wedge)
    drop = valid == 0
    assert 0 < int(drop.sum()) < drop.numel()
    poison = torch.tensor([NAN, float("inf"), 1e30]).repeat(-(-67 * 93 // 3))[:67 * 93].view(1, 1, 67, 93)
    bad = [torch.where(drop, poison.roll(i, -1), t) for i, t in enumerate((rgb, nir, pred))]
    args = dict(crop=crop, window_size=11, patch=PATCH[41])
    benign = tile_metrics_masked_device(rgb.to(dev), nir.to(dev), pred.to(dev), valid.to(dev), **args)
    got = tile_metrics_masked_device(*(t.to(dev) for t in bad), valid.to(dev), **args)
    assert torch.isfinite(got).all() and torch.equal(bits(got), bits(benign))
    close_rows(got, expected(rgb, nir, pred, valid, rect, PATCH[41]), "poison")


# ------------------------------------------------------------------------------------------------ 4. edges
def all_invalid_tile_between_two(dev):
    shape, crop = (3, 67, 93), 41
    rgb, nir, pred = (t.to(dev) for t in Tc.inputs(shape))
    valid = mask_planes(3, 67, 93, centre(67, 93, crop), wedge)
    valid[1] = 0.0
    got = tile_metrics_masked_device(rgb, nir, pred, valid.to(dev), crop=crop, patch=9).cpu()
    assert (got[1, 9:] == 0).all() and torch.isnan(got[1, :9]).all()
    pick = [0, 2]
    two = tile_metrics_masked_device(rgb[pick], nir[pick], pred[pick], valid[pick].to(dev), crop=crop, patch=9).cpu()
    assert torch.equal(bits(two), bits(got[pick])) and torch.isfinite(two).all()


def no_clean_support_but_valid_pixels(dev):
    """12 x 12 with the centre 2 x 2 invalid: every support (window 11, reflected) holds one of them"""
    rgb, nir, pred = Tc.inputs((1, 12, 12))
    valid = torch.ones(1, 1, 12, 12)
    valid[0, 0, 5:7, 5:7] = 0.0
    ref = expected(rgb, nir, pred, valid, (0, 0, 12, 12), 8)
    assert ref[0, 10] == 0 and ref[0, 9] == 140 and math.isnan(ref[0, 2])
    got = tile_metrics_masked_device(rgb.to(dev), nir.to(dev), pred.to(dev), valid.to(dev), patch=8)
    close_rows(got, ref, "12x12 centre 2x2")
    assert torch.isfinite(got[0, [0, 1, 3, 4, 5, 6, 7, 8]]).all()


def patch_without_a_valid_pixel(dev):
    rgb, nir, pred = Tc.inputs((1, 24, 24))
    valid = torch.ones(1, 1, 24, 24)
    valid[0, 0, 8:16, 8:16] = 0.0                                                 # the centred patch of side 8
    ref = expected(rgb, nir, pred, valid, (0, 0, 24, 24), 8, 5)
    assert math.isnan(ref[0, 7]) and ref[0, 10] > 0
    got = tile_metrics_masked_device(rgb.to(dev), nir.to(dev), pred.to(dev), valid.to(dev), window_size=5, patch=8)
    close_rows(got, ref, "empty patch")
    assert torch.isnan(got[0, 7:9]).all()


def identical_images(dev):
    rgb, nir, _ = Tc.inputs((2, 40, 70))
    valid = mask_planes(2, 40, 70, (0, 0, 40, 70), wedge)
    rows = tile_metrics_masked_device(rgb.to(dev), nir.to(dev), nir.clone().to(dev), valid.to(dev), patch=32).cpu()
    col = {k: rows[:, j] for j, k in enumerate(TILE_METRIC_MASKED_COLUMNS)}
    for k in ("l1", "l2", "l1_ndvi", "l1_ndwi", "l1_evi"):
        assert (col[k] == 0).all(), k
    assert (col["psnr"] == float("inf")).all() and (col["ssim"] - 1).abs().max().item() <= TOL
    assert torch.equal(col["patch_mean_nir"], col["patch_mean_pred"]) and (col["n_ssim"] > 0).all()


def values_of_valid(dev):
    """-0.0f is invalid, 2.5f and a denormal are valid, as nirgan_valid_count counts them; integer and bool masks are taken as != 0"""
    rgb, nir, pred = Tc.inputs((1, 24, 24))
    keep = torch.from_numpy(wedge(24, 24))[None, None]
    denormal = float(np.float32(1e-42))
    assert 0.0 < denormal < float(np.finfo(np.float32).tiny)
    fancy = torch.where(keep, torch.tensor([2.5, denormal]).repeat(288).view(1, 1, 24, 24), torch.tensor(-0.0))
    assert (fancy[~keep] == 0).all() and torch.signbit(fancy[~keep]).all()
    args = (rgb.to(dev), nir.to(dev), pred.to(dev))
    base = tile_metrics_masked_device(*args, keep.float().to(dev), patch=8)
    assert base[0, 9] == float(keep.sum())
    for other in (fancy, keep, keep.to(torch.uint8), keep.long()[:, 0] * 7):
        assert torch.equal(bits(tile_metrics_masked_device(*args, other.to(dev), patch=8)), bits(base)), other.dtype
    assert torch.equal(bits(raw_rows(dev, *Tc.inputs((1, 24, 24)), fancy, (0, 0, 24, 24), 11, 8)), bits(base))


# ------------------------------------------------------------------------------------------------ 5. repeatability
def repeatable_and_batch_independent(dev):
    shape, crop = (5, 67, 93), 41
    rgb, nir, pred = (t.to(dev) for t in Tc.inputs(shape))
    valid = mask_planes(5, 67, 93, centre(67, 93, crop), wedge).to(dev)
    a = tile_metrics_masked_device(rgb, nir, pred, valid, crop=crop, patch=9)
    b = tile_metrics_masked_device(rgb, nir, pred, valid, crop=crop, patch=9)
    assert torch.equal(bits(a), bits(b)) and torch.isfinite(a).all()
    for i in range(5):
        alone = tile_metrics_masked_device(rgb[i:i + 1], nir[i:i + 1], pred[i:i + 1], valid[i:i + 1], crop=crop, patch=9)
        assert torch.equal(bits(alone[0]), bits(a[i])), i


# ------------------------------------------------------------------------------------------------ 6. raw entry
def null_rgb_and_no_patch_leave_their_columns(dev):
    shape, rect = (3, 67, 93), centre(67, 93, 41)
    rgb, nir, pred = Tc.inputs(shape)
    valid = mask_planes(3, 67, 93, rect, wedge)
    full = raw_rows(dev, rgb, nir, pred, valid, rect, 11, 9)
    close_rows(full, expected(rgb, nir, pred, valid, rect, 9), "raw entry")
    part = raw_rows(dev, None, nir, pred, valid, rect, 11, 0, rows_fill=-7.0)
    assert (part[:, 4:9] == -7.0).all()
    assert torch.equal(bits(part[:, :4]), bits(full[:, :4])) and torch.equal(bits(part[:, 9:]), bits(full[:, 9:]))


def refusals(be):
    """every bad field of the unmasked entry's test, valid = NULL and ch cw > 2^24: -1 and a message that names the entry, before
    any launch (the pointers lead nowhere a kernel could read 4100 x 4100 floats)"""
    assert be.nirgan_tile_metrics_masked(L.TileMetricsMaskedDesc(), None) == -1 and b"tile_metrics_masked" in be.nirgan_last_error()
    buf = torch.zeros(3 * 20 * 20 + 64)
    d = L.TileMetricsMaskedDesc()
    d.rgb = d.nir = d.pred = d.valid = d.ws = d.rows = buf.data_ptr()
    d.B, d.H, d.W, d.y0, d.x0, d.ch, d.cw = 1, 20, 20, 2, 2, 16, 16
    d.window, d.sigma, d.max_val, d.eps, d.patch, d.ws_elems = 11, 1.5, 1.0, 1e-12, 4, 1 << 20
    bad = [("window", 4, b"window"), ("window", 13, b"window"), ("y0", 5, b"outside"), ("x0", -1, b"outside"), ("cw", 19, b"outside"),
           ("ch", 5, b"radius"), ("patch", 17, b"patch"), ("ws_elems", 10, b"workspace"), ("nir", None, b"null"), ("pred", None, b"null"),
           ("ws", None, b"null"), ("rows", None, b"null"), ("B", 0, b"empty"), ("valid", None, b"null")]
    for field, value, word in bad:
        keep = getattr(d, field)
        setattr(d, field, value)
        assert be.nirgan_tile_metrics_masked(d, None) == -1, field
        msg = be.nirgan_last_error()
        assert b"tile_metrics_masked" in msg and word in msg, (field, msg)
        setattr(d, field, keep)
    d.H = d.W = 4100
    d.y0 = d.x0 = 0
    d.ch = d.cw = 4097                                                            # 4097^2 = 2^24 + 8193
    d.ws_elems = 1 << 40
    assert be.nirgan_tile_metrics_masked(d, None) == -1
    msg = be.nirgan_last_error()
    assert b"tile_metrics_masked" in msg and b"2^24" in msg, msg


WS_ARGS = [(16, 240, 240), (64, 240, 240), (3, 41, 41), (1, 12, 12), (5, 256, 256), (2, 33, 64), (3, 33, 47), (0, 4, 4), (1, 0, 4)]


# ------------------------------------------------------------------------------------------------ 8. calculate_metrics(valid=)
def pooled_expected(nir, pred, valid, window=5):
    """float64 {L1, L2, PSNR, SSIM} over the valid / support-clean pixels of the whole batch"""
    B, _, H, W = nir.shape
    ref = expected(None, nir, pred, valid, (0, 0, H, W), 0, window)
    out = {}
    for name, col, cnt in (("L1", 0, 9), ("L2", 1, 9), ("SSIM", 2, 10)):
        keep = ref[:, cnt] > 0
        out[name] = float((ref[keep, col] * ref[keep, cnt]).sum() / ref[keep, cnt].sum()) if bool(keep.any()) else NAN
    out["PSNR"] = NAN if math.isnan(out["L2"]) else (10.0 * math.log10(1.0 / out["L2"]) if out["L2"] > 0 else float("inf"))
    return out


def calculate_metrics_over_valid(dev):
    """(3, 1, 33, 47), another mask per tile, one of them all zero, against float64 pooled means; a batch without a valid pixel is NaN"""
    _, nir, pred = Tc.inputs((3, 33, 47))
    valid = mask_planes(3, 33, 47, (0, 0, 33, 47), wedge)
    valid[1] = 0.0
    ref = pooled_expected(nir, pred, valid)
    got = calculate_metrics(pred.to(dev), nir.to(dev), phase="val", valid=valid.to(dev))
    assert sorted(got) == ["val/L1", "val/L2", "val/PSNR", "val/SSIM"] and all(isinstance(v, float) for v in got.values())
    for k, v in ref.items():
        g = got["val/" + k]
        bound = PSNR_ABS if k == "PSNR" else TOL * abs(v)
        print(f"calculate_metrics(valid=) {k}: {g:.9g} vs {v:.9g}, err {abs(g - v):.3e} bound {bound:.3e}")
        assert abs(g - v) <= bound, k
    same = calculate_metrics(pred.to(dev), nir.to(dev), phase="val", valid=valid[:, 0].to(dev))          # [B, H, W]
    assert same == got
    none = calculate_metrics(pred.to(dev), nir.to(dev), valid=torch.zeros_like(valid).to(dev))
    assert sorted(none) == ["train/L1", "train/L2", "train/PSNR", "train/SSIM"] and all(math.isnan(v) for v in none.values())


# ------------------------------------------------------------------------------------------------ 9. / 11. the table
def masked_table_rows_equal_single_tile_metrics(dev, model, tiles, table, crop, patch):
    """row i of the masked table against float64 metrics of predict_step on tile i ALONE; ``tiles``: (rgb [3,H,W], nir [1,H,W],
    valid bool-like [H,W], coords or None) per tile"""
    from validation_utils.tile_metrics import MASKED_TABLE_KEYS
    assert tuple(table) == MASKED_TABLE_KEYS and table["id"] == list(range(len(tiles)))
    model.eval()
    got, ref = [], []
    for i, (rgb, nir, valid, coords) in enumerate(tiles):
        rgb, nir = rgb[None].float().cpu(), nir[None].float().cpu()
        with torch.no_grad():
            args = (rgb.to(dev), coords[None].to(dev)) if coords is not None and getattr(model, "with_coords", True) else (rgb.to(dev),)
            pred = model.predict_step(*args).float().cpu()
        H, W = nir.shape[-2:]
        rect = centre(H, W, crop)
        ref.append(expected(rgb, nir, pred, torch.as_tensor(valid).reshape(1, 1, H, W), rect, min(patch, *rect[2:]))[0])
        got.append([table[k][i] for k in TILE_METRIC_MASKED_COLUMNS])
    got, ref = torch.tensor(got, dtype=torch.float64), torch.stack(ref)
    close_rows(got, ref, "masked table")
    return ref


def same_table(a, b):
    """two tables key for key, value for value (NaN equals NaN: floats by repr)"""
    return list(a) == list(b) and all([repr(v) for v in a[k]] == [repr(v) for v in b[k]] for k in a)


def pool_scenes():
    """two uint16 scenes of 4 bands, 48 x 72 and 50 x 50, nodata 0: a solid band over the first 10 rows in all bands and one isolated
    nodata pixel in ONE band; every other value is nonzero"""
    rng = np.random.default_rng(29)
    out = []
    for (h, w), speck in (((48, 72), (30, 41)), ((50, 50), (37, 8))):
        a = rng.integers(200, 6000, size=(4, h, w), dtype=np.uint16)
        a[:, :10, :] = 0
        a[2, speck[0], speck[1]] = 0
        out.append(a)
    return out


def table_from_the_pool(dev, tmp_path, calls=None):
    """evaluate_tiles(masked=True) end to end from a ScenePool: each row against float64 whose mask comes from the RAW scene (a count
    of nodata values per pixel over the bands), the keys, the exact CSV round trip; KeyError without "valid"; masked=False unchanged"""
    import csv
    from nirgan_hip.data import ScenePool
    from validation_utils import MASKED_TABLE_KEYS, TABLE_KEYS, evaluate_tiles
    T = 24
    scenes = pool_scenes()
    pool = ScenePool(scenes, nodata=0, device=dev)
    grid = pool.grid_loader(4, T, max_invalid=T * T // 2, return_valid=True)
    tiles, delivered = [], []
    rows = grid.windows.host.tolist()
    for batch in grid:
        for i in range(batch["nir"].shape[0]):
            s, y0, x0, _ = rows[len(tiles)]
            raw = scenes[s][:, y0:y0 + T, x0:x0 + T]
            valid = torch.from_numpy((raw == 0).sum(axis=0) == 0)
            tiles.append((batch["rgb"][i].clone().cpu(), batch["nir"][i].clone().cpu(), valid, None))
            delivered.append(batch["valid"][i, 0].clone().cpu() != 0)
    assert len(tiles) == len(rows) >= 8 and any(not t[2].all() for t in tiles)
    assert all(torch.equal(a, t[2]) for a, t in zip(delivered, tiles))             # the pool's mask IS the raw scene's
    model = Tc.RgbOnlyModel().to(dev).eval()
    model.with_coords = False
    if calls is not None:
        del calls[:]
    path = tmp_path / "masked.csv"
    table = evaluate_tiles(model, grid, crop=None, batch_size=4, device=dev, csv_path=str(path), patch=8, masked=True)
    if calls is not None:
        assert calls.count("tile_metrics_masked") == len(grid) and "tile_metrics" not in calls
    ref = masked_table_rows_equal_single_tile_metrics(dev, model, tiles, table, None, 8)
    assert (ref[:, 9] > 0).all() and int((ref[:, 10] > 0).sum()) * 2 >= len(tiles)           # the cap, from the restatement
    assert (ref[:, 9] < T * T).any()
    assert all(math.isnan(v) for v in table["x"])
    lines = list(csv.reader(open(path)))
    assert lines[0] == [""] + list(MASKED_TABLE_KEYS) and len(lines) == 1 + len(tiles)
    for i, line in enumerate(lines[1:]):
        assert int(line[0]) == i and int(line[1]) == table["id"][i]
        assert [repr(float(v)) for v in line[2:]] == [repr(table[k][i]) for k in MASKED_TABLE_KEYS[1:]]      # repr round trip: exact
        assert all(v == "nan" for v, k in zip(line[2:], MASKED_TABLE_KEYS[1:]) if math.isnan(table[k][i]))
    # masked=False on the same loader: today's table, from the unmasked entry alone
    plain_loader = pool.grid_loader(4, T, max_invalid=T * T // 2)
    with __import__("pytest").raises(KeyError, match="valid"):
        evaluate_tiles(model, plain_loader, crop=None, batch_size=4, device=dev, patch=8, masked=True)
    if calls is not None:
        del calls[:]
    unmasked = evaluate_tiles(model, grid, crop=None, batch_size=4, device=dev, patch=8)
    if calls is not None:
        assert calls.count("tile_metrics") == len(grid) and "tile_metrics_masked" not in calls
    assert tuple(unmasked) == TABLE_KEYS
    assert same_table(unmasked, evaluate_tiles(model, plain_loader, crop=None, batch_size=4, device=dev, patch=8))
    assert unmasked["l1"] != [table["l1"][i] for i in range(len(tiles))]            # and the mask does change the numbers
