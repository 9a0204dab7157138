"""Case bodies of the valid-pixel masks (nirgan_scene_valid / nirgan_valid_count / nirgan_pix_loss_masked, ``return_valid`` of
nirgan_hip.data, the masked losses of nirgan_hip.functional and the masked step of nirgan_hip.trainer), shared by
tests/test_valid_mask_emulated.py (numpy emulator, CPU) and tests/test_gpu_valid_mask.py (MI355X).

Expected values.  The mask: the restatement of tests/emu_valid_mask.py (numpy integers on the prefix table of tests/emu_scene_pool.py)
and, beside it, a count of nodata values in the RAW scene that never sees a prefix table; both comparisons are bitwise.  The count:
``np.count_nonzero``.  The masked loss: float64 torch (autograd through ``nirgan_oracle.rs_index_pairs``) with the error bounds that
tests/streaming_cases.py holds nirgan_pix_loss to -- the same ``Fx`` pairs, the same operation counts, the divisor 1 / count in the
place of 1 / n and the sums running over the kept pixels; nothing is loosened.  The step: float64 masked means of the step's own
prediction, and the unmasked step itself where the mask is all ones (bitwise).

Guards: every raw output sits between two bands of GUARD elements of a known value and starts as NaN, so an element that was not
written, or one written outside, shows.  Every mask case asserts FROM THE RESTATEMENT that between 10 % and 90 % of its mask is 1 (so
it is checked without a GPU); the draw of a sampled case is the first one for which that holds, found on the restatement's own draw.
A pool without ``nodata`` has no such draw: its mask is asserted to be all ones instead.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import api_cases as A
import emu_scene_pool as E
import emu_scene_scale as Es
import emu_valid_mask as V
import nirgan_oracle as O
import streaming_cases as St
from nirgan_hip import functional as HF
from nirgan_hip import lib as L
from nirgan_hip.data import ScenePool

GUARD = 64
F_GUARD = -12345.0
SHAPES = [(23, 31), (40, 17), (9, 64), (70, 67)]
BANDS = (2, 1, 0, 4)
NODATA = 0
SEED = 0x5EEDC0DE0BADF00D
AUGMENTS = {"none": 1, "flips": 4, "d4": 8}
T_SMALL = 5
SAMPLED = [(B, aug, scales) for B in (1, 3, 17) for aug in ("none", "flips", "d4") for scales in ((1,), (1, 2, 3), (3,))]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_t(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def stream(dev):
    return torch.cuda.current_stream().cuda_stream if torch.device(dev).type == "cuda" else None


def guarded(dev, n, start=float("nan")):
    """(buffer, view of its n inner elements)"""
    buf = torch.full((GUARD + n + GUARD,), F_GUARD, dtype=torch.float32, device=dev)
    buf[GUARD:GUARD + n] = start
    return buf, buf[GUARD:GUARD + n]


def guard_intact(buf, n):
    return bool((buf[:GUARD] == F_GUARD).all()) and bool((buf[GUARD + n:] == F_GUARD).all()) and buf.numel() == n + 2 * GUARD


# ------------------------------------------------------------------------------------------------ the pool
@functools.lru_cache(maxsize=None)
def mask_scenes(kind="u16", seed=11):
    """four scenes [5][H][W]: values 1 .. 65535; 1 % of the pixels nodata in ONE random band (band 3 is not selected: there it does
    not count), plus a solid wedge from the top-left corner of about a quarter of the scene in every band"""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in SHAPES:
        a = rng.integers(1, 65536, size=(5, h, w), dtype=np.uint16)
        speck = rng.random((h, w)) < 0.01
        band = rng.integers(0, 5, size=(h, w))
        for c in range(5):
            a[c][speck & (band == c)] = NODATA
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        a[:, yy / h + xx / w < 0.7] = NODATA
        out.append(a)
    if kind == "u16":
        return tuple(out)
    return tuple(np.where(a == NODATA, np.float32("nan"), a.astype(np.float32)).astype(np.float32) for a in out)


def mask_pool(dev, kind="u16", nodata=True):
    scenes = list(mask_scenes(kind))
    pool = ScenePool(scenes, bands=BANDS, divisor=10000.0 if kind == "u16" else 1.0, nodata=(NODATA if nodata else None), device=dev)
    prefixes = [E.prefix_table(E.invalid_mask(s[list(BANDS)], NODATA)) for s in scenes] if nodata else None
    return scenes, pool, prefixes


def raw_masks(scenes, rows, T):
    """float32 [n][1][T][T] from the RAW scenes: 1 where no pixel of the f x f block is nodata (NaN) in any selected band"""
    out = np.zeros((len(rows), 1, T, T), np.float32)
    for i, (s, y0, x0, word) in enumerate(tuple(int(v) for v in r) for r in rows):
        view, f = (word & 0xFFFFFFFF) & 7, (((word & 0xFFFFFFFF) >> 16) & 7) + 1
        side = f * T
        bad = E.invalid_mask(scenes[s][list(BANDS), y0:y0 + side, x0:x0 + side], NODATA)
        D = ~bad.reshape(T, f, T, f).any(axis=(1, 3))
        ii, jj = E.view_index(view, T)
        out[i, 0] = D[ii, jj].astype(np.float32)
    return out


def in_range(mask, what):
    frac = float(mask.mean())
    assert 0.1 <= frac <= 0.9, f"{what}: {frac:.3f} of the mask is 1"


def pick_draw(prefixes, T, B, views, factors):
    """the first draw whose batch has between 10 % and 90 % of its mask set, on the restatement alone"""
    for draw in range(400):
        rows = Es.draw_scaled(SHAPES, T, B, views, SEED, draw, factors, [1] * len(factors), 0, prefixes, T * T)
        if 0.1 <= float(V.masks_of_rows(SHAPES, prefixes, rows.tolist(), T).mean()) <= 0.9:
            return draw, rows
    raise AssertionError("no draw in 0 .. 399 has a mixed mask")


def sampled_masks(dev, kind, B, augment, scales):
    """rows straight from ``sample(..., return_windows=True, return_valid=True)``, everything accepted: the mask against the
    restatement and against the raw scene, its buffer guarded; ``gather`` gives the same mask for the same rows"""
    T = T_SMALL
    scenes, pool, prefixes = mask_pool(dev, kind)
    draw, rows_want = pick_draw(prefixes, T, B, AUGMENTS[augment], scales)
    out = pool._outputs(B, T)
    buf, inner = guarded(dev, B * T * T)
    out["valid"] = inner.view(B, 1, T, T)
    got = pool.sample(B, T, seed=SEED, draw=draw, augment=augment, max_invalid=T * T, scales=None if scales == (1,) else scales,
                      return_windows=True, return_valid=True, out=out)
    sync(dev)
    rows = got["window"].cpu().numpy()
    assert np.array_equal(rows.view(np.uint32).astype(np.int64), rows_want)
    want = V.masks_of_rows(SHAPES, prefixes, rows.tolist(), T)
    in_range(want, (B, augment, scales))
    assert np.array_equal(want, raw_masks(scenes, rows.tolist(), T)), "the restatement disagrees with the raw scene"
    assert E_same(got["valid"], want), (B, augment, scales, draw)
    assert guard_intact(buf, B * T * T)
    again = pool.gather(got["window"], T, return_valid=True)
    assert E_same(again["valid"], want) and same_t(again["rgb"], got["rgb"]) and same_t(again["nir"], got["nir"])
    plain = pool.sample(B, T, seed=SEED, draw=draw, augment=augment, max_invalid=T * T, scales=None if scales == (1,) else scales)
    assert "valid" not in plain and "window" not in plain and same_t(plain["rgb"], got["rgb"])


def E_same(got, want):
    g = got.detach().cpu().contiguous().numpy()
    return g.shape == want.shape and np.array_equal(g.view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))


def raw_valid(dev, pool, rows, T, host=True, table=None, first=0, n=None, keep=None):
    """one nirgan_scene_valid call on the rows (numpy int32 [m][4]) into a guarded buffer -> (rc, buffer, view [n][1][T][T])"""
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    n = len(rows) - first if n is None else n
    wdev = torch.from_numpy(rows.copy()).to(dev)
    buf, inner = guarded(dev, n * T * T)
    tdev, thost = pool._table(T) if table is None else (torch.from_numpy(table.copy()).to(dev), table)
    d = L.SceneValidDesc()
    d.S, d.table, d.table_host = len(pool.shapes), tdev.data_ptr(), thost.ctypes.data
    d.prefix, d.prefix_elems = (pool.prefix.data_ptr() if pool.prefix is not None else None), pool.prefix_elems
    d.tile, d.window, d.window_host = T, wdev.data_ptr(), (rows.ctypes.data if host else None)
    d.n_windows, d.first, d.n, d.valid = len(rows), first, n, inner.data_ptr()
    rc = L.backend().nirgan_scene_valid(C.byref(d), stream(dev))
    sync(dev)
    if keep is not None:
        keep.extend((wdev, tdev, thost, rows))
    return rc, buf, inner.view(n, 1, T, T)


PLACED = [(67, 1, (2, 0)), (4, 8, (36, 33)), (22, 3, (3, 1))]                  # (T, f, origin) on the 70 x 67 scene


def placed_rows(T, f, origin):
    return np.asarray([(3, origin[0], origin[1], g | ((f - 1) << 16)) for g in range(8)], dtype=np.int32)


def placed_masks(dev, T, f, origin):
    """hand-placed rows on the 70 x 67 scene, all eight views in one call, with and without the host copy: full 64-blocks and a
    partial one (T = 67), the widest factor (T = 4, f = 8), a partial block with a factor (T = 22, f = 3)"""
    scenes, pool, prefixes = mask_pool(dev)
    rows = placed_rows(T, f, origin)
    want = V.masks_of_rows(SHAPES, prefixes, rows.tolist(), T)
    in_range(want, (T, f))
    assert np.array_equal(want, raw_masks(scenes, rows.tolist(), T))
    assert len({want[g].tobytes() for g in range(8)}) == 8, "the eight views of this window do not differ"
    for host in (True, False):
        rc, buf, got = raw_valid(dev, pool, rows, T, host)
        assert rc == 0, L.backend().nirgan_last_error()
        assert E_same(got, want), (T, f, host)
        assert guard_intact(buf, got.numel())
    rc, buf, got = raw_valid(dev, pool, rows, T, True, first=3, n=2)            # rows 3 and 4 of the list alone
    assert rc == 0 and E_same(got, want[3:5]) and guard_intact(buf, got.numel())


def float_pool_masks(dev):
    sampled_masks(dev, "f32", 17, "d4", (1, 2, 3))


def pool_without_nodata_is_all_ones(dev):
    T, B = T_SMALL, 17
    scenes, pool, _ = mask_pool(dev, nodata=False)
    got = pool.sample(B, T, seed=SEED, draw=3, augment="d4", scales=(1, 2, 3), return_windows=True, return_valid=True)
    sync(dev)
    assert got["valid"].shape == (B, 1, T, T) and bool((got["valid"] == 1).all())
    rows = got["window"].cpu().numpy()
    assert np.array_equal(V.masks_of_rows(SHAPES, None, rows.tolist(), T), np.ones((B, 1, T, T), np.float32))
    assert raw_masks(scenes, rows.tolist(), T).mean() < 1.0                      # the pixels ARE nodata; without ``nodata`` nobody says so


def scene_without_a_table(dev):
    """scene 0's table entry is -1, the others keep theirs: ones for its rows, the table's verdict for the rest"""
    T = T_SMALL
    scenes, pool, prefixes = mask_pool(dev)
    table = pool._table(T)[1].copy()
    table[0, 4] = -1
    rows = np.asarray([(0, 2, 3, 5), (3, 20, 10, 6), (0, 0, 0, 0), (1, 8, 2, 3 | (1 << 16)), (3, 30, 20, 2 << 16)], dtype=np.int32)
    want = V.masks_of_rows(SHAPES, [None] + prefixes[1:], rows.tolist(), T)
    in_range(want, "table -1")
    assert (want[[0, 2]] == 1).all() and raw_masks(scenes, rows.tolist(), T)[[0, 2]].mean() < 1.0
    assert np.array_equal(want[[1, 3, 4]], raw_masks(scenes, rows.tolist(), T)[[1, 3, 4]])
    for host in (True, False):
        rc, buf, got = raw_valid(dev, pool, rows, T, host, table=table)
        assert rc == 0 and E_same(got, want) and guard_intact(buf, got.numel()), host


def rows_outside_their_scene(dev):
    """without the host copy the kernel bounds the rows: zeros for them, the neighbours unaffected; with it they are refused, the
    message naming the row"""
    T = T_SMALL
    scenes, pool, prefixes = mask_pool(dev)
    H, W = SHAPES[3]
    good = [(3, 20, 10, 6), (1, 8, 2, 3 | (1 << 16)), (3, 30, 20, 2 << 16), (0, 4, 9, 1)]
    bad = [(len(SHAPES), 0, 0, 0), (3, -1, 0, 0), (3, 0, W - 2 * T + 1, 1 << 16)]
    rows = np.asarray([good[0], bad[0], good[1], bad[1], bad[2], good[2], good[3]], dtype=np.int32)
    want = V.masks_of_rows(SHAPES, prefixes, rows.tolist(), T)
    in_range(want, "rows outside")
    assert not want[[1, 3, 4]].any() and np.array_equal(want[[0, 2, 5, 6]], raw_masks(scenes, [good[0], good[1], good[2], good[3]], T))
    rc, buf, got = raw_valid(dev, pool, rows, T, host=False)
    assert rc == 0 and E_same(got, want) and guard_intact(buf, got.numel())
    be = L.backend()
    for i in (1, 3, 4):
        part = rows.copy()
        for j in (1, 3, 4):
            if j != i:
                part[j] = good[0]
        rc, buf, got = raw_valid(dev, pool, part, T, host=True)
        assert rc != 0 and f"row {i}".encode() in be.nirgan_last_error(), (i, be.nirgan_last_error())
        assert bool(torch.isnan(got).all()) and guard_intact(buf, got.numel()), "the refused call launched something"


def loader_carries_valid(dev):
    """the loader's batches carry ``valid`` in one tensor of its own; ``gather`` of the batch's rows gives the same mask"""
    T, B = T_SMALL, 3
    scenes, pool, prefixes = mask_pool(dev)
    ld = pool.loader(B, T, 3, seed=SEED, augment="d4", max_invalid=T * T, scales=(1, 2), return_valid=True)
    ptrs = set()
    for batch in ld:
        assert sorted(batch) == ["nir", "rgb", "valid"]
        ptrs.add(batch["valid"].data_ptr())
        rows = ld._buffers["window"]
        again = pool.gather(rows, T, return_valid=True)
        sync(dev)
        assert same_t(again["valid"], batch["valid"]) and same_t(again["rgb"], batch["rgb"])
        assert E_same(batch["valid"], V.masks_of_rows(SHAPES, prefixes, rows.cpu().numpy().tolist(), T))
    assert len(ptrs) == 1
    assert sorted(next(iter(pool.loader(B, T, 1, seed=SEED)))) == ["nir", "rgb"]
    grid = pool.grid_loader(4, T, factors=(1, 2), max_invalid=T * T, return_valid=True)
    seen = 0
    for batch in grid:
        n = batch["valid"].shape[0]
        want = V.masks_of_rows(SHAPES, prefixes, grid.windows.host[seen:seen + n].tolist(), T)
        assert E_same(batch["valid"], want)
        seen += n
    assert seen == len(grid.windows) and "valid" not in next(iter(pool.grid_loader(4, T, max_invalid=T * T)))
    # both halves of a split take the keyword as the pool does
    split = pool.split([(3, 40, 30, 24, 30)], guard=1)
    got = split.train.sample(17, T, seed=SEED, draw=1, max_invalid=T * T, scales=(1, 2), return_windows=True, return_valid=True)
    sync(dev)
    assert E_same(got["valid"], V.masks_of_rows(SHAPES, prefixes, got["window"].cpu().numpy().tolist(), T))
    for batch in split.train.loader(B, T, 2, seed=SEED, max_invalid=T * T, return_valid=True):
        assert batch["valid"].shape == (B, 1, T, T)
    held = split.val.grid_loader(4, T, max_invalid=T * T, return_valid=True)
    rows = held.windows.host
    masks = torch.cat([b["valid"].clone() for b in held])
    assert E_same(masks, V.masks_of_rows(SHAPES, prefixes, rows.tolist(), T))
    assert same_t(split.val.gather(rows, T, return_valid=True)["valid"], masks)


def valid_refusals(be):
    """argument errors of nirgan_scene_valid on HOST buffers: nothing is launched by a refused call"""
    keep = {"table": torch.tensor([[0, 6, 7, 20, 0]], dtype=torch.int64), "window": torch.tensor([[0, 1, 1, 0], [0, 0, 0, 0]], dtype=torch.int32),
            "prefix": torch.zeros(7 * 8, dtype=torch.int32), "valid": torch.zeros(2 * 9)}

    def fresh():
        d = L.SceneValidDesc()
        d.S, d.tile, d.n_windows, d.first, d.n = 1, 3, 2, 0, 2
        d.table = d.table_host = keep["table"].data_ptr()
        d.window = d.window_host = keep["window"].data_ptr()
        d.prefix, d.prefix_elems, d.valid = keep["prefix"].data_ptr(), 56, keep["valid"].data_ptr()
        return d
    cases = [(f"null {f}", (lambda f: lambda d: setattr(d, f, None))(f), b"null") for f in ("table", "table_host", "window", "valid")]
    cases += [("S 0", lambda d: setattr(d, "S", 0), b"pool"), ("tile 0", lambda d: setattr(d, "tile", 0), b"tile"),
              ("n 0", lambda d: setattr(d, "n", 0), b"tile"), ("tile 2^16", lambda d: setattr(d, "tile", 1 << 16), b"tile"),
              ("first -1", lambda d: setattr(d, "first", -1), b"first"), ("first 1", lambda d: setattr(d, "first", 1), b"first"),
              ("prefix_elems -1", lambda d: setattr(d, "prefix_elems", -1), b"prefix_elems"),
              ("prefix_elems 55", lambda d: setattr(d, "prefix_elems", 55), b"prefix table of scene 0")]
    for what, change, msg in cases:
        d = fresh()
        change(d)
        assert be.nirgan_scene_valid(C.byref(d), None) != 0 and msg in be.nirgan_last_error(), (what, be.nirgan_last_error())
    assert be.nirgan_scene_valid(None, None) != 0
    for word, msg in ((1 << 3, b"row 1"), (1 << 20, b"row 1")):
        keep["window"][1, 3] = word
        assert be.nirgan_scene_valid(C.byref(fresh()), None) != 0 and msg in be.nirgan_last_error()
    keep["window"][1, 3] = 0
    count = torch.zeros(1, dtype=torch.int32)
    assert be.nirgan_valid_count(None, 4, count.data_ptr(), None) != 0 and b"valid_count" in be.nirgan_last_error()
    assert be.nirgan_valid_count(keep["valid"].data_ptr(), 4, None, None) != 0
    assert be.nirgan_valid_count(keep["valid"].data_ptr(), 0, count.data_ptr(), None) != 0
    assert be.nirgan_valid_count(keep["valid"].data_ptr(), 1 << 31, count.data_ptr(), None) != 0
    d = L.PixLossMaskedDesc()
    assert be.nirgan_pix_loss_masked(C.byref(d), None) != 0 and b"pix_loss_masked" in be.nirgan_last_error()


# ------------------------------------------------------------------------------------------------ count
COUNT_N = (1, 63, 64, 65, 4097)


def count_is_exact(dev, n):
    gen = torch.Generator().manual_seed(n)
    special = torch.zeros(n)
    special[::3] = -0.0
    special[1::3] = 2.5
    special[2::3] = 1e-41                                                        # a denormal
    for what, mask in (("zeros", torch.zeros(n)), ("ones", torch.ones(n)), ("half", (torch.rand(n, generator=gen) < 0.5).float()),
                       ("special", special)):
        want = int(np.count_nonzero(mask.numpy()))
        if what == "special":
            assert want == n - len(range(0, n, 3))
        m = mask.to(dev)
        count = torch.full((3,), -77, dtype=torch.int32, device=dev)
        L.call("nirgan_valid_count", m.data_ptr(), n, count.data_ptr() + 4, stream(dev))
        sync(dev)
        assert count.cpu().tolist() == [-77, want, -77], (what, n, count.cpu().tolist())


# ------------------------------------------------------------------------------------------------ masked loss
LOSS_SHAPES = [(1, 5, 5), (3, 67, 93), (2, 64, 64)]
LOSS_VARIANTS = ["all seven", "log_all, l1 only", "no rgb", "extra"]           # log_all 0 / 1, rgb NULL, with / without extra


@functools.lru_cache(maxsize=None)
def half_mask(shape):
    B, H, W = shape
    gen = torch.Generator().manual_seed(91)
    m = (torch.rand(B, 1, H, W, generator=gen) < 0.5).float()
    assert 0 < m.sum() < m.numel()
    return m


def masked_desc(dev, shape, variant, criterion, valid, count, keep, inputs=None):
    """a nirgan_pix_loss_masked descriptor on guarded sums, gradient and workspace -> (d, sums, grad, buffers)"""
    w, log_all, with_rgb, with_grad, with_extra = St.PIX_VARIANTS[variant]
    rgb, nir, pred, extra = (t.to(dev).contiguous() for t in (inputs if inputs is not None else St.pix_inputs(shape)))
    n = nir.numel()
    bufs = {"sums": guarded(dev, 7), "grad": guarded(dev, n), "ws": guarded(dev, L.PIX_LOSS_WS_ELEMS, 0.0)}
    bufs["sums"][1][:] = St.SUMS0.to(dev)
    valid_, count_ = valid.to(dev).contiguous(), torch.tensor([count], dtype=torch.int32, device=dev)
    d = L.PixLossMaskedDesc()
    d.rgb, d.nir, d.pred = rgb.data_ptr() if with_rgb else None, nir.data_ptr(), pred.data_ptr()
    d.B, d.H, d.W = shape
    d.w_l1, d.w_ndvi, d.w_ndwi, d.w_gndvi, d.w_savi, d.w_msavi, d.w_evi = w
    d.criterion, d.log_all = criterion, log_all
    if with_extra:
        d.extra, d.extra_cs, d.extra_c, d.extra_scale = extra.data_ptr(), St.EXTRA[0], St.EXTRA[1], St.EXTRA[2]
    d.sums, d.grad_pred = bufs["sums"][1].data_ptr(), bufs["grad"][1].data_ptr() if with_grad else None
    d.ws, d.ws_elems = bufs["ws"][1].data_ptr(), L.PIX_LOSS_WS_ELEMS
    d.valid, d.count = valid_.data_ptr(), count_.data_ptr()
    keep.extend((rgb, nir, pred, extra, valid_, count_, bufs))
    return d, bufs["sums"][1], bufs["grad"][1].view(nir.shape), bufs


def loss_guards_intact(bufs):
    return all(guard_intact(buf, inner.numel()) for buf, inner in bufs.values())


def ones_equal_the_unmasked_entry(dev, shape):
    """a mask of ones and count = n: the seven sums and grad_pred are bitwise nirgan_pix_loss's"""
    n = shape[0] * shape[1] * shape[2]
    for variant in LOSS_VARIANTS:
        for criterion in (0, 1):
            keep = []
            d0, sums0, grad0 = St.pix_desc(dev, shape, variant, criterion, keep)
            L.call("nirgan_pix_loss", C.byref(d0), stream(dev))
            d, sums, grad, bufs = masked_desc(dev, shape, variant, criterion, torch.ones(shape[0], 1, *shape[1:]), n, keep)
            L.call("nirgan_pix_loss_masked", C.byref(d), stream(dev))
            sync(dev)
            assert same_t(sums, sums0), (shape, variant, criterion, sums.cpu(), sums0.cpu())
            assert same_t(grad, grad0), (shape, variant, criterion)
            assert loss_guards_intact(bufs)


@functools.lru_cache(maxsize=8)
def masked_case(shape, variant, criterion):
    """``streaming_cases.pix_case`` over the kept pixels of ``half_mask``: float64 sums and gradient by autograd, their bounds from
    the kernel's operations on Fx pairs -- the sums over the kept pixels, 1 / count in the place of 1 / n (the per-thread number of
    additions, which bounds how often a partial sum is rounded, is the grid's and stays)"""
    w, log_all, with_rgb, with_grad, with_extra = St.PIX_VARIANTS[variant]
    w32 = [torch.tensor(v, dtype=torch.float32).double().item() for v in w]
    rgb, nir, pred, extra = St.pix_inputs(shape)
    keep = half_mask(shape).bool()
    n, count = nir.numel(), int(keep.sum())
    y = pred.double().requires_grad_(True)
    x = nir.double()
    active = [k for k in range(1, 7) if log_all or w32[k] != 0]
    pairs = O.rs_index_pairs(rgb.double(), x, y, "loss") if with_rgb else {}
    crit = (lambda a, b: ((a - b).abs() * keep).sum()) if criterion == 0 else (lambda a, b: (((a - b) ** 2) * keep).sum())
    terms = {0: ((y - x).abs() * keep).sum()}
    for k in active:
        terms[k] = crit(*pairs[St.PIX_NAMES[k]])
    total = sum(w32[k] * t for k, t in terms.items()) / count
    total.backward()
    grad = y.grad.clone()
    blocks = St.pix_grid(n)
    ksum = -(-n // (256 * blocks)) + 6 + 4 + -(-blocks // 256) + 8 + 1
    sums, sums_b = St.SUMS0.double().clone(), torch.zeros(7, dtype=torch.float64)
    R, G, Bl = (St.Fx(rgb[:, i:i + 1].double()) for i in range(3))
    d0 = St.fsub(St.Fx(pred.double()), St.Fx(x))
    g = St.Fx(w32[0] * torch.sign(d0.v))
    term_b = {0: (d0.v.abs(), d0.e)}
    for k in active:
        f, df = St.fx_index(k, St.Fx(pred.double()), R, G, Bl)
        a, _ = St.fx_index(k, St.Fx(x), R, G, Bl)
        d = St.fsub(f, a)
        val, dval = (St.Fx(d.v.abs(), d.e), St.Fx(torch.sign(d.v))) if criterion == 0 else (St.fmul(d, d), St.fmul(2.0, d))
        term_b[k] = (val.v, val.e)
        if w32[k] != 0:
            g = St.fadd(g, St.fmul(St.fmul(w32[k], dval), df))
    for k, (v, e) in term_b.items():
        sums[k] += terms[k].detach()
        assert abs((v * keep).sum() - terms[k].detach()) <= 1e-11 * (v * keep).sum()
        sums_b[k] = (e * keep).sum() + ksum * St.U * (St.SUMS0[k].double() + (v * keep).sum())
    g = St.fmul(g, St.Fx(1.0 / count, torch.tensor(St.U / count, dtype=torch.float64)))
    g = St.Fx(g.v * keep, g.e * keep)                                            # a dropped pixel: exactly 0 before the extra term
    assert (g.v - grad).abs().max() <= 1e-11 * grad.abs().max()
    if with_extra:
        ex = extra[..., St.EXTRA[1]].double().reshape(grad.shape)
        s = torch.tensor(St.EXTRA[2], dtype=torch.float32).double().item()
        grad = grad + s * ex
        g = St.fadd(g, St.fmul(s, ex))
    return {"sums": sums, "sums_b": sums_b, "grad": grad, "grad_b": g.e, "active": active, "count": count}


def half_mask_against_float64(dev, shape):
    for variant in LOSS_VARIANTS:
        for criterion in (0, 1):
            c, keep = masked_case(shape, variant, criterion), []
            d, sums, grad, bufs = masked_desc(dev, shape, variant, criterion, half_mask(shape), c["count"], keep)
            L.call("nirgan_pix_loss_masked", C.byref(d), stream(dev))
            sync(dev)
            what = f"{shape} {variant} criterion {criterion}"
            St.within("pix_loss_masked", what + " sums", sums, c["sums"], c["sums_b"])
            idle = [k for k in range(1, 7) if k not in c["active"]]
            assert St.same(sums[idle], St.SUMS0[idle]), what + ": an index that is off moved its sum"
            St.within("pix_loss_masked", what + " grad", grad, c["grad"], c["grad_b"])
            assert loss_guards_intact(bufs)


def extra_term(dev, shape, variant):
    """the fp32 gradient of a dropped pixel: extra_scale * extra[..., c] rounded once, or +0.0"""
    if not St.PIX_VARIANTS[variant][4]:
        return torch.zeros(shape[0], 1, *shape[1:])
    extra = St.pix_inputs(shape)[3]
    return (torch.tensor(St.EXTRA[2], dtype=torch.float32) * extra[..., St.EXTRA[1]]).reshape(shape[0], 1, *shape[1:])


def garbage_at_dropped_pixels(dev, shape):
    """NaN, +Inf and 0 in rgb, nir and pred where the mask is 0, then benign values there: every output bitwise the same and
    finite, the gradient of a dropped pixel exactly the extra term"""
    valid = half_mask(shape)
    dropped = valid == 0
    count = int(valid.sum())
    rgb, nir, pred, extra = St.pix_inputs(shape)
    junk = torch.tensor([float("nan"), float("inf"), 0.0])[torch.arange(nir.numel()).reshape(nir.shape) % 3]

    def with_junk(t):
        return torch.where(dropped.expand_as(t), junk.expand_as(t), t)
    for variant in LOSS_VARIANTS:
        for criterion in (0, 1):
            outs = []
            for inputs in ((with_junk(rgb), with_junk(nir), with_junk(pred), extra), (rgb, nir, pred, extra)):
                keep = []
                d, sums, grad, bufs = masked_desc(dev, shape, variant, criterion, valid, count, keep, inputs)
                L.call("nirgan_pix_loss_masked", C.byref(d), stream(dev))
                sync(dev)
                assert loss_guards_intact(bufs)
                outs.append((sums.cpu().clone(), grad.cpu().clone()))
            (s1, g1), (s2, g2) = outs
            assert same_t(s1, s2) and same_t(g1, g2), (shape, variant, criterion)
            assert bool(torch.isfinite(s1).all()) and bool(torch.isfinite(g1).all())
            assert torch.equal(bits(g1)[dropped], bits(extra_term(dev, shape, variant))[dropped]), (shape, variant, criterion)


def count_zero(dev, shape):
    """no valid pixel: the sums do not move, the gradient is the extra term everywhere; Python's masked loss is 0.0 with a zero
    gradient"""
    zeros = torch.zeros(shape[0], 1, *shape[1:])
    for variant in LOSS_VARIANTS:
        keep = []
        d, sums, grad, bufs = masked_desc(dev, shape, variant, 0, zeros, 0, keep)
        L.call("nirgan_pix_loss_masked", C.byref(d), stream(dev))
        sync(dev)
        assert same_t(sums, St.SUMS0) and same_t(grad, extra_term(dev, shape, variant)) and loss_guards_intact(bufs), variant
    rgb, nir, pred, _ = (t.to(dev) for t in St.pix_inputs(shape))
    pred = pred.clone().requires_grad_(True)
    loss = HF.pix_loss(rgb, nir, pred, St.ALL_W, 0, zeros.to(dev))
    loss.backward()
    assert float(loss.detach()) == 0.0 and bool((pred.grad == 0).all())
    assert bool((HF.index_sums(rgb, nir, pred, 0, zeros.to(dev)) == 0).all())


def python_masked_loss(dev, shape):
    """``pix_loss`` / ``index_sums`` / ``HipL1Loss`` / ``RemoteSensingIndices`` with ``valid``: the masked means of float64, and the
    unmasked calls bitwise where the mask is all ones"""
    from model.pix2pix import HipL1Loss
    from utils.remote_sensing_indices import RemoteSensingIndices
    rgb, nir, pred, _ = (t.to(dev) for t in St.pix_inputs(shape))
    valid = half_mask(shape).to(dev)
    c = masked_case(shape, "all seven", 0)
    p = pred.clone().requires_grad_(True)
    loss = HF.pix_loss(rgb, nir, p, St.ALL_W, 0, valid != 0)                      # a bool mask is taken as valid != 0
    (loss * 2.0).backward()
    w32 = torch.tensor(St.ALL_W, dtype=torch.float32).double()
    want = float((w32 * (c["sums"] - St.SUMS0.double())).sum() / c["count"])
    assert abs(float(loss.detach()) - want) <= 1e-5 * abs(want)
    St.within("python masked", "grad", p.grad / 2.0, c["grad"], c["grad_b"] + St.U * c["grad"].abs())
    ones = torch.ones_like(valid)

    def two_roundings(a, b):
        """The sums ARE bitwise the unmasked entry's (``ones_equal_the_unmasked_entry``); the bridges then divide them on the device,
        the unmasked one by a host scalar -- which torch may turn into a product with the rounded reciprocal -- and the masked one
        by the device's count: a correctly rounded quotient against a product of two rounded factors, at most 2 u apart"""
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return bool(((a - b).abs() <= 2 * St.U * b.abs()).all())
    assert two_roundings(HF.pix_loss(rgb, nir, pred, St.ALL_W, 1, ones), HF.pix_loss(rgb, nir, pred, St.ALL_W, 1))
    assert two_roundings(HF.index_sums(rgb, nir, pred, 1, ones), HF.index_sums(rgb, nir, pred, 1))
    l1 = HipL1Loss()(pred, nir, valid)
    want = float(((pred.double() - nir.double()).abs() * valid.double()).sum() / valid.double().sum())
    assert abs(float(l1) - want) <= 1e-5 * want and two_roundings(HipL1Loss()(pred, nir, ones), HipL1Loss()(pred, nir))
    rs = RemoteSensingIndices(mode="loss", criterion="l1")
    got = rs.get_and_weight_losses(rgb, nir, pred, loss_config=dict(A.RS_W), valid=valid)
    pairs = O.rs_index_pairs(rgb.double().cpu(), nir.double().cpu(), pred.double().cpu(), "loss")
    m = half_mask(shape).double()
    want = sum(A.RS_W["lambda_" + k] * float(((a - b).abs() * m).sum() / m.sum()) for k, (a, b) in pairs.items() if A.RS_W.get("lambda_" + k, 0) > 0)
    assert abs(float(got) - want) <= 1e-5 * want
    logged = rs.get_and_weight_losses(rgb, nir, pred, mode="logging_dict", valid=valid)
    for k, (a, b) in pairs.items():
        want = float(((a - b).abs() * m).sum() / m.sum())
        assert abs(float(logged[f"indices_loss/{k}_error"]) - want) <= 1e-5 * want, k
    with pytest.raises(ValueError):
        HF.pix_loss(rgb, nir, pred, St.ALL_W, 0, valid[:, :, :-1])


def null_valid_or_count_is_refused(dev):
    shape = LOSS_SHAPES[0]
    be = L.backend()
    for field in ("valid", "count"):
        keep = []
        d, sums, grad, bufs = masked_desc(dev, shape, "all seven", 0, half_mask(shape), 3, keep)
        setattr(d, field, None)
        assert be.nirgan_pix_loss_masked(C.byref(d), stream(dev)) != 0 and b"valid or count" in be.nirgan_last_error()
        sync(dev)
        assert same_t(sums, St.SUMS0) and bool(torch.isnan(grad).all()) and loss_guards_intact(bufs), "the refused call launched something"
    for variant, change, msg in (("no rgb", {"w_ndvi": 0.5}, b"rgb"), ("all seven", {"criterion": 2}, b"criterion"),
                                 ("extra", {"extra_c": St.EXTRA[0]}, b"extra"), ("all seven", {"ws_elems": 100}, b"workspace")):
        keep = []
        d, sums, grad, bufs = masked_desc(dev, shape, variant, 0, half_mask(shape), 3, keep)
        for k, v in change.items():
            setattr(d, k, v)
        assert be.nirgan_pix_loss_masked(C.byref(d), stream(dev)) != 0 and msg in be.nirgan_last_error(), variant
        sync(dev)
        assert same_t(sums, St.SUMS0) and bool(torch.isnan(grad).all())


# ------------------------------------------------------------------------------------------------ the step
GOLDEN = "f1_g6_d.npz"                                                           # ngf = ndf = 8, 6 blocks, 2 x 3 x 32 x 32


def golden_model(dev, golden_dir, lambda_rs=1.0, lambda_ssim=0.0, micro_batches=1):
    from model.pix2pix import Px2Px_PL
    z = A.load(golden_dir, GOLDEN)
    m = Px2Px_PL(A.px_config(int(z["n_blocks"]), 8, 0, lambda_rs, lambda_ssim=lambda_ssim))
    A._load_golden_weights(m, z, False)
    m = m.to(dev).train()
    if micro_batches != 1:
        m.fused_trainer().micro_batches = micro_batches
    batch = {"rgb": torch.from_numpy(z["rgb"]).to(dev), "nir": torch.from_numpy(z["nir"]).to(dev)}
    return m, batch


def step_mask(batch, fractions=(0.5,), seed=17):
    """[B,1,H,W] float mask; sample b is valid with probability fractions[b * len(fractions) // B]"""
    B, _, H, W = batch["nir"].shape
    gen = torch.Generator().manual_seed(seed)
    p = torch.tensor([fractions[b * len(fractions) // B] for b in range(B)]).view(B, 1, 1, 1)
    return (torch.rand(B, 1, H, W, generator=gen) < p).float().to(batch["nir"].device)


def ones_step_equals_the_unmasked_step(dev, golden_dir):
    """two steps with valid = ones: LossView and every parameter bitwise those of two steps without valid"""
    runs = []
    for masked in (False, True):
        m, batch = golden_model(dev, golden_dir)
        if masked:
            batch["valid"] = torch.ones_like(batch["nir"])
        views = [m.train_batch(batch).as_dict() for _ in range(2)]
        sync(dev)
        runs.append((views, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}))
    (v0, p0), (v1, p1) = runs
    assert v0 == v1, (v0, v1)
    assert all(torch.equal(bits(p0[k]), bits(p1[k])) for k in p0)
    assert "loss_G_rs" in v0[0] and v0[0] != v0[1]


def half_mask_step_means(dev, golden_dir):
    """loss_G_l1 and loss_G_rs of a masked step: the float64 masked means of the step's own prediction; the divisor is the count"""
    m, batch = golden_model(dev, golden_dir)
    batch["valid"] = step_mask(batch) * 3.0                                      # any non-zero value keeps a pixel
    view = m.train_batch(batch)
    out = view.as_dict()
    tr = m.fused_trainer()
    keep = (batch["valid"] != 0).double().cpu()
    assert view.divisor() == int(keep.sum()) and 0 < view.divisor() < keep.numel()
    rgb, nir, pred = (t.detach().double().cpu() for t in (batch["rgb"], batch["nir"], tr.pred))
    l1 = float(((pred - nir).abs() * keep).sum() / keep.sum())
    pairs = O.rs_index_pairs(rgb, nir, pred, "loss")
    rs = sum(w * float(((pairs[k[7:]][0] - pairs[k[7:]][1]).abs() * keep).sum() / keep.sum()) for k, w in A.RS_W.items() if w > 0)
    print(f"masked step: l1 {out['loss_G_l1']:.9g} vs {l1:.9g}, rs {out['loss_G_rs']:.9g} vs {rs:.9g}")
    assert abs(out["loss_G_l1"] - l1) <= 1e-5 * l1
    assert abs(out["loss_G_rs"] - rs) <= 1e-5 * rs
    unmasked, b2 = golden_model(dev, golden_dir)
    assert unmasked.train_batch(b2).divisor() == keep.numel()


def lightning_and_train_batch_agree(dev, golden_dir, tol):
    """training_step with batch["valid"] (optimizer 0, then 1) and train_batch move G's parameters alike: the gradients within the
    bounds tests/api_cases.py holds each route to against the golden vectors, the parameters within its ``adam_close``"""
    fused, batch = golden_model(dev, golden_dir)
    batch["valid"] = step_mask(batch)
    fused.train_batch(batch)
    gG = {k: v.detach().cpu().clone() for k, v in fused.fused_trainer().flatG.grad_views().items()}
    m, _ = golden_model(dev, golden_dir)
    (opt_d, opt_g), _ = m.configure_optimizers()
    loss_d = m.training_step(batch, 0, 0)
    opt_d.zero_grad()
    loss_d.backward()
    opt_d.step()
    for q in m.netD.parameters():
        q.requires_grad_(False)
    loss_g = m.training_step(batch, 0, 1)
    opt_g.zero_grad()
    loss_g.backward()
    shadow = O.shadowed_bias_keys("G", 6)
    for k, q in m.netG.named_parameters():
        if k not in shadow:
            A.grad_close(q.grad, gG[k], tol, "gG " + k)
    opt_g.step()
    for (k, q), (_, r) in zip(m.netG.named_parameters(), fused.netG.named_parameters()):
        if k not in shadow:
            A.adam_close(q, r, gG[k], "G1 " + k)
    # the mask matters: the unmasked route gives another gradient
    plain, b2 = golden_model(dev, golden_dir)
    plain.train_batch(b2)
    g0 = plain.fused_trainer().flatG.grad.detach().cpu()
    g1 = fused.fused_trainer().flatG.grad.detach().cpu()
    assert (g0 - g1).norm() > 1e-2 * g0.norm()


def micro_batches_share_one_count(dev, golden_dir):
    """B = 4, the first half of the batch 90 % valid and the second 10 %: the gradient of G with two micro-batches is the one-part
    gradient to 1e-5 relative L2 -- a count per micro-batch would weigh the second half's pixels nine times as much"""
    grads = []
    for parts in (1, 2):
        m, batch = golden_model(dev, golden_dir, micro_batches=parts)
        batch = {k: torch.cat([v, v.flip(-1)], 0).contiguous() for k, v in batch.items()}
        batch["valid"] = step_mask(batch, (0.9, 0.1))
        view = m.train_batch(batch)
        assert m.fused_trainer()._state.n == parts and view.divisor() == int(batch["valid"].sum())
        grads.append(m.fused_trainer().flatG.grad.detach().double().cpu().clone())
    err = float((grads[1] - grads[0]).norm() / grads[0].norm())
    print(f"micro-batches 2 vs 1: rel L2 {err:.3e}")
    assert err <= 1e-5, err


def valid_with_ssim_raises(dev, golden_dir):
    m, batch = golden_model(dev, golden_dir, lambda_ssim=0.5)
    batch["valid"] = torch.ones_like(batch["nir"])
    with pytest.raises(NotImplementedError, match="straddle"):
        m.train_batch(batch)
    for q in m.netD.parameters():
        q.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="straddle"):
        m.training_step(batch, 0, 1)
    del batch["valid"]
    m.train_batch(batch)                                                         # without the mask the SSIM term runs as ever


def fit_scenes():
    """two 48 x 48 scenes of 4 bands whose 14 left columns are nodata: a 24 x 24 window holds up to 14 columns of it, and every
    window with more than half of its pixels clean is accepted at ``max_invalid = T*T//2`` -- all but those at x0 = 0 and 1"""
    rng = np.random.default_rng(23)
    out = []
    for _ in range(2):
        a = rng.integers(200, 6000, size=(4, 48, 48), dtype=np.uint16)
        a[:, :, :14] = 0
        out.append(a)
    return out


def fit_with_masks_resumes_bitwise(dev, tmp_path, tile=24):
    """a ``pool.loader(..., max_invalid=T*T//2, return_valid=True)`` feeds ``fit``: epochs of three steps, a checkpoint after the first
    (``fit`` writes checkpoints at epoch ends), a resume for the second: bitwise the uninterrupted two epochs.  The masks are mixed."""
    from model.pix2pix import Px2Px_PL
    from nirgan_hip.fit import fit
    cfg = A.px_config(6, 8, 0, 1.0)

    def fresh(seed):
        torch.manual_seed(seed)
        return Px2Px_PL(cfg).to(dev)
    pool = ScenePool(fit_scenes(), nodata=0, device=dev)

    def loader():
        return pool.loader(2, tile, 3, seed=5, max_invalid=tile * tile // 2, return_valid=True)
    fracs = [float(b["valid"].mean()) for b in loader()]
    assert 0.0 < min(fracs) < 1.0, fracs
    ck = tmp_path / "masked.ckpt"
    full = fresh(0)
    hist = fit(full, loader(), max_epochs=2, log_every=1, device=dev)
    assert len(hist["train"]) == 6
    part = fresh(0)
    fit(part, loader(), max_epochs=1, log_every=0, ckpt_path=str(ck), device=dev)
    resumed = fresh(99)
    fit(resumed, loader(), max_epochs=2, log_every=0, resume_from=str(ck), device=dev)
    moved = False
    for (k, a), (_, b), (_, c) in zip(full.named_parameters(), resumed.named_parameters(), part.named_parameters()):
        assert torch.equal(bits(a), bits(b)), "resumed " + k
        moved = moved or not torch.equal(bits(a), bits(c))
    assert moved, "the second epoch changed nothing"
    # the masks reach the step: the same run without them ends elsewhere
    plain = fresh(0)
    fit(plain, pool.loader(2, tile, 3, seed=5, max_invalid=tile * tile // 2), max_epochs=2, log_every=0, device=dev)
    assert any(not torch.equal(bits(a), bits(b)) for a, b in zip(full.parameters(), plain.parameters()))
