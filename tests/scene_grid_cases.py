"""Case bodies of the explicit window gather and the validation grid (nirgan_scene_gather, ``grid`` / ``gather`` / ``grid_loader`` of
nirgan_hip.data.ScenePool), shared by tests/test_scene_grid_emulated.py (numpy emulator, CPU) and tests/test_gpu_scene_grid.py
(MI355X).

Expected values: what a sampler delivered for the same window rows (replay), ``cut_scaled`` of tests/emu_scene_scale.py and
``centre`` of tests/emu_scene_pool.py on hand-made rows, and the plain double loop ``grid_rows`` of tests/emu_scene_grid.py over
``emu_scene_pool.prefix_table`` for the grid.  Everything is exact, so every comparison is BITWISE; there is no tolerance anywhere in
this file.

Guards and the exactly allocated pool: as in tests/scene_pool_cases.py, whose helpers are used.
"""
import ctypes as C
import math

import numpy as np
import torch

import emu_scene_grid as EG
import emu_scene_pool as E
import emu_scene_scale as ES
import scene_pool_cases as Sc
import scene_scale_cases as Ss
from nirgan_hip import lib as L
from nirgan_hip.data import GridLoader, ScenePool, WindowList

BANDS, SEED = Sc.BANDS, Sc.SEED
KEYS = ("rgb", "nir", "coords")


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    """two device tensors, float32 compared as bit patterns"""
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def make_scenes(shapes, kind, seed, bands=5, low=0):
    rng = np.random.default_rng(seed)
    out = [rng.integers(low, 65536, size=(bands, h, w), dtype=np.uint16) for h, w in shapes]
    return out if kind == "u16" else [a.astype(np.float32) for a in out]


def geo_of(n):
    return [Ss.GEO4[i % 4] for i in range(n)]


def make_pool(dev, scenes, kind, geo=True, **kw):
    bands = BANDS if scenes[0].shape[0] == 5 else (0, 1, 2, 3)
    return ScenePool(scenes, bands=bands, divisor=10000.0 if kind == "u16" else 1.0, geotransforms=geo_of(len(scenes)) if geo else None,
                     device=dev, **kw)


def guarded(dev, n, T, with_coords):
    bufs, views = Sc.guarded_outputs(dev, n, T, with_coords)
    return bufs, {k: v for k, v in views.items() if k != "window"}, views


def expected_rows(scenes, pool, rows, T, geo):
    """the restatement's tiles of explicit rows: dict of numpy arrays"""
    n = len(rows)
    out = {"rgb": np.empty((n, 3, T, T), np.float32), "nir": np.empty((n, 1, T, T), np.float32)}
    if geo is not None:
        out["coords"] = np.empty((n, 2), np.float32)
    for i, (s, y0, x0, word) in enumerate(rows):
        view, f = EG.split_word(word)
        v = ES.cut_scaled(scenes[s], pool.bands, y0, x0, T, f, view, pool.divisor)
        out["rgb"][i], out["nir"][i, 0] = v[:3], v[3]
        if geo is not None:
            out["coords"][i] = E.centre(geo[s], y0, x0, f * T)
    return out


def as_i32(rows):
    return (np.asarray(rows, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------ 1: replay
REPLAY = [("three scenes T2", Sc.SHAPES3, 2, (1, 2), 5), ("three scenes T3", Sc.SHAPES3, 3, (1, 2), 5),
          ("every instance", [(70, 131)], 8, (1, 3, 5, 8), 17), ("factor 7", [(70, 131)], 9, (7,), 2),
          ("second block", [(150, 150)], 70, (1, 2), 3)]


def replay(dev, kind, shapes, T, scales, B):
    """4 batches of a sampler, d4, with ``return_windows``; ``gather`` of their window rows gives rgb, nir and coords again, bitwise,
    into guarded outputs.  ``scales`` None: nirgan_scene_sample's rows; else nirgan_scene_sample_scaled's."""
    scenes = make_scenes(shapes, kind, 100 + T)
    pool = make_pool(dev, scenes, kind)
    factors, views = set(), set()
    for draw in range(4):
        drawn = pool.sample(B, T, seed=SEED, draw=draw, augment="d4", return_windows=True, scales=scales)
        bufs, out, all_views = guarded(dev, B, T, True)
        got = pool.gather(drawn["window"], T, out=out)
        assert sorted(got) == ["coords", "nir", "rgb"]
        for k in KEYS:
            assert got[k].data_ptr() == out[k].data_ptr() and same_bits(got[k], drawn[k]), (k, T, draw, scales)
        assert Sc.guards_intact(bufs, all_views), (T, draw, scales)
        fresh = pool.gather(WindowList(drawn["window"], dev), T)                 # new tensors, a list wrapped by the caller
        assert all(same_bits(fresh[k], drawn[k]) for k in KEYS)
        want = expected_rows(scenes, pool, drawn["window"].cpu().tolist(), T, geo_of(len(scenes)))
        assert all(Ss.same(got[k], want[k]) for k in KEYS), (T, draw, scales)     # and both are the restatement
        factors |= set(ScenePool.window_factor(drawn["window"]).tolist())
        views |= set((drawn["window"][:, 3] & 7).tolist())
    assert factors == set(scales or (1,)), factors
    assert any(v & 4 for v in views) and any(not v & 4 for v in views), views


def replay_exhausted(dev, kind):
    """a scene that is mostly nodata, max_invalid 0: some samples run out of attempts, so their words carry attempt 7 and bit 31,
    others carry a later attempt; the gather ignores both fields and still returns the sampler's tiles"""
    bad = 0 if kind == "u16" else np.nan
    x = make_scenes([(12, 14)], kind, 5, bands=4, low=1)[0]
    x[:, :, :10] = bad
    pool = ScenePool([x], nodata=bad, divisor=10000.0 if kind == "u16" else 1.0, geotransforms=geo_of(1), device=dev)
    exhausted = attempts = 0
    for scales in (None, (1, 2)):
        for draw in range(4):
            drawn = pool.sample(8, 2, seed=SEED, draw=draw, augment="d4", max_invalid=0, return_windows=True, scales=scales)
            bufs, out, all_views = guarded(dev, 8, 2, True)
            got = pool.gather(drawn["window"], 2, out=out)
            assert all(same_bits(got[k], drawn[k]) for k in KEYS), (draw, scales)
            assert Sc.guards_intact(bufs, all_views)
            word = drawn["window"][:, 3].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
            exhausted, attempts = exhausted + int((word >> 31).sum()), attempts + int((((word >> 8) & 0xFF) > 0).sum())
    assert exhausted > 0 and attempts > exhausted                                 # bits 8 .. 15 and 31 were set on some rows


# ------------------------------------------------------------------------------------------------ 2: explicit windows
EXPLICIT_SHAPES = [(24, 29), (31, 24), (26, 27)]
EXPLICIT_FACTORS = (1, 2, 3, 4, 5, 6, 7, 8)                                      # the issue's 1, 2, 3, 5, 8 and the three between
EXPLICIT_T = 3


def explicit_rows():
    """every view x factor x scene, at (0, 0) and at the far corner; every third row carries attempt and exhausted bits"""
    rows = []
    for f in EXPLICIT_FACTORS:
        side = f * EXPLICIT_T
        for view in range(8):
            for s, (H, W) in enumerate(EXPLICIT_SHAPES):
                for y0, x0 in ((0, 0), (H - side, W - side)):
                    word = view | (f - 1) << 16
                    if len(rows) % 3 == 1:
                        word |= (len(rows) % 8) << 8 | 1 << 31
                    rows.append((s, y0, x0, word))
    return rows


def raw_gather(pool, wl, T, first, n, out, coords=True, geo=True):
    """the entry called directly, so that ``coords`` and ``geo`` can be left out on their own"""
    d = L.SceneGatherDesc()
    table, table_host = pool._table(T)
    d.pool, d.pool_elems, d.dtype, d.S, d.C = pool.pool.data_ptr(), pool.pool_elems, pool.dtype, len(pool), pool.C
    d.table, d.table_host = table.data_ptr(), table_host.ctypes.data
    d.geo = pool.geo.data_ptr() if geo and pool.geo is not None else None
    d.band = (C.c_int * 4)(*pool.bands)
    d.tile, d.divisor = T, pool.divisor
    d.window, d.window_host, d.n_windows, d.first, d.n = wl.device.data_ptr(), wl.host.ctypes.data, len(wl), first, n
    d.rgb, d.nir = out["rgb"].data_ptr(), out["nir"].data_ptr()
    d.coords = out["coords"].data_ptr() if coords else None
    stream = torch.cuda.current_stream(pool.device).cuda_stream if pool.device.type == "cuda" else None
    L.call("nirgan_scene_gather", C.byref(d), stream)


def explicit_windows(dev, kind):
    """hand-made rows against ``cut_scaled`` / ``centre``; then the same list with coords = NULL and with geo = NULL: the pixels are
    the same and coords keeps its start value"""
    T, rows = EXPLICIT_T, explicit_rows()
    scenes = make_scenes(EXPLICIT_SHAPES, kind, 31)
    pool = make_pool(dev, scenes, kind)
    wl = WindowList(as_i32(rows), dev)
    assert len(wl) == len(rows) == 8 * 8 * 3 * 2 and wl.host.dtype == np.int32 and wl.device.dtype == torch.int32
    want = expected_rows(scenes, pool, rows, T, geo_of(3))
    bufs, out, all_views = guarded(dev, len(rows), T, True)
    got = pool.gather(wl, T, out=out)
    for k in KEYS:
        assert Ss.same(got[k], want[k]), k
    assert Sc.guards_intact(bufs, all_views)
    for coords, geo in ((False, True), (True, False)):
        bufs, out, all_views = guarded(dev, len(rows), T, True)
        raw_gather(pool, wl, T, 0, len(rows), out, coords=coords, geo=geo)
        assert Ss.same(out["rgb"], want["rgb"]) and Ss.same(out["nir"], want["nir"])
        assert bool(torch.isnan(out["coords"]).all()) and Sc.guards_intact(bufs, all_views)
    nogeo = make_pool(dev, scenes, kind, geo=False)                               # the Python route without geotransforms
    got = nogeo.gather(wl, T)
    assert sorted(got) == ["nir", "rgb"] and Ss.same(got["rgb"], want["rgb"]) and Ss.same(got["nir"], want["nir"])


def explicit_parts(dev, kind):
    """a 7-row list cut as (0, 7), as (0, 3) then (3, 4), and as (6, 1): the same rows bitwise, each into guarded outputs"""
    T = EXPLICIT_T
    rows = explicit_rows()[5::29][:7]
    assert len(rows) == 7 and len({EG.split_word(r[3]) for r in rows}) == 7
    scenes = make_scenes(EXPLICIT_SHAPES, kind, 31)
    pool = make_pool(dev, scenes, kind)
    wl = WindowList(as_i32(rows), dev)
    want = expected_rows(scenes, pool, rows, T, geo_of(3))
    for first, n in ((0, 7), (0, 3), (3, 4), (6, 1)):
        bufs, out, all_views = guarded(dev, n, T, True)
        got = pool.gather(wl, T, first=first, count=n, out=out)
        for k in KEYS:
            assert Ss.same(got[k], want[k][first:first + n]), (k, first, n)
        assert Sc.guards_intact(bufs, all_views), (first, n)
    tail = pool.gather(wl, T, first=3)                                            # count defaults to the rest
    assert Ss.same(tail["rgb"], want["rgb"][3:])


def workload_width(dev):
    """the workload's tile: 300 x 517 at f = 1 and 520 x 530 at f = 2, T = 256, all 8 views, windows at the far corner"""
    T = 256
    shapes = [(300, 517), (520, 530)]
    scenes = make_scenes(shapes, "u16", 3, bands=4)
    pool = make_pool(dev, scenes, "u16")
    rows = [(0, 300 - T, 517 - T, v) for v in range(8)] + [(1, 520 - 2 * T, 530 - 2 * T, v | 1 << 16) for v in range(8)]
    want = expected_rows(scenes, pool, rows, T, geo_of(2))
    bufs, out, all_views = guarded(dev, 16, T, True)
    got = pool.gather(as_i32(rows), T, out=out)
    for k in KEYS:
        assert Ss.same(got[k], want[k]), k
    assert Sc.guards_intact(bufs, all_views)


# ------------------------------------------------------------------------------------------------ 3: the grid
GRID_SHAPES = Ss.SHAPES4                                                          # (17, 19), (15, 15), (7, 9), (31, 26)
GRID_T = 5
GRID_CASES = [dict(factors=(f,), stride=stride, cover=cover) for f in (1, 2, 3) for stride in (None, f * GRID_T - 1, 1, 40) for cover in (True, False)]
GRID_CASES += [dict(factors=(1, 2, 3)), dict(factors=(3, 1, 2), stride=4, cover=False), dict(factors=(1, 2, 3), scenes=[2, 0]),
               dict(factors=(2,), scenes=[3], stride=7)]


def nodata_scenes(kind):
    """no nodata but where it is put: every 37th pixel of every scene in one of the selected bands, and a 4 x 4 patch at each
    scene's corner (16 invalid pixels: more than 3 per block at factors 1 and 2)"""
    bad = 0 if kind == "u16" else np.nan
    scenes = make_scenes(GRID_SHAPES, kind, 77, low=1)
    for x in scenes:
        flat = x.reshape(5, -1)
        for n, p in enumerate(range(0, flat.shape[1], 37)):
            flat[BANDS[n % 4], p] = bad
        x[BANDS[1], :4, :4] = bad
    return scenes, bad


def check_grid(pool, prefixes=None, **kw):
    tile = kw.pop("tile", GRID_T)
    wl = pool.grid(tile, **kw)
    kept, rejected = EG.grid_rows(GRID_SHAPES, tile, prefixes=prefixes, **kw)
    assert isinstance(wl, WindowList) and len(wl) == len(kept)
    assert wl.host.dtype == np.int32 and np.array_equal(wl.host, np.asarray(kept, dtype=np.int32)), kw
    assert wl.device.dtype == torch.int32 and np.array_equal(wl.device.cpu().numpy(), wl.host)
    return kept, rejected


def grid_is_the_double_loop(dev):
    """without nodata: strides L, L - 1, 1 and past every scene, cover on and off, three factors, a scene subset in its own order;
    the scenes smaller than L give nothing; with cover and stride <= L every scene that holds a window is covered completely"""
    pool = make_pool(dev, make_scenes(GRID_SHAPES, "u16", 77), "u16")
    assert pool.prefix is None
    for kw in GRID_CASES:
        kept, rejected = check_grid(pool, **dict(kw))
        assert kept and not rejected
        factors, stride, cover = kw["factors"], kw.get("stride"), kw.get("cover", True)
        for f in factors:
            side = f * GRID_T
            mine = [r for r in kept if EG.split_word(r[3])[1] == f]
            holding = {s for s in kw.get("scenes", range(4)) if min(GRID_SHAPES[s]) >= side}
            assert {r[0] for r in mine} == holding, (kw, f)
            if cover and (stride is None or stride <= side):
                for s in holding:
                    seen = np.zeros(GRID_SHAPES[s], dtype=bool)
                    for _, y0, x0, _ in (r for r in mine if r[0] == s):
                        seen[y0:y0 + side, x0:x0 + side] = True
                    assert seen.all(), (kw, f, s)
        if stride is None:                                                        # the default stride does not overlap but at the cover rows
            assert all(r[1] % (EG.split_word(r[3])[1] * GRID_T) == 0 or r[1] == GRID_SHAPES[r[0]][0] - EG.split_word(r[3])[1] * GRID_T for r in kept)
    order = [r[0] for r in EG.grid_rows(GRID_SHAPES, GRID_T, factors=(1,), scenes=[2, 0])[0]]
    assert order == sorted(order, reverse=True) and set(order) == {0, 2}          # scene 2 first, as named
    assert {EG.split_word(r[3])[1] for r in check_grid(pool, factors=(3, 1))[0] if r[0] == 2} == {1}      # 7 x 9: factor 1 only
    assert len([r for r in check_grid(pool, factors=(3,))[0] if r[0] == 1]) == 1  # 15 x 15: one window of side 15


def grid_rejects_like_the_sampler(dev, kind):
    """nodata, max_invalid 0 and 3 (per f x f block): the kept rows are those of the double loop over ``prefix_table``; every case
    keeps a window and rejects one"""
    scenes, bad = nodata_scenes(kind)
    pool = make_pool(dev, scenes, kind, nodata=bad)
    P = [E.prefix_table(E.invalid_mask(s[list(BANDS)], bad)) for s in scenes]
    for s in range(4):
        assert Sc.same(pool.invalid_prefix(s), P[s])
    for max_invalid in (0, 3):
        for kw in (dict(factors=(1,)), dict(factors=(2,), stride=3), dict(factors=(1, 2, 3), stride=5, cover=False), dict(factors=(1, 2), scenes=[2, 0])):
            kept, rejected = check_grid(pool, prefixes=P, max_invalid=max_invalid, **kw)
            assert len(kept) >= 1 and len(rejected) >= 1, (max_invalid, kw, len(kept), len(rejected))
    loose = check_grid(pool, prefixes=P, max_invalid=25, factors=(1, 2, 3))
    assert not loose[1]                                                           # a whole window's worth allowed: nothing is rejected


def grid_refusals(dev):
    import pytest
    pool = make_pool(dev, make_scenes(GRID_SHAPES, "u16", 77), "u16")
    with pytest.raises(ValueError, match="tile 40.*factors \\(1, 2\\)"):
        pool.grid(40, factors=(2, 1))
    with pytest.raises(ValueError, match="scale 9"):
        pool.grid(4, factors=(9,))
    with pytest.raises(ValueError, match="named twice"):
        pool.grid(4, factors=(2, 2))
    for stride in (0, -3, 1.5):
        with pytest.raises(ValueError, match="stride"):
            pool.grid(4, stride=stride)
    with pytest.raises(ValueError, match="max_invalid"):
        pool.grid(4, max_invalid=-1)
    with pytest.raises(ValueError, match="scenes"):
        pool.grid(4, scenes=[4])
    with pytest.raises(ValueError, match="rank"):
        pool.grid_loader(2, 4, rank=3, world=3)
    with pytest.raises(ValueError, match="int32"):
        pool.gather(np.zeros((2, 4), dtype=np.int64), 4)
    with pytest.raises(ValueError, match="int32"):
        pool.gather(torch.zeros((2, 3), dtype=torch.int32), 4)
    wl = pool.grid(4)
    for kw in (dict(first=-1), dict(first=len(wl)), dict(first=1, count=len(wl)), dict(count=0)):
        with pytest.raises(ValueError, match="windows"):
            pool.gather(wl, 4, **kw)
    good = {k: v for k, v in pool._outputs(2, 4).items() if k != "window"}
    for k, bad in (("rgb", torch.zeros((3, 3, 4, 4), device=dev)), ("nir", torch.zeros((2, 1, 4, 4), dtype=torch.float64, device=dev)),
                   ("coords", torch.zeros((2, 4), device=dev)[:, ::2])):
        with pytest.raises(ValueError, match=f"out\\['{k}'\\]"):               # an output of another size would be written past its end
            pool.gather(wl, 4, count=2, out={**good, k: bad})
    with pytest.raises(RuntimeError, match="scene_gather.*row 1"):               # the entry's own refusal reaches Python
        pool.gather(np.array([[0, 0, 0, 0], [0, 14, 0, 0]], dtype=np.int32), 4)


# ------------------------------------------------------------------------------------------------ 4: the loader
def loader_pool(dev):
    scenes = make_scenes(GRID_SHAPES, "u16", 77)
    return scenes, make_pool(dev, scenes, "u16")


def loader_is_fixed(dev):
    """two full iterations bitwise equal, batch by batch, and equal to the restatement of the grid's rows; len, the partial last
    batch, one set of buffers, no set_epoch, no __getitem__"""
    scenes, pool = loader_pool(dev)
    ld = pool.grid_loader(4, GRID_T, factors=(1, 2))
    rows = EG.grid_rows(GRID_SHAPES, GRID_T, factors=(1, 2))[0]
    assert isinstance(ld, GridLoader) and len(ld.windows) == len(rows) and len(rows) % 4 != 0
    assert len(ld) == math.ceil(len(rows) / 4) and not hasattr(ld, "set_epoch") and not hasattr(ld, "__getitem__")
    assert np.array_equal(ld.factor_of_row, [EG.split_word(r[3])[1] for r in rows])
    first = [{k: v.clone() for k, v in b.items()} for b in ld]
    second = [{k: v.clone() for k, v in b.items()} for b in ld]
    assert len(first) == len(second) == len(ld) and [b["rgb"].shape[0] for b in first] == [4] * (len(ld) - 1) + [len(rows) % 4]
    want = expected_rows(scenes, pool, rows, GRID_T, geo_of(4))
    for i, (a, b) in enumerate(zip(first, second)):
        assert sorted(a) == ["coords", "nir", "rgb"]
        for k in KEYS:
            assert same_bits(a[k], b[k]) and Ss.same(a[k], want[k][4 * i:4 * i + 4]), (i, k)
            assert a[k].shape[1:] == want[k].shape[1:]
    ptrs = {b["rgb"].data_ptr() for b in ld} | {b["rgb"].data_ptr() for b in ld}
    assert len(ptrs) == 1, "the loader allocates per step"


def loader_ranks_and_factors(dev):
    """world 3: the ranks' rows are disjoint, in order, and interleave to the grid; by_factor partitions the rows"""
    scenes, pool = loader_pool(dev)
    full = pool.grid(GRID_T, factors=(1, 2, 3)).host
    ranks = [pool.grid_loader(4, GRID_T, factors=(1, 2, 3), rank=r, world=3) for r in range(3)]
    for r, ld in enumerate(ranks):
        assert np.array_equal(ld.windows.host, full[r::3])
    assert sum(len(ld.windows) for ld in ranks) == len(full)
    merged = np.empty_like(full)
    for r, ld in enumerate(ranks):
        merged[r::3] = ld.windows.host
    assert np.array_equal(merged, full)
    whole = pool.gather(WindowList(full, dev), GRID_T)
    got = torch.cat([b["rgb"].clone() for b in ranks[1]])
    assert same_bits(got, whole["rgb"][1::3])
    ld = pool.grid_loader(4, GRID_T, factors=(1, 2, 3))
    parts = list(ld.by_factor())
    assert [f for f, _ in parts] == [1, 2, 3] and all(isinstance(p, GridLoader) for _, p in parts)
    assert np.array_equal(np.concatenate([p.windows.host for _, p in parts]), full)      # factor is the outer order of the grid
    for f, p in parts:
        assert set(p.factor_of_row.tolist()) == {f} and len(p) == math.ceil(len(p.windows) / 4)
        rows = torch.cat([b["nir"].clone() for b in p])
        assert same_bits(rows, whole["nir"][torch.from_numpy(ld.factor_of_row == f).to(rows.device)])


def fit_scenes():
    rng = np.random.default_rng(22)
    return [rng.integers(200, 6000, size=(4, 40, 50), dtype=np.uint16) for _ in range(2)]


def fit_and_evaluate(fresh, dev):
    """``fit`` walks a grid loader as its ``val_loader`` (two epochs: two finite val/L1), and ``evaluate_tiles`` returns one row per
    grid window with the gathered coords"""
    from nirgan_hip.fit import fit
    from validation_utils import evaluate_tiles
    pool = ScenePool(fit_scenes(), geotransforms=geo_of(2), device=dev)
    val = pool.grid_loader(16, 16)
    assert len(val.windows) == 2 * 3 * 4 and len(val) == 2                        # rows 0, 16, 24; columns 0, 16, 32, 34
    model = fresh(0)
    history = fit(model, pool.loader(2, 16, 3, seed=5), val, max_epochs=2, log_every=0, device=dev)
    assert len(history["val"]) == 2 and all(math.isfinite(v["val/L1"]) for v in history["val"])
    table = evaluate_tiles(model, val, crop=12)
    coords = pool.gather(val.windows, 16)["coords"].cpu()
    assert len(table["id"]) == len(val.windows)
    assert table["x"] == [float(v) for v in coords[:, 0]] and table["y"] == [float(v) for v in coords[:, 1]]
    again = evaluate_tiles(model, val, crop=12)                                   # a fixed set: the table of a second pass is the same
    assert again["l1"] == table["l1"] and again["x"] == table["x"]


# ------------------------------------------------------------------------------------------------ 5: argument errors
def _host_problem():
    """a valid descriptor on HOST buffers (nothing is launched by a refused call): two 6 x 7 scenes of 4 bands, tile 2, three rows"""
    keep = {"pool": torch.zeros(2 * 4 * 6 * 7, dtype=torch.int16), "table": torch.tensor([[0, 6, 7, 0, -1], [168, 6, 7, 0, 5]], dtype=torch.int64),
            "window": torch.from_numpy(as_i32([[0, 0, 0, 0], [1, 2, 3, 1 << 16 | 5], [1, 0, 1, 1 << 31 | 2 << 16 | 7 << 8 | 3]]).copy()),
            "rgb": torch.zeros(3 * 3 * 4), "nir": torch.zeros(3 * 4), "coords": torch.zeros(6)}
    d = L.SceneGatherDesc()
    d.pool, d.pool_elems, d.dtype, d.S, d.C = keep["pool"].data_ptr(), 2 * 4 * 6 * 7, L.SCENE_U16, 2, 4
    d.table = d.table_host = keep["table"].data_ptr()
    d.band = (C.c_int * 4)(0, 1, 2, 3)
    d.tile, d.divisor = 2, 10000.0
    d.window = d.window_host = keep["window"].data_ptr()
    d.n_windows, d.first, d.n = 3, 0, 3
    d.rgb, d.nir = keep["rgb"].data_ptr(), keep["nir"].data_ptr()
    return keep, d


def _table(d, keep, rows):
    keep["table"] = torch.tensor(rows, dtype=torch.int64)
    d.table = d.table_host = keep["table"].data_ptr()
    d.S = len(rows)


def _row(d, keep, i, row):
    keep["window"][i] = torch.from_numpy(as_i32([row])[0].copy())


def gather_refusals():
    """(what, mutate(d, keep), word of the message) -- each refusal the header lists for nirgan_scene_gather"""
    def put(field, value):
        return lambda d, k: setattr(d, field, value)
    out = [(f"null {f}", put(f, None), b"null") for f in ("pool", "table", "table_host", "window", "window_host", "rgb", "nir")]
    out += [("dtype", put("dtype", 2), b"dtype"), ("dtype -1", put("dtype", -1), b"dtype"), ("S 0", put("S", 0), b"bad pool"), ("C 3", put("C", 3), b"C must")]
    out += [(f"band {v}", put("band", (C.c_int * 4)(0, 1, v, 3)), b"band") for v in (4, -1)]
    out += [(f"tile {v}", put("tile", v), b"2^31") for v in (0, -3, 1 << 16)]
    out += [(f"n {v}", put("n", v), b"2^31") for v in (0, -1)]
    out += [("n*T*T", lambda d, k: (setattr(d, "n", 1 << 30), setattr(d, "n_windows", 1 << 30)), b"2^31")]
    out += [("first -1", put("first", -1), b"n_windows"), ("first + n", put("first", 1), b"n_windows"), ("n_windows", put("n_windows", 2), b"n_windows"),
            ("first huge", put("first", (1 << 63) - 1), b"n_windows")]
    out += [("divisor 0", put("divisor", 0.0), b"divisor"), ("divisor nan", put("divisor", float("nan")), b"divisor")]
    out += [("extent 0", lambda d, k: _table(d, k, [[0, 0, 7, 0, -1], [168, 6, 7, 0, -1]]), b"extent"),
            ("extent 2^31", lambda d, k: _table(d, k, [[0, 6, 1 << 31, 0, -1], [168, 6, 7, 0, -1]]), b"extent"),
            ("outside", lambda d, k: _table(d, k, [[0, 6, 7, 0, -1], [169, 6, 7, 0, -1]]), b"scene 1 lies outside the pool"),
            ("offset", lambda d, k: _table(d, k, [[-1, 6, 7, 0, -1], [168, 6, 7, 0, -1]]), b"scene 0 lies outside the pool"),
            ("pool_elems", put("pool_elems", 2 * 4 * 6 * 7 - 1), b"outside the pool")]
    out += [("s 2", lambda d, k: _row(d, k, 1, (2, 0, 0, 0)), b"row 1"), ("s -1", lambda d, k: _row(d, k, 0, (-1, 0, 0, 0)), b"row 0"),
            ("y0 -1", lambda d, k: _row(d, k, 2, (0, -1, 0, 0)), b"row 2"), ("x0 -1", lambda d, k: _row(d, k, 2, (0, 0, -1, 0)), b"row 2"),
            ("y0 + L", lambda d, k: _row(d, k, 1, (1, 3, 3, 1 << 16)), b"row 1"), ("x0 + L", lambda d, k: _row(d, k, 1, (1, 2, 4, 1 << 16)), b"row 1"),
            ("f 4", lambda d, k: _row(d, k, 0, (0, 0, 0, 3 << 16)), b"row 0"), ("bit 3", lambda d, k: _row(d, k, 2, (0, 0, 0, 8)), b"row 2"),
            ("bit 19", lambda d, k: _row(d, k, 1, (0, 0, 0, 1 << 19)), b"row 1"), ("bit 30", lambda d, k: _row(d, k, 0, (0, 0, 0, 1 << 30)), b"row 0"),
            ("window 2^31", lambda d, k: (setattr(d, "tile", 1 << 14), setattr(d, "n", 1), _row(d, k, 0, (0, 0, 0, 2 << 16))), b"row 0")]
    return out


def entry_rejects_bad_arguments(be):
    """through the raw entry of ``be`` (the emulator or the real library: a refused call launches nothing, so no GPU is needed); a
    bad row outside [first, first + n) is not this call's business"""
    assert be.nirgan_scene_gather(None, None) == -1 and b"scene_gather" in be.nirgan_last_error()
    for what, mutate, word in gather_refusals():
        for with_coords in (False, True):
            keep, d = _host_problem()
            if with_coords:
                d.coords = keep["coords"].data_ptr()
            mutate(d, keep)
            assert be.nirgan_scene_gather(C.byref(d), None) == -1, what
            msg = be.nirgan_last_error()
            assert b"scene_gather" in msg and word in msg, (what, msg)
            assert not keep["rgb"].any() and not keep["nir"].any() and not keep["coords"].any(), what


def emulator_accepts_what_is_valid(be):
    """the host problem itself is valid (emulator only: the real library would launch): so each refusal above is its mutation's;
    and a bad row outside the rows of the call is not looked at"""
    keep, d = _host_problem()
    assert be.nirgan_scene_gather(C.byref(d), None) == 0
    keep, d = _host_problem()
    _row(d, keep, 0, (5, -1, -1, 1 << 30))
    d.first, d.n = 1, 2
    assert be.nirgan_scene_gather(C.byref(d), None) == 0
