"""Case bodies of hold-out inside a scene pool (nirgan_scene_sample_origins, ``split`` / ``split_blocks`` of
nirgan_hip.data.ScenePool and the two halves of a ``PoolSplit``), shared by tests/test_scene_split_emulated.py (numpy emulator, CPU)
and tests/test_gpu_scene_split.py (MI355X).

Expected values: what ``nirgan_scene_sample_scaled`` / ``nirgan_scene_sample`` deliver for the same call (equivalence on whole-scene
rows), the restatement of tests/emu_scene_split.py (``draw_origins``, with ``cut_scaled`` / ``centre`` of the older restatements), a
brute-force mask for the sweep, and counts worked out by hand.  Everything is exact, so every comparison is BITWISE; there is no
tolerance anywhere in this file.

Guards and the exactly allocated pool: as in tests/scene_pool_cases.py, whose helpers are used.
"""
import ctypes as C
import math

import numpy as np
import torch

import emu_scene_grid as EG
import emu_scene_pool as E
import emu_scene_split as EP
import scene_grid_cases as Sg
import scene_pool_cases as Sc
import scene_scale_cases as Ss
from nirgan_hip import lib as L
from nirgan_hip.data import GridLoader, PoolSplit, ScenePool, SceneLoader, WindowList, block_key, origin_rectangles

BANDS, SEED, AUGMENTS = Sc.BANDS, Sc.SEED, Sc.AUGMENTS
KEYS4 = ("rgb", "nir", "coords", "window")

# the pool of the restatement cases: three scenes, three held-out rectangles (y, x, h, w) per scene
SHAPES = [(23, 31), (40, 17), (12, 12)]
HELD = {0: [(4, 6, 9, 11)], 1: [(0, 0, 13, 17), (30, 5, 10, 12)], 2: []}
VAL = [(s, *r) for s in sorted(HELD) for r in HELD[s]]
GEO = Ss.GEO4[:3]
T3, SCALES, WEIGHTS = 3, (1, 2, 3), (3, 2, 1)
# admissible windows per scene, worked out by hand: (guard, side) -> counts
COUNTS = {(0, 3): (466, 255, 100), (0, 6): (260, 144, 49), (0, 9): (124, 81, 16),
          (2, 3): (354, 177, 100), (2, 6): (183, 96, 49), (2, 9): (60, 45, 16)}


def scenes_of(shapes, kind, seed, bands=5, low=0):
    return Sg.make_scenes(shapes, kind, seed, bands=bands, low=low)


def pool_of(dev, scenes, kind, geo=None, **kw):
    bands = BANDS if scenes[0].shape[0] == 5 else (0, 1, 2, 3)
    return ScenePool(scenes, bands=bands, divisor=10000.0 if kind == "u16" else 1.0, geotransforms=geo, device=dev, **kw)


def tables_of(split, T, factors):
    """per scale the host rows of the origin table, as lists of Python ints"""
    return [split.train.origins(T, f).tolist() for f in factors]


def expected(scenes, pool, split, geo, T, B, views, seed, draw, scales, weights=None, sample0=0, prefixes=None, max_invalid=0):
    """the restatement's batch: (dict of numpy arrays rgb, nir, window and, with geo, coords; the row each sample was drawn from)"""
    factors = tuple(sorted(scales)) if scales is not None else (1,)
    win, which = EP.draw_origins(tables_of(split, T, factors), T, B, views, seed, draw, factors, Ss.weights_of(factors, weights), sample0,
                                 prefixes, max_invalid)
    out = Sg.expected_rows(scenes, pool, win.tolist(), T, geo)
    out["window"] = win.astype(np.uint32).view(np.int32).reshape(B, 4)
    return out, which


def check_batch(dev, pool, split, scenes, geo, T, B, augment, seed, draw, scales, weights=None, sample0=0, prefixes=None, max_invalid=0):
    bufs, views = Sc.guarded_outputs(dev, B, T, geo is not None)
    got = split.train.sample(B, T, seed=seed, draw=draw, sample0=sample0, augment=augment, max_invalid=max_invalid, return_windows=True,
                             out=views, scales=scales, scale_weights=weights)
    want, which = expected(scenes, pool, split, geo, T, B, AUGMENTS[augment], seed, draw, scales, weights, sample0, prefixes, max_invalid)
    assert set(got) == set(want)
    for k in want:
        assert Ss.same(got[k], want[k]), (k, T, B, augment, draw, scales)
    assert Sc.guards_intact(bufs, views), (T, B, augment, draw, scales)
    return got, want, which


# ------------------------------------------------------------------------------------------------ 1: equivalence on whole-scene rows
EQUIVALENCE = [(3, 1, "none", (1, 2, 3)), (4, 17, "d4", (1, 2, 3)), (3, 257, "flips", (1, 2, 3)), (4, 1, "d4", (2,)), (3, 17, "flips", (2,)),
               (4, 257, "none", (2,))]


def whole_scene_rows_are_the_scaled_sampler(dev, kind, T, B, augment, scales):
    """a split that holds nothing out: its origin table is one row per scene that holds a window (the 7 x 9 scene is left out at
    sides past 7), and rgb, nir, coords and window of 3 draws are bitwise what nirgan_scene_sample_scaled writes; half of every scene
    is nodata and max_invalid 2, so attempts past the first are compared as well"""
    bad = 0 if kind == "u16" else float("nan")
    scenes = Ss.scenes4(kind)
    for a in scenes:
        a[:, :, : a.shape[2] // 2] = bad
    pool = ScenePool(scenes, bands=BANDS, divisor=10000.0 if kind == "u16" else 1.0, geotransforms=Ss.GEO4, nodata=bad, device=dev)
    split = pool.split([])
    assert isinstance(split, PoolSplit) and split.rectangles == []
    for f in scales:
        side = f * T
        rows = split.train.origins(T, f)
        holding = [s for s, (h, w) in enumerate(Ss.SHAPES4) if h >= side and w >= side]
        assert rows[:, 0].tolist() == holding and not rows[:, 1:3].any()
        assert rows[:, 3:5].tolist() == [[Ss.SHAPES4[s][0] - side + 1, Ss.SHAPES4[s][1] - side + 1] for s in holding]
        assert split.train.windows(T, f) == pool.windows(T, f) == int(rows[-1, 5])
    attempts = set()
    for draw in range(3):
        kw = dict(seed=SEED, draw=draw, augment=augment, max_invalid=2, return_windows=True, scales=scales)
        a = pool.sample(B, T, **kw)
        bufs, views = Sc.guarded_outputs(dev, B, T, True)
        b = split.train.sample(B, T, out=views, **kw)
        assert sorted(a) == sorted(b) == sorted(KEYS4)
        for k in KEYS4:
            assert Sg.same_bits(a[k], b[k]), (k, draw)                            # bit patterns: an accepted window may hold NaNs
        assert Sc.guards_intact(bufs, views), draw
        attempts |= set(((a["window"][:, 3] >> 8) & 0xFF).tolist())
    assert B == 1 or len(attempts) > 1


def factor_one_is_scene_sample(dev, kind):
    """``scales=None`` and ``scales=(1,)`` on the train half of an empty split against ``pool.sample`` without scales"""
    bad = 0 if kind == "u16" else float("nan")
    for nodata in (None, bad):
        scenes = Ss.scenes4(kind)
        if nodata is not None:
            for a in scenes:
                a[:, :, : a.shape[2] // 2] = nodata
        pool = ScenePool(scenes, bands=BANDS, divisor=10000.0 if kind == "u16" else 1.0, geotransforms=Ss.GEO4, nodata=nodata, device=dev)
        split = pool.split([])
        for augment in ("none", "flips", "d4"):
            for draw in range(2):
                kw = dict(seed=SEED, draw=draw, augment=augment, max_invalid=2, return_windows=True)
                a = pool.sample(17, 4, **kw)
                for scales in (None, (1,)):
                    b = split.train.sample(17, 4, scales=scales, **kw)
                    assert all(Sg.same_bits(a[k], b[k]) for k in KEYS4), (augment, draw, scales)
        plain = split.train.sample(5, 4, seed=SEED, draw=0)
        assert sorted(plain) == ["coords", "nir", "rgb"]


def workload_tile(dev):
    """the workload's tile on one 600 x 700 scene, factors 1 and 2, B 2: whole-scene rows against the scaled sampler, then a 60 x 150
    rectangle held out against the restatement"""
    rng = np.random.default_rng(3)
    scenes = [rng.integers(0, 65536, size=(4, 600, 700), dtype=np.uint16)]
    pool = ScenePool(scenes, device=dev)
    whole, split = pool.split([]), pool.split([(0, 0, 0, 60, 150)], guard=3)
    factors = set()
    for draw in Ss.draws_with_both_routes((600, 700), 256, None, 2, scales=(1, 2)):
        kw = dict(seed=SEED, draw=draw, return_windows=True, scales=(1, 2))
        a, b = pool.sample(2, 256, **kw), whole.train.sample(2, 256, **kw)
        assert all(Sg.same_bits(a[k], b[k]) for k in ("rgb", "nir", "window")), draw
        factors |= set(ScenePool.window_factor(a["window"]).tolist())
        got, _, _ = check_batch(dev, pool, split, scenes, None, 256, 2, "d4", SEED, draw, (1, 2))
        assert not split.overlap(got["window"], 256, guard=3).any()
    assert factors == {1, 2}


# ------------------------------------------------------------------------------------------------ 2: the sweep
def sweep_is_the_brute_force_mask():
    """``origin_rectangles`` against a painted mask: the rectangles are disjoint, cover exactly the admissible origins, and their
    areas are the counts worked out by hand; then 60 random cases"""
    for (guard, side), counts in COUNTS.items():
        for s, shape in enumerate(SHAPES):
            rows = origin_rectangles(shape, side, HELD[s], guard)
            covered, disjoint = EP.mask_of_rows(shape, side, rows)
            assert disjoint and np.array_equal(covered, EP.admissible_mask(shape, side, HELD[s], guard)), (guard, side, s)
            assert sum(oh * ow for _, _, oh, ow in rows) == counts[s] == int(covered.sum()), (guard, side, s)
            assert rows == sorted(rows)
    assert sum(COUNTS[(0, 3)]) == 821 and sum((h - 2) * (w - 2) for h, w in SHAPES) == 1279
    assert origin_rectangles((5, 9), 6, [], 0) == [] and origin_rectangles((6, 9), 6, [], 0) == [(0, 0, 1, 4)]
    assert origin_rectangles((6, 9), 3, [(0, 0, 6, 9)], 0) == []                  # everything held out
    rng = np.random.default_rng(16)
    for case in range(60):
        H, W = (int(v) for v in rng.integers(6, 30, size=2))
        side, guard = int(rng.integers(1, 7)), int(rng.integers(0, 4))
        held = []
        for _ in range(int(rng.integers(0, 5))):                                   # overlapping rectangles are fine for the sweep itself
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            held.append((y, x, int(rng.integers(1, H - y + 1)), int(rng.integers(1, W - x + 1))))
        rows = origin_rectangles((H, W), side, held, guard)
        mask = EP.admissible_mask((H, W), side, held, guard)
        if mask is None:
            assert rows == []
            continue
        covered, disjoint = EP.mask_of_rows((H, W), side, rows)
        assert disjoint and np.array_equal(covered, mask), (case, H, W, side, guard, held)


def tables_and_counts(dev):
    """``windows`` / ``origins`` of the train half: the hand counts, cum restarting per table, the guard widening the rectangles"""
    pool = pool_of(dev, scenes_of(SHAPES, "u16", 1), "u16")
    for guard in (0, 2):
        split = pool.split(VAL, guard=guard)
        assert split.rectangles == VAL and split.guard == guard
        for f in SCALES:
            counts = COUNTS[(guard, f * T3)]
            rows = split.train.origins(T3, f)
            assert rows.dtype == np.int64 and rows.shape[1] == L.SCENE_ORIGIN_COLS
            assert split.train.windows(T3, f) == sum(counts) == int(rows[-1, 5])
            assert np.array_equal(np.cumsum(rows[:, 3] * rows[:, 4]), rows[:, 5])
            assert [int((rows[rows[:, 0] == s][:, 3] * rows[rows[:, 0] == s][:, 4]).sum()) for s in range(3)] == list(counts)
    assert pool.windows(T3) == 1279


# ------------------------------------------------------------------------------------------------ 3: the restatement
def nodata_scenes(kind):
    """values from 1 up, then nodata on every 11th pixel of every scene in one of the selected bands"""
    bad = 0 if kind == "u16" else np.nan
    scenes = scenes_of(SHAPES, kind, 41, low=1)
    for x in scenes:
        flat = x.reshape(5, -1)
        for n, p in enumerate(range(0, flat.shape[1], 11)):
            flat[BANDS[n % 4], p] = bad
    return scenes, bad


def restatement(dev, kind, with_nodata, guard):
    """T 3, scales (1, 2, 3) weighted (3, 2, 1), d4, B 257, four draws: every output against the restatement.  Among the samples are
    some drawn from the FIRST row of every scale -- for scales 1 and 2 that is where a cum that did not restart would show -- and
    from its last row; with nodata, attempts past the first and exhausted samples occur."""
    if with_nodata:
        scenes, bad = nodata_scenes(kind)
        pool = pool_of(dev, scenes, kind, geo=GEO, nodata=bad)
        prefixes = [E.prefix_table(E.invalid_mask(s[list(BANDS)], bad)) for s in scenes]
    else:
        scenes, prefixes = scenes_of(SHAPES, kind, 41), None
        pool = pool_of(dev, scenes, kind, geo=GEO)
    split = pool.split(VAL, guard=guard)
    last = [len(split.train.origins(T3, f)) - 1 for f in SCALES]
    seen, attempts, exhausted = set(), set(), 0
    for draw in range(4):
        got, want, which = check_batch(dev, pool, split, scenes, GEO, T3, 257, "d4", SEED, draw, SCALES, WEIGHTS, prefixes=prefixes, max_invalid=0)
        _, f, _, attempt, ex = Ss.words(want)
        seen |= {(SCALES.index(int(a)), i) for a, i in zip(f, which)}
        attempts |= set(attempt.tolist())
        exhausted += int(ex.sum())
        assert not split.overlap(got["window"], T3, guard=guard).any()
    for k in range(3):
        assert (k, 0) in seen and (k, last[k]) in seen, (k, sorted(seen))
    assert (len(attempts) > 2 and exhausted > 0) == with_nodata, (attempts, exhausted)


def a_table_of_hundreds_of_rows(dev):
    """200 x 300, ``split_blocks(block=8)``: more than 300 rows per scale, so the bisection runs nine levels deep; B 257 against the
    restatement, and rows from all over the table are hit"""
    scenes = scenes_of([(200, 300)], "u16", 9, bands=4)
    pool = pool_of(dev, scenes, "u16")
    split = pool.split_blocks(8, 0.3, seed=11)
    rows = [len(split.train.origins(4, f)) for f in (1, 2)]
    assert min(rows) >= 300, rows
    hit = set()
    for draw in range(2):
        got, _, which = check_batch(dev, pool, split, scenes, None, 4, 257, "d4", SEED, draw, (1, 2))
        hit |= set(which)
        assert not split.overlap(got["window"], 4).any()
    assert len(hit) > 150 and min(hit) < 20 and max(hit) > min(rows) - 20, (len(hit), min(hit), max(hit))


# ------------------------------------------------------------------------------------------------ 4: the guarantee
def painted(shapes, rows, T):
    masks = [np.zeros(s, dtype=bool) for s in shapes]
    for s, y0, x0, word in rows:
        side = EG.split_word(word)[1] * T
        masks[s][y0:y0 + side, x0:x0 + side] = True
    return masks


def guarantee(dev, guard):
    """Two scenes, the first mostly nodata, max_invalid 0: of 4096 samples some run out of attempts (bit 31) -- the case in which
    rejection alone would deliver any window -- and still no training row holds a held-out pixel, nor one of the rectangles widened
    by the guard; every validation row lies fully inside one rectangle; the pixels painted by the two halves are disjoint."""
    shapes = [(40, 50), (30, 30)]
    scenes = scenes_of(shapes, "u16", 23, bands=4, low=1)
    scenes[0][:, :, 6:] = 0
    scenes[0][:, 20:, :6] = 0
    val = [(0, 8, 0, 14, 20), (0, 30, 30, 10, 20), (1, 0, 12, 12, 12), (1, 20, 0, 10, 9)]
    pool = pool_of(dev, scenes, "u16", nodata=0)
    split = pool.split(val, guard=guard)
    got = split.train.sample(4096, 3, seed=SEED, draw=0, augment="d4", max_invalid=0, return_windows=True, scales=(1, 2))
    rows = got["window"].cpu().numpy()
    word = rows[:, 3].astype(np.int64) & 0xFFFFFFFF
    assert 0 < int((word >> 31).sum()) < 4096 and set(ScenePool.window_factor(rows).tolist()) == {1, 2}
    assert set(rows[word >> 31 == 1][:, 0].tolist()) == {0}                       # only the nodata scene exhausts
    assert not split.overlap(rows, 3).any()
    assert not split.overlap(got["window"], 3, guard=guard).any()
    assert not split.overlap(WindowList(rows, dev), 3, guard=split.guard).any()
    grid = split.val.grid(3, factors=(1, 2), max_invalid=9)
    side = 3 * ScenePool.window_factor(grid.host).astype(np.int64)
    assert np.array_equal(split.overlap(grid, 3), side * side)
    for s, y0, x0, w in grid.host.tolist():
        L_ = EG.split_word(w)[1] * 3
        assert any(r[0] == s and r[1] <= y0 and y0 + L_ <= r[1] + r[3] and r[2] <= x0 and x0 + L_ <= r[2] + r[4] for r in val), (s, y0, x0, w)
    train, held = painted(shapes, rows.tolist(), 3), painted(shapes, grid.host.tolist(), 3)
    for s, (a, b) in enumerate(zip(train, held)):
        assert a.any() and not (a & b).any(), s
        if guard:                                                                 # and the training pixels keep their distance
            wide = np.zeros_like(b)
            for r in (r for r in val if r[0] == s):
                wide[max(0, r[1] - guard):r[1] + r[3] + guard, max(0, r[2] - guard):r[2] + r[4] + guard] = True
            assert not (a & wide).any(), s
    # the pool's own sampler does cross the rectangles: the audit is not blind
    plain = pool.sample(4096, 3, seed=SEED, draw=0, max_invalid=0, return_windows=True, scales=(1, 2))
    assert split.overlap(plain["window"], 3).any()


def val_grid_is_the_double_loop(dev, kind):
    """``split.val.grid`` against the plain double loop per rectangle: order factor, rectangle as given, row, column; ``grid``'s start
    rule inside each rectangle; the nodata filter of the sampler"""
    scenes, bad = nodata_scenes(kind)
    pool = pool_of(dev, scenes, kind, nodata=bad)
    val = [VAL[2], VAL[0], VAL[1]]                                                # not in scene order: the given order is kept
    split = pool.split(val)
    P = [E.prefix_table(E.invalid_mask(s[list(BANDS)], bad)) for s in scenes]
    for kw in (dict(factors=(1,)), dict(factors=(2, 1), stride=2), dict(factors=(1, 2, 3), cover=False), dict(factors=(1, 2), stride=5, max_invalid=1),
               dict(factors=(1,), max_invalid=9)):
        want, rejected = [], 0
        for f in sorted(kw["factors"]):
            side = f * T3
            step = kw.get("stride") or side
            for s, ry, rx, rh, rw in val:
                if rh < side or rw < side:
                    continue
                for y0 in EG.starts(rh, side, step, kw.get("cover", True)):
                    for x0 in EG.starts(rw, side, step, kw.get("cover", True)):
                        y, x = ry + y0, rx + x0
                        n = int(P[s][y + side][x + side]) - int(P[s][y][x + side]) - int(P[s][y + side][x]) + int(P[s][y][x])
                        if n <= kw.get("max_invalid", 0) * f * f:
                            want.append((s, y, x, (f - 1) << 16))
                        else:
                            rejected += 1
        wl = split.val.grid(T3, **kw)
        assert isinstance(wl, WindowList) and np.array_equal(wl.host, np.asarray(want, dtype=np.int32)), kw
        assert np.array_equal(wl.device.cpu().numpy(), wl.host)
        assert (rejected > 0) == (kw.get("max_invalid", 0) < 9), (kw, rejected)


# ------------------------------------------------------------------------------------------------ 5: uniformity (restatement, CPU)
def uniformity_of_the_restatement():
    """200 000 draws over the 821 admissible windows of side 3 (guard 0): every window hit, and Pearson's chi-square against the
    uniform law below its 1 - 1e-9 quantile (820 degrees of freedom: 1086.7).  The device is bitwise the restatement, so this runs on
    the CPU; the table is ``origin_rectangles``'s, which ``sweep_is_the_brute_force_mask`` ties to the mask."""
    from scipy.stats import chi2
    n = 200000
    rows, cum = [], 0
    for s, shape in enumerate(SHAPES):
        for oy, ox, oh, ow in origin_rectangles(shape, 3, HELD[s], 0):
            cum += oh * ow
            rows.append((s, oy, ox, oh, ow, cum))
    assert cum == 821
    win, _ = EP.draw_origins([rows], 3, n, 8, 0x1234567890ABCDEF, 0, (1,), (1,))
    index, cells = [np.full((h - 2, w - 2), -1, dtype=np.int64) for h, w in SHAPES], 0
    for s, shape in enumerate(SHAPES):
        mask = EP.admissible_mask(shape, 3, HELD[s], 0)
        index[s][mask] = cells + np.arange(int(mask.sum()))
        cells += int(mask.sum())
    cell = np.array([index[s][y0, x0] for s, y0, x0, _ in win.tolist()])
    assert cells == 821 and cell.min() >= 0                                       # no draw outside the admissible windows
    counts = np.bincount(cell, minlength=821)
    stat = float(((counts - n / 821.0) ** 2 / (n / 821.0)).sum())
    bound = float(chi2.ppf(1.0 - 1e-9, 820))
    print(f"chi-square over 821 windows: {stat:.1f}, bound {bound:.1f}, least count {counts.min()}")
    assert counts.min() > 0 and stat < bound
    views = np.bincount(win[:, 3] & 7, minlength=8)
    assert float(((views - n / 8.0) ** 2 / (n / 8.0)).sum()) < float(chi2.ppf(1.0 - 1e-9, 7)), views


# ------------------------------------------------------------------------------------------------ 6: replay
def replay(dev, kind):
    """``pool.gather`` (and ``split.val.gather``) of a training batch's window rows gives the batch again, bitwise"""
    scenes, bad = nodata_scenes(kind)
    pool = pool_of(dev, scenes, kind, geo=GEO, nodata=bad)
    split = pool.split(VAL, guard=1)
    for draw in range(3):
        drawn = split.train.sample(17, T3, seed=SEED, draw=draw, max_invalid=0, return_windows=True, scales=SCALES)
        bufs, out, all_views = Sg.guarded(dev, 17, T3, True)
        got = pool.gather(drawn["window"], T3, out=out)
        assert all(Sg.same_bits(got[k], drawn[k]) for k in Sg.KEYS), draw
        assert Sc.guards_intact(bufs, all_views)
        again = split.val.gather(drawn["window"], T3)
        assert all(Sg.same_bits(again[k], drawn[k]) for k in Sg.KEYS), draw


# ------------------------------------------------------------------------------------------------ 7: loaders
def loader_epochs_and_ranks(dev):
    """``split.train.loader`` is a ``SceneLoader``: step i of epoch e is draw e * steps + i, rank r takes samples r * B ..; one set of
    buffers"""
    pool = pool_of(dev, scenes_of(SHAPES, "u16", 41), "u16", geo=GEO)
    split = pool.split(VAL)
    kw = dict(scales=(1, 2), scale_weights=(2, 1), augment="flips")
    ld = split.train.loader(3, T3, 2, seed=9, **kw)
    assert isinstance(ld, SceneLoader) and len(ld) == 2

    def epoch_of(loader):
        return [b["rgb"].clone() for b in loader]

    def direct(e):
        return [split.train.sample(3, T3, seed=9, draw=2 * e + i, **kw)["rgb"] for i in range(2)]
    first, second = epoch_of(ld), epoch_of(ld)
    assert all(torch.equal(a, b) for a, b in zip(first, direct(0))) and all(torch.equal(a, b) for a, b in zip(second, direct(1)))
    ld.set_epoch(5)
    assert all(torch.equal(a, b) for a, b in zip(epoch_of(ld), direct(5)))
    assert len({b["rgb"].data_ptr() for b in ld} | {b["rgb"].data_ptr() for b in ld}) == 1, "the loader allocates per step"
    assert sorted(next(iter(ld))) == ["coords", "nir", "rgb"]
    step, steps = 2, 3
    full = split.train.sample(8, T3, seed=SEED, draw=1 * steps + step, return_windows=True, **kw)
    for rank in (0, 1):
        part = split.train.loader(4, T3, steps, seed=SEED, rank=rank, world=2, **kw)
        part.set_epoch(1)
        batches = [{k: v.clone() for k, v in b.items()} for b in part]
        for k in ("rgb", "nir", "coords"):
            assert torch.equal(batches[step][k], full[k][4 * rank:4 * rank + 4]), (rank, k)
    assert not split.overlap(full["window"], T3).any()


def val_loader_is_fixed(dev):
    """two passes of ``split.val.grid_loader`` are bitwise equal and equal to the restatement of the grid's rows; rank sharding;
    ``by_factor``"""
    scenes = scenes_of(SHAPES, "u16", 41)
    pool = pool_of(dev, scenes, "u16", geo=GEO)
    split = pool.split(VAL)
    full = split.val.grid(T3, factors=(1, 2, 3))
    ld = split.val.grid_loader(4, T3, factors=(1, 2, 3))
    assert isinstance(ld, GridLoader) and np.array_equal(ld.windows.host, full.host) and len(ld) == math.ceil(len(full) / 4)
    first = [{k: v.clone() for k, v in b.items()} for b in ld]
    second = [{k: v.clone() for k, v in b.items()} for b in ld]
    want = Sg.expected_rows(scenes, pool, full.host.tolist(), T3, GEO)
    for i, (a, b) in enumerate(zip(first, second)):
        for k in Sg.KEYS:
            assert Sg.same_bits(a[k], b[k]) and Ss.same(a[k], want[k][4 * i:4 * i + 4]), (i, k)
    ranks = [split.val.grid_loader(4, T3, factors=(1, 2, 3), rank=r, world=3) for r in range(3)]
    for r, part in enumerate(ranks):
        assert np.array_equal(part.windows.host, full.host[r::3])
    parts = list(ld.by_factor())
    assert [f for f, _ in parts] == [1, 2, 3] and np.array_equal(np.concatenate([p.windows.host for _, p in parts]), full.host)
    side = ScenePool.window_factor(full.host).astype(np.int64) * T3
    assert np.array_equal(split.overlap(full, T3), side * side)


def fit_scenes():
    rng = np.random.default_rng(24)
    return [rng.integers(200, 6000, size=(4, 64, 72), dtype=np.uint16) for _ in range(2)]


def fit_resume_and_validate(fresh, dev, tmp_path, tile=16):
    """``fit`` on the train half with the val half's grid loader as ``val_loader``: two epochs + checkpoint + resume for a third ==
    three uninterrupted epochs, parameters bitwise, and a finite val/L1 per epoch"""
    from nirgan_hip.fit import fit
    pool = ScenePool(fit_scenes(), device=dev)
    split = pool.split([(0, 0, 0, 16, 72), (1, 32, 36, 32, 36)], guard=2)
    val = split.val.grid_loader(4, tile, factors=(1, 2))
    assert len(val.windows) == 5 + 2 * 3 + 2                                      # 16 x 72 at side 16: columns 0, 16, 32, 48 and 56; 32 x 36: 2 x 3, and 1 x 2 at side 32
    assert split.train.windows(tile, 2) == (64 - 18 - 31) * 41 + 33 * 3           # rows from 18 of scene 0; columns 0 .. 2 of scene 1
    ck = tmp_path / "split.ckpt"

    def loader():
        return split.train.loader(2, tile, 3, seed=5, scales=(1, 2))
    full = fresh(0)
    h3 = fit(full, loader(), val, max_epochs=3, log_every=1, device=dev)
    assert len(h3["train"]) == 9 and len(h3["val"]) == 3 and all(math.isfinite(v["val/L1"]) for v in h3["val"])
    part = fresh(0)
    fit(part, loader(), val, max_epochs=2, log_every=0, ckpt_path=str(ck), device=dev)
    resumed = fresh(99)
    fit(resumed, loader(), val, max_epochs=3, log_every=0, resume_from=str(ck), device=dev)
    moved = False
    for (k, a), (_, b), (_, c) in zip(full.named_parameters(), resumed.named_parameters(), part.named_parameters()):
        assert torch.equal(a.detach().cpu(), b.detach().cpu()), "resumed " + k
        moved = moved or not torch.equal(a.detach().cpu(), c.detach().cpu())
    assert moved, "the third epoch changed nothing"
    for draw in range(9):
        rows = split.train.sample(2, tile, seed=5, draw=draw, return_windows=True, scales=(1, 2))["window"]
        assert not split.overlap(rows, tile, guard=2).any()


# ------------------------------------------------------------------------------------------------ 8: split_blocks
def split_blocks_examples(dev):
    """the pinned key and the two pinned lattices; the rectangles are full cells, disjoint, and make up the asked share"""
    assert block_key(7, 0, 0, 0) == 0x9C01479161BC5D78
    assert block_key(7 + (1 << 64), 0, 0, 0) == block_key(7, 0, 0, 0) and block_key(-1, 0, 0, 0) == block_key((1 << 64) - 1, 0, 0, 0)
    shapes = [(50, 70), (33, 90)]
    pool = pool_of(dev, scenes_of(shapes, "u16", 2, bands=4), "u16")
    quarter = pool.split_blocks(16, 0.25, seed=7)
    assert quarter.rectangles == [(0, 0, 32, 16, 32), (0, 16, 32, 16, 16), (1, 16, 0, 16, 32), (1, 16, 48, 16, 16)]
    half = pool.split_blocks(16, 0.5, seed=7, guard=1)
    assert half.rectangles == [(0, 0, 32, 16, 32), (0, 16, 0, 16, 16), (0, 16, 32, 16, 16), (0, 32, 0, 16, 48), (1, 16, 0, 16, 32), (1, 16, 48, 16, 32)]
    assert half.guard == 1 and sum(r[3] * r[4] for r in quarter.rectangles) == 6 * 256 and sum(r[3] * r[4] for r in half.rectangles) == 11 * 256
    tiny = pool.split_blocks(16, 0.001, seed=7)                                   # at least one cell
    assert sum(r[3] * r[4] for r in tiny.rectangles) == 256
    stacked = pool_of(dev, scenes_of([(64, 48)], "u16", 2, bands=4), "u16").split_blocks(16, 0.99, seed=1)
    assert stacked.rectangles == [(0, 0, 0, 64, 48)]                              # all 12 cells: three-cell runs, stacked over four block rows
    other = pool.split_blocks(16, 0.25, seed=8)
    assert other.rectangles != quarter.rectangles


# ------------------------------------------------------------------------------------------------ 9: refusals
def _host_problem():
    """a valid descriptor on HOST buffers (nothing is launched by a refused call): two scenes of 4 bands, 6 x 7 and 8 x 8, tile 2,
    factors 1 and 3 (sides 2 and 6), B 2; scale 0 owns rows 0 .. 2, scale 1 rows 3 .. 4"""
    rows = [[0, 0, 0, 5, 6, 30], [1, 0, 0, 3, 7, 51], [1, 4, 2, 3, 5, 66], [0, 0, 0, 1, 2, 2], [1, 1, 0, 2, 3, 8]]
    keep = {"pool": torch.zeros(4 * 6 * 7 + 4 * 8 * 8, dtype=torch.int16), "table": torch.tensor([[0, 6, 7, 0, -1], [168, 8, 8, 0, -1]], dtype=torch.int64),
            "origins": torch.tensor(rows, dtype=torch.int64), "rgb": torch.zeros(2 * 3 * 4), "nir": torch.zeros(2 * 4),
            "window": torch.zeros(8, dtype=torch.int32), "prefix": torch.zeros(7 * 8, dtype=torch.int32)}
    d = L.SceneOriginsDesc()
    d.pool, d.pool_elems, d.dtype, d.S, d.C = keep["pool"].data_ptr(), 4 * 6 * 7 + 4 * 8 * 8, L.SCENE_U16, 2, 4
    d.table = d.table_host = keep["table"].data_ptr()
    d.origins = d.origins_host = keep["origins"].data_ptr()
    d.band = (C.c_int * 4)(0, 1, 2, 3)
    d.tile, d.B, d.views, d.divisor = 2, 2, 8, 10000.0
    d.rgb, d.nir, d.window = keep["rgb"].data_ptr(), keep["nir"].data_ptr(), keep["window"].data_ptr()
    d.K, d.R = 2, 5
    d.factor, d.weight = (C.c_int * 8)(1, 3), (C.c_uint32 * 8)(1, 1)
    d.first, d.count = (C.c_int * 8)(0, 3), (C.c_int * 8)(3, 2)
    return keep, d


def _table(d, keep, rows):
    keep["table"] = torch.tensor(rows, dtype=torch.int64)
    d.table = d.table_host = keep["table"].data_ptr()
    d.S = len(rows)


def _origin(d, keep, i, row):
    keep["origins"][i] = torch.tensor(row, dtype=torch.int64)


def _tiling(d, first, count, R=None, K=None):
    d.first, d.count = (C.c_int * 8)(*first), (C.c_int * 8)(*count)
    if R is not None:
        d.R = R
    if K is not None:
        d.K = K


def _scales(d, factors, weights):
    d.K = len(factors)
    d.factor, d.weight = (C.c_int * 8)(*factors), (C.c_uint32 * 8)(*weights)


def entry_refusals():
    """(what, mutate(d, keep), word of the message) -- each refusal the header lists for nirgan_scene_sample_origins"""
    def put(field, value):
        return lambda d, k: setattr(d, field, value)
    big = (1 << 31) - 1
    out = [(f"null {f}", put(f, None), b"null") for f in ("pool", "table", "table_host", "origins", "origins_host", "rgb", "nir", "window")]
    out += [("dtype", put("dtype", 2), b"dtype"), ("S 0", put("S", 0), b"bad pool"), ("C 3", put("C", 3), b"C must")]
    out += [(f"views {v}", put("views", v), b"views") for v in (0, 3, 16)]
    out += [(f"band {v}", put("band", (C.c_int * 4)(0, 1, v, 3)), b"band") for v in (4, -1)]
    out += [("B 0", put("B", 0), b"2^31"), ("tile 0", put("tile", 0), b"2^31"), ("tile 2^16", put("tile", 1 << 16), b"2^31"), ("B*T*T", put("B", 1 << 30), b"2^31")]
    out += [("divisor 0", put("divisor", 0.0), b"divisor"), ("divisor nan", put("divisor", float("nan")), b"divisor"), ("max_invalid", put("max_invalid", -1), b"max_invalid")]
    out += [("pool_elems -1", put("pool_elems", -1), b"negative pool_elems"), ("prefix_elems -1", put("prefix_elems", -1), b"negative pool_elems")]
    out += [("K 0", put("K", 0), b"K 0"), ("K 9", put("K", 9), b"K 9")]
    out += [("factor 9", lambda d, k: _scales(d, (1, 9), (1, 1)), b"factor 9"), ("factor 0", lambda d, k: _scales(d, (0, 3), (1, 1)), b"factor 0"),
            ("unsorted", lambda d, k: _scales(d, (3, 1), (1, 1)), b"increasing"), ("equal", lambda d, k: _scales(d, (3, 3), (1, 1)), b"increasing"),
            ("weight 0", lambda d, k: _scales(d, (1, 3), (1, 0)), b"weight of factor 3"),
            ("weights 2^32", lambda d, k: _scales(d, (1, 3), (1 << 31, 1 << 31)), b"2^32"),
            ("window 2^31", lambda d, k: (setattr(d, "tile", 1 << 14), setattr(d, "B", 1)), b"of factor 3")]
    out += [("extent 0", lambda d, k: _table(d, k, [[0, 0, 7, 0, -1], [168, 8, 8, 0, -1]]), b"extent"),
            ("extent 2^31", lambda d, k: _table(d, k, [[0, 6, 7, 0, -1], [168, 8, 1 << 31, 0, -1]]), b"extent"),
            ("outside", lambda d, k: _table(d, k, [[0, 6, 7, 0, -1], [169, 8, 8, 0, -1]]), b"scene 1 lies outside the pool"),
            ("offset", lambda d, k: _table(d, k, [[-1, 6, 7, 0, -1], [168, 8, 8, 0, -1]]), b"scene 0 lies outside the pool"),
            ("pool_elems", put("pool_elems", 4 * 6 * 7 + 4 * 8 * 8 - 1), b"outside the pool"),
            ("prefix null", lambda d, k: _table(d, k, [[0, 6, 7, 0, 0], [168, 8, 8, 0, -1]]), b"prefix is null"),
            ("prefix size", lambda d, k: (setattr(d, "prefix", k["prefix"].data_ptr()), setattr(d, "prefix_elems", 55), _table(d, k, [[0, 6, 7, 0, 0], [168, 8, 8, 0, -1]])),
             b"prefix_elems")]
    out += [("R 0", put("R", 0), b"R 0"), ("R -1", put("R", -1), b"R -1"),
            ("count 0", lambda d, k: _tiling(d, (0, 3), (3, 0), R=3), b"factor 3"), ("count -1", lambda d, k: _tiling(d, (0, 3), (-1, 2)), b"factor 1"),
            ("gap", lambda d, k: _tiling(d, (0, 4), (3, 1)), b"tile"), ("overlap", lambda d, k: _tiling(d, (0, 2), (3, 2)), b"tile"),
            ("first 1", lambda d, k: _tiling(d, (1, 3), (2, 2)), b"tile"), ("swapped", lambda d, k: _tiling(d, (2, 0), (3, 2)), b"tile"),
            ("short", lambda d, k: _tiling(d, (0, 3), (3, 1)), b"tile"), ("past R", lambda d, k: _tiling(d, (0, 3), (3, 3)), b"tile"),
            ("R too large", put("R", 6), b"tile"), ("huge count", lambda d, k: _tiling(d, (0, 3), (3, big)), b"tile")]
    out += [("scene 2", lambda d, k: _origin(d, k, 1, [2, 0, 0, 3, 7, 51]), b"row 1"), ("scene -1", lambda d, k: _origin(d, k, 3, [-1, 0, 0, 1, 2, 2]), b"row 3"),
            ("oh 0", lambda d, k: _origin(d, k, 2, [1, 4, 2, 0, 5, 51]), b"row 2"), ("ow 0", lambda d, k: _origin(d, k, 0, [0, 0, 0, 5, 0, 0]), b"row 0"),
            ("ow -1", lambda d, k: _origin(d, k, 4, [1, 1, 0, 2, -1, 0]), b"row 4"),
            ("oy -1", lambda d, k: _origin(d, k, 0, [0, -1, 0, 5, 6, 30]), b"row 0"), ("ox -1", lambda d, k: _origin(d, k, 4, [1, 1, -1, 2, 3, 8]), b"row 4"),
            ("oy + oh", lambda d, k: _origin(d, k, 2, [1, 5, 2, 3, 5, 66]), b"row 2"), ("ox + ow", lambda d, k: _origin(d, k, 2, [1, 4, 3, 3, 5, 66]), b"row 2"),
            ("oy + oh at side 6", lambda d, k: _origin(d, k, 3, [0, 0, 0, 2, 2, 4]), b"row 3"), ("ox + ow at side 6", lambda d, k: _origin(d, k, 4, [1, 1, 1, 2, 3, 8]), b"row 4"),
            ("oh 2^62", lambda d, k: _origin(d, k, 0, [0, 0, 0, 1 << 62, 6, 30]), b"row 0"), ("oy 2^63-1", lambda d, k: _origin(d, k, 0, [0, (1 << 63) - 1, 0, 5, 6, 30]), b"row 0"),
            ("cum", lambda d, k: _origin(d, k, 1, [1, 0, 0, 3, 7, 50]), b"row 1: cum"),
            ("cum does not restart", lambda d, k: (_origin(d, k, 3, [0, 0, 0, 1, 2, 68]), _origin(d, k, 4, [1, 1, 0, 2, 3, 74])), b"row 3: cum"),
            ("cum of the last row", lambda d, k: _origin(d, k, 4, [1, 1, 0, 2, 3, 9]), b"row 4: cum")]
    # a pool of 2^63 - 1 elements holds one 4-band scene of just under 2^61 pixels: only rectangles that overlap reach 2^62 origins
    wide = (1 << 30) - 1
    out += [("2^62 origins", lambda d, k: (setattr(d, "tile", 1), setattr(d, "pool_elems", (1 << 63) - 1), _scales(d, (1,), (1,)), _tiling(d, (0,), (3,), R=3),
                                         _table(d, k, [[0, big, wide, 0, -1]]), [_origin(d, k, i, [0, 0, 0, big, wide, (i + 1) * big * wide]) for i in range(3)]), b"2^62")]
    return out


def entry_rejects_bad_arguments(be):
    """through the raw entry of ``be`` (the emulator or the real library: a refused call launches nothing, so no GPU is needed)"""
    assert be.nirgan_scene_sample_origins(None, None) == -1 and b"scene_sample_origins" in be.nirgan_last_error()
    for what, mutate, word in entry_refusals():
        keep, d = _host_problem()
        mutate(d, keep)
        assert be.nirgan_scene_sample_origins(C.byref(d), None) == -1, what
        msg = be.nirgan_last_error()
        assert b"scene_sample_origins" in msg and word in msg, (what, msg)
        assert not keep["rgb"].any() and not keep["nir"].any() and not keep["window"].any(), what


def emulator_accepts_what_is_valid(be):
    """the host problem itself is valid (emulator only: the real library would launch), so each refusal above is its mutation's; a
    wrong column 3 of the scene table is not looked at, and overlapping rectangles are not refused"""
    keep, d = _host_problem()
    assert be.nirgan_scene_sample_origins(C.byref(d), None) == 0
    win = keep["window"].view(2, 4)
    assert bool((win[:, 0] >= 0).all()) and bool((win[:, 0] < 2).all())
    keep, d = _host_problem()
    _table(d, keep, [[0, 6, 7, 123456, -1], [168, 8, 8, -5, -1]])
    _origin(d, keep, 1, [0, 0, 0, 3, 6, 48])                                      # scene 0 again, under row 0
    _origin(d, keep, 2, [1, 4, 2, 3, 5, 63])
    assert be.nirgan_scene_sample_origins(C.byref(d), None) == 0


def python_refusals(dev):
    import pytest
    pool = pool_of(dev, scenes_of(SHAPES, "u16", 1), "u16")
    for val, word in (([(3, 0, 0, 2, 2)], "scene 3"), ([(-1, 0, 0, 2, 2)], "scene -1"), ([(0, 0, 0, 0, 2)], "empty or not inside"),
                      ([(0, -1, 0, 2, 2)], "not inside"), ([(0, 20, 0, 4, 2)], "not inside scene 0"), ([(0, 0, 30, 2, 2)], "not inside"),
                      ([(0, 0, 0, 2)], "integers"), ([(0, 0, 0, 2.5, 2)], "integers"), ([(0, 0, 0, 4, 4), (0, 3, 3, 4, 4)], "overlap"),
                      ([(1, 0, 0, 4, 4), (1, 0, 0, 4, 4)], "overlap")):
        with pytest.raises(ValueError, match=word):
            pool.split(val)
    assert len(pool.split([(0, 0, 0, 4, 4), (1, 0, 0, 4, 4), (0, 4, 0, 4, 4), (0, 0, 4, 4, 4)]).rectangles) == 4      # touching is not overlapping
    for guard in (-1, 1.5, True):
        with pytest.raises(ValueError, match="guard"):
            pool.split(VAL, guard=guard)
    for block in (0, -4, 2.5):
        with pytest.raises(ValueError, match="block"):
            pool.split_blocks(block, 0.2, seed=1)
    for fraction in (0, 1, -0.5, 1.5):
        with pytest.raises(ValueError, match="val_fraction"):
            pool.split_blocks(4, fraction, seed=1)
    with pytest.raises(ValueError, match="no scene holds a full 64 x 64 block"):
        pool.split_blocks(64, 0.2, seed=1)
    split = pool.split(VAL)
    with pytest.raises(ValueError, match="scale 6: no 18 x 18 window"):           # 23 x 31 minus its rectangle leaves none; the others are too small
        split.train.sample(2, T3, seed=1, draw=0, scales=(1, 6))
    with pytest.raises(ValueError, match="scale 6"):
        split.train.windows(T3, 6)
    with pytest.raises(ValueError, match="scale 8: the window"):
        split.train.sample(1, 1 << 13, seed=1, draw=0, scales=(8,))
    with pytest.raises(ValueError, match="scale 9"):
        split.train.sample(2, T3, seed=1, draw=0, scales=(9,))
    with pytest.raises(ValueError, match="scale_weights without scales"):
        split.train.sample(2, T3, seed=1, draw=0, scale_weights=(1,))
    with pytest.raises(ValueError, match="scale_weights without scales"):
        split.train.loader(2, T3, 3, seed=1, scale_weights=(1,))
    with pytest.raises(ValueError, match="augment"):
        split.train.sample(2, T3, seed=1, draw=0, augment="flip")
    with pytest.raises(ValueError, match="positive"):
        split.train.sample(0, T3, seed=1, draw=0)
    with pytest.raises(ValueError, match="rank"):
        split.train.loader(2, T3, 3, seed=1, rank=2, world=2)
    with pytest.raises(ValueError, match="rank"):
        split.val.grid_loader(2, T3, rank=3, world=3)
    with pytest.raises(ValueError, match="grid is empty.*held-out"):
        split.val.grid(5, factors=(3,))
    with pytest.raises(ValueError, match="grid is empty"):
        pool.split([]).val.grid(T3)
    with pytest.raises(ValueError, match="stride"):
        split.val.grid(T3, stride=0)
    with pytest.raises(ValueError, match="max_invalid"):
        split.val.grid(T3, max_invalid=-1)
    with pytest.raises(ValueError, match="named twice"):
        split.val.grid(T3, factors=(2, 2))
