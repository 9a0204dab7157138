"""Case bodies of the device-resident scene pool (nirgan_scene_invalid_prefix / nirgan_scene_sample, nirgan_hip.data.ScenePool and
its loader, the ``set_epoch`` hook of ``fit``), shared by tests/test_scene_pool_emulated.py (numpy emulator, CPU) and
tests/test_gpu_scene_pool.py (MI355X).

Expected values: the restatement of tests/emu_scene_pool.py (``draw_windows`` / ``cut`` / ``centre`` / ``prefix_table``) applied to the
same scenes: Python-int index arithmetic, ``np.float32(v) / np.float32(divisor)``, float64 coords, ``np.cumsum``.  Everything is
exact, so every comparison is BITWISE (``torch.equal`` / ``np.array_equal``); there is no tolerance anywhere in this file.

Guards: every output of a raw sample sits between two bands of GUARD elements of a known value; the outputs themselves start as NaN
(-1 for the window words), so an element that was not written shows as a mismatch.  The pool is allocated exactly (ScenePool
concatenates the scenes without padding), so a read one row or one plane past a scene lands in the next scene and shows as a
mismatch as well.
"""
import ctypes as C

import numpy as np
import torch

import emu_scene_pool as E
from nirgan_hip import lib as L
from nirgan_hip.data import ScenePool

GUARD = 64
F_GUARD, I_GUARD = -12345.0, -77
SHAPES3 = [(7, 9), (5, 5), (13, 8)]                                             # odd widths, odd plane offsets, one scene of one 5 x 5 window
BANDS = (2, 1, 0, 4)
GEO3 = [(11.25, 1.0 / 8192, 48.5, -1.0 / 8192), (-70.123456789, 8.983152841195215e-05, -33.4, -8.983152841195215e-05),
        (151.2, 0.0001, -33.86, -0.00013)]
SEED = 0x5EEDC0DE12345678
AUGMENTS = {"none": 1, "flips": 4, "d4": 8}


def scenes3(kind="u16", seed=7):
    """three scenes [5][H][W]: uint16 over the whole range, or the same values as float32"""
    rng = np.random.default_rng(seed)
    out = [rng.integers(0, 65536, size=(5, h, w), dtype=np.uint16) for h, w in SHAPES3]
    return out if kind == "u16" else [a.astype(np.float32) for a in out]


def pool3(dev, kind="u16", **kw):
    scenes = scenes3(kind)
    kw.setdefault("divisor", 10000.0 if kind == "u16" else 1.0)
    kw.setdefault("geotransforms", GEO3)
    return scenes, ScenePool(scenes, bands=BANDS, device=dev, **kw)


def expected(scenes, bands, divisor, geo, T, B, views, seed, draw, sample0=0, prefixes=None, max_invalid=0):
    """the restatement's batch: dict of numpy arrays rgb, nir, window (int32 bit patterns) and, with geo, coords"""
    win = E.draw_windows([s.shape[1:] for s in scenes], T, B, views, seed, draw, sample0, prefixes, max_invalid)
    out = {"rgb": np.empty((B, 3, T, T), np.float32), "nir": np.empty((B, 1, T, T), np.float32),
           "window": win.astype(np.uint32).view(np.int32).reshape(B, 4)}
    if geo is not None:
        out["coords"] = np.empty((B, 2), np.float32)
    for b, (s, y0, x0, word) in enumerate(win.tolist()):
        v = E.cut(scenes[s], bands, y0, x0, T, word & 7, divisor)
        out["rgb"][b], out["nir"][b, 0] = v[:3], v[3]
        if geo is not None:
            out["coords"][b] = E.centre(geo[s], y0, x0, T)
    return out


def guarded_outputs(dev, B, T, with_coords):
    """the four outputs, each inside its own guarded buffer: (buffers, dict of views)"""
    bufs, views = {}, {}
    spec = {"rgb": ((B, 3, T, T), torch.float32), "nir": ((B, 1, T, T), torch.float32), "window": ((B, 4), torch.int32)}
    if with_coords:
        spec["coords"] = ((B, 2), torch.float32)
    for name, (shape, dt) in spec.items():
        n = int(np.prod(shape))
        guard, start = (F_GUARD, float("nan")) if dt == torch.float32 else (I_GUARD, -1)
        buf = torch.full((GUARD + n + GUARD,), guard, dtype=dt, device=dev)
        buf[GUARD:GUARD + n] = start
        bufs[name], views[name] = buf, buf[GUARD:GUARD + n].view(shape)
    return bufs, views


def guards_intact(bufs, views):
    for name, buf in bufs.items():
        n = views[name].numel()
        g = F_GUARD if buf.dtype == torch.float32 else I_GUARD
        if not (bool((buf[:GUARD] == g).all()) and bool((buf[GUARD + n:] == g).all()) and buf[GUARD + n:].numel() == GUARD):
            return False
    return True


def same(got, want):
    """bitwise equality of a device tensor and a numpy array (float32 compared as bit patterns)"""
    g = got.detach().cpu().contiguous().numpy()
    if g.dtype == np.float32:
        return g.shape == want.shape and np.array_equal(g.view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))
    return g.shape == want.shape and np.array_equal(g, want)


def check_batch(dev, pool, scenes, T, B, augment, seed, draw, sample0=0, prefixes=None, max_invalid=0, geo=GEO3):
    bufs, views = guarded_outputs(dev, B, T, geo is not None)
    got = pool.sample(B, T, seed=seed, draw=draw, sample0=sample0, augment=augment, max_invalid=max_invalid, return_windows=True, out=views)
    want = expected(scenes, pool.bands, pool.divisor, geo, T, B, AUGMENTS[augment], seed, draw, sample0, prefixes, max_invalid)
    assert set(got) == set(want)
    for k in want:
        assert same(got[k], want[k]), (k, T, B, augment, draw)
    assert guards_intact(bufs, views), (T, B, augment, draw)
    return want


# ------------------------------------------------------------------------------------------------ sampling
def sampling_is_bitwise(dev, kind, T, B, augment):
    """rgb, nir, coords and window of 8 consecutive draws against the restatement, outputs guarded"""
    scenes, pool = pool3(dev, kind)
    seen_views = set()
    for draw in range(40, 48):
        want = check_batch(dev, pool, scenes, T, B, augment, SEED, draw)
        seen_views |= set((want["window"][:, 3] & 7).tolist())
    assert seen_views <= set(range(AUGMENTS[augment]))
    plain = pool.sample(B, T, seed=SEED, draw=40, augment=augment)
    assert sorted(plain) == ["coords", "nir", "rgb"] and plain["rgb"].shape == (B, 3, T, T) and plain["nir"].shape == (B, 1, T, T)


def workload_width_small(dev):
    """the workload's tile on a single scene just larger than it: 300 x 517, tile 256, B = 2 (blocks of the gather past the first, the
    transposing views through LDS at full blocks)"""
    rng = np.random.default_rng(3)
    scenes = [rng.integers(0, 65536, size=(4, 300, 517), dtype=np.uint16)]
    pool = ScenePool(scenes, device=dev)
    views = set()
    for draw in range(4):
        want = check_batch(dev, pool, scenes, 256, 2, "d4", SEED, draw, geo=None)
        views |= set((want["window"][:, 3] & 7).tolist())
    assert any(v & 4 for v in views) and any(not v & 4 for v in views), views    # both paths of the gather ran


SEED_8_VIEWS = 0x5EEDC0DE12345693                                                # the 9 samples of draw 0 take all 8 views between them
PARTIAL_TILES = (65, 70)


def partial_second_block(dev, kind, T):
    """one 4 x 150 x 131 scene, tile 65 or 70, B = 9, d4: the second 64-block of the gather is partial along the rows AND along the
    columns (1 or 6 of 64), in the plain views and in the transposing ones -- all 8 occur in the one draw.  rgb, nir, coords and window
    bitwise against the restatement, outputs guarded; the float32 scene holds NaN, which passes through like any value."""
    rng = np.random.default_rng(65)
    scene = rng.integers(0, 65536, size=(4, 150, 131), dtype=np.uint16)
    if kind == "f32":
        scene = scene.astype(np.float32)
        scene[rng.random(scene.shape) < 0.01] = np.nan
    geo = [GEO3[1]]
    pool = ScenePool([scene], bands=(2, 1, 0, 3), divisor=10000.0 if kind == "u16" else 1.0, geotransforms=geo, device=dev)
    want = check_batch(dev, pool, [scene], T, 9, "d4", SEED_8_VIEWS, 0, geo=geo)
    assert set((want["window"][:, 3] & 7).tolist()) == set(range(8))
    assert kind == "u16" or np.isnan(want["rgb"]).any()


def small_scenes_are_never_chosen(dev):
    """tile 6: the 5 x 5 scene holds no window and is never drawn; tile 14: nothing holds one and the call raises"""
    import pytest
    scenes, pool = pool3(dev)
    assert pool.windows(6) == 2 * 4 + 8 * 3 and pool.windows(5) == 3 * 5 + 1 + 9 * 4 and pool.windows(14) == 0
    drawn = set()
    for draw in range(8):
        drawn |= set(check_batch(dev, pool, scenes, 6, 17, "flips", SEED, draw)["window"][:, 0].tolist())
    assert drawn == {0, 2}
    with pytest.raises(ValueError, match="window"):
        pool.sample(2, 14, seed=SEED, draw=0)


def views_follow_the_tile_views_rule(dev):
    """the gather's view g is view g of nirgan_tile_views_expand: restated here with np.flip / np.swapaxes, not with index arrays"""
    scenes, pool = pool3(dev)
    got = pool.sample(17, 5, seed=SEED, draw=3, augment="d4", return_windows=True)
    win = got["window"].cpu().numpy()
    rgb = got["rgb"].cpu().numpy()
    assert len(set((win[:, 3] & 7).tolist())) >= 4
    for b, (s, y0, x0, word) in enumerate(win.tolist()):
        x = scenes[s][list(BANDS[:3]), y0:y0 + 5, x0:x0 + 5]
        g = word & 7
        y = np.flip(x, -1) if g & 1 else x
        y = np.flip(y, -2) if g & 2 else y
        y = np.swapaxes(y, -1, -2) if g & 4 else y
        assert np.array_equal(rgb[b], y.astype(np.float32) / np.float32(10000.0)), (b, g)


# ------------------------------------------------------------------------------------------------ prefix table
PREFIX_SHAPES = [(1, 1), (2, 63), (3, 64), (65, 65), (5, 257)]


def prefix_scene(H, W, kind, nodata=0):
    """[5][H][W] without nodata, then every third pixel gets nodata (NaN) in a different one of the four selected bands"""
    rng = np.random.default_rng(H * 1000 + W)
    x = rng.integers(1, 65536, size=(5, H, W), dtype=np.uint16)
    x = x if kind == "u16" else x.astype(np.float32)
    flat = x.reshape(5, -1)
    for n, p in enumerate(range(0, H * W, 3)):
        flat[BANDS[n % 4], p] = nodata if kind == "u16" else np.nan
    return x


def prefix_is_cumsum(dev, H, W, kind):
    """the device's table against np.cumsum; a 5-element scene in front puts the scene at an odd offset, one behind it catches a
    read past the last plane"""
    front = np.full((5, 1, 1), 9, dtype=np.uint16 if kind == "u16" else np.float32)
    x = prefix_scene(H, W, kind)
    pool = ScenePool([front, x, front.copy()], bands=BANDS, nodata=0, device=dev)
    invalid = np.zeros(H * W, dtype=bool)
    invalid[::3] = True
    want = np.zeros((H + 1, W + 1), dtype=np.int64)
    want[1:, 1:] = np.cumsum(np.cumsum(invalid.reshape(H, W), axis=0), axis=1)
    got = pool.invalid_prefix(1).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want), (H, W, kind)
    assert np.array_equal(pool.invalid_prefix(0).cpu().numpy(), np.zeros((2, 2))) and np.array_equal(pool.invalid_prefix(2).cpu().numpy(), np.zeros((2, 2)))
    assert np.array_equal(got, E.prefix_table(E.invalid_mask(x[list(BANDS)], 0)))
    if kind == "u16":                                                             # an unselected band (3) holding nodata does not count
        y = x.copy()
        y[3] = 0
        assert np.array_equal(ScenePool([y], bands=BANDS, nodata=0, device=dev).invalid_prefix(0).cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ rejection
def rejection_cases(dev):
    """12 x 12, the left 7 columns nodata, tile 5, max_invalid 0: only x0 = 7 holds no invalid pixel.  An attempt succeeds with
    probability 1/8, so a sample runs out of its 8 attempts with probability (7/8)^8 = 0.34: every window that is NOT flagged as
    exhausted has x0 >= 7, the flagged ones are the restatement's, and the attempt numbers are the restatement's everywhere."""
    rng = np.random.default_rng(5)
    x = rng.integers(1, 65536, size=(4, 12, 12), dtype=np.uint16)
    x[:, :, :7] = 0
    pool = ScenePool([x], nodata=0, device=dev)
    P = [E.prefix_table(E.invalid_mask(x[[0, 1, 2, 3]], 0))]
    assert same(pool.invalid_prefix(0), P[0])
    taken = flagged = 0
    attempts = set()
    for draw in range(8):
        want = check_batch(dev, pool, [x], 5, 17, "d4", SEED, draw, prefixes=P, max_invalid=0, geo=None)
        word = want["window"][:, 3].astype(np.int64) & 0xFFFFFFFF
        done = (word >> 31) == 0
        assert (want["window"][done, 2] >= 7).all()
        assert (((word >> 8) & 0xFF)[~done] == E.ATTEMPTS - 1).all()
        taken, flagged = taken + int(done.sum()), flagged + int((~done).sum())
        attempts |= set(((word >> 8) & 0xFF)[done].tolist())
    assert taken > 0 and flagged > 0 and len(attempts) > 2                        # both ends of the rule were exercised
    # max_invalid = 25: every window passes at attempt 0
    for draw in range(4):
        want = check_batch(dev, pool, [x], 5, 17, "d4", SEED, draw, prefixes=P, max_invalid=25, geo=None)
        assert ((want["window"][:, 3].astype(np.int64) & 0xFFFFFF00) == 0).all()
    # all nodata: every sample is flagged and still holds the last attempt's window
    z = np.zeros((4, 12, 12), dtype=np.uint16)
    zpool = ScenePool([z], nodata=0, device=dev)
    Pz = [E.prefix_table(E.invalid_mask(z, 0))]
    want = check_batch(dev, zpool, [z], 5, 17, "d4", SEED, 9, prefixes=Pz, max_invalid=0, geo=None)
    assert ((want["window"][:, 3].astype(np.int64) & 0xFFFFFF00) == (1 << 31 | (E.ATTEMPTS - 1) << 8)).all()
    last = E.draw_windows([(12, 12)], 5, 17, 8, SEED, 9)                          # without a table attempt 0 is taken ...
    assert not np.array_equal(last[:, 1:3], want["window"][:, 1:3])               # ... and it is not the window of attempt 7
    # a float pool rejects on NaN
    f = x.astype(np.float32)
    f[:, :, :7] = np.nan
    fpool = ScenePool([f], nodata=float("nan"), divisor=1.0, device=dev)
    assert same(fpool.invalid_prefix(0), P[0])
    check_batch(dev, fpool, [f], 5, 17, "flips", SEED, 2, prefixes=P, max_invalid=0, geo=None)


# ------------------------------------------------------------------------------------------------ determinism and sharding
def determinism_and_sharding(dev):
    scenes, pool = pool3(dev)
    a = pool.sample(8, 4, seed=SEED, draw=11, return_windows=True)
    b = pool.sample(8, 4, seed=SEED, draw=11, return_windows=True)
    assert all(same(a[k], b[k].cpu().numpy()) for k in a)
    other = pool.sample(8, 4, seed=SEED, draw=12, return_windows=True)
    assert not torch.equal(other["window"], a["window"])
    reseeded = pool.sample(8, 4, seed=SEED + 1, draw=11, return_windows=True)
    assert not torch.equal(reseeded["window"], a["window"])
    # rank 1 of 2 at batch size 4 draws samples 4 .. 7 of the logical batch of 8
    step, steps = 2, 3
    full = pool.sample(8, 4, seed=SEED, draw=1 * steps + step, return_windows=True)
    ld = pool.loader(4, 4, steps, seed=SEED, rank=1, world=2)
    ld.set_epoch(1)
    batches = [{k: v.clone() for k, v in batch.items()} for batch in ld]
    assert len(batches) == len(ld) == steps and sorted(batches[0]) == ["coords", "nir", "rgb"]
    for k in ("rgb", "nir", "coords"):
        assert torch.equal(batches[step][k], full[k][4:]), k
    rank0 = pool.loader(4, 4, steps, seed=SEED, rank=0, world=2)
    rank0.set_epoch(1)
    assert torch.equal(list(rank0)[step]["rgb"], full["rgb"][:4])                  # the loader's tensors hold its last batch


def loader_epochs_and_buffers(dev):
    scenes, pool = pool3(dev)
    ld = pool.loader(3, 4, 2, seed=9, augment="flips")

    def epoch_of(loader):
        return [b["rgb"].clone() for b in loader]

    def direct(e):
        return [pool.sample(3, 4, seed=9, draw=2 * e + i, augment="flips")["rgb"] for i in range(2)]
    first, second = epoch_of(ld), epoch_of(ld)                                    # without set_epoch: epochs 0, 1
    assert all(torch.equal(a, b) for a, b in zip(first, direct(0))) and all(torch.equal(a, b) for a, b in zip(second, direct(1)))
    ld.set_epoch(5)
    assert all(torch.equal(a, b) for a, b in zip(epoch_of(ld), direct(5)))
    assert all(torch.equal(a, b) for a, b in zip(epoch_of(ld), direct(6)))        # and on from there
    ptrs = {b["rgb"].data_ptr() for b in ld} | {b["rgb"].data_ptr() for b in ld}
    assert len(ptrs) == 1, "the loader allocates per step"


def from_npz_round_trip(dev, tmp_path):
    scenes = scenes3()
    paths = []
    for i, (s, g) in enumerate(zip(scenes, GEO3)):
        paths.append(str(tmp_path / f"scene{i}.npz"))
        np.savez(paths[-1], data=s, geotransform=np.asarray(g))
    pool = ScenePool.from_npz(paths, bands=BANDS, device=dev)
    _, ref = pool3(dev)
    a, b = pool.sample(5, 4, seed=1, draw=2, return_windows=True), ref.sample(5, 4, seed=1, draw=2, return_windows=True)
    assert sorted(a) == ["coords", "nir", "rgb", "window"] and all(torch.equal(a[k], b[k]) for k in a)
    np.savez(paths[0], data=scenes[0])
    assert "coords" not in ScenePool.from_npz(paths[:1], bands=BANDS, device=dev).sample(1, 4, seed=1, draw=2)


# ------------------------------------------------------------------------------------------------ uniformity (restatement, CPU)
def uniformity_of_the_restatement():
    """20 000 draws over the windows of the 3-scene pool at tile 4 (24 + 4 + 50 = 78 windows): Pearson's chi-square against the
    uniform law below its 1 - 1e-9 quantile, and every window hit.  The device is bitwise the restatement, so this runs on the CPU."""
    from scipy.stats import chi2
    n = 20000
    win = E.draw_windows(SHAPES3, 4, n, 8, SEED, 0)
    cum = [0] + E.window_counts(SHAPES3, 4)
    cell = np.array([cum[s] + y0 * (SHAPES3[s][1] - 3) + x0 for s, y0, x0, _ in win.tolist()])
    counts = np.bincount(cell, minlength=cum[-1])
    assert cum[-1] == 78 and counts.shape == (78,) and counts.min() > 0
    stat = float(((counts - n / 78.0) ** 2 / (n / 78.0)).sum())
    bound = float(chi2.ppf(1.0 - 1e-9, 77))
    print(f"chi-square over 78 windows: {stat:.2f}, bound {bound:.2f}")
    assert stat < bound
    views = np.bincount(win[:, 3] & 7, minlength=8)
    vstat = float(((views - n / 8.0) ** 2 / (n / 8.0)).sum())
    assert vstat < float(chi2.ppf(1.0 - 1e-9, 7)), views


# ------------------------------------------------------------------------------------------------ fit
def fit_scenes():
    rng = np.random.default_rng(21)
    return [rng.integers(200, 6000, size=(4, 40, 40), dtype=np.uint16) for _ in range(2)]


def fit_resume_equals_uninterrupted(fresh, dev, tmp_path, tile=16):
    """two epochs + checkpoint + resume for a third == three uninterrupted epochs, parameters bitwise (``fit`` names the epoch to the
    loader; the resumed run's loader is a NEW one that has never seen epochs 0 and 1)"""
    from nirgan_hip.fit import fit
    pool = ScenePool(fit_scenes(), device=dev)
    ck = tmp_path / "pool.ckpt"
    full = fresh(0)
    h3 = fit(full, pool.loader(2, tile, 3, seed=5), max_epochs=3, log_every=1, device=dev)
    assert len(h3["train"]) == 9
    part = fresh(0)
    fit(part, pool.loader(2, tile, 3, seed=5), max_epochs=2, log_every=0, ckpt_path=str(ck), device=dev)
    resumed = fresh(99)
    fit(resumed, pool.loader(2, tile, 3, seed=5), max_epochs=3, log_every=0, resume_from=str(ck), device=dev)
    moved = False
    for (k, a), (_, b), (_, c) in zip(full.named_parameters(), resumed.named_parameters(), part.named_parameters()):
        assert torch.equal(a.detach().cpu(), b.detach().cpu()), "resumed " + k
        moved = moved or not torch.equal(a.detach().cpu(), c.detach().cpu())
    assert moved, "the third epoch changed nothing"
    # the epochs differ: a loader stuck at epoch 0 would not give the same run
    ld = pool.loader(2, tile, 3, seed=5)
    e0 = [b["rgb"].clone() for b in ld]
    e1 = [b["rgb"].clone() for b in ld]
    assert not any(torch.equal(a, b) for a, b in zip(e0, e1))


# ------------------------------------------------------------------------------------------------ argument errors
def _host_problem():
    """a valid descriptor on HOST buffers (nothing is launched by a refused call): one 6 x 7 scene of 4 bands, tile 3, B 2"""
    keep = {"pool": torch.zeros(4 * 6 * 7, dtype=torch.int16), "table": torch.tensor([[0, 6, 7, 4 * 5, -1]], dtype=torch.int64),
            "rgb": torch.zeros(2 * 3 * 9), "nir": torch.zeros(2 * 9), "window": torch.zeros(8, dtype=torch.int32),
            "prefix": torch.zeros(7 * 8, dtype=torch.int32)}
    d = L.SceneSampleDesc()
    d.pool, d.pool_elems, d.dtype, d.S, d.C = keep["pool"].data_ptr(), 4 * 6 * 7, L.SCENE_U16, 1, 4
    d.table = d.table_host = keep["table"].data_ptr()
    d.band = (C.c_int * 4)(0, 1, 2, 3)
    d.tile, d.B, d.views, d.divisor = 3, 2, 8, 10000.0
    d.rgb, d.nir, d.window = keep["rgb"].data_ptr(), keep["nir"].data_ptr(), keep["window"].data_ptr()
    return keep, d


def _table(d, keep, rows):
    keep["table"] = torch.tensor(rows, dtype=torch.int64)
    d.table = d.table_host = keep["table"].data_ptr()
    d.S = len(rows)


def sample_refusals():
    """(what, mutate(d, keep), word of the message) -- each refusal the header lists for nirgan_scene_sample"""
    big = (1 << 31) - 1
    out = [(f"null {f}", (lambda f: lambda d, k: setattr(d, f, None))(f), b"null") for f in ("pool", "table", "table_host", "rgb", "nir", "window")]
    out += [(f"views {v}", (lambda v: lambda d, k: setattr(d, "views", v))(v), b"views") for v in (0, 2, 3, 16, -4)]
    out += [(f"band {v}", (lambda v: lambda d, k: setattr(d, "band", (C.c_int * 4)(0, 1, v, 3)))(v), b"band") for v in (4, -1)]
    out += [(f"B {v}", (lambda v: lambda d, k: setattr(d, "B", v))(v), b"2^31") for v in (0, -1)]
    out += [(f"tile {v}", (lambda v: lambda d, k: setattr(d, "tile", v))(v), b"2^31") for v in (0, -3, 1 << 16)]
    out += [("B*T*T", lambda d, k: setattr(d, "B", 1 << 28), b"2^31")]
    out += [("divisor 0", lambda d, k: setattr(d, "divisor", 0.0), b"divisor"), ("divisor nan", lambda d, k: setattr(d, "divisor", float("nan")), b"divisor")]
    out += [("max_invalid", lambda d, k: setattr(d, "max_invalid", -1), b"max_invalid")]
    out += [("dtype", lambda d, k: setattr(d, "dtype", 2), b"dtype"), ("C 3", lambda d, k: setattr(d, "C", 3), b"C must"), ("S 0", lambda d, k: setattr(d, "S", 0), b"bad pool")]
    out += [("no window", lambda d, k: (setattr(d, "tile", 7), _table(d, k, [[0, 6, 7, 0, -1]])), b"no scene holds")]
    out += [("2^62 windows", lambda d, k: (setattr(d, "tile", 1), _table(d, k, [[0, big, big, big * big, -1], [0, big, big, 2 * big * big, -1]])), b"2^62")]
    out += [("cum", lambda d, k: _table(d, k, [[0, 6, 7, 19, -1]]), b"cum_windows"), ("extent", lambda d, k: _table(d, k, [[0, 0, 7, 0, -1]]), b"extent"),
            ("outside", lambda d, k: _table(d, k, [[1, 6, 7, 20, -1]]), b"outside the pool"), ("offset", lambda d, k: _table(d, k, [[-1, 6, 7, 20, -1]]), b"outside the pool"),
            ("prefix null", lambda d, k: _table(d, k, [[0, 6, 7, 20, 0]]), b"prefix is null"),
            ("prefix size", lambda d, k: (setattr(d, "prefix", k["prefix"].data_ptr()), setattr(d, "prefix_elems", 55), _table(d, k, [[0, 6, 7, 20, 0]])), b"prefix_elems")]
    return out


def prefix_refusals():
    return [("null pool", lambda d: setattr(d, "pool", None), b"null"), ("null prefix", lambda d: setattr(d, "prefix", None), b"null"),
            ("dtype", lambda d: setattr(d, "dtype", 5), b"dtype"), ("H 0", lambda d: setattr(d, "H", 0), b"shape"), ("W -1", lambda d: setattr(d, "W", -1), b"shape"),
            ("C 0", lambda d: setattr(d, "C", 0), b"shape"), ("table", lambda d: (setattr(d, "H", 1 << 16), setattr(d, "W", 1 << 15)), b"2^31"),
            ("band", lambda d: setattr(d, "band", (C.c_int * 4)(0, 1, 2, 4)), b"band"), ("offset", lambda d: setattr(d, "offset", 1), b"outside the pool"),
            ("negative offset", lambda d: setattr(d, "offset", -1), b"outside the pool"), ("nodata", lambda d: setattr(d, "nodata", 65536), b"nodata"),
            ("nodata -1", lambda d: setattr(d, "nodata", -1), b"nodata")]


def entries_reject_bad_arguments(be):
    """through the raw entries of ``be`` (the emulator or the real library: a refused call launches nothing, so no GPU is needed)"""
    assert be.nirgan_scene_sample(None, None) == -1 and b"scene_sample" in be.nirgan_last_error()
    assert be.nirgan_scene_invalid_prefix(None, None) == -1 and b"scene_invalid_prefix" in be.nirgan_last_error()
    for what, mutate, word in sample_refusals():
        keep, d = _host_problem()
        mutate(d, keep)
        assert be.nirgan_scene_sample(C.byref(d), None) == -1, what
        msg = be.nirgan_last_error()
        assert b"scene_sample" in msg and word in msg, (what, msg)
        assert not keep["rgb"].any() and not keep["window"].any(), what
    for what, mutate, word in prefix_refusals():
        keep, _ = _host_problem()
        p = L.ScenePrefixDesc()
        p.pool, p.pool_elems, p.dtype, p.offset, p.C, p.H, p.W = keep["pool"].data_ptr(), 4 * 6 * 7, L.SCENE_U16, 0, 4, 6, 7
        p.band = (C.c_int * 4)(0, 1, 2, 3)
        p.prefix = keep["prefix"].data_ptr()
        mutate(p)
        assert be.nirgan_scene_invalid_prefix(C.byref(p), None) == -1, what
        msg = be.nirgan_last_error()
        assert b"scene_invalid_prefix" in msg and word in msg, (what, msg)
        assert not keep["prefix"].any(), what


def python_refusals(dev):
    import pytest
    scenes = scenes3()
    with pytest.raises(ValueError, match="uint16 or all float32"):
        ScenePool([scenes[0], scenes[1].astype(np.float32)], device=dev)
    with pytest.raises(ValueError, match="uint16 or all float32"):
        ScenePool([scenes[0].astype(np.int32)], device=dev)
    with pytest.raises(ValueError, match="bands"):
        ScenePool(scenes, bands=(0, 1, 2, 5), device=dev)
    with pytest.raises(ValueError, match="bands"):
        ScenePool([s[:4] for s in scenes] + [scenes[0]], device=dev)
    with pytest.raises(ValueError, match="divisor"):
        ScenePool(scenes, divisor=0, device=dev)
    with pytest.raises(ValueError, match="geotransforms"):
        ScenePool(scenes, geotransforms=GEO3[:2], device=dev)
    _, pool = pool3(dev)
    with pytest.raises(ValueError, match="augment"):
        pool.sample(2, 4, seed=1, draw=0, augment="flip")
    with pytest.raises(ValueError, match="rank"):
        pool.loader(2, 4, 3, seed=1, rank=2, world=2)
    with pytest.raises(ValueError, match="positive"):
        pool.sample(0, 4, seed=1, draw=0)
    tensors = ScenePool([torch.from_numpy(s.astype(np.float32)) for s in scenes], bands=BANDS, divisor=1.0, device=dev)
    assert torch.equal(tensors.sample(3, 4, seed=2, draw=1)["rgb"], pool3(dev, "f32")[1].sample(3, 4, seed=2, draw=1)["rgb"])
