"""Case bodies of the multi-scale sampler (nirgan_scene_sample_scaled, ``scales`` / ``scale_weights`` of nirgan_hip.data.ScenePool
and its loader), shared by tests/test_scene_scale_emulated.py (numpy emulator, CPU) and tests/test_gpu_scene_scale.py (MI355X).

Expected values: the restatement of tests/emu_scene_scale.py (``draw_scaled`` / ``cut_scaled``) and ``centre`` of
tests/emu_scene_pool.py applied to the same scenes.  Everything is exact, so every comparison is BITWISE; the one exception is the
payload of a NaN, which the header does not fix (a float pool's NaN "propagates"): where the restatement has a NaN the device must
have one, whatever its bits.  ``agrees_with_avg_pool`` alone has a tolerance, derived there.

Guards and the exactly allocated pool: as in tests/scene_pool_cases.py, whose helpers are used.
"""
import ctypes as C

import numpy as np
import torch

import emu_scene_pool as E
import emu_scene_scale as ES
import scene_pool_cases as Sc
from nirgan_hip import lib as L
from nirgan_hip.data import ScenePool

SHAPES4 = [(17, 19), (15, 15), (7, 9), (31, 26)]                                # 15 x 15: one window at side 15; 7 x 9: factor 1 only
BANDS = Sc.BANDS
GEO4 = Sc.GEO3 + [(2.3522, 1.0 / 4096, 48.8566, -1.0 / 4096)]
SEED = Sc.SEED
AUGMENTS = Sc.AUGMENTS


def scenes4(kind="u16", seed=11):
    rng = np.random.default_rng(seed)
    out = [rng.integers(0, 65536, size=(5, h, w), dtype=np.uint16) for h, w in SHAPES4]
    return out if kind == "u16" else [a.astype(np.float32) for a in out]


def pool4(dev, kind="u16", **kw):
    scenes = scenes4(kind)
    kw.setdefault("divisor", 10000.0 if kind == "u16" else 1.0)
    kw.setdefault("geotransforms", GEO4)
    return scenes, ScenePool(scenes, bands=BANDS, device=dev, **kw)


def weights_of(scales, weights):
    return tuple(weights) if weights is not None else (1,) * len(scales)


def expected(scenes, bands, divisor, geo, T, B, views, seed, draw, scales, weights=None, sample0=0, prefixes=None, max_invalid=0):
    """the restatement's batch: dict of numpy arrays rgb, nir, window (int32 bit patterns) and, with geo, coords"""
    win = ES.draw_scaled([s.shape[1:] for s in scenes], T, B, views, seed, draw, scales, weights_of(scales, weights), sample0, prefixes, max_invalid)
    out = {"rgb": np.empty((B, 3, T, T), np.float32), "nir": np.empty((B, 1, T, T), np.float32),
           "window": win.astype(np.uint32).view(np.int32).reshape(B, 4)}
    if geo is not None:
        out["coords"] = np.empty((B, 2), np.float32)
    for b, (s, y0, x0, word) in enumerate(win.tolist()):
        f = ((word >> 16) & 7) + 1
        v = ES.cut_scaled(scenes[s], bands, y0, x0, T, f, word & 7, divisor)
        out["rgb"][b], out["nir"][b, 0] = v[:3], v[3]
        if geo is not None:
            out["coords"][b] = E.centre(geo[s], y0, x0, f * T)
    return out


def same(got, want):
    """bitwise equality of a device tensor and a numpy array; a NaN of the restatement asks for a NaN, not for its payload"""
    g = got.detach().cpu().contiguous().numpy()
    if g.shape != want.shape:
        return False
    if g.dtype != np.float32:
        return np.array_equal(g, want)
    w = np.ascontiguousarray(want, dtype=np.float32)
    nan = np.isnan(w)
    return np.array_equal(np.isnan(g), nan) and np.array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan])


def check_batch(dev, pool, scenes, T, B, augment, seed, draw, scales, weights=None, sample0=0, prefixes=None, max_invalid=0, geo=GEO4):
    bufs, views = Sc.guarded_outputs(dev, B, T, geo is not None)
    got = pool.sample(B, T, seed=seed, draw=draw, sample0=sample0, augment=augment, max_invalid=max_invalid, return_windows=True, out=views,
                      scales=scales, scale_weights=weights)
    want = expected(scenes, pool.bands, pool.divisor, geo, T, B, AUGMENTS[augment], seed, draw, scales, weights, sample0, prefixes, max_invalid)
    assert set(got) == set(want)
    for k in want:
        assert same(got[k], want[k]), (k, T, B, augment, draw, scales)
    assert Sc.guards_intact(bufs, views), (T, B, augment, draw, scales)
    return got, want


def words(want):
    """(scene, factor, view, attempt, exhausted) columns of a restated batch"""
    w = want["window"][:, 3].astype(np.int64) & 0xFFFFFFFF
    return want["window"][:, 0], ((w >> 16) & 7) + 1, w & 7, (w >> 8) & 0xFF, w >> 31


# ------------------------------------------------------------------------------------------------ 1 and 11: sampling
def agrees_with_avg_pool(got, scenes, bands, divisor, T):
    """Independent of the restatement: every output against float64 ``avg_pool2d`` of the float64 source window named by the
    DEVICE's window words, turned with flip / transpose and divided in float64.  Bound 2^-22 relative: the two correctly rounded
    float32 operations (mean, division) err by at most 2^-24 each, about 2^-23 together, the float pool's float64 sum adds 2^-46;
    the factor two keeps this a check of the formula, the bitwise cases pin the bits."""
    win = got["window"].cpu().numpy()
    out = torch.cat([got["rgb"], got["nir"]], dim=1).cpu().double()
    for b, (s, y0, x0, word) in enumerate(win.tolist()):
        g, f = word & 7, ((word >> 16) & 7) + 1
        x = torch.from_numpy(scenes[s][list(bands), y0:y0 + f * T, x0:x0 + f * T].astype(np.float64))
        y = torch.nn.functional.avg_pool2d(x[None], f)[0]
        y = torch.flip(y, (-1,)) if g & 1 else y
        y = torch.flip(y, (-2,)) if g & 2 else y
        y = y.transpose(-1, -2) if g & 4 else y
        y = y / float(np.float32(divisor))
        err = (out[b] - y).abs()
        assert bool((err <= 2.0 ** -22 * y.abs()).all()), (b, g, f, float((err / y.abs().clamp_min(1e-300)).max()))


def sampling_is_bitwise(dev, kind, T, B, augment, scales):
    """rgb, nir, coords and window of 8 consecutive draws against the restatement, outputs guarded; the 7 x 9 scene never at f > 1;
    and every output against float64 avg_pool2d (case 11)"""
    scenes, pool = pool4(dev, kind)
    seen = set()
    for draw in range(40, 48):
        got, want = check_batch(dev, pool, scenes, T, B, augment, SEED, draw, scales)
        s, f, view, _, _ = words(want)
        assert set(f.tolist()) <= set(scales) and set(view.tolist()) <= set(range(AUGMENTS[augment]))
        assert not ((s == 2) & (f > 1)).any()
        seen |= set(f.tolist())
        agrees_with_avg_pool(got, scenes, pool.bands, pool.divisor, T)
    if B == 17:
        assert seen == set(scales)
    plain = pool.sample(B, T, seed=SEED, draw=40, augment=augment, scales=scales)
    assert sorted(plain) == ["coords", "nir", "rgb"] and plain["rgb"].shape == (B, 3, T, T) and plain["nir"].shape == (B, 1, T, T)


def small_scene_only_at_native_resolution(dev):
    """tile 5: the 15 x 15 scene holds exactly one window at factor 3; the 7 x 9 scene holds windows of factor 1 only: over 2 x 256
    samples it is never chosen at f > 1 and is chosen at f = 1"""
    scenes, pool = pool4(dev)
    assert pool.windows(5) == 13 * 15 + 11 * 11 + 3 * 5 + 27 * 22 and pool.windows(5, 1) == pool.windows(5)
    assert pool.windows(5, 2) == 8 * 10 + 6 * 6 + 22 * 17 and pool.windows(5, 3) == 3 * 5 + 1 + 17 * 12 and pool.windows(5, 7) == 0
    at = {1: set(), 2: set(), 3: set()}
    for draw in (0, 1):
        got, want = check_batch(dev, pool, scenes, 5, 256, "d4", SEED, draw, (1, 2, 3))
        s, f, _, _, _ = words(want)
        for k in at:
            at[k] |= set(s[f == k].tolist())
        assert torch.equal(ScenePool.window_factor(got["window"]).cpu(), torch.from_numpy(f).to(torch.int32))
    assert 2 in at[1] and 2 not in at[2] | at[3] and at[2] <= {0, 1, 3} and at[3] <= {0, 1, 3} and {0, 3} <= at[2] & at[3], at


# ------------------------------------------------------------------------------------------------ 2: factor 1 is the old entry
def factor_one_is_scene_sample(dev, kind, augment):
    """``scales=(1,)`` through the new entry against ``sample()`` without ``scales``: rgb, nir, coords and window words, with and
    without a prefix table (attempts past the first)"""
    for nodata in (None, 0 if kind == "u16" else float("nan")):
        scenes = scenes4(kind)
        if nodata is not None:
            for a in scenes:
                a[:, :, : a.shape[2] // 2] = nodata
        pool = ScenePool(scenes, bands=BANDS, divisor=10000.0 if kind == "u16" else 1.0, geotransforms=GEO4, nodata=nodata, device=dev)
        attempts = set()
        for draw in range(3):
            a = pool.sample(17, 4, seed=SEED, draw=draw, augment=augment, max_invalid=2, return_windows=True)
            b = pool.sample(17, 4, seed=SEED, draw=draw, augment=augment, max_invalid=2, return_windows=True, scales=(1,))
            assert sorted(a) == sorted(b) == ["coords", "nir", "rgb", "window"]
            for k in ("window", "coords"):
                assert torch.equal(a[k], b[k]), (k, draw)
            for k in ("rgb", "nir"):                                              # bit patterns: an accepted window may hold up to 2 NaNs
                assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (k, draw)
            attempts |= set(((a["window"][:, 3] >> 8) & 0xFF).tolist())
        assert (len(attempts) > 1) == (nodata is not None)


# ------------------------------------------------------------------------------------------------ 3, 4, 5: shapes
def draws_with_both_routes(shape, T, f, B, want_factors=None, scales=None, weights=None, limit=64):
    """the first draws whose restated windows show a view >= 4 and a view < 4 (and, if asked, every factor)"""
    picked, views, factors = [], set(), set()
    scales = scales or (f,)
    for draw in range(limit):
        win = ES.draw_scaled([shape], T, B, 8, SEED, draw, scales, weights_of(scales, weights))
        v, fs = set((win[:, 3] & 7).tolist()), set((((win[:, 3] >> 16) & 7) + 1).tolist())
        new_v = {x >= 4 for x in v} - {x >= 4 for x in views}
        if new_v or fs - factors:
            picked.append(draw)
            views |= v
            factors |= fs
        if {x >= 4 for x in views} == {True, False} and factors == set(scales):
            return picked
    raise AssertionError("no such draws")


def block_boundaries(dev, kind):
    """tiles that are no multiple of the 64-block, through both routes of the gather: 210 x 231 at T = 67, f = 3 (blocks of 64 and 3,
    source chunks of 192 and 9) and 150 x 141 at T = 70, f = 2"""
    for (H, W), T, f in (((210, 231), 67, 3), ((150, 141), 70, 2)):
        rng = np.random.default_rng(H)
        x = rng.integers(0, 65536, size=(4, H, W), dtype=np.uint16)
        scenes = [x if kind == "u16" else x.astype(np.float32)]
        pool = ScenePool(scenes, divisor=10000.0 if kind == "u16" else 1.0, device=dev)
        views = set()
        for draw in draws_with_both_routes((H, W), T, f, 2):
            _, want = check_batch(dev, pool, scenes, T, 2, "d4", SEED, draw, (f,), geo=None)
            views |= set(words(want)[2].tolist())
        assert any(v >= 4 for v in views) and any(v < 4 for v in views), views


def every_factor(dev, kind):
    """each factor is its own instance of the gather's block routine, and the kernel that holds them comes in two widths (factors to
    4, factors to 8): all eight at T = 8 on small scenes, and 4 .. 7 at T = 65 (a second block of one row and one column) on one
    470 x 460 scene, through both routes"""
    scenes, all8 = scenes4(kind), tuple(range(1, 9))
    scenes.append(np.random.default_rng(64).integers(0, 65536, size=(5, 70, 66)).astype(scenes[0].dtype))
    pool = ScenePool(scenes, bands=BANDS, divisor=10000.0 if kind == "u16" else 1.0, device=dev)
    seen = set()
    for draw in range(3):
        got, want = check_batch(dev, pool, scenes, 8, 17, "d4", SEED, draw, all8, geo=None)
        seen |= set(words(want)[1].tolist())
        agrees_with_avg_pool(got, scenes, pool.bands, pool.divisor, 8)
    assert seen == set(all8), seen
    x = np.random.default_rng(65).integers(0, 65536, size=(4, 470, 460), dtype=np.uint16)
    scenes = [x if kind == "u16" else x.astype(np.float32)]
    pool = ScenePool(scenes, divisor=10000.0 if kind == "u16" else 1.0, device=dev)
    for draw in draws_with_both_routes((470, 460), 65, None, 2, scales=(4, 5, 6, 7)):
        check_batch(dev, pool, scenes, 65, 2, "d4", SEED, draw, (4, 5, 6, 7), geo=None)
    for draw in draws_with_both_routes((470, 460), 65, 4, 2):                     # factor 4 again, in the instance that stops at 4
        check_batch(dev, pool, scenes, 65, 2, "d4", SEED, draw, (4,), geo=None)


def top_of_the_factor_range(dev):
    """T = 9, f = 8 on an 80 x 75 scene of 65535s: the block sum 64 * 65535 is the largest there is, and every output is
    fdiv_rn(65535, divisor)"""
    scenes = [np.full((4, 80, 75), 65535, dtype=np.uint16)]
    pool = ScenePool(scenes, device=dev)
    assert pool.windows(9, 8) == 9 * 4
    for draw in range(3):
        got, _ = check_batch(dev, pool, scenes, 9, 3, "d4", SEED, draw, (8,), geo=None)
        one = np.float32(65535.0) / np.float32(10000.0)
        assert bool((got["rgb"].cpu() == float(one)).all()) and bool((got["nir"].cpu() == float(one)).all())
    rng = np.random.default_rng(8)                                                # and ordinary values at the same shape
    scenes = [rng.integers(0, 65536, size=(4, 80, 75), dtype=np.uint16)]
    check_batch(dev, ScenePool(scenes, device=dev), scenes, 9, 3, "d4", SEED, 1, (8,), geo=None)


def workload_width_small(dev):
    """the workload's tile on one 520 x 600 scene, factors 1 and 2, B = 2: full 64-blocks, 16 of them per plane"""
    rng = np.random.default_rng(3)
    scenes = [rng.integers(0, 65536, size=(4, 520, 600), dtype=np.uint16)]
    pool = ScenePool(scenes, device=dev)
    factors, views = set(), set()
    for draw in draws_with_both_routes((520, 600), 256, None, 2, scales=(1, 2)):
        _, want = check_batch(dev, pool, scenes, 256, 2, "d4", SEED, draw, (1, 2), geo=None)
        factors |= set(words(want)[1].tolist())
        views |= set(words(want)[2].tolist())
    assert factors == {1, 2} and any(v >= 4 for v in views) and any(v < 4 for v in views)


# ------------------------------------------------------------------------------------------------ 6: rejection
def rejection_bound(dev, kind, f, max_invalid):
    """One scene of 4f rows and 4f + 1 columns, tile 4: two windows.  max_invalid * f * f invalid pixels lie in columns both windows
    hold, one more in the last column: the window at x0 = 0 holds exactly the bound and is accepted, the one at x0 = 1 holds one more
    and is rejected.  So every sample that is not flagged ends at x0 = 0, on a later attempt wherever an earlier one drew x0 = 1."""
    side = 4 * f
    bad = 0 if kind == "u16" else np.nan
    rng = np.random.default_rng(100 * f + max_invalid)
    x = rng.integers(1, 65536, size=(4, side, side + 1), dtype=np.uint16)
    x = x if kind == "u16" else x.astype(np.float32)
    n = max_invalid * f * f
    for i in range(n):                                                            # in columns 1 .. side - 1, each in another band
        x[i % 4, 1 + i // (side - 1), 1 + i % (side - 1)] = bad
    x[3, side - 1, side] = bad
    pool = ScenePool([x], nodata=bad, divisor=10000.0 if kind == "u16" else 1.0, device=dev)
    P = [E.prefix_table(E.invalid_mask(x, bad))]
    assert Sc.same(pool.invalid_prefix(0), P[0])
    assert int(P[0][side, side]) == n and int(P[0][side, side + 1] - P[0][side, 1]) == n + 1
    later = flagged = 0
    for draw in range(2):
        _, want = check_batch(dev, pool, [x], 4, 17, "d4", SEED, draw, (f,), prefixes=P, max_invalid=max_invalid, geo=None)
        _, fs, _, attempt, exhausted = words(want)
        assert (fs == f).all() and (want["window"][exhausted == 0, 2] == 0).all() and (attempt[exhausted == 1] == E.ATTEMPTS - 1).all()
        later, flagged = later + int(((attempt > 0) & (exhausted == 0)).sum()), flagged + int(exhausted.sum())
    assert later > 0 and flagged < 6                                             # (1/2)^8 per sample: 34 samples flag at most a few
    # one more allowed per block: every window passes at attempt 0
    _, want = check_batch(dev, pool, [x], 4, 17, "d4", SEED, 0, (f,), prefixes=P, max_invalid=max_invalid + 1, geo=None)
    assert (words(want)[3] == 0).all() and (words(want)[4] == 0).all()


def exhausted_keeps_the_scale(dev):
    """all nodata: every sample is flagged, holds attempt 7's window, and its word still names the factor that was drawn"""
    z = np.zeros((4, 12, 14), dtype=np.uint16)
    pool = ScenePool([z], nodata=0, device=dev)
    P = [E.prefix_table(E.invalid_mask(z, 0))]
    got, want = check_batch(dev, pool, [z], 4, 17, "d4", SEED, 9, (1, 2, 3), prefixes=P, max_invalid=0, geo=None)
    _, f, _, attempt, exhausted = words(want)
    assert (exhausted == 1).all() and (attempt == E.ATTEMPTS - 1).all()
    assert f.tolist() == ES.draw_factors(17, SEED, 9, (1, 2, 3), (1, 1, 1)) and set(f.tolist()) == {1, 2, 3}
    assert bool((got["rgb"] == 0).all())


# ------------------------------------------------------------------------------------------------ 7: the mix of scales
MIX_N, MIX_DRAW = 4096, 0


def scale_mix_of_the_restatement():
    """weights (3, 1): the share of factor 1 among 4096 samples within 0.75 +- 0.05 (binomial sigma 0.0068: 7 sigma)"""
    f = np.array(ES.draw_factors(MIX_N, SEED, MIX_DRAW, (1, 2), (3, 1)))
    share = float((f == 1).mean())
    print(f"share of factor 1: {share:.4f}")
    assert abs(share - 0.75) <= 0.05
    return f


def scale_mix(dev):
    f = scale_mix_of_the_restatement()
    scenes, pool = pool4(dev)
    got = pool.sample(MIX_N, 4, seed=SEED, draw=MIX_DRAW, return_windows=True, scales=(2, 1), scale_weights=(1, 3))   # sorted with their weights
    drawn = ScenePool.window_factor(got["window"]).cpu().numpy()
    assert np.array_equal(drawn, f)
    assert abs(float((drawn == 1).mean()) - 0.75) <= 0.05


def scale_does_not_depend_on_rejection(dev):
    """half of one scene nodata, max_invalid 0: the factors drawn are those of the same call with nothing rejected"""
    scenes = scenes4()
    for a in scenes:
        a[a == 0] = 1
    scenes[3][:, :, :13] = 0
    pool = ScenePool(scenes, bands=BANDS, nodata=0, geotransforms=GEO4, device=dev)
    P = [E.prefix_table(E.invalid_mask(s[list(BANDS)], 0)) for s in scenes]
    kw = dict(seed=SEED, draw=5, return_windows=True, scales=(1, 2, 3), scale_weights=(2, 1, 1))
    strict = pool.sample(256, 4, max_invalid=0, **kw)
    loose = pool.sample(256, 4, max_invalid=1 << 20, **kw)
    fa, fb = ScenePool.window_factor(strict["window"]).cpu().numpy(), ScenePool.window_factor(loose["window"]).cpu().numpy()
    assert np.array_equal(fa, fb)                                                 # sample by sample, so as multisets too
    assert sorted(fa.tolist()) == sorted(ES.draw_factors(256, SEED, 5, (1, 2, 3), (2, 1, 1)))
    assert not torch.equal(strict["window"], loose["window"]) and bool(((strict["window"][:, 3] >> 8) & 0xFF).any())
    assert not bool(((loose["window"][:, 3] >> 8) & 0xFF).any())
    check_batch(dev, pool, scenes, 4, 64, "d4", SEED, 5, (1, 2, 3), (2, 1, 1), prefixes=P, max_invalid=0)


# ------------------------------------------------------------------------------------------------ 8: determinism and sharding
SCALES, WEIGHTS = (1, 2, 3), (4, 2, 1)


def determinism_and_sharding(dev):
    scenes, pool = pool4(dev)
    kw = dict(seed=SEED, return_windows=True, scales=SCALES, scale_weights=WEIGHTS)
    a, b = pool.sample(8, 4, draw=11, **kw), pool.sample(8, 4, draw=11, **kw)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(pool.sample(8, 4, draw=12, **kw)["window"], a["window"])
    halves = [pool.sample(4, 4, draw=11, sample0=s0, **kw) for s0 in (0, 4)]
    for k in a:
        assert torch.equal(torch.cat([h[k] for h in halves]), a[k]), k
    # rank 1 of 2 at batch size 4 draws samples 4 .. 7 of the logical batch of 8
    step, steps = 2, 3
    full = pool.sample(8, 4, draw=1 * steps + step, **kw)
    ld = pool.loader(4, 4, steps, seed=SEED, rank=1, world=2, scales=SCALES, scale_weights=WEIGHTS)
    ld.set_epoch(1)
    batches = [{k: v.clone() for k, v in batch.items()} for batch in ld]
    assert len(batches) == len(ld) == steps and sorted(batches[0]) == ["coords", "nir", "rgb"]
    for k in ("rgb", "nir", "coords"):
        assert torch.equal(batches[step][k], full[k][4:]), k
    assert len(set(ScenePool.window_factor(full["window"]).tolist())) > 1


def loader_epochs_and_buffers(dev):
    scenes, pool = pool4(dev)
    ld = pool.loader(3, 4, 2, seed=9, augment="flips", scales=(3, 1), scale_weights=(1, 2))

    def epoch_of(loader):
        return [b["rgb"].clone() for b in loader]

    def direct(e):
        return [pool.sample(3, 4, seed=9, draw=2 * e + i, augment="flips", scales=(1, 3), scale_weights=(2, 1))["rgb"] for i in range(2)]
    first, second = epoch_of(ld), epoch_of(ld)                                    # without set_epoch: epochs 0, 1
    assert all(torch.equal(a, b) for a, b in zip(first, direct(0))) and all(torch.equal(a, b) for a, b in zip(second, direct(1)))
    ld.set_epoch(5)
    assert all(torch.equal(a, b) for a, b in zip(epoch_of(ld), direct(5)))
    assert all(torch.equal(a, b) for a, b in zip(epoch_of(ld), direct(6)))        # and on from there
    ptrs = {b["rgb"].data_ptr() for b in ld} | {b["rgb"].data_ptr() for b in ld}
    assert len(ptrs) == 1, "the loader allocates per step"
    native = [pool.sample(3, 4, seed=9, draw=i, augment="flips")["rgb"] for i in range(2)]
    assert not all(torch.equal(a, b) for a, b in zip(first, native))             # the scaled loader is not the native one


# ------------------------------------------------------------------------------------------------ 9: fit
def fit_resume_equals_uninterrupted(fresh, dev, tmp_path, tile=16):
    """two epochs + checkpoint + resume for a third == three uninterrupted epochs on a SCALED loader, parameters bitwise (the
    pattern of scene_pool_cases.fit_resume_equals_uninterrupted; 40 x 40 scenes hold windows of sides 16 and 32)"""
    from nirgan_hip.fit import fit
    pool = ScenePool(Sc.fit_scenes(), device=dev)

    def loader():
        return pool.loader(2, tile, 3, seed=5, scales=(1, 2), scale_weights=(1, 1))
    ck = tmp_path / "scaled.ckpt"
    full = fresh(0)
    h3 = fit(full, loader(), max_epochs=3, log_every=1, device=dev)
    assert len(h3["train"]) == 9
    part = fresh(0)
    fit(part, loader(), max_epochs=2, log_every=0, ckpt_path=str(ck), device=dev)
    resumed = fresh(99)
    fit(resumed, loader(), max_epochs=3, log_every=0, resume_from=str(ck), device=dev)
    moved = False
    for (k, a), (_, b), (_, c) in zip(full.named_parameters(), resumed.named_parameters(), part.named_parameters()):
        assert torch.equal(a.detach().cpu(), b.detach().cpu()), "resumed " + k
        moved = moved or not torch.equal(a.detach().cpu(), c.detach().cpu())
    assert moved, "the third epoch changed nothing"
    factors = set()
    for draw in range(9):
        factors |= set(ScenePool.window_factor(pool.sample(2, tile, seed=5, draw=draw, return_windows=True, scales=(1, 2))["window"]).tolist())
    assert factors == {1, 2}                                                      # the run did train on both resolutions
    native = fresh(0)
    fit(native, pool.loader(2, tile, 3, seed=5), max_epochs=3, log_every=0, device=dev)
    assert any(not torch.equal(a.detach().cpu(), b.detach().cpu()) for a, b in zip(full.parameters(), native.parameters()))


# ------------------------------------------------------------------------------------------------ 10: refusals
def _host_problem():
    """a valid descriptor on HOST buffers (nothing is launched by a refused call): one 6 x 7 scene of 4 bands, tile 2, factors
    1 and 3 (sides 2 and 6), B 2"""
    keep = {"pool": torch.zeros(4 * 6 * 7, dtype=torch.int16), "table": torch.tensor([[[0, 6, 7, 5 * 6, -1]], [[0, 6, 7, 1 * 2, -1]]], dtype=torch.int64),
            "rgb": torch.zeros(2 * 3 * 4), "nir": torch.zeros(2 * 4), "window": torch.zeros(8, dtype=torch.int32)}
    d = L.SceneScaledDesc()
    d.pool, d.pool_elems, d.dtype, d.S, d.C = keep["pool"].data_ptr(), 4 * 6 * 7, L.SCENE_U16, 1, 4
    d.table = d.table_host = keep["table"].data_ptr()
    d.band = (C.c_int * 4)(0, 1, 2, 3)
    d.tile, d.B, d.views, d.divisor = 2, 2, 8, 10000.0
    d.rgb, d.nir, d.window = keep["rgb"].data_ptr(), keep["nir"].data_ptr(), keep["window"].data_ptr()
    d.K = 2
    d.factor, d.weight = (C.c_int * 8)(1, 3), (C.c_uint32 * 8)(1, 1)
    return keep, d


def _scales(d, keep, factors, weights, cums):
    keep["table"] = torch.tensor([[[0, 6, 7, c, -1]] for c in cums], dtype=torch.int64)
    d.table = d.table_host = keep["table"].data_ptr()
    d.K = len(factors)
    d.factor, d.weight = (C.c_int * 8)(*factors), (C.c_uint32 * 8)(*weights)


def entry_refusals():
    """(what, mutate(d, keep), word of the message)"""
    out = [(f"null {f}", (lambda f: lambda d, k: setattr(d, f, None))(f), b"null") for f in ("pool", "table", "table_host", "rgb", "nir", "window")]
    out += [("views", lambda d, k: setattr(d, "views", 3), b"views"), ("band", lambda d, k: setattr(d, "band", (C.c_int * 4)(0, 1, 4, 3)), b"band"),
            ("B", lambda d, k: setattr(d, "B", 0), b"2^31"), ("tile", lambda d, k: setattr(d, "tile", 0), b"2^31"),
            ("divisor", lambda d, k: setattr(d, "divisor", 0.0), b"divisor"), ("max_invalid", lambda d, k: setattr(d, "max_invalid", -1), b"max_invalid"),
            ("dtype", lambda d, k: setattr(d, "dtype", 2), b"dtype"), ("C 3", lambda d, k: setattr(d, "C", 3), b"C must")]
    out += [("K 0", lambda d, k: setattr(d, "K", 0), b"K 0"), ("K 9", lambda d, k: setattr(d, "K", 9), b"K 9"), ("K -1", lambda d, k: setattr(d, "K", -1), b"K -1")]
    out += [("factor 9", lambda d, k: _scales(d, k, (1, 9), (1, 1), (30, 0)), b"factor 9"), ("factor 0", lambda d, k: _scales(d, k, (0, 1), (1, 1), (30, 30)), b"factor 0"),
            ("unsorted", lambda d, k: _scales(d, k, (3, 1), (1, 1), (2, 30)), b"increasing"), ("equal", lambda d, k: _scales(d, k, (1, 1), (1, 1), (30, 30)), b"increasing"),
            ("weight 0", lambda d, k: _scales(d, k, (1, 3), (1, 0), (30, 2)), b"weight of factor 3"),
            ("weights 2^32", lambda d, k: _scales(d, k, (1, 3), (1 << 31, 1 << 31), (30, 2)), b"2^32"),
            ("window 2^31", lambda d, k: (setattr(d, "tile", 1 << 14), setattr(d, "B", 1), _scales(d, k, (1, 3), (1, 1), (0, 0))), b"of factor 3"),
            ("no window", lambda d, k: _scales(d, k, (1, 3, 4), (1, 1, 1), (30, 2, 0)), b"window of factor 4"),
            ("wrong side", lambda d, k: _scales(d, k, (1, 3), (1, 1), (30, 30)), b"cum_windows"),
            ("wrong side, first", lambda d, k: _scales(d, k, (1, 3), (1, 1), (2, 2)), b"cum_windows"),
            ("outside", lambda d, k: setattr(d, "pool_elems", 4 * 6 * 7 - 1), b"outside the pool")]
    return out


def entry_rejects_bad_arguments(be):
    """through the raw entry of ``be`` (the emulator or the real library: a refused call launches nothing, so no GPU is needed)"""
    assert be.nirgan_scene_sample_scaled(None, None) == -1 and b"scene_sample_scaled" in be.nirgan_last_error()
    for what, mutate, word in entry_refusals():
        keep, d = _host_problem()
        mutate(d, keep)
        assert be.nirgan_scene_sample_scaled(C.byref(d), None) == -1, what
        msg = be.nirgan_last_error()
        assert b"scene_sample_scaled" in msg and word in msg, (what, msg)
        assert not keep["rgb"].any() and not keep["window"].any(), what


def python_refusals(dev):
    import pytest
    _, pool = pool4(dev)
    for bad, word in (((0, 1), "scale 0"), ((1, 9), "scale 9"), ((1, 2, 2), "scale 2 is named twice"), ((1.5,), "scale 1.5"), ((), "1 .. 8 factors"),
                      (tuple(range(1, 10)), "factors"), (3, "sequence")):
        with pytest.raises(ValueError, match=word):
            pool.sample(2, 4, seed=1, draw=0, scales=bad)
    for weights, word in (((1,), "as long as"), ((1, 0), "scale 2: the weight 0"), ((1, -3), "scale 2: the weight -3"), ((1, 0.5), "scale 2: the weight 0.5"),
                          ((1 << 31, 1 << 31), "2\\^32")):
        with pytest.raises(ValueError, match=word):
            pool.sample(2, 4, seed=1, draw=0, scales=(1, 2), scale_weights=weights)
    with pytest.raises(ValueError, match="scale_weights without scales"):
        pool.sample(2, 4, seed=1, draw=0, scale_weights=(1,))
    with pytest.raises(ValueError, match="scale 8: no scene of the pool holds a 32 x 32 window"):
        pool.sample(2, 4, seed=1, draw=0, scales=(1, 8))
    with pytest.raises(ValueError, match="scale 8: the window"):
        pool.sample(1, 1 << 13, seed=1, draw=0, scales=(8,))
    with pytest.raises(ValueError, match="scale 9"):
        pool.loader(2, 4, 3, seed=1, scales=(9,))
    with pytest.raises(ValueError, match="scale_weights without scales"):
        pool.loader(2, 4, 3, seed=1, scale_weights=(1,))
    with pytest.raises(ValueError, match="augment"):
        pool.sample(2, 4, seed=1, draw=0, augment="flip", scales=(1,))
    assert ScenePool.window_factor(np.array([[0, 0, 0, 5 << 16 | 7 << 8 | 3], [0, 0, 0, -1]])).tolist() == [6, 8]
