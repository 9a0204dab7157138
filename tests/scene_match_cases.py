"""Case bodies of the scene histogram matching (nirgan_hip.inference.scene_histogram / scene_match_lut / histogram_match_scene,
predict_scene(match=...), ScenePool.band_histogram; nirgan_scene_hist / nirgan_scene_match_lut / nirgan_scene_lut_apply), shared by
tests/test_scene_match_emulated.py (numpy emulator, CPU) and tests/test_gpu_scene_match.py (MI355X).

Every comparison is BITWISE and leaves no element out.  The references:
  the count    np.bincount;
  the table    tests/emu_scene_match.py (match_table: the header's operations written out in float64), which
               restatement_equals_the_oracle pins to oracle.match_histograms_plane on every input used here;
  the apply    numpy indexing.
"""
import ctypes as C

import numpy as np
import torch

from emu_scene_match import CODES, apply_table, histogram, interp_table, match_plane, match_table, move_off
from nirgan_hip import lib as L
from nirgan_hip.data import ScenePool
from nirgan_hip.inference import histogram_match, histogram_match_scene, predict_scene, scene_histogram, scene_match_lut
from scene_predict_cases import host, same_bits, upload
from tile_blend_cases import stream_of, tile_ramp

u16 = np.uint16
COUNT_SIZES = (1, 63, 64, 65, 4097, 61 * 83)
WRAP = (2100, 4100)                                                              # more vectors than one pass of either grid holds
GUARD = 64                                                                       # guard words / codes on each side of an output
NEW_ENTRIES = ("nirgan_scene_hist", "nirgan_scene_match_lut", "nirgan_scene_lut_apply")


# ------------------------------------------------------------------------------------------------ inputs
def main_input():
    """(source 61 x 83 with the triangle y/H + x/W < 0.5 at nodata 0, reference 23 x 31 with a 5 x 7 corner at 0), seed 7"""
    rng = np.random.default_rng(7)
    H, W = 61, 83
    src = np.clip(np.rint(rng.normal(3000.0, 800.0, size=(H, W))), 1, 65535).astype(u16)
    yy, xx = np.mgrid[0:H, 0:W]
    src[yy / H + xx / W < 0.5] = 0
    ref = np.clip(np.rint(rng.gamma(2.0, 1500.0, size=(23, 31))), 1, 65535).astype(u16)
    ref[:5, :7] = 0
    return src, ref


def from_counts(counts):
    return np.concatenate([np.full(n, v, dtype=u16) for v, n in counts.items()])


TIES = [({5: 2, 6: 4, 9: 1, 12: 1}, {10: 4, 11: 4}, {5: 10, 6: 10, 9: 11, 12: 11}),       # y = 10, 10.5, 10.75, 11
        ({5: 2, 6: 4, 9: 1, 12: 1}, {11: 4, 12: 4}, {5: 11, 6: 12, 9: 12, 12: 12})]       # y = 11, 11.5, 11.75, 12: ties go to even


def ramp_input():
    """(every code once as 256 x 256, 64 x 64 from normal(20000, 9000))"""
    rng = np.random.default_rng(8)
    return np.arange(CODES, dtype=u16).reshape(256, 256), np.clip(np.rint(rng.normal(20000.0, 9000.0, size=(64, 64))), 0, 65535).astype(u16)


def nodata_inputs():
    """[(source, reference, nodata, reference_nodata)]: codes 0, 7 and 65535, different on the two sides, with table values landing
    on the reserved code (the reference is dense around it)"""
    rng = np.random.default_rng(9)
    out = []
    for nd, rnd in ((0, 7), (7, 65535), (65535, 0)):
        centre = min(max(nd, 30), 65505)                                        # 0 .. 60 or 65475 .. 65535: the reserved code is a reference code
        src = rng.integers(1000, 1400, size=(37, 53)).astype(u16)
        src[rng.random(src.shape) < 0.2] = nd
        ref = np.clip(centre + rng.integers(-30, 31, size=(29, 41)), 0, 65535).astype(u16)
        ref[ref == rnd] = centre                                                 # the reference's own nodata only where it is planted
        ref[:3, :4] = rnd
        out.append((src, ref, nd, rnd))
    return out


def table_inputs():
    """[(src_hist, ref_hist, nodata)] of every input above"""
    src, ref = main_input()
    out = [(histogram(src, 0), histogram(ref, 0), 0)]
    out += [(histogram(from_counts(s)), histogram(from_counts(r)), None) for s, r, _ in TIES]
    a, b = ramp_input()
    out.append((histogram(a), histogram(b), None))
    out += [(histogram(s, nd), histogram(r, rnd), nd) for s, r, nd, rnd in nodata_inputs()]
    return out


# ------------------------------------------------------------------------------------------------ CPU: the restatement
def restatement_equals_the_oracle():
    """np.rint(oracle.match_histograms_plane(valid source codes, valid reference codes)) == table[valid source codes], up to the
    nodata move; and the unrounded values agree bitwise in float64"""
    import nirgan_oracle as O
    cases = [(*main_input(), 0, 0)] + [(from_counts(s), from_counts(r), None, None) for s, r, _ in TIES] + [(*ramp_input(), None, None)] + nodata_inputs()
    for src, ref, nd, rnd in cases:
        vs = src[src != nd].astype(np.float64) if nd is not None else src.reshape(-1).astype(np.float64)
        vr = ref[ref != rnd].astype(np.float64) if rnd is not None else ref.reshape(-1).astype(np.float64)
        want = O.match_histograms_plane(vs, vr)
        hs, hr = histogram(src, nd), histogram(ref, rnd)
        codes = vs.astype(np.int64)
        assert np.array_equal(interp_table(hs, hr)[codes].view(np.uint64), want.view(np.uint64))
        assert np.array_equal(move_off(np.rint(want).astype(np.int64), nd), match_table(hs, hr, nd)[codes].astype(np.int64))


def main_input_is_a_real_test():
    src, ref = main_input()
    valid = float((src != 0).mean())
    assert 0.10 <= valid <= 0.95
    lut = match_table(histogram(src, 0), histogram(ref, 0), 0)
    present = np.unique(src[src != 0]).astype(np.int64)
    assert (lut[present] != present).any()
    y = interp_table(histogram(src, 0), histogram(ref, 0))[present]
    assert (y != np.rint(y)).mean() > 0.5                                        # most values are fractional: the rounding is exercised


def ties_by_hand():
    for s, r, want in TIES:
        lut = match_table(histogram(from_counts(s)), histogram(from_counts(r)))
        assert {v: int(lut[v]) for v in s} == want


# ------------------------------------------------------------------------------------------------ helpers on the device
def offset_plane(a, dev, shift):
    """flat uint16 array -> an exactly allocated device tensor of len(a) + shift codes, and its view from element ``shift``"""
    buf = torch.empty(a.size + shift, dtype=torch.int16, device=dev)
    view = buf[shift:]
    view.copy_(torch.from_numpy(a.reshape(-1).view(np.int16)))
    return buf, view


def guarded_table(dev, fill):
    """int64 [GUARD + 65536 + GUARD], the table view"""
    buf = torch.full((GUARD + CODES + GUARD,), -77, dtype=torch.int64, device=dev)
    table = buf[GUARD:GUARD + CODES]
    table.copy_(torch.from_numpy(fill))
    return buf, table


def table_guards_intact(buf):
    return bool((buf[:GUARD] == -77).all()) and bool((buf[GUARD + CODES:] == -77).all())


def hist_desc(plane, hist, nodata=None):
    d = L.SceneMatchDesc()
    d.plane, d.n, d.hist = plane.data_ptr(), plane.numel(), hist.data_ptr()
    d.has_nodata, d.nodata = int(nodata is not None), int(nodata or 0)
    return d


def count(plane, hist, dev, nodata=None):
    L.check(L.backend().nirgan_scene_hist(C.byref(hist_desc(plane, hist, nodata)), stream_of(dev)), "scene_hist")


def dev_hist(h, dev):
    return torch.from_numpy(np.ascontiguousarray(h, dtype=np.int64)).to(dev)


# ------------------------------------------------------------------------------------------------ the count alone
def count_sizes(dev, n, shift):
    """n codes starting at element ``shift`` of an exact allocation; nodata 3 left out; a table pre-filled near 2^33 between guards"""
    a = np.random.default_rng(20 + n).integers(0, 9, size=n).astype(u16)
    a[::5] = 60000 + (np.arange(len(a[::5])) % 5000)                             # far codes too: outside any window
    _, plane = offset_plane(a, dev, shift)
    before = (np.arange(CODES, dtype=np.int64) * 3 + (1 << 33) - 5)
    buf, table = guarded_table(dev, before)
    count(plane, table, dev, nodata=3)
    assert table_guards_intact(buf)
    assert np.array_equal(host(table), before + histogram(a, 3))
    assert same_bits(host(plane), a)


def count_every_code_once(dev):
    a = np.random.default_rng(21).permutation(CODES).astype(u16)
    table = torch.zeros(CODES, dtype=torch.int64, device=dev)
    count(upload(a, dev), table, dev)
    assert np.array_equal(host(table), np.ones(CODES, dtype=np.int64))


def count_one_code(dev):
    """2^20 pixels of ONE code: the most contended case"""
    a = np.full(1 << 20, 4321, dtype=u16)
    table = torch.zeros(CODES, dtype=torch.int64, device=dev)
    count(upload(a, dev), table, dev)
    assert np.array_equal(host(table), histogram(a))


def count_pools(dev):
    """two calls into one table = bincount of the concatenation; the Python entry with ``into``"""
    src, ref = main_input()
    table = torch.zeros(CODES, dtype=torch.int64, device=dev)
    count(upload(src.reshape(-1), dev), table, dev, 0)
    count(upload(ref.reshape(-1), dev), table, dev, 0)
    want = histogram(np.concatenate([src.reshape(-1), ref.reshape(-1)]), 0)
    assert np.array_equal(host(table), want)
    h = scene_histogram(upload(src, dev), 0)
    assert h.dtype == torch.int64 and tuple(h.shape) == (CODES,)
    assert scene_histogram(ref, 0, into=h) is h and np.array_equal(host(h), want)        # a numpy plane is uploaded
    assert np.array_equal(host(scene_histogram(upload(src, dev))), histogram(src))       # nodata=None: every pixel counts


def wrap_plane():
    rng = np.random.default_rng(22)
    a = np.clip(np.rint(rng.normal(3000.0, 800.0, size=WRAP)), 0, 65535).astype(u16)
    a[:, :300] = 0
    far = rng.random(WRAP) < 0.01
    a[far] = rng.integers(0, CODES, size=int(far.sum())).astype(u16)
    return a


def count_and_apply_wrap(dev):
    """2100 x 4100: both grids wrap; the count with nodata, the apply in place with a permutation table"""
    a = wrap_plane()
    plane = upload(a.copy(), dev)                                                # rewritten in place below
    table = torch.zeros(CODES, dtype=torch.int64, device=dev)
    count(plane, table, dev, 0)
    assert np.array_equal(host(table), histogram(a, 0))
    lut = np.random.default_rng(23).permutation(CODES).astype(u16)
    run_apply(plane.view(-1), plane.view(-1), upload(lut, dev), dev, 0)
    assert same_bits(host(plane), apply_table(a, lut, 0))


# ------------------------------------------------------------------------------------------------ the apply alone
def run_apply(src, dst, lut, dev, nodata=None):
    d = L.SceneMatchDesc()
    d.plane, d.n, d.lut, d.out = src.data_ptr(), src.numel(), lut.data_ptr(), dst.data_ptr()
    d.has_nodata, d.nodata = int(nodata is not None), int(nodata or 0)
    L.check(L.backend().nirgan_scene_lut_apply(C.byref(d), stream_of(dev)), "scene_lut_apply")


def apply_sizes(dev, n, shift_in, shift_out):
    """a random permutation table: a wrong index cannot hide; out of place into guarded codes, then in place"""
    rng = np.random.default_rng(30 + n)
    a = rng.integers(0, CODES, size=n).astype(u16)
    a[::7] = 7
    lut_h = rng.permutation(CODES).astype(u16)
    lut = upload(lut_h, dev)
    _, plane = offset_plane(a, dev, shift_in)
    buf = torch.full((GUARD + shift_out + n + GUARD,), -21555, dtype=torch.int16, device=dev)
    out = buf[GUARD + shift_out:GUARD + shift_out + n]
    for nodata in (None, 7):
        out.fill_(-1)
        run_apply(plane, out, lut, dev, nodata)
        assert bool((buf[:GUARD + shift_out] == -21555).all()) and bool((buf[GUARD + shift_out + n:] == -21555).all())
        assert same_bits(host(out), apply_table(a, lut_h, nodata))
        assert same_bits(host(plane), a)
    run_apply(plane, plane, lut, dev, 7)
    assert same_bits(host(plane), apply_table(a, lut_h, 7))


# ------------------------------------------------------------------------------------------------ the table alone
def tables(dev):
    """all 65 536 entries against the restatement for every input, the totals, twice bitwise"""
    for hs, hr, nd in table_inputs():
        s, r = dev_hist(hs, dev), dev_hist(hr, dev)
        lut = torch.full((CODES,), -1, dtype=torch.int16, device=dev)
        totals = torch.full((2,), -1, dtype=torch.int64, device=dev)
        d = L.SceneMatchDesc()
        d.src_hist, d.ref_hist, d.lut, d.totals = s.data_ptr(), r.data_ptr(), lut.data_ptr(), totals.data_ptr()
        d.has_nodata, d.nodata = int(nd is not None), int(nd or 0)
        L.check(L.backend().nirgan_scene_match_lut(C.byref(d), stream_of(dev)), "scene_match_lut")
        want = match_table(hs, hr, nd)
        assert same_bits(host(lut), want)
        assert host(totals).tolist() == [int(hs.sum()), int(hr.sum())]
        assert (np.diff(want.astype(np.int64)) >= 0).all()                       # the table is non-decreasing
        again = scene_match_lut(s, r, nd)
        assert same_bits(host(again), want)
        assert same_bits(host(s), hs) and same_bits(host(r), hr)


def ties_on_the_device(dev):
    for s, r, want in TIES:
        a = from_counts(s)
        got = host(histogram_match_scene(upload(a, dev), upload(from_counts(r), dev)))
        assert same_bits(got, np.array([want[int(v)] for v in a], dtype=u16))


# ------------------------------------------------------------------------------------------------ the whole route
def main_route(dev):
    src, ref = main_input()
    plane = upload(src.copy(), dev)                                              # rewritten in place at the end
    got = histogram_match_scene(plane, upload(ref, dev), nodata=0)
    want = match_plane(src, ref, 0, 0)
    assert got.shape == plane.shape and got.dtype == plane.dtype and got.data_ptr() != plane.data_ptr()
    assert same_bits(host(got), want) and same_bits(host(plane), src)
    assert (want[src != 0] != src[src != 0]).mean() > 0.9                        # nearly every valid pixel changes code
    assert same_bits(host(histogram_match_scene(plane, scene_histogram(upload(ref, dev), 0), nodata=0)), want)       # a histogram reference
    assert same_bits(host(histogram_match_scene(src, ref, nodata=0)), want)      # numpy planes
    assert histogram_match_scene(plane, upload(ref, dev), nodata=0, out=plane) is plane and same_bits(host(plane), want)  # in place


def properties(dev):
    src, ref = main_input()
    valid = src[src != 0]
    plane = upload(valid, dev)
    assert same_bits(host(histogram_match_scene(plane, plane)), valid)           # matched to itself: unchanged
    assert same_bits(host(histogram_match_scene(upload(src, dev), upload(src, dev), nodata=0)), src)
    one = np.full((4, 5), 777, dtype=u16)
    got = host(histogram_match_scene(upload(src, dev), upload(one, dev), nodata=0))
    assert same_bits(got, np.where(src == 0, 0, 777).astype(u16))                # a one-code reference
    empty = np.zeros((6, 6), dtype=u16)
    assert same_bits(host(histogram_match_scene(upload(empty, dev), upload(ref, dev), nodata=0)), empty)     # all-nodata source
    assert same_bits(host(histogram_match_scene(upload(src, dev), upload(empty, dev), nodata=0)), src)       # all-nodata reference
    ident = host(scene_match_lut(scene_histogram(upload(empty, dev), 0), scene_histogram(upload(ref, dev), 0), 0))
    assert same_bits(ident, np.arange(CODES, dtype=u16))                         # the identity, nodata move not applied


def nodata_codes(dev):
    for src, ref, nd, rnd in nodata_inputs():
        lut = match_table(histogram(src, nd), histogram(ref, rnd))               # before the move
        present = np.unique(src[src != nd]).astype(np.int64)
        assert (lut[present] == nd).any()                                        # a table value lands on the reserved code
        got = host(histogram_match_scene(upload(src, dev), upload(ref, dev), nodata=nd, reference_nodata=rnd))
        assert same_bits(got, match_plane(src, ref, nd, rnd))
        assert not (got[src != nd] == nd).any() and (got[src == nd] == nd).all()
        moved = 65534 if nd == 65535 else nd + 1
        assert (got[src != nd] == moved).any()


# ------------------------------------------------------------------------------------------------ predict_scene / ScenePool
TILING = dict(tile=32, margin=4, overlap=6)


def predict_scene_matches(dev):
    """match=plane == predict_scene() then histogram_match_scene == the restatement; match=histogram == match=plane"""
    rng = np.random.default_rng(40)
    a = rng.integers(1, 10000, size=(3, 61, 83)).astype(u16)
    yy, xx = np.mgrid[0:61, 0:83]
    a[1][yy / 61 + xx / 83 < 0.5] = 0
    _, ref = main_input()
    scene = upload(a, dev)
    for nodata_out, rnd in ((None, None), (7, 0), (65535, 0)):
        kw = dict(nodata=0, batch=3, **TILING, **({} if nodata_out is None else {"nodata_out": nodata_out}))
        plain = predict_scene(tile_ramp, scene, **kw)
        got = predict_scene(tile_ramp, scene, match=upload(ref, dev), match_nodata=rnd, **kw)
        nd = 0 if nodata_out is None else nodata_out
        ref_nd = 0 if rnd is None else rnd                                       # match_nodata defaults to nodata
        want = match_plane(host(plain), ref, nd, ref_nd)
        assert same_bits(host(got), want)
        assert same_bits(host(histogram_match_scene(plain, upload(ref, dev), nodata=nd, reference_nodata=ref_nd)), want)
        bad = (a == 0).any(axis=0)
        assert (host(got)[bad] == nd).all() and not (host(got)[~bad] == nd).any()
        by_hist = predict_scene(tile_ramp, scene, match=scene_histogram(upload(ref, dev), ref_nd), **kw)
        assert same_bits(host(by_hist), want)
        assert same_bits(host(predict_scene(tile_ramp, a, match=ref, match_nodata=rnd, **kw)), want)        # numpy on both sides


def predict_scene_without_nodata_reserves_nothing(dev):
    a = np.random.default_rng(41).integers(0, 10000, size=(3, 40, 50)).astype(u16)
    ref = np.random.default_rng(42).integers(0, 40, size=(17, 19)).astype(u16)     # dense around 0: table values land on code 0
    plain = host(predict_scene(tile_ramp, upload(a, dev), **TILING))
    got = host(predict_scene(tile_ramp, upload(a, dev), match=upload(ref, dev), **TILING))
    assert same_bits(got, match_plane(plain, ref, None, None))
    assert (got == 0).any()


def python_refusals(dev):
    a = upload(np.random.default_rng(43).integers(1, 10000, size=(3, 40, 50)).astype(u16), dev)
    ref = upload(np.arange(600, dtype=u16).reshape(20, 30), dev)
    calls = [lambda: predict_scene(tile_ramp, a, match=ref, out="float32", **TILING),
             lambda: predict_scene(tile_ramp, a, match=ref, out="float16", **TILING),
             lambda: predict_scene(tile_ramp, a, match=ref.to(torch.float32), **TILING),
             lambda: predict_scene(tile_ramp, a, match=ref[:, ::2], **TILING),
             lambda: predict_scene(tile_ramp, a, match=torch.zeros(100, dtype=torch.int64, device=ref.device), **TILING),
             lambda: histogram_match_scene(ref, ref.to(torch.float32)),
             lambda: histogram_match_scene(ref.to(torch.float32), ref),
             lambda: histogram_match_scene(ref, ref, nodata=65536),
             lambda: histogram_match_scene(ref, ref, out=torch.empty(5, dtype=torch.int16, device=ref.device)),
             lambda: scene_histogram(ref, nodata=-1),
             lambda: scene_histogram(ref, into=torch.zeros(CODES, dtype=torch.int32, device=ref.device)),
             lambda: scene_histogram(np.zeros((3, 3), dtype=np.int32)),
             lambda: scene_match_lut(torch.zeros(CODES, dtype=torch.int64, device=ref.device), torch.zeros(7, dtype=torch.int64, device=ref.device))]
    for i, call in enumerate(calls):
        try:
            call()
        except ValueError:
            continue
        raise AssertionError(f"call {i} was taken")


POOL_SHAPES = [(23, 31), (40, 17), (9, 64)]


def pool_arrays():
    rng = np.random.default_rng(44)
    arrays = [rng.integers(0, 300, size=(4, h, w)).astype(u16) for h, w in POOL_SHAPES]
    return arrays


def band_histogram(dev):
    """against bincount over the RAW scenes; a subset; a float pool raises"""
    arrays = pool_arrays()
    pool = ScenePool(arrays, bands=(3, 0, 1, 2), divisor=5000.0, nodata=0, device=dev)
    for band in (0, 3):
        want = sum(histogram(a[band], 0) for a in arrays)
        got = pool.band_histogram(band)
        assert got.dtype == torch.int64 and np.array_equal(host(got), want)
    assert np.array_equal(host(pool.band_histogram(2, scenes=[2, 0])), histogram(arrays[2][2], 0) + histogram(arrays[0][2], 0))
    raw = ScenePool(arrays, device=dev)                                          # no nodata: every code counts
    assert np.array_equal(host(raw.band_histogram(1)), sum(histogram(a[1]) for a in arrays))
    for call in (lambda: pool.band_histogram(4), lambda: pool.band_histogram(0, scenes=[3]),
                 lambda: ScenePool([a.astype(np.float32) for a in arrays], device=dev).band_histogram(0)):
        try:
            call()
        except ValueError:
            continue
        raise AssertionError("band_histogram took a bad argument")


class Spy:
    """passes every call on to the backend under it and keeps the names of the new entries it saw"""

    def __init__(self, inner):
        self.inner, self.seen = inner, []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        if name not in NEW_ENTRIES:
            return fn

        def spied(ref, stream=None):
            self.seen.append(name)
            return fn(ref, stream)
        return spied


def pool_predict(dev):
    """ScenePool.predict(match=...) == predict_scene(match=...) on the same array; no launch of the new entries without match"""
    arrays = [np.random.default_rng(45 + i).integers(1, 10000, size=(4, h, w)).astype(u16) for i, (h, w) in enumerate([(40, 50), (61, 83)])]
    arrays[1][0, :20, :30] = 0
    pool = ScenePool(arrays, bands=(3, 0, 1, 2), divisor=5000.0, nodata=0, device=dev)
    real = ScenePool(pool_arrays(), bands=(0, 1, 2, 3), nodata=0, device=dev)
    ref_hist = real.band_histogram(3)
    kw = dict(batch=3, window="cosine", **TILING)
    before = L.backend()
    spy = Spy(before)
    L.set_backend(spy)
    try:
        plain = pool.predict(tile_ramp, 1, **kw)
        assert spy.seen == []
        got = pool.predict(tile_ramp, 1, match=ref_hist, **kw)
        assert spy.seen == ["nirgan_scene_hist", "nirgan_scene_match_lut", "nirgan_scene_lut_apply"]
    finally:
        L.set_backend(before)
    want = apply_table(host(plain), match_table(histogram(host(plain), 0), host(ref_hist), 0), 0)
    assert same_bits(host(got), want)
    ref = predict_scene(tile_ramp, arrays[1], bands=(3, 0, 1), divisor=5000.0, nodata=0, match=ref_hist, **kw)
    assert same_bits(host(got), host(ref))
    bad = (arrays[1][[3, 0, 1]] == 0).any(axis=0)
    assert (host(got)[bad] == 0).all() and not (host(got)[~bad] == 0).any()


# ------------------------------------------------------------------------------------------------ GPU only
def close_to_the_float_entry(dev):
    """equal sizes, no nodata: within +-1 of rint of inference.histogram_match on the float32 conversions (both evaluate the same
    piecewise-linear function with errors far below 0.5: only a value next to a half-integer can round apart)"""
    rng = np.random.default_rng(50)
    a = np.clip(np.rint(rng.normal(3000.0, 800.0, size=(64, 96))), 1, 65535).astype(u16)
    b = np.clip(np.rint(rng.gamma(2.0, 1500.0, size=(64, 96))), 1, 65535).astype(u16)
    new = host(histogram_match_scene(upload(a, dev), upload(b, dev))).astype(np.int64)
    fa = torch.from_numpy(a.astype(np.float32))[None, None].to(dev)
    fb = torch.from_numpy(b.astype(np.float32))[None, None].to(dev)
    old = np.rint(histogram_match(fa, fb)[0, 0].cpu().numpy().astype(np.float64)).astype(np.int64)
    diff = np.abs(new - old)
    print(f"new entry against the float entry: max |difference| {int(diff.max())}, {int((diff > 0).sum())} of {diff.size} pixels differ")
    assert diff.max() <= 1


# ------------------------------------------------------------------------------------------------ refusals before any launch
FAKE = 0x10000                                                                   # a non-null "device address" that no refused call may touch


def entries_reject_bad_arguments(be):
    """every descriptor below is refused with NIRGAN_ERR_ARG and a message naming the entry; device memory is never touched (the
    addresses are not memory), so this runs against the real library without a GPU"""
    entries = {"scene_hist": be.nirgan_scene_hist, "scene_match_lut": be.nirgan_scene_match_lut, "scene_lut_apply": be.nirgan_scene_lut_apply}

    def good():
        d = L.SceneMatchDesc()
        d.plane, d.n, d.has_nodata, d.nodata = FAKE, 5063, 1, 0
        d.hist, d.src_hist, d.ref_hist, d.totals, d.lut, d.out = FAKE + 0x100000, FAKE + 0x200000, FAKE + 0x300000, FAKE + 0x400000, FAKE + 0x500000, FAKE + 0x600000
        return d

    def refused(which, change, word=None):
        for name in ([which] if isinstance(which, str) else which):
            d = good()
            change(d)
            rc = entries[name](C.byref(d), None)
            msg = be.nirgan_last_error()
            msg = msg.decode() if isinstance(msg, bytes) else msg
            assert rc == -1 and name in msg, (name, rc, msg)
            if word:
                assert word in msg, (name, msg)

    planes, everyone = ["scene_hist", "scene_lut_apply"], list(entries)
    for fn in entries.values():
        assert fn(None, None) == -1
    refused(planes, lambda d: setattr(d, "plane", None), "null")
    refused("scene_hist", lambda d: setattr(d, "hist", None), "null")
    for field in ("src_hist", "ref_hist", "lut"):
        refused("scene_match_lut", lambda d, f=field: setattr(d, f, None), "null")
    for field in ("lut", "out"):
        refused("scene_lut_apply", lambda d, f=field: setattr(d, f, None), "null")
    for n in (0, -1, 2 ** 31, 2 ** 40):
        refused(planes, lambda d, n=n: setattr(d, "n", n), "n")
    for nd in (-1, 65536):
        refused(everyone, lambda d, nd=nd: setattr(d, "nodata", nd), "nodata")
    refused(planes, lambda d: setattr(d, "plane", FAKE + 1), "aligned")
    refused("scene_lut_apply", lambda d: setattr(d, "out", FAKE + 0x600001), "aligned")
    refused("scene_hist", lambda d: setattr(d, "hist", FAKE + 0x100004), "aligned")
    for field in ("src_hist", "ref_hist", "lut", "totals"):
        refused("scene_match_lut", lambda d, f=field: setattr(d, f, getattr(d, f) + 4), "aligned")
    refused("scene_lut_apply", lambda d: setattr(d, "lut", d.lut + 2), "aligned")
    refused("scene_lut_apply", lambda d: setattr(d, "out", d.plane + 2), "overlap")
    refused("scene_lut_apply", lambda d: setattr(d, "out", d.plane + 2 * 5062), "overlap")
    refused("scene_lut_apply", lambda d: setattr(d, "out", d.plane - 2 * 5062), "overlap")
