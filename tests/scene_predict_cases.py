"""Case bodies of the in-place scene prediction (nirgan_hip.inference.predict_scene / ScenePool.predict, nirgan_scene_tile_invalid /
nirgan_scene_tile_gather / nirgan_scene_finish), shared by tests/test_scene_predict_emulated.py (numpy emulator, CPU) and
tests/test_gpu_scene_predict.py (MI355X).

Every comparison is BITWISE (``same_bits``: the arrays' raw words, so NaN and -0 count) and leaves no element out.  The references:
  the float path   predict_tiled(blend="blend") on the host-converted scene a[bands].astype(float32) / float32(divisor), same tiling;
  the geometry     restated here per tile from core = tile - 2 margin, stride = core - overlap, tiles per axis 1 if H <= core else
                   ceil((H - core) / stride) + 1, usable region of tile (ti, tj) = rows [ti stride, + core) x columns [tj stride, + core)
                   clipped to the scene;
  the entries      tests/emu_scene_predict.py (cut_tiles / tile_centres / quantise), itself written from the header.
The stand-in models depend on the position inside a tile, so a geometry error shows.
"""
import ctypes as C
import math

import numpy as np
import torch

from emu_backend import obj
from emu_scene_predict import OUT_F16, OUT_F32, OUT_U16, cut_tiles, quantise, tile_centres
from nirgan_hip import lib as L
from nirgan_hip.data import ScenePool
from nirgan_hip.inference import predict_scene, predict_tiled
from tile_blend_cases import Recorder, guarded, guards_intact, stream_of, tile_offset, tile_ramp

f32 = np.float32
TILING = (32, 4, 6)                                                              # tile, margin, overlap: core 24, stride 18
SCENES = [(3, 61, 83), (3, 20, 20), (5, 24, 100)]                                # 20 x 20: smaller than a tile, more than one reflection away
BATCHES = (1, 3, 8)
NODATA = 0
GEO = (11.25, 9.0e-5, 47.5, -9.0e-5)                                             # lon0, dlon, lat0, dlat
KINDS = {"uint16": OUT_U16, "float16": OUT_F16, "float32": OUT_F32}


# ------------------------------------------------------------------------------------------------ helpers
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def host(t):
    """a device result as numpy; int16 bit patterns come back as uint16"""
    a = t.detach().cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def scene_u16(shape, seed=0):
    """uint16 [C][H][W], values 1 .. 9999: no pixel is NODATA"""
    return np.random.default_rng(seed + 1000 * shape[1] + shape[2]).integers(1, 10000, size=shape, dtype=np.uint16)


def scene_of(shape, kind, seed=0):
    a = scene_u16(shape, seed)
    return a if kind == "u16" else a.astype(f32)


def upload(a, dev):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def float_scene(a, bands, divisor):
    return (a[list(bands)].astype(f32) / f32(divisor)).astype(f32)


def bands_of(shape):
    return (0, 1, 2) if shape[0] == 3 else (2, 0, 1)


def per_axis(extent, core, stride):
    return 1 if extent <= core else math.ceil((extent - core) / stride) + 1


def regions(H, W, tiling):
    """[(y0, y1, x0, x1)] of every tile's clipped usable region, in tile order"""
    tile, margin, overlap = tiling
    core = tile - 2 * margin
    stride = core - overlap
    return [(i * stride, min(i * stride + core, H), j * stride, min(j * stride + core, W))
            for i in range(per_axis(H, core, stride)) for j in range(per_axis(W, core, stride))]


def brute_counts(bad, tiling):
    return np.array([int(bad[y0:y1, x0:x1].sum()) for y0, y1, x0, x1 in regions(*bad.shape, tiling)], dtype=np.int64)


def brute_run_list(bad, tiling):
    return [t for t, (y0, y1, x0, x1) in enumerate(regions(*bad.shape, tiling)) if not bad[y0:y1, x0:x1].all()]


def punch(a, bands, kind):
    """nodata into a [C][H][W] scene (H >= 90, W >= 120): a rectangle that swallows whole tiles (in one band only), one that cuts
    tiles (in another band), a diagonal edge -> the bool mask of invalid pixels"""
    _, H, W = a.shape
    hole = f32("nan") if kind == "f32" else NODATA
    bad = np.zeros((H, W), dtype=bool)
    bad[0:45, 30:W] = True                                                       # swallows the usable regions of several tiles
    a[bands[1], 0:45, 30:W] = hole
    cut = np.zeros((H, W), dtype=bool)
    cut[60:71, 5:29] = True                                                      # cuts tiles
    a[bands[2], 60:71, 5:29] = hole
    yy, xx = np.mgrid[0:H, 0:W]
    diag = yy + xx >= H + W - 60                                                 # the far corner behind a diagonal edge
    for b in bands:
        a[b][diag] = hole
    return bad | cut | diag


def desc_of(scene, shape, bands, tiling, nodata=None, divisor=10000.0):
    d = L.ScenePredictDesc()
    d.scene = scene if isinstance(scene, int) else scene.data_ptr()
    d.dtype = L.SCENE_F32 if (not isinstance(scene, int) and scene.dtype == torch.float32) else L.SCENE_U16
    d.C, d.H, d.W = shape
    d.band = (C.c_int * 3)(*bands)
    d.has_nodata, d.nodata = int(nodata is not None), int(nodata or 0)
    d.divisor = divisor
    d.tile, d.margin, d.overlap = tiling
    return d


# ------------------------------------------------------------------------------------------------ equals the float path
def equals_the_float_path(dev, shape, kind, batch):
    """out="float32", no nodata: bitwise predict_tiled(blend="blend") on the host-converted scene, both windows and overlap = 0"""
    tile, margin, overlap = TILING
    bands, divisor = bands_of(shape), 10000.0
    a = scene_of(shape, kind)
    ref_in = torch.from_numpy(float_scene(a, bands, divisor))[None].to(dev)
    for model in (tile_ramp, tile_offset):
        for window, ov in (("linear", overlap), ("cosine", overlap), ("linear", 0)):
            got = predict_scene(model, upload(a, dev), bands=bands, divisor=divisor, tile=tile, margin=margin, overlap=ov, window=window,
                                batch=batch, out="float32")
            ref = predict_tiled(model, ref_in, tile=tile, margin=margin, batch=batch, blend="blend", overlap=ov, window=window)[0, 0]
            assert got.shape == (shape[1], shape[2]) and got.dtype == torch.float32
            assert same_bits(host(got), host(ref)), (model.__name__, window, ov)


def flips_equal_the_float_path(dev):
    shape, (tile, margin, overlap) = SCENES[0], TILING
    a = scene_u16(shape, 3)
    got = predict_scene(tile_ramp, upload(a, dev), tile=tile, margin=margin, overlap=overlap, batch=8, tta="flips", out="float32")
    ref_in = torch.from_numpy(float_scene(a, (0, 1, 2), 10000.0))[None].to(dev)
    ref = predict_tiled(tile_ramp, ref_in, tile=tile, margin=margin, batch=8, blend="blend", overlap=overlap, tta="flips")[0, 0]
    assert same_bits(host(got), host(ref))


def numpy_scene_is_uploaded_as_it_is(dev):
    shape, (tile, margin, overlap) = SCENES[0], TILING
    a = scene_u16(shape, 4)
    one = predict_scene(tile_ramp, a, tile=tile, margin=margin, overlap=overlap)
    two = predict_scene(tile_ramp, upload(a, dev), tile=tile, margin=margin, overlap=overlap)
    assert one.dtype == torch.int16 and same_bits(host(one), host(two))


# ------------------------------------------------------------------------------------------------ the gather entry alone
def gather_alone(dev, shape, kind, tiling, every=None, with_coords=True):
    """guarded outputs, an exactly allocated scene, a list with gaps (``every``: keep tiles t with t % every != 1; None: all), the
    list cut in launches of 5 and the rest"""
    tile, margin, overlap = tiling
    bands = bands_of(shape)
    a = scene_of(shape, kind, 5)
    dev_scene = upload(a, dev)                                                   # exactly C * H * W elements
    nt = len(regions(shape[1], shape[2], tiling))
    ids_host = np.array([t for t in range(nt) if every is None or t % every != 1], dtype=np.int32)
    ids = torch.from_numpy(ids_host.copy()).to(dev)
    n = len(ids_host)
    tbuf, tiles = guarded(n * 3 * tile * tile, -3.0, -7.0, dev)
    cbuf, coords = guarded(n * 2, -3.0, -7.0, dev)
    geo = torch.tensor(GEO, dtype=torch.float64).to(dev)
    be, st = L.backend(), stream_of(dev)
    d = desc_of(dev_scene, shape, bands, tiling, divisor=7.0)
    first = min(5, n)
    for i0, m in ((0, first), (first, n - first)):
        if m == 0:
            continue
        d.ids, d.ids_host, d.n = ids.data_ptr() + 4 * i0, ids_host.ctypes.data + 4 * i0, m
        d.tiles = tiles.data_ptr() + 4 * i0 * 3 * tile * tile
        d.geo, d.coords = (geo.data_ptr(), coords.data_ptr() + 8 * i0) if with_coords else (None, None)
        L.check(be.nirgan_scene_tile_gather(C.byref(d), st), "scene_tile_gather")
    assert guards_intact(tbuf, n * 3 * tile * tile, -7.0) and guards_intact(cbuf, n * 2, -7.0)
    assert same_bits(host(tiles).reshape(n, 3, tile, tile), cut_tiles(a, bands, ids_host, tile, margin, overlap, 7.0))
    if with_coords:
        assert same_bits(host(coords).reshape(n, 2), tile_centres(GEO, ids_host, shape[1], shape[2], *tiling))
    else:
        assert bool((coords == -3.0).all())


def gather_wide(dev):
    """40 x 9000 at stride 8, every other tile: 2813 tiles of 32 x 32, more quads than one pass of the gather's grid holds"""
    shape, tiling = (3, 40, 9000), (32, 12, 0)
    assert (len(regions(shape[1], shape[2], tiling)) // 2 - 5) * 3 * 32 * 8 > 8192 * 256
    gather_alone(dev, shape, "u16", tiling, every=2)


# ------------------------------------------------------------------------------------------------ counts
def counts_are_the_brute_force_count(dev, shape, kind, tiling):
    bands = bands_of(shape)
    a = scene_of(shape, kind, 6)
    bad = punch(a, bands, kind)
    dev_scene = upload(a, dev)
    nt = len(regions(shape[1], shape[2], tiling))
    cbuf, counts = guarded(nt, -3.0, -7.0, dev)                                  # float words; the entry writes int32 into them
    d = desc_of(dev_scene, shape, bands, tiling, nodata=NODATA)
    d.counts = counts.data_ptr()
    L.check(L.backend().nirgan_scene_tile_invalid(C.byref(d), stream_of(dev)), "scene_tile_invalid")
    assert guards_intact(cbuf, nt, -7.0)
    got = host(counts).view(np.int32).astype(np.int64)
    want = brute_counts(bad, tiling)
    assert np.array_equal(got, want)
    areas = np.array([(y1 - y0) * (x1 - x0) for y0, y1, x0, x1 in regions(shape[1], shape[2], tiling)])
    assert (want == areas).any() and ((want > 0) & (want < areas)).any() and (want == 0).any()       # the scene exercises all three


def counts_wide(dev):
    """40 x 9000 at stride 6: more tiles than workgroups in the grid"""
    shape, tiling = (3, 40, 9000), (32, 12, 2)
    a = np.random.default_rng(16).integers(0, 6, size=shape, dtype=np.uint16)
    a[:, :, 100:400] = NODATA
    bad = (a == NODATA).any(axis=0)
    nt = len(regions(shape[1], shape[2], tiling))
    assert nt > 8192
    dev_scene = upload(a, dev)
    counts = torch.full((nt,), -1, dtype=torch.int32, device=dev)
    d = desc_of(dev_scene, shape, (0, 1, 2), tiling, nodata=NODATA)
    d.counts = counts.data_ptr()
    L.check(L.backend().nirgan_scene_tile_invalid(C.byref(d), stream_of(dev)), "scene_tile_invalid")
    assert np.array_equal(host(counts).astype(np.int64), brute_counts(bad, tiling))


# ------------------------------------------------------------------------------------------------ skipping
SKIP_SHAPE = (4, 96, 130)


def skipping(dev, kind, out, window="linear", batch=3, tta="none"):
    """the tiles the model saw are exactly the brute-force list; every valid pixel is bitwise the float path run on ALL tiles after the
    same quantisation done in numpy; every invalid pixel is nodata_out"""
    tile, margin, overlap = TILING
    shape, bands, divisor = SKIP_SHAPE, (0, 1, 2), 10000.0
    a = scene_of(shape, kind, 7)
    bad = punch(a, bands, kind)
    run_list = brute_run_list(bad, TILING)
    assert 0 < len(run_list) < len(regions(shape[1], shape[2], TILING))
    nodata_out = {"uint16": 7, "float16": -2.0, "float32": float("nan")}[out]
    rec = Recorder(tile_ramp)
    got = predict_scene(rec, upload(a, dev), bands=bands, divisor=divisor, nodata=NODATA, tile=tile, margin=margin, overlap=overlap,
                        window=window, batch=batch, tta=tta, out=out, scale=10000.0, nodata_out=nodata_out)
    if tta == "none":
        seen, _ = rec.tiles()
        assert same_bits(seen, cut_tiles(a, bands, run_list, tile, margin, overlap, divisor))
    ref_in = torch.from_numpy(float_scene(a, bands, divisor))[None].to(dev)
    ref = host(predict_tiled(tile_ramp, ref_in, tile=tile, margin=margin, batch=batch, blend="blend", overlap=overlap, window=window, tta=tta)[0, 0])
    want = quantise(ref, bad, KINDS[out], 10000.0, nodata_out)                   # the mask puts nodata_out on every invalid pixel
    g = host(got)
    assert same_bits(g, want)
    assert same_bits(g[bad], np.full(int(bad.sum()), nodata_out).astype(want.dtype))
    if out == "uint16":
        assert not (g[~bad] == 7).any()
    return rec


def without_nodata_nothing_is_skipped(dev, kind):
    """nodata=None: the scene's holes are ordinary values, every tile runs"""
    tile, margin, overlap = TILING
    a = scene_u16(SKIP_SHAPE, 8) if kind == "u16" else scene_u16(SKIP_SHAPE, 8).astype(f32)
    a[:, 0:45, 30:] = 0
    rec = Recorder(tile_ramp)
    got = predict_scene(rec, upload(a, dev), tile=tile, margin=margin, overlap=overlap, batch=8, out="float32")
    assert sum(len(x) for x in rec.inputs) == len(regions(SKIP_SHAPE[1], SKIP_SHAPE[2], TILING))
    ref_in = torch.from_numpy(float_scene(a, (0, 1, 2), 10000.0))[None].to(dev)
    ref = predict_tiled(tile_ramp, ref_in, tile=tile, margin=margin, batch=8, blend="blend", overlap=overlap)[0, 0]
    assert same_bits(host(got), host(ref))


def all_nodata_scene(dev):
    a = np.zeros((3, 40, 50), dtype=np.uint16)
    rec = Recorder(tile_ramp)
    got = predict_scene(rec, upload(a, dev), nodata=0, tile=32, margin=4)
    assert rec.inputs == [] and same_bits(host(got), np.zeros((40, 50), dtype=np.uint16))


# ------------------------------------------------------------------------------------------------ the finish entry alone
def finish_values():
    """(v float32 [n], scale): exact .5 ties on both sides of even codes, negatives, values past 65535, NaN, infinities, values landing
    on the codes 0, 7 and 65535, and float16 ties"""
    ties = [0.5, 1.5, 2.5, 3.5, 6.5, 7.5, 8.5, 65533.5, 65534.5, 65535.5, 0.49999997, 0.50000006]
    codes = [0.0, 0.2, 7.0, 7.4, 6.6, 65535.0, 65534.6, 65535.4, 8.0, 1.0, 65534.0]
    wild = [-0.5, -0.0, -3.0, -1e9, 65536.0, 70000.0, 1e9, 3e38, float("inf"), float("-inf"), float("nan")]
    half = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 65504.0, 65519.99, 65520.0, 2.0 ** -25, 2.0 ** -24, 3 * 2.0 ** -25, 1e-8]
    return np.array(ties + codes + wild + half, dtype=f32)


def finish_alone(dev, kind, out, nodata_out, width, shift=0):
    """hand-made blended values under a scene with a few nodata pixels; ``width`` 24: H * W is a multiple of four, 23: it is odd and the
    last quad is partial; ``shift`` = 1: blended and out start four bytes off every vector alignment (element-wise accesses)"""
    H, W, scale = 3, width, 1.0
    special = finish_values()
    assert H * W >= len(special)                                                 # every special value is in the scene
    v = np.concatenate([special, (np.random.default_rng(9).random(H * W - len(special)) * 70000.0 - 2000.0).astype(f32)])
    shape, bands = (3, H, W), (0, 1, 2)
    a = scene_of(shape, kind, 10)
    hole = f32("nan") if kind == "f32" else NODATA
    bad = np.zeros((H, W), dtype=bool)
    bad[1, 3], bad[2, W - 1], bad[0, 0] = True, True, True
    a[1, 1, 3], a[2, 2, W - 1], a[0, 0, 0] = hole, hole, hole
    dev_scene = upload(a, dev)
    bbuf, blended = guarded(H * W, 0.0, -7.0, dev, shift)
    blended.copy_(torch.from_numpy(v))
    esize = 4 if out == "float32" else 2
    words = (H * W * esize + 3) // 4                                             # the output lives in float words between the guards
    obuf, outw = guarded(words, -3.0, -7.0, dev, shift)
    d = desc_of(dev_scene, shape, bands, TILING, nodata=NODATA)
    d.blended, d.out, d.out_kind = blended.data_ptr(), outw.data_ptr(), KINDS[out]
    d.scale, d.nodata_out = scale, nodata_out
    L.check(L.backend().nirgan_scene_finish(C.byref(d), stream_of(dev)), "scene_finish")
    assert guards_intact(bbuf, H * W, -7.0, shift) and guards_intact(obuf, words, -7.0, shift)
    raw = host(outw).view(np.uint8)
    assert same_bits(raw[H * W * esize:], np.full(words, -3.0, dtype=f32).view(np.uint8)[H * W * esize:])     # the half word behind an odd count
    got = raw[:H * W * esize].view({"uint16": np.uint16, "float16": np.float16, "float32": f32}[out]).reshape(H, W)
    vv = v.reshape(H, W)
    if out == "uint16":                                                          # the issue's statement, written out
        with np.errstate(over="ignore", invalid="ignore"):
            t = np.rint(f32(vv) * f32(scale))
        q = np.clip(np.where(np.isnan(t), 0, t), 0, 65535).astype(np.int64)
        q = np.where(q == nodata_out, 65534 if nodata_out == 65535 else nodata_out + 1, q)
        want = np.where(bad | np.isnan(t), nodata_out, q).astype(np.uint16)
        assert not (got[~bad & ~np.isnan(vv)] == nodata_out).any()
    elif out == "float16":
        with np.errstate(over="ignore"):
            want = np.where(bad, f32(nodata_out), vv).astype(np.float16)
    else:
        want = np.where(bad, f32(nodata_out), vv).astype(f32)
    assert same_bits(got, want)
    assert same_bits(want, quantise(vv, bad, KINDS[out], scale, nodata_out))      # the restatement says the same


def finish_wraps_its_grid(dev):
    """2100 x 4100 pixels: more quads than one pass of the finish's grid holds"""
    H, W = 2100, 4100
    rng = np.random.default_rng(11)
    a = rng.integers(0, 4, size=(3, H, W), dtype=np.uint16)                      # NODATA = 0 in a quarter of each band
    v = torch.from_numpy(rng.random((H, W), dtype=f32)).to(dev)
    scene = upload(a, dev)
    out = torch.empty(H, W, dtype=torch.int16, device=dev)
    d = desc_of(scene, (3, H, W), (0, 1, 2), TILING, nodata=NODATA)
    d.blended, d.out, d.out_kind, d.scale, d.nodata_out = v.data_ptr(), out.data_ptr(), OUT_U16, 10000.0, 0.0
    L.check(L.backend().nirgan_scene_finish(C.byref(d), stream_of(dev)), "scene_finish")
    assert same_bits(host(out), quantise(host(v), (a == 0).any(axis=0), OUT_U16, 10000.0, 0))


# ------------------------------------------------------------------------------------------------ coords
class CoordModel:
    """a two-argument model with the SatCLIP hook: keeps the coords it was asked to embed and the embeddings every call received"""

    def __init__(self):
        self.coords, self.embeds, self.sizes = [], [], []

    def satclip_get_inject(self, coords):
        self.coords.append(coords.detach().cpu().clone())
        return torch.cat([coords, coords.flip(1)], dim=1) * 0.5                  # an "embedding" that is a function of the location

    def __call__(self, x, e):
        self.embeds.append(e.detach().cpu().clone())
        self.sizes.append(x.shape[0])
        return x[:, :1] + e[:, :1, None, None]


def coords_per_tile(dev, tta="none"):
    """embeds="coords": per-tile coords equal the float64 formula (edge tiles with a clipped usable region included, skipped tiles left
    out), the model receives the embeddings row by row in tile order"""
    tile, margin, overlap = TILING
    shape, bands = SKIP_SHAPE, (0, 1, 2)
    a = scene_u16(shape, 12)
    bad = punch(a, bands, "u16")
    run_list = brute_run_list(bad, TILING)
    m = CoordModel()
    predict_scene(m, upload(a, dev), nodata=NODATA, geotransform=GEO, tile=tile, margin=margin, overlap=overlap, batch=4, embeds="coords", tta=tta)
    want = np.empty((len(run_list), 2), dtype=f32)
    regs = regions(shape[1], shape[2], TILING)
    for k, t in enumerate(run_list):
        y0, y1, x0, x1 = regs[t]
        cy, cx = np.float64(y0 + (y1 - y0) // 2) + 0.5, np.float64(x0 + (x1 - x0) // 2) + 0.5
        want[k] = f32(np.float64(GEO[0]) + cx * np.float64(GEO[1])), f32(np.float64(GEO[2]) + cy * np.float64(GEO[3]))
    assert any(y1 - y0 < tile - 2 * margin or x1 - x0 < tile - 2 * margin for y0, y1, x0, x1 in (regs[t] for t in run_list))
    got = torch.cat(m.coords).numpy()
    assert same_bits(got, want)
    k = L.TTA_VIEWS[tta]
    rows = np.repeat(np.concatenate([want, want[:, ::-1]], axis=1) * f32(0.5), k, axis=0)       # every view gets its tile's row
    assert same_bits(torch.cat(m.embeds).numpy(), rows.astype(f32))
    assert max(m.sizes) <= 4


def one_row_for_every_tile(dev):
    tile, margin, overlap = TILING
    a = scene_u16(SCENES[0], 13)
    seen = []

    def model(x, e):
        seen.append(e.detach().cpu().clone())
        return x[:, :1] * e[:, :1, None, None]
    row = torch.tensor([[0.5, 2.0, -1.0]]).to(dev)
    got = predict_scene(model, upload(a, dev), tile=tile, margin=margin, overlap=overlap, batch=5, embeds=row, out="float32")
    assert all(bool((e == row.cpu()).all()) and e.shape[1] == 3 for e in seen)
    assert sum(len(e) for e in seen) == len(regions(SCENES[0][1], SCENES[0][2], TILING))
    ref_in = torch.from_numpy(float_scene(a, (0, 1, 2), 10000.0))[None].to(dev)
    ref = predict_tiled(lambda x: x[:, :1] * 0.5, ref_in, tile=tile, margin=margin, batch=5, blend="blend", overlap=overlap)[0, 0]
    assert same_bits(host(got), host(ref))


# ------------------------------------------------------------------------------------------------ ScenePool.predict
class Spy:
    """passes every call on to the backend under it and keeps the scene address the new entries were handed"""

    def __init__(self, inner):
        self.inner, self.scene_ptrs = inner, []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)
        if name not in ("nirgan_scene_tile_invalid", "nirgan_scene_tile_gather", "nirgan_scene_finish"):
            return fn

        def spied(ref, stream=None):
            self.scene_ptrs.append(int(obj(ref).scene))
            return fn(ref, stream)
        return spied


def pool_predict(dev, kind):
    """ScenePool.predict equals predict_scene on the same array, and the entries read the pool's own buffer"""
    tile, margin, overlap = TILING
    shapes = [(4, 40, 50), SKIP_SHAPE]
    arrays = [scene_of(s, kind, 14 + i) for i, s in enumerate(shapes)]
    bad = punch(arrays[1], (3, 0, 1), kind)
    geos = [(1.0, 1e-4, 2.0, -1e-4), GEO]
    pool = ScenePool(arrays, bands=(3, 0, 1, 2), divisor=5000.0, nodata=NODATA, geotransforms=geos, device=dev)
    kw = dict(tile=tile, margin=margin, overlap=overlap, batch=3, out="uint16", window="cosine")
    before = L.backend()
    spy = Spy(before)
    L.set_backend(spy)
    try:
        got = pool.predict(tile_ramp, 1, **kw)
        m = CoordModel()
        pool.predict(m, 1, embeds="coords", **kw)
    finally:
        L.set_backend(before)
    esize = 2 if kind == "u16" else 4
    assert pool.scene(1).data_ptr() == pool.pool.data_ptr() + esize * pool.offsets[1]
    assert spy.scene_ptrs and set(spy.scene_ptrs) == {pool.pool.data_ptr() + esize * pool.offsets[1]}
    ref = predict_scene(tile_ramp, arrays[1], bands=(3, 0, 1), divisor=5000.0, nodata=NODATA, **kw)
    assert same_bits(host(got), host(ref))
    assert same_bits(host(got)[bad], np.zeros(int(bad.sum()), dtype=np.uint16))
    run_list = brute_run_list(bad, TILING)
    assert same_bits(torch.cat(m.coords).numpy(), tile_centres(GEO, run_list, SKIP_SHAPE[1], SKIP_SHAPE[2], *TILING))
    for key in ("bands", "divisor", "nodata", "geotransform"):
        try:
            pool.predict(tile_ramp, 0, **{key: None})
        except TypeError:
            continue
        raise AssertionError(f"ScenePool.predict took {key}")


def python_refusals(dev):
    a = upload(scene_u16((3, 40, 50)), dev)
    bad = [dict(tile=30), dict(tile=32, margin=16), dict(tile=32, margin=4, overlap=13), dict(window="hann"), dict(out="int8"), dict(tta="spin"),
           dict(bands=(0, 1, 3)), dict(bands=(0, 1)), dict(embeds="coords"), dict(embeds="lonlat"), dict(nodata=70000)]
    for kw in bad:
        try:
            predict_scene(tile_ramp, a, **{"tile": 32, "margin": 4, **kw})
        except ValueError:
            continue
        raise AssertionError(f"predict_scene took {kw}")
    for scene in (a[:2], a.to(torch.float64), a[:, :, ::2]):
        try:
            predict_scene(tile_ramp, scene, tile=32, margin=4)
        except ValueError:
            continue
        raise AssertionError("predict_scene took a bad scene")


# ------------------------------------------------------------------------------------------------ refusals before any launch
FAKE = 0x10000                                                                   # a non-null "device address" that no refused call may touch


def entries_reject_bad_arguments(be):
    """every descriptor below is refused with NIRGAN_ERR_ARG and a message naming the entry; device memory is never touched (the
    addresses are not memory), so this runs against the real library without a GPU"""
    ids_host = np.array([0, 1, 2], dtype=np.int32)
    entries = {"scene_tile_invalid": be.nirgan_scene_tile_invalid, "scene_tile_gather": be.nirgan_scene_tile_gather,
               "scene_finish": be.nirgan_scene_finish}

    def good():
        d = desc_of(FAKE, (3, 61, 83), (0, 1, 2), TILING, nodata=0)
        d.counts, d.ids, d.ids_host, d.n, d.tiles = FAKE, FAKE, ids_host.ctypes.data, 3, FAKE
        d.blended, d.out, d.out_kind, d.scale, d.nodata_out = FAKE, FAKE, OUT_U16, 10000.0, 0.0
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

    everyone = list(entries)
    for name, fn in entries.items():
        assert fn(None, None) == -1
    refused(everyone, lambda d: setattr(d, "scene", None), "null")
    refused("scene_tile_invalid", lambda d: setattr(d, "counts", None), "null")
    for field in ("ids", "ids_host", "tiles"):
        refused("scene_tile_gather", lambda d, f=field: setattr(d, f, None), "null")
    for field in ("blended", "out"):
        refused("scene_finish", lambda d, f=field: setattr(d, f, None), "null")
    refused(everyone, lambda d: setattr(d, "C", 2), "C")
    refused(everyone, lambda d: setattr(d, "band", (C.c_int * 3)(0, 1, 3)), "band")
    refused(everyone, lambda d: setattr(d, "band", (C.c_int * 3)(-1, 1, 2)), "band")

    def huge_plane(d):
        d.H, d.W = 65536, 32768                                                  # H * W = 2^31
    refused(everyone, huge_plane, "2^31")

    def huge_tiles(d):
        d.tile, d.margin, d.overlap, d.n = 16384, 4, 6, 3                        # n * 3 * tile^2 = 9 * 2^28 >= 2^31; ids 0 .. 2 need W > core
        d.H, d.W = 20000, 60000
    refused("scene_tile_gather", huge_tiles, "2^31")
    refused("scene_tile_gather", lambda d: setattr(d, "n", 0))
    for bad_ids, word in (([0, 2, 2], "predecessor"), ([1, 0, 2], "predecessor"), ([0, 1, 20], "outside"), ([-1, 0, 1], "outside")):
        keep = np.array(bad_ids, dtype=np.int32)
        refused("scene_tile_gather", lambda d, k=keep: setattr(d, "ids_host", k.ctypes.data), word)
    refused("scene_tile_gather", lambda d: setattr(d, "tiles", FAKE + 4), "aligned")
    refused(everyone, lambda d: setattr(d, "dtype", 2), "dtype")
    refused("scene_finish", lambda d: setattr(d, "out_kind", 3), "out_kind")
    refused("scene_finish", lambda d: setattr(d, "nodata_out", 65536.0), "nodata_out")
    refused("scene_finish", lambda d: setattr(d, "nodata_out", 6.5), "nodata_out")
    refused("scene_finish", lambda d: setattr(d, "nodata_out", float("nan")), "nodata_out")
    refused(everyone, lambda d: setattr(d, "divisor", 0.0), "divisor")
    refused(everyone, lambda d: setattr(d, "divisor", float("nan")), "divisor")
    refused(everyone, lambda d: setattr(d, "margin", 16), "margin")
    refused(everyone, lambda d: setattr(d, "margin", -1), "margin")
    refused(everyone, lambda d: setattr(d, "overlap", 13), "overlap")
    refused(everyone, lambda d: setattr(d, "overlap", -1), "overlap")
    refused(everyone, lambda d: setattr(d, "tile", 30), "tile")
    refused(everyone, lambda d: setattr(d, "nodata", 65536), "nodata")
    assert 20 >= len(regions(61, 83, TILING))                                    # id 20 above is out of range for this scene


# ------------------------------------------------------------------------------------------------ GPU only
def real_generator(dev):
    """A small 6-block generator (the configuration of the other real-generator inference tests), uint16 scene 96 x 130 with a nodata
    corner, tile 64: bitwise predict_tiled on the float scene plus numpy quantisation on every valid pixel, nodata_out elsewhere.
    batch = 1 on both sides: skipping changes how many tiles share a model call, and only a batch of one is the same call either way
    (a convolution library may pick its algorithm by batch size)."""
    from model import networks
    torch.manual_seed(0)
    net = networks.define_G(3, 1, 8, "resnet_6blocks", "instance", False, "normal", 0.02).to(dev).eval()
    shape, (tile, margin, overlap) = (3, 96, 130), (64, 4, 14)
    a = scene_u16(shape, 15)
    a[:, 0:60, 0:70] = NODATA                                                    # swallows tile 0's usable region (rows 0 .. 55, columns 0 .. 55)
    bad = (a == NODATA).any(axis=0)
    run_list = brute_run_list(bad, (tile, margin, overlap))
    assert 0 not in run_list and len(run_list) == 5
    rec = Recorder(net)
    got = predict_scene(rec, upload(a, dev), nodata=NODATA, tile=tile, margin=margin, overlap=overlap, batch=1)
    assert sum(len(x) for x in rec.inputs) == 5
    ref_in = torch.from_numpy(float_scene(a, (0, 1, 2), 10000.0))[None].to(dev)
    ref = host(predict_tiled(net, ref_in, tile=tile, margin=margin, batch=1, blend="blend", overlap=overlap)[0, 0])
    assert np.isfinite(ref[~bad]).all()
    assert same_bits(host(got), quantise(ref, bad, OUT_U16, 10000.0, 0))
