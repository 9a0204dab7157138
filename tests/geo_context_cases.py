"""Shared bodies of the geo-context tests (nirgan_point_regions / nirgan_raster_lookup and validation_utils.geo_ablation /
plot_val_spiders): run on the numpy emulator (tests/test_geo_context_emulated.py, device "cpu") and on the MI355X
(tests/test_gpu_geo_context.py, device "cuda:0").

Two oracles for the polygon entry.
  1. The float64 numpy statement of include/nirgan_hip.h (tests/emu_geo_context.statement_regions): EXACT equality on every point
     of every set, for slab_verts 8, 64 and the default -- tiny slabs put slab boundaries inside rings, on closing edges and
     between rings of different regions.
  2. An independent one that shares nothing with the statement: closed-form membership from the coordinates alone (grid, square
     with hole, enclave, two-part multipolygon, the repeated-closing-vertex pair) or ``matplotlib.path.Path.contains_points``
     (triangle, "C", star: no holes to interpret).  Membership of a point within rounding of an edge is not defined independently
     of the arithmetic, so this oracle applies to points farther than 1e-9 x the layer's extent from every edge (distance in
     float64), and at most 1 % of a set may be dropped for that reason (asserted).  The near-edge set is compared with the
     statement only.

Point sets, all seeded: uniform over 1.5 x the layer's extent (N = 1, 257, 1000; some miss every box); the integer lattice over the
extent + 2 on every side (y equal to vertex ys, rays along horizontal edges and through vertices: the half-open straddle rule), with
the lattice points that lie ON an edge moved to the near-edge set, for the star also integer x at the ys of 64 of its vertices; and
the near-edge set: v0 + t (v1 - v0) rounded to float64 and the same nudged by +-1..4 ulp in x or in y, at least 2000 points.
"""
import functools
import json
import math
import os

import numpy as np
import torch

from emu_geo_context import statement_raster, statement_regions

SLABS = (8, 64, 0)
LAYERS = ("triangle", "c_shape", "square_hole", "two_parts", "enclave", "closing_vertex", "grid", "star")
UNIFORM_N = (1, 257, 1000)


def _square(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


@functools.lru_cache(maxsize=None)
def layer_arrays(name):
    """(verts [V, 2] float64, ring_start, ring_region, n_regions) -- rings as lists of vertices first"""
    if name == "triangle":
        rings = [(0, [(0, 0), (4, 0), (1, 3)])]
    elif name == "c_shape":
        rings = [(0, [(0, 0), (4, 0), (4, 1), (1, 1), (1, 3), (4, 3), (4, 4), (0, 4)])]
    elif name == "square_hole":
        rings = [(0, _square(0, 0, 6, 6)), (0, _square(2, 2, 4, 4))]
    elif name == "two_parts":
        rings = [(0, _square(0, 0, 2, 2)), (0, _square(3, 1, 5, 4))]
    elif name == "enclave":                    # B inside A's hole, listed after A
        rings = [(0, _square(0, 0, 6, 6)), (0, _square(2, 2, 4, 4)), (1, _square(2, 2, 4, 4))]
    elif name == "closing_vertex":             # the same square with and without its first vertex repeated at the end
        rings = [(0, _square(0, 0, 2, 2) + [(0, 0)]), (1, _square(3, 0, 5, 2))]
    elif name == "grid":                       # 3 x 24 unit squares, region 3 * floor(x) + floor(y): 72 regions, three bitset words
        rings = [(3 * i + j, _square(i, j, i + 1, j + 1)) for i in range(24) for j in range(3)]
    elif name == "star":                       # 1500 vertices, star-shaped about the origin, seeded radial jitter
        rng = np.random.default_rng(1500)
        k = np.arange(1500)
        rad = 1.0 + 0.5 * (k % 2) + 0.2 * rng.random(1500)
        ang = 2 * np.pi * k / 1500
        rings = [(0, list(zip((rad * np.cos(ang)).tolist(), (rad * np.sin(ang)).tolist())))]
    else:
        raise KeyError(name)
    verts = np.asarray([p for _, ring in rings for p in ring], dtype=np.float64).reshape(-1, 2)
    ring_start = np.cumsum([0] + [len(ring) for _, ring in rings]).astype(np.int32)
    ring_region = np.asarray([g for g, _ in rings], dtype=np.int32)
    for a in (verts, ring_start, ring_region):
        a.setflags(write=False)
    return verts, ring_start, ring_region, int(ring_region.max()) + 1


def extent(name):
    v = layer_arrays(name)[0]
    lo, hi = v.min(axis=0), v.max(axis=0)
    return lo, hi, float((hi - lo).max())


def edges(name):
    """every edge of the layer, closing edges included: (v0 [E, 2], v1 [E, 2])"""
    verts, rs, _, _ = layer_arrays(name)
    a, b = [], []
    for r in range(len(rs) - 1):
        v = verts[rs[r]:rs[r + 1]]
        a.append(v)
        b.append(np.roll(v, -1, axis=0))
    return np.concatenate(a), np.concatenate(b)


def edge_distance(name, pts):
    """float64 distance of every point to the nearest edge (segment) of the layer"""
    v0, v1 = edges(name)
    e = v1 - v0
    ee = (e * e).sum(axis=1)
    out = np.full(pts.shape[0], np.inf)
    for at in range(0, pts.shape[0], 2048):
        p = pts[at:at + 2048, None, :]
        t = np.clip(((p - v0[None]) * e[None]).sum(axis=2) / np.where(ee > 0, ee, 1.0)[None], 0.0, 1.0)
        near = v0[None] + t[..., None] * e[None]
        out[at:at + 2048] = np.sqrt(((p - near) ** 2).sum(axis=2)).min(axis=1)
    return out


def _in(pts, x0, y0, x1, y1):
    return (pts[:, 0] > x0) & (pts[:, 0] < x1) & (pts[:, 1] > y0) & (pts[:, 1] < y1)


def independent_regions(name, pts):
    """membership from the coordinates alone (closed form) or from matplotlib's Path -- valid away from the edges"""
    if name in ("triangle", "c_shape", "star"):
        return np.where(_path_inside(name, pts), 0, -1)
    if name == "square_hole":
        return np.where(_in(pts, 0, 0, 6, 6) & ~_in(pts, 2, 2, 4, 4), 0, -1)
    if name == "two_parts":
        return np.where(_in(pts, 0, 0, 2, 2) | _in(pts, 3, 1, 5, 4), 0, -1)
    if name == "enclave":
        return np.where(_in(pts, 2, 2, 4, 4), 1, np.where(_in(pts, 0, 0, 6, 6), 0, -1))
    if name == "closing_vertex":
        return np.where(_in(pts, 0, 0, 2, 2), 0, np.where(_in(pts, 3, 0, 5, 2), 1, -1))
    if name == "grid":
        fx, fy = np.floor(pts[:, 0]), np.floor(pts[:, 1])
        return np.where(_in(pts, 0, 0, 24, 3), 3 * fx + fy, -1).astype(np.int64)
    raise KeyError(name)


def _path_inside(name, pts):
    from matplotlib.path import Path
    verts = layer_arrays(name)[0]                                               # one ring, no holes
    return Path(np.concatenate([verts, verts[:1]]), closed=True).contains_points(pts)


@functools.lru_cache(maxsize=None)
def uniform_points(name, n):
    lo, hi, _ = extent(name)
    mid, half = (lo + hi) / 2, 0.75 * (hi - lo)
    rng = np.random.default_rng(1000 * LAYERS.index(name) + n)
    pts = mid + half * (2 * rng.random((n, 2)) - 1)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _lattice(name):
    lo, hi, ext = extent(name)
    xs = np.arange(math.floor(lo[0]) - 2, math.ceil(hi[0]) + 3, dtype=np.float64)
    ys = np.arange(math.floor(lo[1]) - 2, math.ceil(hi[1]) + 3, dtype=np.float64)
    pts = np.stack(np.meshgrid(xs, ys, indexing="ij"), axis=-1).reshape(-1, 2)
    if name == "star":                          # integer x at the y of 64 vertices (its vertices are not integers)
        vy = layer_arrays(name)[0][::24][:64, 1]
        pts = np.concatenate([pts, np.stack(np.meshgrid(xs, vy, indexing="ij"), axis=-1).reshape(-1, 2)])
    on_edge = edge_distance(name, pts) <= 1e-9 * ext
    return pts[~on_edge], pts[on_edge]


def integer_points(name):
    return _lattice(name)[0]


@functools.lru_cache(maxsize=None)
def near_edge_points(name):
    """on the edges as float64 rounds them, and 1..4 ulp either side in x or in y; the lattice points that lie on edges too"""
    v0, v1 = edges(name)
    use = np.unique(np.linspace(0, v0.shape[0] - 1, min(v0.shape[0], 64)).astype(int))
    T = max(3, -(-2000 // (17 * len(use))) + 1)
    t = np.linspace(0.0, 1.0, T)[None, :, None]
    base = (v0[use][:, None, :] + t * (v1[use] - v0[use])[:, None, :]).reshape(-1, 2)
    sets = [base]
    for axis in (0, 1):
        for k in (1, 2, 3, 4):
            for toward in (-np.inf, np.inf):
                p = base.copy()
                for _ in range(k):
                    p[:, axis] = np.nextafter(p[:, axis], toward)
                sets.append(p)
    pts = np.concatenate(sets + [_lattice(name)[1]])
    assert pts.shape[0] >= 2000
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def statement_of(name, which, n=0):
    pts = {"uniform": lambda: uniform_points(name, n), "integer": lambda: integer_points(name), "near": lambda: near_edge_points(name)}[which]()
    verts, rs, rr, G = layer_arrays(name)
    out = statement_regions(pts, verts, rs, rr, G)
    out.setflags(write=False)
    return out


def make_layer(dev, name, properties=None):
    from validation_utils import PolygonLayer
    verts, rs, rr, G = layer_arrays(name)
    return PolygonLayer.from_arrays(verts, rs, rr, G, properties, device=dev)


def device_regions(dev, layer, pts, slab):
    from validation_utils import points_in_regions
    got = points_in_regions(torch.from_numpy(pts[:, 0].copy()), torch.from_numpy(pts[:, 1].copy()), layer, slab_verts=slab)
    assert got.dtype == torch.int64 and got.device == torch.device(dev) and tuple(got.shape) == (pts.shape[0],)
    return got.cpu().numpy()


def check_against_both(dev, name, which, n=0):
    """every slab size against the statement, exactly, on every point; then (not for the near-edge set) the independent oracle on
    the points away from the edges, of which at most 1 % may be dropped"""
    pts = {"uniform": lambda: uniform_points(name, n), "integer": lambda: integer_points(name), "near": lambda: near_edge_points(name)}[which]()
    want = statement_of(name, which, n)
    layer = make_layer(dev, name)
    got = None
    for slab in SLABS:
        got = device_regions(dev, layer, pts, slab)
        wrong = np.flatnonzero(got != want)
        assert wrong.size == 0, (name, which, n, slab, wrong[:5], pts[wrong[:5]], got[wrong[:5]], want[wrong[:5]])
    if which == "near":
        return
    _, _, ext = extent(name)
    far = edge_distance(name, pts) > 1e-9 * ext
    dropped = int((~far).sum())
    print(f"{name} {which} {n}: {pts.shape[0]} points, {dropped} within 1e-9 x extent of an edge, {int((want >= 0).sum())} inside")
    assert dropped <= 0.01 * pts.shape[0], (name, which, dropped)
    ind = independent_regions(name, pts[far])
    wrong = np.flatnonzero(got[far] != ind)
    assert wrong.size == 0, (name, which, n, pts[far][wrong[:5]], got[far][wrong[:5]], ind[wrong[:5]])
    if which == "uniform" and n == 1000:
        assert (want >= 0).any() and (want < 0).any()                           # the set sees both sides
        boxes = layer.region_box.cpu().numpy()
        miss = ((pts[:, None, 0] < boxes[None, :, 0]) | (pts[:, None, 0] > boxes[None, :, 2])
                | (pts[:, None, 1] < boxes[None, :, 1]) | (pts[:, None, 1] > boxes[None, :, 3])).all(axis=1)
        assert miss.any()                                                       # some points miss every box


def region_boxes_are_the_vertex_extents(dev):
    for name in LAYERS:
        verts, rs, rr, G = layer_arrays(name)
        box = make_layer(dev, name).region_box.cpu().numpy()
        for g in range(G):
            v = np.concatenate([verts[rs[r]:rs[r + 1]] for r in range(len(rr)) if rr[r] == g])
            assert box[g].tolist() == [v[:, 0].min(), v[:, 1].min(), v[:, 0].max(), v[:, 1].max()], (name, g)
    from validation_utils import PolygonLayer                                   # a region without rings: the empty box, and nobody is in it
    lay = PolygonLayer.from_arrays(np.asarray(_square(0, 0, 1, 1), dtype=np.float64), [0, 4], [1], 3, device=dev)
    assert lay.region_box.cpu().tolist() == [[math.inf, math.inf, -math.inf, -math.inf], [0.0, 0.0, 1.0, 1.0], [math.inf, math.inf, -math.inf, -math.inf]]
    assert device_regions(dev, lay, np.asarray([[0.5, 0.5], [2.0, 0.5]]), 0).tolist() == [1, -1]


def special_points_and_empty_problems(dev):
    """NaN / infinite coordinates are outside; float32 coordinates widen exactly; no points, no regions, no rings"""
    from validation_utils import PolygonLayer, points_in_regions
    layer = make_layer(dev, "enclave")
    nan, inf = math.nan, math.inf
    pts = np.asarray([[nan, 1.0], [1.0, nan], [inf, 1.0], [-inf, 1.0], [1.0, inf], [1.0, -inf], [1.0, 1.0], [3.0, 3.0]])
    want = statement_regions(pts, *layer_arrays("enclave"))
    assert want.tolist() == [-1, -1, -1, -1, -1, -1, 0, 1]
    for slab in SLABS:
        assert device_regions(dev, layer, pts, slab).tolist() == want.tolist()
    x32 = torch.tensor([0.1, 2.1, 3.9, 5.7], dtype=torch.float32)
    y32 = torch.tensor([0.3, 2.2, 2.1, 7.1], dtype=torch.float32)
    got = points_in_regions(x32, y32, layer).cpu().numpy()
    wide = np.stack([x32.double().numpy(), y32.double().numpy()], axis=1)
    assert got.tolist() == statement_regions(wide, *layer_arrays("enclave")).tolist() == [0, 1, 1, -1]
    assert points_in_regions([0.5, 3.0], [0.5, 3.0], layer).tolist() == [0, 1]      # lists
    assert tuple(points_in_regions([], [], layer).shape) == (0,)
    none = PolygonLayer.from_arrays(np.zeros((0, 2)), [0], [], 0, device=dev)
    assert points_in_regions([1.0, 2.0], [1.0, 2.0], none).tolist() == [-1, -1]
    bare = PolygonLayer.from_arrays(np.zeros((0, 2)), [0], [], 2, device=dev)       # regions without a single ring
    assert points_in_regions([1.0], [1.0], bare).tolist() == [-1]


# ---------------------------------------------------------------------------------------------------------------- raster
RASTER_U8 = (np.arange(35, dtype=np.uint8).reshape(7, 5) + 1)
RASTER_I16 = (np.arange(35, dtype=np.int16).reshape(7, 5) * 37 - 500)
RASTER_I16[2, 3] = RASTER_I16[6, 0] = -7                                           # nodata cells
GENERAL = (-3.3, 0.7, 10.1, -0.9)                                                 # x0, dx, y0, dy: north to south
POW2_UP = (-2.0, 0.25, -1.0, 0.5)                                                 # positive dy, steps that are powers of two
POW2_DOWN = (-2.0, 0.25, 2.5, -0.5)
RASTERS = [("u8", RASTER_U8, None), ("i16", RASTER_I16, -7), ("i32", RASTER_I16.astype(np.int32) * 1000, -7000)]


def raster_points(transform, H=7, W=5):
    """(points, expected (row, col) or None): cell centres; >= 1e-6 cells from a border; outside on each of the four sides"""
    x0, dx, y0, dy = transform
    rng = np.random.default_rng(75)
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    r, c = r.reshape(-1), c.reshape(-1)
    centres = np.stack([x0 + (c + 0.5) * dx, y0 + (r + 0.5) * dy], axis=1)
    f = 1e-6 + (1 - 2e-6) * rng.random((8, r.size, 2))
    inner = np.stack([x0 + (c[None] + f[..., 0]) * dx, y0 + (r[None] + f[..., 1]) * dy], axis=2).reshape(-1, 2)
    cells = np.concatenate([np.stack([r, c], axis=1)] + [np.stack([r, c], axis=1)] * 8)
    out = np.asarray([[x0 - 0.5 * dx, y0 + 2.5 * dy], [x0 + (W + 0.5) * dx, y0 + 2.5 * dy], [x0 + 2.5 * dx, y0 - 0.5 * dy],
                      [x0 + 2.5 * dx, y0 + (H + 0.5) * dy], [x0 - 1e6 * abs(dx), y0 - 1e6 * abs(dy)], [math.nan, y0 + dy], [x0 + dx, math.nan],
                      [math.inf, y0 + dy], [x0 + dx, -math.inf]])
    return np.concatenate([centres, inner]), cells, out


def border_points(transform, H=7, W=5):
    """points exactly on cell borders (power-of-two steps: x0 + c * dx is exact and so is the division): border c belongs to cell c"""
    x0, dx, y0, dy = transform
    r, c = np.meshgrid(np.arange(H + 1), np.arange(W + 1), indexing="ij")
    r, c = r.reshape(-1), c.reshape(-1)
    return np.stack([x0 + c * dx, y0 + r * dy], axis=1), np.stack([r, c], axis=1)


def _lookup(dev, raster, pts):
    from validation_utils import raster_lookup
    got = raster_lookup(torch.from_numpy(pts[:, 0].copy()), torch.from_numpy(pts[:, 1].copy()), raster)
    assert got.dtype == torch.int64 and got.device == torch.device(dev)
    return got.cpu().numpy()


def raster_lookup_cases(dev):
    from validation_utils import RasterLayer
    for _, array, nodata in RASTERS:
        clean = array.astype(np.int64)
        if nodata is not None:
            clean = np.where(clean == nodata, 0, clean)
        for transform in (GENERAL, POW2_UP, POW2_DOWN):
            layer = RasterLayer(array, transform, nodata, device=dev)
            pts, cells, outside = raster_points(transform)
            got = _lookup(dev, layer, pts)
            assert got.tolist() == statement_raster(pts, array, *transform, nodata).tolist()
            assert got.tolist() == clean[cells[:, 0], cells[:, 1]].tolist()          # the independent expectation
            assert _lookup(dev, layer, outside).tolist() == [0] * len(outside) == statement_raster(outside, array, *transform, nodata).tolist()
        for transform in (POW2_UP, POW2_DOWN):
            layer = RasterLayer(array, transform, nodata, device=dev)
            pts, cells = border_points(transform)
            want = np.where((cells[:, 0] < 7) & (cells[:, 1] < 5), clean[np.minimum(cells[:, 0], 6), np.minimum(cells[:, 1], 4)], 0)
            got = _lookup(dev, layer, pts)
            assert got.tolist() == statement_raster(pts, array, *transform, nodata).tolist() == want.tolist()
    wide = RasterLayer(RASTER_U8.astype(np.int64), GENERAL, device=dev)             # other integer dtypes go through int32
    assert wide.array.dtype == torch.int32 and _lookup(dev, wide, raster_points(GENERAL)[0][:35]).tolist() == RASTER_U8.reshape(-1).tolist()


# ---------------------------------------------------------------------------------------------------------------- the join
CONTINENTS = ("Africa", "Asia", "Europe", "Oceania")
ECONOMIES = ("1. Developed region: G7", "2. Developed region: nonG7", "6. Developing region", "7. Least developed region", "9. Other", None, 5)
LEGEND = {"id": list(range(1, 31)), "Code": ["Af", "Am", "Aw", "BWh", "BWk", "BSh", "BSk", "Csa", "Csb", "Csc", "Cwa", "Cwb", "Cwc", "Cfa", "Cfb",
                                              "Cfc", "Dsa", "Dsb", "Dsc", "Dsd", "Dwa", "Dwb", "Dwc", "Dwd", "Dfa", "Dfb", "Dfc", "Dfd", "ET", "EF"]}


def world_layer(dev):
    """the grid layer as a world of 72 countries"""
    props = {"SOV_A3": [f"C{g:02d}" for g in range(72)], "CONTINENT": [CONTINENTS[g % 4] for g in range(72)],
             "ECONOMY": [ECONOMIES[g % 7] for g in range(72)], "NAME": [f"country {g}" for g in range(72)]}
    return make_layer(dev, "grid", props)


def koppen_layer(dev):
    """ids 1..30 in 12 x 3 cells of 2 x 1 over the grid's extent, north to south; id 40 is not in the legend, 255 is nodata"""
    from validation_utils import RasterLayer
    a = (np.arange(36, dtype=np.uint8).reshape(3, 12) % 30) + 1
    a[0, 0], a[1, 5] = 255, 40
    return RasterLayer(a, (0.0, 2.0, 3.0, -1.0), nodata=255, device=dev), a


def table_of(n, seed=5):
    """a validation table of n rows: points over 1.25 x the grid's extent, metrics with a NaN"""
    rng = np.random.default_rng(seed)
    x = (12 + 15 * (2 * rng.random(n) - 1)).tolist()
    y = (1.5 + 1.9 * (2 * rng.random(n) - 1)).tolist()
    ssim, psnr = rng.random(n).tolist(), (20 + 10 * rng.random(n)).tolist()
    psnr[n // 2] = math.nan
    return {"id": list(range(n)), "x": x, "y": y, "ssim": ssim, "psnr": psnr, "l1": rng.random(n).tolist()}


def join_end_to_end(dev, n, tmp_path):
    """append_info_to_df + clean_economy against the closed-form grid membership and the raster by hand; GeoJSON round trip; the
    radar charts of two joined tables"""
    from validation_utils import append_info_to_df, clean_economy, plot_radar_comparison, read_geojson_table, summarize_by, write_geojson
    from validation_utils.geo_ablation import ECONOMY_CLASSES
    world, (koppen, ids) = world_layer(dev), koppen_layer(dev)
    table = table_of(n)
    joined = append_info_to_df(table, world, koppen, LEGEND)
    assert list(joined) == ["id", "x", "y", "ssim", "psnr", "l1", "Country", "Continent", "ECONOMY", "Koppen_Class"]
    assert all(joined[k] == table[k] for k in table)
    pts = np.stack([table["x"], table["y"]], axis=1)
    far = edge_distance("grid", pts) > 1e-9 * 24
    assert far.all()                                                            # seeded: no row within rounding of a border
    region = independent_regions("grid", pts)
    assert (region < 0).any() and (region >= 0).sum() > n // 2
    codes = dict(zip(LEGEND["id"], LEGEND["Code"]))
    for i in range(n):
        g = int(region[i])
        assert joined["Country"][i] == (None if g < 0 else f"C{g:02d}")
        assert joined["Continent"][i] == (None if g < 0 else CONTINENTS[g % 4])
        assert joined["ECONOMY"][i] == (None if g < 0 else ECONOMIES[g % 7])
        inside = 0 <= pts[i, 0] < 24 and 0 < pts[i, 1] <= 3
        k = int(ids[int(math.floor(3 - pts[i, 1])), int(math.floor(pts[i, 0] / 2))]) if inside else 0
        assert joined["Koppen_Class"][i] == ("U" if k in (0, 255, 40) else codes[k][0].upper()), (i, k)
    assert {"U", "A", "B", "C", "D", "E"} == set(joined["Koppen_Class"])
    cleaned = clean_economy(joined)
    assert "ECONOMY" not in cleaned and list(cleaned)[-1] == "economy"
    for i in range(n):
        e = joined["ECONOMY"][i]
        assert cleaned["economy"][i] == (ECONOMY_CLASSES[int(e[0])] if isinstance(e, str) and int(e[0]) in ECONOMY_CLASSES else "Unknown")
    path = tmp_path / "joined" / "table.geojson"
    write_geojson(cleaned, str(path))
    back = read_geojson_table(str(path))
    assert list(back) == list(cleaned)
    for k in cleaned:
        assert all((a == b) or (isinstance(a, float) and math.isnan(a) and math.isnan(b)) for a, b in zip(cleaned[k], back[k])), k
    doc = json.load(open(path))
    assert doc["type"] == "FeatureCollection" and len(doc["features"]) == n
    assert doc["features"][3]["geometry"] == {"type": "Point", "coordinates": [table["x"][3], table["y"][3]]}
    other = dict(cleaned, psnr=[v - 1.0 for v in cleaned["psnr"]], ssim=[0.9 * v for v in cleaned["ssim"]])
    for data_type, out_name, file in (("Continent", "", "metrics_radar_satclip_Continent.png"),
                                      ("Koppen_Class", "E 003", "metrics_radar_satclip_E_003_Koppen_Class.png"),
                                      ("economy", "E003", "metrics_radar_satclip_E003_economy.png")):
        img = plot_radar_comparison(cleaned, other, data_type, out_name=out_name, folder=str(tmp_path / "graphs"))
        size = img.size if hasattr(img, "size") and not isinstance(img, np.ndarray) else img.shape[1::-1]
        assert min(size) > 100 and os.path.getsize(tmp_path / "graphs" / file) > 1000
    s = summarize_by(cleaned, "Continent")
    assert s["Continent"] == sorted(CONTINENTS) and all(20 < v < 30 for v in s["psnr"])
    return joined
