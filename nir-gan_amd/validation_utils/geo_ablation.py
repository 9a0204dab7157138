"""MI355X-native counterpart of the reference's ``validation_utils/geo_ablation.py``: the geo-context join of the validation table.

The reference joins every tile's lon / lat to a country layer with ``geopandas.sjoin`` and to a Koeppen raster with one
``rasterstats.point_query`` (one raster open) per point in a Python loop.  Here a layer is flattened and uploaded ONCE
(``PolygonLayer`` / ``RasterLayer``), a table's points go through ONE ``nirgan_point_regions`` / ``nirgan_raster_lookup`` call and
ONE host copy each, and the rest -- property lookup, the Koeppen letter, the economy map, GeoJSON -- is plain Python on the
project's tables (a dict of equal-length lists, as ``evaluate_tiles`` returns).  ``get_countries``, ``get_climate_zones``,
``final_touch``, ``append_info_to_df`` and ``clean_economy`` keep the reference's names and semantics; they return a new table.

Deviations, on purpose:
  * Planar coordinates: no antimeridian wrapping, no geodesic edges (neither ``sjoin`` nor the reference's layer has them).
  * Where regions overlap the LOWEST region index wins; ``sjoin`` would duplicate the row.
  * A point exactly on an edge belongs to whatever the crossing statement of include/nirgan_hip.h gives: unspecified.
  * The raster lookup reads the cell that CONTAINS the point.  The reference's ``point_query`` interpolates bilinearly between
    class ids and truncates with ``int()``, which blends neighbouring ids at class borders; that is not restated.
  * Layers come from GeoJSON (stdlib ``json``), arrays or ``.npz``: reading ``.shp`` / ``.tif`` is out of scope (no pyshp /
    rasterio here) -- convert once.
"""
import csv
import ctypes as C
import json
import math
import os

import numpy as np
import torch

from nirgan_hip import lib as L
from utils.calculate_metrics import _stream

ECONOMY_CLASSES = {1: "Developed: G7", 2: "Developed: Non G7", 3: "Emerging: BRIC", 4: "Emerging: MIKT", 5: "Emerging: G20",
                   6: "Developing", 7: "Least Developed"}                       # geo_ablation.py:77-83
CONTEXT_COLUMNS = ("Country", "Continent", "ECONOMY", "Koppen_Class")
_RASTER_DTYPES = {torch.uint8: L.RASTER_U8, torch.int16: L.RASTER_I16, torch.int32: L.RASTER_I32}


def _default_device():
    return torch.device("cpu" if L.is_emulated() else "cuda:0")


def _check_device(dev):
    if dev.type != "cuda" and not L.is_emulated():
        raise RuntimeError("nirgan_hip runs on MI355X (cuda device) only; there is no CPU path")


class PolygonLayer:
    """A polygon layer as the flat arrays of include/nirgan_hip.h, on the device: ``verts`` float64 [V, 2], ``ring_start`` int32
    [R + 1], ``ring_region`` int32 [R] (non-decreasing; holes and multipolygon parts are further rings of their region) and the
    per-region boxes (``nirgan_region_boxes``, once).  ``properties``: dict column -> list with one value per region."""

    def __init__(self, verts, ring_start, ring_region, n_regions=None, properties=None, device=None):
        v = np.array(verts, dtype=np.float64).reshape(-1, 2)                   # a copy: the caller's array is never aliased
        rs = np.ascontiguousarray(np.asarray(ring_start, dtype=np.int64)).reshape(-1)
        rr = np.ascontiguousarray(np.asarray(ring_region, dtype=np.int64)).reshape(-1)
        if rs.size != rr.size + 1 or rs[0] != 0 or rs[-1] != v.shape[0] or (np.diff(rs) < 0).any():
            raise ValueError("ring_start must be non-decreasing with R + 1 entries, start at 0 and end at the vertex count")
        G = int(n_regions) if n_regions is not None else (int(rr.max()) + 1 if rr.size else 0)
        if rr.size and ((np.diff(rr) < 0).any() or rr.min() < 0 or rr.max() >= G):
            raise ValueError("ring_region must be non-decreasing and lie in 0 .. n_regions-1")
        if not np.isfinite(v).all():
            raise ValueError("vertices must be finite")
        if max(v.shape[0], rs.size, G) >= 2 ** 31:
            raise ValueError("layer too large")
        self.properties = {k: list(col) for k, col in (properties or {}).items()}
        for k, col in self.properties.items():
            if len(col) != G:
                raise ValueError(f"property '{k}' has {len(col)} values for {G} regions")
        self.n_verts, self.n_rings, self.n_regions = v.shape[0], rr.size, G
        self.ring_start_host, self.ring_region_host = rs.astype(np.int32), rr.astype(np.int32)     # kept: the entries check them
        self.device = torch.device(device) if device is not None else _default_device()
        _check_device(self.device)
        self.verts = torch.from_numpy(v).to(self.device)
        self.ring_start = torch.from_numpy(self.ring_start_host).to(self.device)
        self.ring_region = torch.from_numpy(self.ring_region_host).to(self.device)
        self.region_box = torch.empty((G, 4), dtype=torch.float64, device=self.device)
        L.check(L.backend().nirgan_region_boxes(C.byref(self._desc()), _stream(self.device)), "region_boxes")

    def _desc(self):
        d = L.PointRegionsDesc()
        d.n_verts, d.n_rings, d.n_regions = self.n_verts, self.n_rings, self.n_regions
        d.verts, d.ring_start, d.ring_region = self.verts.data_ptr(), self.ring_start.data_ptr(), self.ring_region.data_ptr()
        d.region_box = self.region_box.data_ptr()
        d.ring_start_host, d.ring_region_host = self.ring_start_host.ctypes.data, self.ring_region_host.ctypes.data
        return d

    @classmethod
    def from_arrays(cls, verts, ring_start, ring_region, n_regions=None, properties=None, device=None):
        return cls(verts, ring_start, ring_region, n_regions, properties, device)

    @classmethod
    def from_geojson(cls, path_or_dict, device=None):
        """A FeatureCollection (or a list of features) of ``Polygon`` / ``MultiPolygon`` geometries, read with the stdlib: one region
        per feature in file order, every ring (outer rings and holes alike) as it stands, ``properties`` as per-region columns
        (``None`` where a feature lacks a key).  Other geometry types and null geometries give a region without rings."""
        if isinstance(path_or_dict, (str, os.PathLike)):
            with open(path_or_dict) as f:
                path_or_dict = json.load(f)
        feats = path_or_dict["features"] if isinstance(path_or_dict, dict) else list(path_or_dict)
        verts, ring_start, ring_region = [], [0], []
        keys = []
        for ft in feats:
            for k in (ft.get("properties") or {}):
                if k not in keys:
                    keys.append(k)
        for g, ft in enumerate(feats):
            geom = ft.get("geometry") or {}
            polys = {"Polygon": [geom.get("coordinates")], "MultiPolygon": geom.get("coordinates")}.get(geom.get("type"), [])
            for poly in polys or []:
                for ring in poly:
                    verts.extend((float(p[0]), float(p[1])) for p in ring)
                    ring_start.append(len(verts))
                    ring_region.append(g)
        props = {k: [(ft.get("properties") or {}).get(k) for ft in feats] for k in keys}
        return cls(np.asarray(verts, dtype=np.float64).reshape(-1, 2), ring_start, ring_region, len(feats), props, device)


class RasterLayer:
    """A north-up raster of class ids on the device: ``array`` [H, W] of uint8 / int16 / int32 (other integer dtypes are converted
    to int32 where their values fit), ``transform`` = (x0, dx, y0, dy) -- the x / y of the outer corner of cell [0][0] and the cell
    steps, dy negative for a raster stored north to south -- and ``nodata`` (cells equal to it read as 0)."""

    def __init__(self, array, transform, nodata=None, device=None):
        a = array.detach().cpu() if torch.is_tensor(array) else torch.from_numpy(np.ascontiguousarray(np.asarray(array)))
        if a.dim() != 2 or a.numel() == 0:
            raise ValueError(f"the raster must be a non-empty [H, W] array, got {tuple(a.shape)}")
        if a.dtype not in _RASTER_DTYPES:
            if a.is_floating_point() or a.is_complex() or a.dtype == torch.bool:
                raise ValueError(f"the raster must hold integer class ids, got {a.dtype}")
            wide = a.to(torch.int64)
            if wide.min() < -2 ** 31 or wide.max() >= 2 ** 31:
                raise ValueError("raster values do not fit int32")
            a = wide.to(torch.int32)
        self.transform = tuple(float(t) for t in transform)
        if len(self.transform) != 4:
            raise ValueError("transform must be (x0, dx, y0, dy)")
        self.nodata = None if nodata is None else int(nodata)
        self.device = torch.device(device) if device is not None else _default_device()
        _check_device(self.device)
        self.array = a.contiguous().to(self.device)

    @classmethod
    def from_npz(cls, path, device=None):
        """``array``, ``transform`` (4 values) and optionally ``nodata`` of a ``.npz`` file"""
        with np.load(path) as z:
            nodata = z["nodata"].item() if "nodata" in z.files else None
            return cls(z["array"], z["transform"].tolist(), nodata, device)


def _points(x, y, device):
    """x, y as one float64 [N, 2] tensor on ``device`` (float32 widens exactly)"""
    xs, ys = (t.detach() if torch.is_tensor(t) else torch.as_tensor(np.asarray(t)) for t in (x, y))
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    if xs.numel() != ys.numel():
        raise ValueError(f"x and y differ in length: {xs.numel()} and {ys.numel()}")
    if xs.numel() >= 2 ** 31:
        raise ValueError("too many points")
    return torch.stack([xs.to(device=device, dtype=torch.float64), ys.to(device=device, dtype=torch.float64)], dim=1).contiguous()


def points_in_regions(x, y, layer: PolygonLayer, slab_verts: int = 0) -> torch.Tensor:
    """The region index of every point (x[i], y[i]) in ``layer``, -1 outside all: an int64 tensor on the layer's device, no host
    sync.  Even-odd rule, the lowest index where regions overlap; ``slab_verts`` never changes the result (include/nirgan_hip.h)."""
    pts = _points(x, y, layer.device)
    N = pts.shape[0]
    be = L.backend()
    region = torch.full((N,), -1, dtype=torch.int32, device=layer.device)
    ws = torch.empty(max(int(be.nirgan_point_regions_ws_bytes(N, layer.n_regions)), 4) // 4, dtype=torch.int32, device=layer.device)
    d = layer._desc()
    d.points, d.n_points, d.slab_verts = pts.data_ptr(), N, int(slab_verts)
    d.ws, d.ws_bytes, d.region = ws.data_ptr(), ws.numel() * 4, region.data_ptr()
    L.check(be.nirgan_point_regions(C.byref(d), _stream(layer.device)), "point_regions")
    return region.to(torch.int64)


def raster_lookup(x, y, raster: RasterLayer) -> torch.Tensor:
    """The value of the cell of ``raster`` that contains every point, 0 outside the raster or on nodata: an int64 tensor on the
    raster's device, no host sync."""
    pts = _points(x, y, raster.device)
    N = pts.shape[0]
    value = torch.zeros((N,), dtype=torch.int32, device=raster.device)
    d = L.RasterLookupDesc()
    d.points, d.n_points = pts.data_ptr(), N
    d.H, d.W, d.dtype, d.raster = raster.array.shape[0], raster.array.shape[1], _RASTER_DTYPES[raster.array.dtype], raster.array.data_ptr()
    d.x0, d.dx, d.y0, d.dy = raster.transform
    d.has_nodata, d.nodata = int(raster.nodata is not None), raster.nodata or 0
    d.value = value.data_ptr()
    L.check(L.backend().nirgan_raster_lookup(C.byref(d), _stream(raster.device)), "raster_lookup")
    return value.to(torch.int64)


def _rows(table):
    n = {len(col) for col in table.values()}
    if len(n) > 1:
        raise ValueError("the table's columns differ in length")
    return n.pop() if n else 0


def get_countries(table, world: PolygonLayer):
    """``Country`` (the layer's ``SOV_A3``), ``Continent`` (``CONTINENT``) and ``ECONOMY`` of every row's (x, y): a left join --
    rows outside every region get ``None``.  Where regions overlap the lowest region index wins (``sjoin`` would duplicate the row)."""
    for key in ("SOV_A3", "CONTINENT", "ECONOMY"):
        if key not in world.properties:
            raise KeyError(f"get_countries: the layer has no '{key}' property")
    region = points_in_regions(table["x"], table["y"], world).cpu().tolist()               # the table's ONE host copy
    out = {k: list(v) for k, v in table.items()}
    for col, key in (("Country", "SOV_A3"), ("Continent", "CONTINENT"), ("ECONOMY", "ECONOMY")):
        src = world.properties[key]
        out[col] = [None if g < 0 else src[g] for g in region]
    return out


def _legend_codes(legend):
    """id -> code from a dict id -> code, a dict of columns {"id": [..], "Code": [..]}, or the path of the reference's legend CSV"""
    if legend is None:
        return {}
    if isinstance(legend, (str, os.PathLike)):
        with open(legend, newline="") as f:
            rows = list(csv.DictReader(f))
        return {int(r["id"]): r["Code"] for r in rows}
    if "id" in legend and "Code" in legend:
        return {int(i): c for i, c in zip(legend["id"], legend["Code"])}
    return {int(i): c for i, c in legend.items()}


def get_climate_zones(table, koppen: RasterLayer, legend):
    """``Koppen_Class``: the first letter, upper-cased, of the legend code of the raster id under every row's (x, y); id 0 (outside
    the raster, nodata: the reference's "Unknown" row) and ids the legend does not know give ``"U"`` (geo_ablation.py:43-52).
    Without a raster (``koppen=None``) every row is ``"U"``."""
    codes = _legend_codes(legend)
    n = _rows(table)
    ids = [0] * n if koppen is None else raster_lookup(table["x"], table["y"], koppen).cpu().tolist()
    out = {k: list(v) for k, v in table.items()}
    out["Koppen_Class"] = ["U" if i == 0 or not codes.get(i) else str(codes[i])[0].upper() for i in ids]
    return out


def final_touch(table, cols_to_keep=()):
    """the columns ``cols_to_keep`` + id, x, y, ssim and the four context columns, each once, in that order (the reference's
    ``geometry`` column is the pair x, y here)"""
    keep = []
    for k in list(cols_to_keep) + ["id", "x", "y", "ssim"] + list(CONTEXT_COLUMNS):
        if k not in keep and k != "geometry":
            keep.append(k)
    return {k: list(table[k]) for k in keep}


def append_info_to_df(table, world: PolygonLayer, koppen: RasterLayer = None, legend=None):
    """The reference's join (geo_ablation.py:64-71): the table's own columns plus Country, Continent, ECONOMY, Koppen_Class.  The
    reference reads its layers from hard-coded paths; here they are arguments."""
    original = list(table.keys())
    out = get_countries(table, world)
    out = get_climate_zones(out, koppen, legend)
    return final_touch(out, cols_to_keep=original)


def clean_economy(table):
    """``ECONOMY`` replaced by ``economy``: the class named by the leading digit of a string value (geo_ablation.py:77-83),
    ``"Unknown"`` for an unmapped digit, a string without one, or a non-string."""
    names = []
    for v in table["ECONOMY"]:
        num = int(v[0]) if isinstance(v, str) and v[:1].isdigit() else 999
        names.append(ECONOMY_CLASSES.get(num, "Unknown"))
    out = {k: list(col) for k, col in table.items() if k != "ECONOMY"}
    out["economy"] = names
    return out


_INFINITIES = {"Infinity": math.inf, "-Infinity": -math.inf}
FLOAT_COLUMNS_MEMBER = "nirgan_float_columns"           # a foreign member of the FeatureCollection (RFC 7946, 6.1)


def _plain(v):
    return v.item() if isinstance(v, (np.floating, np.integer)) else v


def _json_value(v):
    """strict JSON: NaN as null, an infinity as the string "Infinity" / "-Infinity" (the bare tokens are not JSON)"""
    v = _plain(v)
    if isinstance(v, float) and not math.isfinite(v):
        return None if math.isnan(v) else ("Infinity" if v > 0 else "-Infinity")
    return v


def write_geojson(table, path):
    """The table as a FeatureCollection of Points at (x, y) with every column as a property, in strict JSON (no ``NaN`` /
    ``Infinity`` tokens: GDAL, geopandas and browsers read it).  Finite floats are written by ``repr`` and read back exactly; NaN is
    written as ``null``, an infinity (the PSNR of an exact prediction) as the string ``"Infinity"`` / ``"-Infinity"``; a row whose x
    or y is not finite gets a null geometry.  The columns that hold nothing but floats are named in the collection's foreign member
    ``nirgan_float_columns``, which is what lets ``read_geojson_table`` give them back exactly."""
    n = _rows(table)
    floats = [k for k, col in table.items() if n and all(isinstance(_plain(v), float) for v in col)]
    feats = []
    for i in range(n):
        x, y = _json_value(table["x"][i]), _json_value(table["y"][i])
        geom = {"type": "Point", "coordinates": [x, y]} if isinstance(x, (int, float)) and isinstance(y, (int, float)) else None
        feats.append({"type": "Feature", "properties": {k: _json_value(col[i]) for k, col in table.items()}, "geometry": geom})
    folder = os.path.dirname(os.path.abspath(path))
    os.makedirs(folder, exist_ok=True)
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", FLOAT_COLUMNS_MEMBER: floats, "features": feats}, f, allow_nan=False)


def read_geojson_table(path):
    """The features' properties as columns in file order.  A file of ``write_geojson`` reads back EXACTLY in its float columns
    (``nirgan_float_columns``): ``null`` is NaN and the infinity strings are infinities there, also in a column that is all NaN.
    Everywhere else values come as JSON has them: ``null`` is ``None``, and a NaN or an infinity that sat in a column of mixed
    types stays ``None`` / the string.  A file without the member (written by something else): ``null`` reads as NaN in a column
    that has a float elsewhere, and the infinity strings as infinities in such a column."""
    with open(path) as f:
        doc = json.load(f)
    feats = doc["features"]
    keys = []
    for ft in feats:
        for k in ft["properties"]:
            if k not in keys:
                keys.append(k)
    table = {k: [ft["properties"].get(k) for ft in feats] for k in keys}
    named = doc.get(FLOAT_COLUMNS_MEMBER)
    for k, col in table.items():
        if (k in named) if named is not None else any(isinstance(v, float) for v in col):
            table[k] = [float("nan") if v is None else _INFINITIES.get(v, v) if isinstance(v, str) else v for v in col]
    return table
