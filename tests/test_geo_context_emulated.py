"""The geo-context join without a GPU: the host logic (validation_utils.geo_ablation / plot_val_spiders, the layers, the GeoJSON
reader and writer, spider_validation_callback with layers) on the numpy statement of nirgan_point_regions / nirgan_raster_lookup
(tests/emu_geo_context.py), the point sets' own conditions and the independent oracle, the argument checks and struct layout of the
real library, and the resource usage of the shipped kernels (hipcc cross-compiles).  Bodies shared with tests/test_gpu_geo_context.py."""
import ctypes as C
import csv
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import geo_context_cases as G
import tile_metric_cases as Tc
from emu_geo_context import EmuGeoContext, kernel_walk_regions
from nirgan_hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def emu():
    be = EmuGeoContext()
    L.set_backend(be)
    yield be
    L.set_backend(None)


@pytest.mark.parametrize("name", G.LAYERS)
def test_point_sets_hold_their_conditions(name):
    """on the CPU alone: the uniform and integer sets are well inside the 1 % cap of the independent oracle, the statement and the
    independent oracle agree on them, the near-edge set has its 2000 points and really sits within rounding of the edges"""
    _, _, ext = G.extent(name)
    for which, n in [("uniform", n) for n in G.UNIFORM_N] + [("integer", 0)]:
        pts = G.uniform_points(name, n) if which == "uniform" else G.integer_points(name)
        far = G.edge_distance(name, pts) > 1e-9 * ext
        assert (~far).sum() <= 0.001 * pts.shape[0], (which, n)
        assert (G.statement_of(name, which, n)[far] == G.independent_regions(name, pts[far])).all(), (which, n)
    ints = G.integer_points(name)
    vy = np.unique(G.layer_arrays(name)[0][:, 1])
    assert np.isin(ints[:, 1], vy).sum() >= 8                                  # rays through vertices and along horizontal edges
    near = G.near_edge_points(name)
    assert near.shape[0] >= 2000 and (G.edge_distance(name, near) < 1e-12 * ext).mean() > 0.95
    inside = G.statement_of(name, "near")
    assert (inside >= 0).any() and (inside < 0).any()


@pytest.mark.parametrize("name", G.LAYERS)
def test_port_of_the_kernel_walk_equals_the_statement(name):
    """the numpy port of point_regions_kernel's control flow (tests/emu_geo_context.kernel_walk_regions): slabs of 1, 3, 8, 64 and
    2048 vertices, with the vertex axis cut into as many chunks as the entry would (target 1024 blocks) and not at all (target 1),
    on the uniform, integer and near-edge sets -- equal to the statement on every point.  Needs no library."""
    verts, rs, rr, n_regions = G.layer_arrays(name)
    sets = [(G.uniform_points(name, 257), G.statement_of(name, "uniform", 257)), (G.integer_points(name), G.statement_of(name, "integer")),
            (G.near_edge_points(name), G.statement_of(name, "near"))]
    for pts, want in sets:
        for slab in ((1, 3, 8, 64, 2048) if verts.shape[0] < 500 else (8, 64, 2048)):   # the star: 1500 slabs of one vertex say nothing new
            for target in (1024, 1):
                got = kernel_walk_regions(pts, verts, rs, rr, n_regions, slab, target)
                wrong = np.flatnonzero(got != want)
                assert wrong.size == 0, (name, slab, target, pts[wrong[:5]], got[wrong[:5]], want[wrong[:5]])
    # an empty ring inside a slab, between two rings of one region and at the very end
    v = np.asarray(G._square(0, 0, 2, 2) + G._square(3, 0, 5, 2), dtype=np.float64)
    pts = np.asarray([[1.0, 1.0], [4.0, 1.0], [2.5, 1.0], [6.0, 1.0]])
    for slab in (1, 3, 8):
        assert kernel_walk_regions(pts, v, [0, 4, 4, 8, 8], [0, 0, 1, 1], 2, slab).tolist() == [0, 1, -1, -1]


@pytest.mark.parametrize("n", G.UNIFORM_N)
@pytest.mark.parametrize("name", G.LAYERS)
def test_uniform_points_against_the_statement_and_the_independent_oracle(emu, name, n):
    G.check_against_both("cpu", name, "uniform", n)
    assert emu.calls == ["region_boxes"] + ["point_regions"] * 3


@pytest.mark.parametrize("name", G.LAYERS)
def test_integer_points_against_the_statement_and_the_independent_oracle(emu, name):
    G.check_against_both("cpu", name, "integer")


@pytest.mark.parametrize("name", G.LAYERS)
def test_near_edge_points_against_the_statement(emu, name):
    G.check_against_both("cpu", name, "near")


def test_region_boxes_are_the_vertex_extents(emu):
    G.region_boxes_are_the_vertex_extents("cpu")


def test_special_points_and_empty_problems(emu):
    G.special_points_and_empty_problems("cpu")


def test_raster_lookup_cases(emu):
    G.raster_lookup_cases("cpu")
    assert set(emu.calls) == {"raster_lookup"}


def test_join_radar_charts_and_geojson_end_to_end(emu, tmp_path):
    G.join_end_to_end("cpu", 1000, tmp_path)
    assert emu.calls.count("point_regions") == 1 and emu.calls.count("raster_lookup") == 1      # ONE call each per table


# ---------------------------------------------------------------------------------------------------------------- host logic
WORLD = {"type": "FeatureCollection", "features": [
    {"type": "Feature", "properties": {"SOV_A3": "AAA", "CONTINENT": "Europe", "ECONOMY": "2. Developed region: nonG7"},
     "geometry": {"type": "Polygon", "coordinates": [[[0, 0], [6, 0], [6, 6], [0, 6], [0, 0]], [[2, 2], [4, 2], [4, 4], [2, 4], [2, 2]]]}},
    {"type": "Feature", "properties": {"SOV_A3": "BBB", "CONTINENT": "Asia", "ECONOMY": "7. Least developed region", "POP": 12},
     "geometry": {"type": "MultiPolygon", "coordinates": [[[[2, 2], [4, 2], [4, 4], [2, 4]]], [[[8, 0], [9, 0], [9, 1]]]]}},
    {"type": "Feature", "properties": {"SOV_A3": "LIN"}, "geometry": {"type": "LineString", "coordinates": [[0, 0], [1, 1]]}},
    {"type": "Feature", "properties": None, "geometry": None}]}


def test_geojson_layers_flatten_polygons_multipolygons_holes_and_properties(emu, tmp_path):
    from validation_utils import PolygonLayer, points_in_regions
    path = tmp_path / "world.geojson"
    path.write_text(json.dumps(WORLD))
    for src in (WORLD, str(path), WORLD["features"]):
        lay = PolygonLayer.from_geojson(src, device="cpu")
        assert (lay.n_verts, lay.n_rings, lay.n_regions) == (17, 4, 4)
        assert lay.ring_start.tolist() == [0, 5, 10, 14, 17] and lay.ring_region.tolist() == [0, 0, 1, 1]
        assert lay.verts.dtype == torch.float64 and lay.verts[5:10].tolist() == [[2, 2], [4, 2], [4, 4], [2, 4], [2, 2]]
        assert lay.verts[14:].tolist() == [[8, 0], [9, 0], [9, 1]]
        assert lay.properties == {"SOV_A3": ["AAA", "BBB", "LIN", None], "CONTINENT": ["Europe", "Asia", None, None],
                                  "ECONOMY": ["2. Developed region: nonG7", "7. Least developed region", None, None], "POP": [None, 12, None, None]}
        assert lay.region_box[:2].tolist() == [[0, 0, 6, 6], [2, 0, 9, 4]] and lay.region_box[2].tolist() == [math.inf, math.inf, -math.inf, -math.inf]
        assert points_in_regions([1.0, 3.0, 8.75, 7.0, 0.5], [1.0, 3.0, 0.5, 3.0, 0.5], lay).tolist() == [0, 1, 1, -1, 0]
    assert emu.calls.count("region_boxes") == 3                                 # built and uploaded ONCE per layer
    for bad in (dict(ring_start=[0, 3, 2, 4]), dict(ring_start=[0, 2, 3]), dict(ring_start=[1, 2, 3, 4]), dict(ring_region=[0, 2, 1]),
                dict(ring_region=[0, 1, 5]), dict(ring_region=[-1, 0, 1]), dict(verts=np.full((4, 2), np.nan))):
        args = dict(verts=np.zeros((4, 2)), ring_start=[0, 1, 2, 4], ring_region=[0, 1, 1], n_regions=2)
        args.update(bad)
        with pytest.raises(ValueError):
            PolygonLayer.from_arrays(device="cpu", **args)
    with pytest.raises(ValueError, match="property"):
        PolygonLayer.from_arrays(np.zeros((4, 2)), [0, 4], [0], 1, {"SOV_A3": ["a", "b"]}, device="cpu")
    L.set_backend(None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        PolygonLayer.from_geojson(WORLD, device="cpu")


def test_raster_layers_from_arrays_and_npz(emu, tmp_path):
    from validation_utils import RasterLayer, raster_lookup
    np.savez(tmp_path / "koppen.npz", array=G.RASTER_I16, transform=np.asarray(G.GENERAL), nodata=np.asarray(-7))
    np.savez(tmp_path / "plain.npz", array=G.RASTER_U8, transform=np.asarray(G.POW2_UP))
    a, b = RasterLayer.from_npz(tmp_path / "koppen.npz", device="cpu"), RasterLayer.from_npz(tmp_path / "plain.npz", device="cpu")
    assert a.array.dtype == torch.int16 and a.nodata == -7 and a.transform == G.GENERAL and b.array.dtype == torch.uint8 and b.nodata is None
    x0, dx, y0, dy = G.GENERAL
    assert raster_lookup([x0 + 3.5 * dx, x0 + 3.5 * dx], [y0 + 2.5 * dy, y0 + 1.5 * dy], a).tolist() == [0, int(G.RASTER_I16[1, 3])]   # nodata, a cell
    for bad in (np.zeros((3, 4)), np.zeros((2, 3, 4), dtype=np.uint8), np.zeros((0, 4), dtype=np.uint8), np.full((2, 2), 2 ** 40)):
        with pytest.raises(ValueError):
            RasterLayer(bad, G.GENERAL, device="cpu")
    with pytest.raises(ValueError):
        RasterLayer(G.RASTER_U8, (0.0, 1.0, 0.0), device="cpu")
    with pytest.raises(RuntimeError, match="raster_lookup"):
        raster_lookup([0.0], [0.0], RasterLayer(G.RASTER_U8, (0.0, 0.0, 0.0, 1.0), device="cpu"))
    with pytest.raises(ValueError, match="length"):
        raster_lookup([0.0, 1.0], [0.0], a)


def test_join_columns_left_join_koppen_letters_and_clean_economy(emu):
    from validation_utils import (PolygonLayer, RasterLayer, append_info_to_df, clean_economy, final_touch, get_climate_zones,
                                  get_countries)
    world = PolygonLayer.from_geojson(WORLD, device="cpu")
    table = {"id": [0, 1, 2, 3], "x": [1.0, 3.0, 7.0, 8.75], "y": [1.0, 3.0, 3.0, 0.5], "ssim": [0.5, 0.6, 0.7, 0.8], "extra": ["a", "b", "c", "d"]}
    c = get_countries(table, world)
    assert list(c) == ["id", "x", "y", "ssim", "extra", "Country", "Continent", "ECONOMY"] and "Country" not in table
    assert c["Country"] == ["AAA", "BBB", None, "BBB"] and c["Continent"] == ["Europe", "Asia", None, "Asia"]       # a left join: None outside
    assert c["ECONOMY"] == ["2. Developed region: nonG7", "7. Least developed region", None, "7. Least developed region"]
    with pytest.raises(KeyError, match="SOV_A3"):
        get_countries(table, PolygonLayer.from_arrays(np.zeros((3, 2)), [0, 3], [0], 1, device="cpu"))
    # ids under the four points: 3 ("Aw"), 8 ("csa": lower case in the legend), 0 (the id of no valid data), 77 (not in the legend)
    ids = np.zeros((4, 10), dtype=np.uint8)
    ids[3, 1], ids[1, 3], ids[3, 8] = 3, 8, 77
    koppen = RasterLayer(ids, (0.0, 1.0, 4.0, -1.0), device="cpu")
    for legend in ({3: "Aw", 8: "csa"}, {"id": [3, 8], "Code": ["Aw", "csa"]}):
        k = get_climate_zones(table, koppen, legend)
        assert k["Koppen_Class"] == ["A", "C", "U", "U"] and "Koppen_Class" not in table
    assert get_climate_zones(table, None, None)["Koppen_Class"] == ["U"] * 4
    joined = append_info_to_df(table, world, koppen, {3: "Aw", 8: "csa"})
    assert list(joined) == ["id", "x", "y", "ssim", "extra", "Country", "Continent", "ECONOMY", "Koppen_Class"]
    assert list(final_touch(dict(joined, more=[1, 2, 3, 4]))) == ["id", "x", "y", "ssim", "Country", "Continent", "ECONOMY", "Koppen_Class"]
    eco = clean_economy({"id": list(range(8)), "ECONOMY": ["1. Developed region: G7", "5. Emerging region: G20", "7. Least developed region",
                                                            "9. Unmapped", "", None, 3, float("nan")]})
    assert list(eco) == ["id", "economy"]
    assert eco["economy"] == ["Developed: G7", "Emerging: G20", "Least Developed", "Unknown", "Unknown", "Unknown", "Unknown", "Unknown"]


def test_legend_csv_of_the_reference_layout(emu, tmp_path):
    from validation_utils import RasterLayer, get_climate_zones
    path = tmp_path / "koppen_zones.csv"
    path.write_text('id,Code,Description,Color\n1,Af,"Tropical, rainforest","[0, 0, 255]"\n29,ET,"Polar, tundra","[178, 178, 178]"\n')
    koppen = RasterLayer(np.asarray([[1, 29]], dtype=np.int32), (0.0, 1.0, 0.0, 1.0), device="cpu")
    assert get_climate_zones({"x": [0.5, 1.5], "y": [0.5, 0.5]}, koppen, str(path))["Koppen_Class"] == ["A", "E"]


def test_geojson_round_trip_is_exact(emu, tmp_path):
    from validation_utils import read_geojson_table, write_geojson
    nan, inf = float("nan"), float("inf")
    table = {"id": [0, 1, 2], "x": [0.1, -179.99999999999997, 1e-300], "y": [1 / 3, 89.99999999999999, -5e-324],
             "psnr": [inf, 27.123456789012345, nan], "l1": [-inf, -0.0, 5e-324], "patch": [nan, nan, nan],
             "Country": ["AAA", None, "C C"], "n": [1, 2, 3], "mixed": [None, inf, "Infinity"]}
    path = tmp_path / "deep" / "t.geojson"
    write_geojson(table, str(path))
    back = read_geojson_table(str(path))
    assert list(back) == list(table)
    for k in ("id", "x", "y", "Country", "n"):
        assert back[k] == table[k] and [type(v) for v in back[k]] == [type(v) for v in table[k]], k
    for k in ("psnr", "l1", "patch"):                                           # NaN, both infinities, -0.0, an all-NaN column: bit for bit
        assert np.asarray(back[k], dtype=np.float64).tobytes() == np.asarray(table[k], dtype=np.float64).tobytes(), k
        assert all(type(v) is float for v in back[k]), k
    assert back["mixed"] == [None, "Infinity", "Infinity"]                      # not a float column: as JSON has it (documented)

    def strict(token):
        raise AssertionError(f"the file holds the bare token {token}")
    doc = json.load(open(path), parse_constant=strict)                          # strict JSON: no NaN / Infinity tokens
    assert doc["nirgan_float_columns"] == ["x", "y", "psnr", "l1", "patch"]
    assert [f["geometry"]["coordinates"] for f in doc["features"]] == [[x, y] for x, y in zip(table["x"], table["y"])]
    assert doc["features"][2]["properties"]["psnr"] is None and doc["features"][0]["properties"]["psnr"] == "Infinity"
    assert doc["features"][0]["properties"]["l1"] == "-Infinity"
    for x in (nan, inf, -inf):                                                  # no finite coordinates: a null geometry
        write_geojson({"x": [x], "y": [1.0]}, str(path))
        assert json.load(open(path), parse_constant=strict)["features"][0]["geometry"] is None
    # a file written by something else: no member -- null is NaN where the column has a float
    doc.pop("nirgan_float_columns")
    path.write_text(json.dumps(doc))
    other = read_geojson_table(str(path))
    assert other["psnr"][0] == inf and math.isnan(other["psnr"][2]) and other["patch"] == [None] * 3 and other["Country"] == table["Country"]
    with pytest.raises(ValueError, match="length"):
        write_geojson({"x": [1.0], "y": [1.0, 2.0]}, str(path))


def test_summarize_by_equals_pandas_groupby_mean():
    import pandas as pd
    from validation_utils import summarize_by
    rng = np.random.default_rng(3)
    n = 300
    table = {"Continent": [("Europe", "Africa", "Asia", None, "Oceania")[i] for i in rng.integers(0, 5, n)],
             "psnr": (20 + 10 * rng.random(n)).tolist(), "ssim": rng.random(n).tolist()}
    table["psnr"][7] = float("nan")
    table["Continent"][0], table["Continent"][1] = "Oceania", "Africa"          # an unsorted key
    lone = table["Continent"].index("Europe")
    table["Continent"] = ["Antarctica" if i == lone else c for i, c in enumerate(table["Continent"])]
    table["ssim"][lone] = float("nan")                                          # a category whose only value is NaN
    got = summarize_by(table, "Continent")
    want = pd.DataFrame(table).groupby("Continent").agg({"psnr": "mean", "ssim": "mean"}).reset_index()
    assert got["Continent"] == want["Continent"].tolist() == sorted(set(c for c in table["Continent"] if c is not None))
    for m in ("psnr", "ssim"):
        for a, b in zip(got[m], want[m].tolist()):
            assert (math.isnan(a) and math.isnan(b)) or a == b, (m, a, b)
    assert math.isnan(got["ssim"][got["Continent"].index("Antarctica")])
    assert list(summarize_by(table, "Continent", metrics=("ssim",))) == ["Continent", "ssim"]


def test_plot_radar_comparison_returns_an_image_and_writes_the_reference_file_name(tmp_path):
    from validation_utils import plot_radar_comparison
    import validation_utils.plot_val_spiders as P
    sc = {"Koppen_Class": ["A", "B", "U", "C", "A", "E"], "psnr": [30.0, 28.0, 1.0, 27.0, 32.0, 25.0], "ssim": [0.9, 0.8, 0.0, 0.7, 0.95, 0.6]}
    no = {"Koppen_Class": ["B", "A", "C", "D", "U"], "psnr": [26.0, 29.0, 25.0, 20.0, 2.0], "ssim": [0.7, 0.85, 0.6, 0.5, 0.1]}
    img = plot_radar_comparison(sc, no, "Koppen_Class", out_name="E 086", folder=str(tmp_path / "out"))
    assert os.listdir(tmp_path / "out") == ["metrics_radar_satclip_E_086_Koppen_Class.png"]
    a = np.asarray(img.convert("RGB")) if hasattr(img, "convert") else np.asarray(img)[..., :3]
    assert a.shape[0] >= 500 and a.shape[1] >= 1000 and len(np.unique(a.reshape(-1, 3), axis=0)) > 3     # 12 x 6 inches at 100 dpi, drawn on
    assert sc["Koppen_Class"][2] == "U" and len(no["psnr"]) == 5                                         # the tables are not modified
    import matplotlib.pyplot as plt
    assert plt.get_fignums() == []
    plot_radar_comparison(sc, no, "Koppen_Class", folder=str(tmp_path / "out"))
    assert "metrics_radar_satclip_Koppen_Class.png" in os.listdir(tmp_path / "out")
    with pytest.raises(ValueError, match="share no"):
        plot_radar_comparison({"economy": ["a"], "psnr": [1.0], "ssim": [1.0]}, {"economy": ["b"], "psnr": [1.0], "ssim": [1.0]}, "economy",
                              folder=str(tmp_path / "out"))
    assert P.KOPPEN_LABELS == {"A": "Tropical", "B": "Arid", "C": "Temperate", "D": "Continental", "E": "Polar", "U": "Undetermined"}
    src = open(P.__file__).read()
    assert "__main__" not in src and "listdir" not in src                      # no script body: importing it does nothing


def test_spider_validation_callback_writes_the_geojson_with_layers_and_only_the_csv_without(emu, tmp_path):
    from validation_utils import PolygonLayer, RasterLayer, read_geojson_table, spider_validation_callback
    rgb, nir, _ = Tc.inputs((3, 244, 244))
    ds = [{"rgb": rgb[i], "nir": nir[i], "coords": torch.tensor([(1.0, 1.0), (3.0, 3.0), (7.0, 3.0)][i])} for i in range(3)]
    plain = spider_validation_callback(Tc.ScaleModel().eval(), ds, satclip=True, folder=str(tmp_path / "plain"), epoch_no=4)
    assert os.listdir(tmp_path / "plain") == ["validation_metrics.csv"] and "Country" not in plain
    assert "point_regions" not in emu.calls and "raster_lookup" not in emu.calls
    world = PolygonLayer.from_geojson(WORLD, device="cpu")
    koppen = RasterLayer(np.full((8, 8), 29, dtype=np.uint8), (0.0, 1.0, 8.0, -1.0), device="cpu")
    joined = spider_validation_callback(Tc.ScaleModel().eval(), ds, satclip=True, folder=str(tmp_path / "spiders"), epoch_no=4,
                                        world=world, koppen=koppen, legend={29: "ET"})
    assert sorted(os.listdir(tmp_path / "spiders")) == ["validation_metrics.csv", "validation_metrics_ablation_satclip_True_e4.geojson"]
    assert list(csv.reader(open(tmp_path / "spiders" / "validation_metrics.csv"))) == list(csv.reader(open(tmp_path / "plain" / "validation_metrics.csv")))
    assert joined["Country"] == ["AAA", "BBB", None] and joined["Koppen_Class"] == ["E", "E", "E"]
    assert joined["economy"] == ["Developed: Non G7", "Least Developed", "Unknown"] and "ECONOMY" not in joined
    assert all(joined[k] == plain[k] for k in plain)
    back = read_geojson_table(str(tmp_path / "spiders" / "validation_metrics_ablation_satclip_True_e4.geojson"))
    assert back == joined


# ---------------------------------------------------------------------------------------------------------------- the real library
def _regions_desc(keep):
    """a valid descriptor over host memory (never launched: every call below fails its checks first, or has nothing to do)"""
    verts, rs, rr, _ = G.layer_arrays("enclave")
    bufs = dict(pts=np.zeros((4, 2)), verts=verts.copy(), rs=rs.copy(), rr=rr.copy(), box=np.zeros((2, 4)), ws=np.zeros(4, np.int32),
                region=np.zeros(4, np.int32))
    keep.append(bufs)
    d = L.PointRegionsDesc()
    d.points, d.n_points, d.n_verts, d.verts = bufs["pts"].ctypes.data, 4, 12, bufs["verts"].ctypes.data
    d.ring_start, d.ring_region, d.n_rings, d.n_regions = bufs["rs"].ctypes.data, bufs["rr"].ctypes.data, 3, 2
    d.region_box, d.ring_start_host, d.ring_region_host = bufs["box"].ctypes.data, bufs["rs"].ctypes.data, bufs["rr"].ctypes.data
    d.slab_verts, d.ws, d.ws_bytes, d.region = 0, bufs["ws"].ctypes.data, 16, bufs["region"].ctypes.data
    return d, bufs


REGION_ARGUMENTS = [("points", None, b"null"), ("verts", None, b"null"), ("ring_start", None, b"null"), ("ring_region", None, b"null"),
                    ("region_box", None, b"null"), ("ws", None, b"null"), ("region", None, b"null"), ("n_points", -1, b"negative"),
                    ("n_verts", -1, b"negative"), ("n_rings", -1, b"negative"), ("n_regions", -1, b"negative"), ("slab_verts", -1, b"slab_verts"),
                    ("slab_verts", 2049, b"slab_verts"), ("ws_bytes", 15, b"workspace"), ("n_verts", 11, b"n_verts"), ("n_regions", 1, b"ring_region")]


@pytest.mark.parametrize("which", ["library", "emulator"])
def test_bad_arguments_are_rejected_before_any_launch(which):
    """the real library without a GPU (an argument error returns before any launch; so does an empty problem), and the emulator's
    restatement of the same checks"""
    be = L.backend() if which == "library" else EmuGeoContext()
    assert (which == "library") == (not getattr(be, "is_emulator", True) and not L.is_emulated())
    keep = []
    d, bufs = _regions_desc(keep)
    for field, value, word in REGION_ARGUMENTS:
        old = getattr(d, field)
        setattr(d, field, value)
        assert be.nirgan_point_regions(C.byref(d), None) == -1, field
        msg = be.nirgan_last_error()
        assert b"point_regions" in msg and word in msg, (field, msg)
        setattr(d, field, old)
    for name, at, value, word in (("rr", 0, 1, b"ring_region"), ("rr", 0, -1, b"ring_region"), ("rs", 3, 11, b"ring_start"),
                                  ("rs", 1, 9, b"ring_start"), ("rs", 0, 1, b"ring_start")):
        old = bufs[name][at]
        bufs[name][at] = value
        for entry, who in ((be.nirgan_point_regions, b"point_regions"), (be.nirgan_region_boxes, b"region_boxes")):
            assert entry(C.byref(d), None) == -1, (name, at)
            assert who in be.nirgan_last_error() and word in be.nirgan_last_error(), (name, at, be.nirgan_last_error())
        bufs[name][at] = old
    d.region_box = None
    assert be.nirgan_region_boxes(C.byref(d), None) == -1 and b"region_boxes" in be.nirgan_last_error() and b"null" in be.nirgan_last_error()
    d.region_box = bufs["box"].ctypes.data
    for field in ("n_points", "n_regions"):                                     # nothing to do: success, nothing launched, nothing written
        d2, b2 = _regions_desc(keep)
        setattr(d2, field, 0)
        if field == "n_regions":
            b2["rr"][:] = 0
            d2.ring_region_host = None
        b2["region"][:] = 7
        assert be.nirgan_point_regions(C.byref(d2), None) == 0 and b2["region"].tolist() == [7] * 4
    r = L.RasterLookupDesc()
    raster = np.zeros((7, 5), dtype=np.uint8)
    r.points, r.n_points, r.H, r.W, r.dtype, r.raster = bufs["pts"].ctypes.data, 4, 7, 5, L.RASTER_U8, raster.ctypes.data
    r.x0, r.dx, r.y0, r.dy, r.value = 0.0, 1.0, 0.0, -1.0, bufs["region"].ctypes.data
    for field, value, word in (("points", None, b"null"), ("raster", None, b"null"), ("value", None, b"null"), ("n_points", -1, b"negative"),
                               ("H", 0, b"empty"), ("W", -3, b"empty"), ("dtype", 3, b"dtype"), ("dx", 0.0, b"transform"), ("dy", 0.0, b"transform"),
                               ("x0", math.nan, b"transform"), ("dy", math.nan, b"transform")):
        old = getattr(r, field)
        setattr(r, field, value)
        assert be.nirgan_raster_lookup(C.byref(r), None) == -1, field
        assert b"raster_lookup" in be.nirgan_last_error() and word in be.nirgan_last_error(), (field, be.nirgan_last_error())
        setattr(r, field, old)
    r.n_points = 0
    assert be.nirgan_raster_lookup(C.byref(r), None) == 0


def test_workspace_size_is_the_documented_formula():
    be, emu = L.backend(), EmuGeoContext()
    assert not L.is_emulated()
    for n, g in [(1, 1), (1000, 32), (1000, 33), (2000, 250), (100000, 72), (0, 5), (5, 0), (-1, 5), (2 ** 31 - 1, 2 ** 31 - 1)]:
        want = n * ((g + 31) // 32) * 4 if n > 0 and g > 0 else 0
        assert be.nirgan_point_regions_ws_bytes(n, g) == emu.nirgan_point_regions_ws_bytes(n, g) == want, (n, g)


def test_struct_layout_matches_the_header(tmp_path):
    pairs = [("nirgan_point_regions_desc", L.PointRegionsDesc), ("nirgan_raster_lookup_desc", L.RasterLookupDesc)]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "nirgan_hip.h"\nint main(void){\n'
    src += 'printf("%d %d %d %d\\n", NIRGAN_GEO_SLAB_MAX, NIRGAN_RASTER_U8, NIRGAN_RASTER_I16, NIRGAN_RASTER_I32);\n'
    for cname, ct in pairs:
        src += f'printf("%zu", sizeof({cname}));\n'
        for name, _ in ct._fields_:
            src += f'printf(" %zu", offsetof({cname}, {name}));\n'
        src += 'printf("\\n");\n'
    src += "return 0;}\n"
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert [int(x) for x in lines[0].split()] == [L.GEO_SLAB_MAX, L.RASTER_U8, L.RASTER_I16, L.RASTER_I32]
    for (cname, ct), line in zip(pairs, lines[1:]):
        nums = [int(x) for x in line.split()]
        assert nums[0] == C.sizeof(ct), cname
        assert nums[1:] == [getattr(ct, name).offset for name, _ in ct._fields_], cname
        assert nums[-1] == getattr(ct, ct._fields_[-1][0]).offset                # the last field, as tests/test_capi_exports.py checks its structs


def test_shipped_kernels_use_no_scratch_spill_nothing_fit_the_lds_and_do_not_fuse_the_crossing(tmp_path):
    """csrc/geocontext.hip compiled for gfx950; only the kernel descriptors, the metadata and the instruction names are read: no
    private segment, no spilled register, the slab within the CU's 160 KB of LDS (four blocks per CU), and no fused float64
    multiply-add in the kernel that evaluates the crossing statement besides the box margin's (one, outside the edge loop)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = tmp_path / "geocontext.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-result", "--cuda-device-only", "-S",
                    os.path.join(ROOT, "nir-gan_amd", "csrc", "geocontext.hip"), "-o", str(asm)], check=True, timeout=600)
    text = asm.read_text()
    names = re.findall(r"\.amdhsa_kernel\s+(\S+)", text)
    assert len(names) == 4 and all(any(k in n for n in names) for k in ("point_regions_kernel", "point_regions_pick_kernel",
                                                                         "region_boxes_kernel", "raster_lookup_kernel"))
    for name in names:
        start = text.index(".amdhsa_kernel " + name)
        desc = text[start:text.index(".end_amdhsa_kernel", start)]
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", desc).group(1))
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", desc).group(1))
        md = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?.*\.vgpr_spill_count:\s+(\d+)", text)
        print(f"{name}: LDS {lds} B, private segment {scratch} B, vgpr_spill_count {md and md.group(1)}")
        assert scratch == 0 and md and int(md.group(1)) == 0
        if "point_regions_kernel" in name:
            assert lds == (L.GEO_SLAB_MAX + 1) * 16 and 4 * lds <= 160 * 1024
            body = text[text.index(name + ":"):start]
            fused = re.findall(r"\bv_(?:fma|fmac)_f64\S*", body)
            print(f"{name}: fused float64 multiply-adds {fused}, v_mul_f64 {len(re.findall(r'v_mul_f64', body))}")
            assert len(fused) <= 1 and len(re.findall(r"v_mul_f64", body)) >= 2
