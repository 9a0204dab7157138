"""nirgan_point_regions / nirgan_raster_lookup on the MI355X: every point of every set bitwise against the float64 numpy statement for
slab_verts 8, 64 and the default, the independent oracle away from the edges (bodies, layers and point sets:
tests/geo_context_cases.py), the raw entry on addresses shifted by one element inside guarded buffers, bitwise repeatability, and a
1000-row table through append_info_to_df and plot_radar_comparison end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

import geo_context_cases as G
from nirgan_hip import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("n", G.UNIFORM_N)
@pytest.mark.parametrize("name", G.LAYERS)
def test_uniform_points_against_the_statement_and_the_independent_oracle(name, n):
    G.check_against_both(DEV, name, "uniform", n)


@pytest.mark.parametrize("name", G.LAYERS)
def test_integer_points_against_the_statement_and_the_independent_oracle(name):
    G.check_against_both(DEV, name, "integer")


@pytest.mark.parametrize("name", G.LAYERS)
def test_near_edge_points_against_the_statement(name):
    G.check_against_both(DEV, name, "near")


def test_region_boxes_are_the_vertex_extents():
    G.region_boxes_are_the_vertex_extents(DEV)


def test_special_points_and_empty_problems():
    G.special_points_and_empty_problems(DEV)


def test_raster_lookup_cases():
    G.raster_lookup_cases(DEV)


GUARD = 64


def _guarded(values, dtype, fill):
    """[guard | one element | values | guard] on the device: the payload starts one element past the guard band"""
    n = values.numel()
    buf = torch.full((2 * GUARD + 1 + n,), fill, dtype=dtype, device=DEV)
    buf[GUARD + 1:GUARD + 1 + n] = values.to(DEV).reshape(-1)
    return buf, buf.data_ptr() + (GUARD + 1) * buf.element_size()


def _guards_intact(buf, n, fill):
    host = buf.cpu()
    same = (lambda t: bool(torch.isnan(t).all())) if fill != fill else (lambda t: bool((t == fill).all()))
    return same(host[:GUARD + 1]) and same(host[GUARD + 1 + n:])


@pytest.mark.parametrize("name,slab", [("star", 64), ("grid", 8), ("enclave", 0)])
def test_raw_entries_on_shifted_addresses_inside_guarded_buffers_and_two_runs_are_bitwise_equal(name, slab):
    """points and the raster's points at an address shifted by one float64 (8-byte, not 16-byte aligned), outputs and the workspace
    shifted by one int32; nothing outside the payloads changes, the result is the statement's, and a second run equals the first"""
    be = L.backend()
    layer = G.make_layer(DEV, name)
    pts = np.concatenate([G.uniform_points(name, 1000), G.near_edge_points(name)[:1000]])
    want = np.concatenate([G.statement_of(name, "uniform", 1000), G.statement_of(name, "near")[:1000]])
    N, words = pts.shape[0], (layer.n_regions + 31) // 32
    nan = float("nan")
    pbuf, pptr = _guarded(torch.from_numpy(pts), torch.float64, nan)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    runs = []
    for _ in range(2):
        rbuf, rptr = _guarded(torch.full((N,), 12345, dtype=torch.int32), torch.int32, -77)
        wbuf, wptr = _guarded(torch.full((N * words,), -1, dtype=torch.int32), torch.int32, -77)       # a dirty workspace: the entry zeroes it
        d = layer._desc()
        d.points, d.n_points, d.slab_verts = pptr, N, slab
        d.ws, d.ws_bytes, d.region = wptr, N * words * 4, rptr
        assert be.nirgan_point_regions_ws_bytes(N, layer.n_regions) == N * words * 4
        L.check(be.nirgan_point_regions(C.byref(d), stream), "point_regions")
        torch.cuda.synchronize()
        assert _guards_intact(rbuf, N, -77) and _guards_intact(wbuf, N * words, -77) and _guards_intact(pbuf, 2 * N, nan)
        runs.append(rbuf[GUARD + 1:GUARD + 1 + N].cpu().numpy())
    assert (runs[0] == want).all() and (runs[0] == runs[1]).all()
    assert torch.equal(pbuf[GUARD + 1:GUARD + 1 + 2 * N].cpu(), torch.from_numpy(pts).reshape(-1))      # the input is untouched
    # the raster entry on the same shifted points
    from emu_geo_context import statement_raster
    lo, hi, ext = G.extent(name)
    transform = (float(lo[0]) - 0.1 * ext, 1.5 * ext / 5, float(hi[1]) + 0.1 * ext, -1.5 * ext / 7)
    raster = torch.from_numpy(G.RASTER_I16.copy()).to(DEV)
    vbuf, vptr = _guarded(torch.full((N,), 12345, dtype=torch.int32), torch.int32, -77)
    r = L.RasterLookupDesc()
    r.points, r.n_points, r.H, r.W, r.dtype, r.raster = pptr, N, 7, 5, L.RASTER_I16, raster.data_ptr()
    r.x0, r.dx, r.y0, r.dy = transform
    r.has_nodata, r.nodata, r.value = 1, -7, vptr
    L.check(be.nirgan_raster_lookup(C.byref(r), stream), "raster_lookup")
    torch.cuda.synchronize()
    assert _guards_intact(vbuf, N, -77) and _guards_intact(pbuf, 2 * N, nan)
    got = vbuf[GUARD + 1:GUARD + 1 + N].cpu().numpy()
    assert (got == statement_raster(pts, G.RASTER_I16, *transform, -7)).all() and (got != 0).any() and (got == 0).any()


def test_a_1000_row_table_through_the_join_and_the_radar_charts(tmp_path):
    G.join_end_to_end(DEV, 1000, tmp_path)
