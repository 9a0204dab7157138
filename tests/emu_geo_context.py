"""numpy statement of the geo-context entries of include/nirgan_hip.h (nirgan_region_boxes / nirgan_point_regions / _ws_bytes and
nirgan_raster_lookup) -- TEST INFRASTRUCTURE ONLY, installed with ``nirgan_hip.lib.set_backend`` like tests/emu_class_metrics.py,
which it extends so that one emulator serves a whole validation run.

``statement_regions`` is the header's crossing statement word for word in float64 numpy (numpy rounds every operation on its own and
never fuses a multiply-add): no boxes, no slabs, one ring at a time against all points.  ``statement_raster`` is the header's cell
rule.  Both are the oracle the device is held to bitwise, on the emulator and on the MI355X (tests/geo_context_cases.py).  Contract
enforced: the argument checks come before any work and name the entry, ``region`` / ``value`` are overwritten, the workspace is
zeroed and must be large enough, n_regions == 0 leaves ``region`` untouched.
"""
import ctypes as C

import numpy as np

from emu_backend import arr, obj
from emu_class_metrics import EmuClassMetrics

SLAB_MAX = 2048
RASTER_CTYPES = {0: (C.c_uint8, np.uint8), 1: (C.c_int16, np.int16), 2: (C.c_int32, np.int32)}


def statement_regions(points, verts, ring_start, ring_region, n_regions, chunk=4096):
    """region [N] int64: the lowest region whose rings are crossed an odd number of times in total, or -1"""
    points, verts = np.asarray(points, dtype=np.float64).reshape(-1, 2), np.asarray(verts, dtype=np.float64).reshape(-1, 2)
    out = np.full(points.shape[0], -1, dtype=np.int64)
    for at in range(0, points.shape[0], chunk):
        px, py = points[at:at + chunk, 0][:, None], points[at:at + chunk, 1][:, None]
        odd = np.zeros((px.shape[0], max(int(n_regions), 1)), dtype=bool)
        for r in range(len(ring_region)):
            v = verts[ring_start[r]:ring_start[r + 1]]
            if v.shape[0] == 0:
                continue
            x0, y0 = v[:, 0][None, :], v[:, 1][None, :]
            x1, y1 = np.roll(x0, -1, axis=1), np.roll(y0, -1, axis=1)            # the closing edge: last vertex -> first
            with np.errstate(invalid="ignore", over="ignore"):
                straddles = (y0 > py) != (y1 > py)
                d = (x1 - x0) * (py - y0) - (px - x0) * (y1 - y0)
                crossing = straddles & np.where(y1 > y0, d > 0, d < 0)
            odd[:, ring_region[r]] ^= (crossing.sum(axis=1) & 1).astype(bool)
        out[at:at + chunk] = np.where(odd.any(axis=1), odd.argmax(axis=1), -1)
    return out


def _crossings(v0, v1, px, py):
    """[N] parity of the crossings of the edges v0[k] -> v1[k] by every point: the statement, edge by edge"""
    x0, y0, x1, y1 = v0[None, :, 0], v0[None, :, 1], v1[None, :, 0], v1[None, :, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        straddles = (y0 > py[:, None]) != (y1 > py[:, None])
        d = (x1 - x0) * (py[:, None] - y0) - (px[:, None] - x0) * (y1 - y0)
        return ((straddles & np.where(y1 > y0, d > 0, d < 0)).sum(axis=1) & 1).astype(bool)


def kernel_walk_regions(points, verts, ring_start, ring_region, n_regions, slab, target_blocks=1024):
    """A numpy PORT of the control flow of csrc/geocontext.hip (point_regions_kernel + the pick launch + region_boxes), kept line by
    line with it: the vertex-axis cut of the entry, the binary search for a chunk's first ring, per slab the staged vertices
    [a, a + slab] (``sv``: reading a vertex the kernel did not stage raises), the ring walk with its skips, the closing edge taken by
    the slab that holds the ring's last vertex, the box test with its left margin, the parity flush as XOR into the uint32 bitset,
    the lowest set bit.  Points are the vector axis (a lane's ``inbox`` masks its flush; the wave ballot only saves work).  It is the
    CPU check of everything the statement does not have -- slabs, the ring walk, the box -- against ``statement_regions``."""
    points, verts = np.asarray(points, dtype=np.float64).reshape(-1, 2), np.asarray(verts, dtype=np.float64).reshape(-1, 2)
    N, V, R, G = points.shape[0], verts.shape[0], len(ring_region), int(n_regions)
    out = np.full(N, -1, dtype=np.int64)
    if N == 0 or G == 0:
        return out
    px, py = points[:, 0], points[:, 1]
    words = (G + 31) // 32
    ws = np.zeros((N, words), dtype=np.uint32)
    box = np.empty((G, 4))
    box[:] = (np.inf, np.inf, -np.inf, -np.inf)
    for r in range(R):
        v = verts[ring_start[r]:ring_start[r + 1]]
        if v.shape[0]:
            box[ring_region[r], :2] = np.minimum(box[ring_region[r], :2], v.min(axis=0))
            box[ring_region[r], 2:] = np.maximum(box[ring_region[r], 2:], v.max(axis=0))
    nslab, npc = -(-V // slab), -(-N // 256)
    if nslab > 0 and R > 0:
        nvc = min(-(-target_blocks // npc), nslab)
        slabs_per_chunk = -(-nslab // nvc)
        nvc = -(-nslab // slabs_per_chunk)
        for vc in range(nvc):
            s_first, s_last = vc * slabs_per_chunk, min(vc * slabs_per_chunk + slabs_per_chunk, nslab)
            a0 = s_first * slab
            lo, hi = 0, R
            while lo < hi:
                mid = (lo + hi) >> 1
                if ring_start[mid + 1] > a0:
                    hi = mid
                else:
                    lo = mid + 1
            r, cur = lo, -1
            par, inbox = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)

            def flush():
                if cur >= 0:
                    ws[par & inbox, cur >> 5] ^= np.uint32(1 << (cur & 31))
            for s in range(s_first, s_last):
                a, b = s * slab, min(s * slab + slab, V)
                staged = min(a + slab + 1, V) - a                              # sv[j] for j <= slab and a + j < V
                sv = verts[a:a + staged]
                while r < R:
                    r_lo, r_hi = int(ring_start[r]), int(ring_start[r + 1])
                    if r_lo >= b:
                        break
                    if r_hi <= r_lo or r_hi <= a or r_lo < 0 or r_hi > V:
                        r += 1
                        continue
                    g = int(ring_region[r])
                    if g != cur:
                        flush()
                        par[:] = False
                        cur, inbox = g, np.zeros(N, dtype=bool)
                        if 0 <= g < G:
                            xmin, ymin, xmax, ymax = box[g]
                            with np.errstate(invalid="ignore"):
                                xlo = xmin - ((xmax - xmin) + abs(xmin)) * 2.0 ** -40
                                inbox = (py >= ymin) & (py <= ymax) & (px <= xmax) & (px >= xlo)
                    if inbox.any():
                        lo_e, hi_e = max(a, r_lo), min(b, r_hi)
                        last = min(hi_e, r_hi - 1)
                        assert 0 <= lo_e - a and last - a < staged, "a vertex the kernel did not stage"
                        if last > lo_e:
                            par ^= _crossings(sv[lo_e - a:last - a], sv[lo_e + 1 - a:last + 1 - a], px, py)
                        if hi_e == r_hi:                                        # the closing edge, from vertex r_hi - 1
                            par ^= _crossings(sv[last - a:last - a + 1], verts[r_lo:r_lo + 1], px, py)
                    if r_hi <= b:
                        r += 1
                    else:
                        break
            flush()
    hit = ws != 0
    first = hit.argmax(axis=1)
    bits = ws[np.arange(N), first].astype(np.int64)
    low = np.log2((bits & -bits).clip(min=1)).astype(np.int64)
    out[hit.any(axis=1)] = (32 * first + low)[hit.any(axis=1)]
    return out


def statement_raster(points, raster, x0, dx, y0, dy, nodata=None):
    """value [N] int64: the cell that contains the point; 0 outside, for NaN and on nodata"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    H, W = raster.shape
    with np.errstate(invalid="ignore", over="ignore"):
        col = np.floor((points[:, 0] - np.float64(x0)) / np.float64(dx))
        row = np.floor((points[:, 1] - np.float64(y0)) / np.float64(dy))
        ok = (col >= 0) & (col < W) & (row >= 0) & (row < H)
    out = np.zeros(points.shape[0], dtype=np.int64)
    out[ok] = raster[row[ok].astype(np.int64), col[ok].astype(np.int64)]
    if nodata is not None:
        out[out == nodata] = 0
    return out


def typed_at(ptr, n, ctype):
    if hasattr(ptr, "value"):
        ptr = ptr.value
    return np.ctypeslib.as_array((ctype * int(n)).from_address(int(ptr)))


class EmuGeoContext(EmuClassMetrics):
    def nirgan_point_regions_ws_bytes(self, n_points, n_regions):
        if n_points <= 0 or n_regions <= 0:
            return 0
        return n_points * ((n_regions + 31) // 32) * 4

    def _layer_error(self, d, who):
        if min(d.n_points, d.n_verts, d.n_rings, d.n_regions) < 0:
            return f"{who}: negative count"
        if d.slab_verts < 0 or d.slab_verts > SLAB_MAX:
            return f"{who}: slab_verts must lie in 0..{SLAB_MAX}"
        if d.ring_region_host:
            rr = arr(d.ring_region_host, d.n_rings, np.int32) if d.n_rings else np.zeros(0, np.int32)
            if rr.size and (rr.min() < 0 or rr.max() >= d.n_regions):
                return f"{who}: ring_region outside 0..n_regions-1"
            if (np.diff(rr) < 0).any():
                return f"{who}: ring_region decreases"
        if d.ring_start_host:
            rs = arr(d.ring_start_host, d.n_rings + 1, np.int32)
            if rs[0] != 0:
                return f"{who}: ring_start[0] is not 0"
            if (np.diff(rs) < 0).any():
                return f"{who}: ring_start decreases"
            if rs[-1] != d.n_verts:
                return f"{who}: ring_start[n_rings] is not n_verts"
        return None

    @staticmethod
    def _layer(d):
        verts = arr(d.verts, 2 * d.n_verts, np.float64).reshape(-1, 2) if d.n_verts else np.zeros((0, 2))
        rs = arr(d.ring_start, d.n_rings + 1, np.int32)
        rr = arr(d.ring_region, d.n_rings, np.int32) if d.n_rings else np.zeros(0, np.int32)
        return verts, rs, rr

    def nirgan_region_boxes(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("region_boxes")
        err = self._layer_error(d, "region_boxes")
        if err:
            return self._fail(err)
        if d.n_regions == 0:
            return 0
        if not (d.region_box and d.ring_start and (d.n_rings == 0 or d.ring_region) and (d.n_verts == 0 or d.verts)):
            return self._fail("region_boxes: null pointer")
        verts, rs, rr = self._layer(d)
        box = arr(d.region_box, 4 * d.n_regions, np.float64).reshape(-1, 4)
        box[:] = (np.inf, np.inf, -np.inf, -np.inf)
        for r in range(d.n_rings):
            v = verts[rs[r]:rs[r + 1]]
            if v.shape[0]:
                g = rr[r]
                box[g, :2] = np.minimum(box[g, :2], v.min(axis=0))
                box[g, 2:] = np.maximum(box[g, 2:], v.max(axis=0))
        return 0

    def nirgan_point_regions(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("point_regions")
        err = self._layer_error(d, "point_regions")
        if err:
            return self._fail(err)
        if d.n_points == 0 or d.n_regions == 0:
            return 0
        if not (d.points and d.region and d.ws and d.region_box and d.ring_start and (d.n_rings == 0 or d.ring_region)
                and (d.n_verts == 0 or d.verts)):
            return self._fail("point_regions: null pointer")
        need = self.nirgan_point_regions_ws_bytes(d.n_points, d.n_regions)
        if d.ws_bytes < need:
            return self._fail("point_regions: workspace too small")
        verts, rs, rr = self._layer(d)
        pts = arr(d.points, 2 * d.n_points, np.float64).reshape(-1, 2)
        got = statement_regions(pts, verts, rs, rr, d.n_regions)
        ws = arr(d.ws, need // 4, np.int32).reshape(d.n_points, -1)                   # the bitset the device leaves: the lowest odd region's bit
        ws[:] = 0                                                                     # (the device sets every odd region's; only the lowest is read)
        hit = got >= 0
        ws[hit, got[hit] // 32] = (np.uint32(1) << (got[hit] % 32).astype(np.uint32)).view(np.int32)
        arr(d.region, d.n_points, np.int32)[:] = got
        return 0

    def nirgan_raster_lookup(self, ref, stream=None):
        d = obj(ref)
        self.calls.append("raster_lookup")
        if d.n_points < 0:
            return self._fail("raster_lookup: negative count")
        if d.H <= 0 or d.W <= 0:
            return self._fail("raster_lookup: empty raster")
        if d.dtype not in RASTER_CTYPES:
            return self._fail("raster_lookup: unknown dtype")
        if d.dx == 0 or d.dy == 0 or any(v != v for v in (d.x0, d.dx, d.y0, d.dy)):
            return self._fail("raster_lookup: transform needs non-zero steps and no NaN")
        if d.n_points == 0:
            return 0
        if not (d.points and d.raster and d.value):
            return self._fail("raster_lookup: null pointer")
        ct, _ = RASTER_CTYPES[d.dtype]
        raster = typed_at(d.raster, d.H * d.W, ct).reshape(d.H, d.W)
        pts = arr(d.points, 2 * d.n_points, np.float64).reshape(-1, 2)
        arr(d.value, d.n_points, np.int32)[:] = statement_raster(pts, raster, d.x0, d.dx, d.y0, d.dy, d.nodata if d.has_nodata else None)
        return 0
