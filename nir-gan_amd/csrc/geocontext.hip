// The geo-context join of the validation table: nirgan_region_boxes / nirgan_point_regions (points against a polygon
// layer, even-odd rule) and nirgan_raster_lookup (the cell of a north-up raster that holds each point).
//
// The crossing predicate of an edge (x0,y0) -> (x1,y1) and a point (px,py) is the header's, every operation an individually rounded
// float64 operation (floating-point contraction is OFF in gc_crossing: a fused d changes sign for points a few ulp from an edge):
//     straddles = (y0 > py) != (y1 > py);  d = (x1 - x0) * (py - y0) - (px - x0) * (y1 - y0);  crossing = straddles && (y1 > y0 ? d > 0 : d < 0)
// It depends on the edge and the point alone, so the parity of a region's crossings is the XOR of the parities of ANY partition of
// its edges: the launch below cuts the edge axis at slab boundaries and combines with integer XOR, which is associative and
// commutative -- the result cannot depend on the cut, on the slab size or on the order blocks arrive in.  No float atomics.
//
// Launch 1, point_regions_kernel: block = (vertex chunk, 256 points), a thread owns one point of every chunk it is given.  The vertex
// chunk is a run of whole slabs of `slab` vertices; per slab the vertices [a, a + slab] go to LDS as double2 and every edge read in
// the loop is ONE 16-byte broadcast (the edge's start is carried in registers).  The rings that meet the slab are walked in order
// (ring_start / ring_region are uniform reads); at a change of region the lane's parity is flushed -- one atomicXor of the region's
// bit in the uint32 bitset ws[point][word], only where the parity is odd -- and the new region's box is tested: a ring is skipped by
// the whole wave when no lane's point lies in the box (a ballot).  A ring's closing edge (last vertex -> first) is taken by the slab
// that holds the last vertex; the first vertex is a uniform global read, it may lie slabs away.
// The box test is exact on three sides and has a margin on the fourth: above ymax / below ymin no edge straddles, right of xmax the
// predicate is false for every straddling edge in floating point too (monotone rounding), but left of xmin it is true only where the
// two rounded products differ -- so the left side is skipped only beyond xmin - 2^-40 (width + |xmin|), where they provably do.
// Launch 2, point_regions_pick_kernel: the lowest set bit of a point's words, or -1.
//
// nirgan_region_boxes: one block per region; its rings are consecutive (ring_region is non-decreasing), so are its vertices; min / max
// through wave shuffles and LDS.  A region without vertices gets the empty box (+inf, +inf, -inf, -inf).
#include <math.h>
#include "common.h"

namespace {

constexpr int GC_THREADS = 256;
constexpr int GC_SLAB_MAX = NIRGAN_GEO_SLAB_MAX;         // vertices per slab at most: (2048 + 1) * 16 B of LDS
constexpr int GC_SLAB_DEFAULT = 2048;
constexpr int GC_TARGET_BLOCKS = 1024;                   // 256 CUs x 4 blocks: below it the grid is also cut along the vertex axis

struct RegionsP {
    const double* points; const double* verts;                // [n][2], 8-byte aligned is enough: read as two doubles
    const int32_t* ring_start; const int32_t* ring_region;
    const double* box;
    uint32_t* ws; int32_t* region;
    int N, V, R, G, words;
    int slab, nslab, slabs_per_chunk, nvc;               // nvc vertex chunks of slabs_per_chunk slabs
};

__device__ __forceinline__ int gc_crossing(double x0, double y0, double x1, double y1, double px, double py) {
#pragma clang fp contract(off)
    const bool straddles = (y0 > py) != (y1 > py);
    const double a = (x1 - x0) * (py - y0);
    const double b = (px - x0) * (y1 - y0);
    const double d = a - b;
    return (straddles && (y1 > y0 ? d > 0.0 : d < 0.0)) ? 1 : 0;
}

__global__ __launch_bounds__(GC_THREADS) void point_regions_kernel(const RegionsP p) {
    __shared__ double2 sv[GC_SLAB_MAX + 1];
    const int tid = threadIdx.x;
    const int vc = blockIdx.x % p.nvc;
    const int64_t pt = int64_t(blockIdx.x / p.nvc) * GC_THREADS + tid;
    const bool live = pt < p.N;
    double px = 0.0, py = 0.0;
    if (live) { px = p.points[2 * pt]; py = p.points[2 * pt + 1]; }
    const int s_first = vc * p.slabs_per_chunk;
    const int s_last = min(s_first + p.slabs_per_chunk, p.nslab);
    // the first ring that reaches past this chunk's first edge: the lowest r with ring_start[r + 1] > a0
    const int a0 = s_first * p.slab;
    int r = 0;
    {
        int lo = 0, hi = p.R;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (p.ring_start[mid + 1] > a0) hi = mid; else lo = mid + 1;
        }
        r = lo;
    }
    int cur = -1, par = 0;
    bool inbox = false;
    for (int s = s_first; s < s_last; ++s) {
        const int a = s * p.slab, b = min(a + p.slab, p.V);
        __syncthreads();                                                        // the previous slab has been read
        for (int j = tid; j <= p.slab; j += GC_THREADS)
            if (a + j < p.V) sv[j] = make_double2(p.verts[2 * int64_t(a + j)], p.verts[2 * int64_t(a + j) + 1]);
        __syncthreads();
        while (r < p.R) {
            const int r_lo = p.ring_start[r], r_hi = p.ring_start[r + 1];
            if (r_lo >= b) break;
            if (r_hi <= r_lo || r_hi <= a || r_lo < 0 || r_hi > p.V) { ++r; continue; }   // an empty ring, one behind, or a malformed entry: nothing is read
            const int g = p.ring_region[r];
            if (g != cur) {
                if (par && inbox) atomicXor(p.ws + pt * p.words + (cur >> 5), 1u << (cur & 31));
                par = 0; cur = g; inbox = false;
                if (g >= 0 && g < p.G) {
                    const double xmin = p.box[4 * g], ymin = p.box[4 * g + 1], xmax = p.box[4 * g + 2], ymax = p.box[4 * g + 3];
                    const double xlo = xmin - ((xmax - xmin) + fabs(xmin)) * 0x1p-40;
                    inbox = live && py >= ymin && py <= ymax && px <= xmax && px >= xlo;
                }
            }
            if (__ballot(inbox) != 0ull) {
                const int lo = max(a, r_lo), hi = min(b, r_hi);
                const int last = min(hi, r_hi - 1);                             // edges lo .. last-1 run to the next vertex
                double2 v0 = sv[lo - a];
                for (int e = lo; e < last; ++e) {
                    const double2 v1 = sv[e + 1 - a];
                    par ^= gc_crossing(v0.x, v0.y, v1.x, v1.y, px, py);
                    v0 = v1;
                }
                if (hi == r_hi) {                                               // the closing edge: v0 is vertex r_hi - 1 here
                    const double2 v1 = make_double2(p.verts[2 * int64_t(r_lo)], p.verts[2 * int64_t(r_lo) + 1]);
                    par ^= gc_crossing(v0.x, v0.y, v1.x, v1.y, px, py);
                }
            }
            if (r_hi <= b) ++r; else break;                                     // the ring goes on in the next slab
        }
    }
    if (par && inbox) atomicXor(p.ws + pt * p.words + (cur >> 5), 1u << (cur & 31));
}

__global__ __launch_bounds__(GC_THREADS) void point_regions_pick_kernel(const uint32_t* __restrict__ ws, int N, int words, int32_t* __restrict__ region) {
    const int64_t pt = int64_t(blockIdx.x) * GC_THREADS + threadIdx.x;
    if (pt >= N) return;
    int out = -1;
    for (int w = 0; w < words; ++w) {
        const uint32_t bits = ws[pt * words + w];
        if (bits) { out = 32 * w + __ffs(int(bits)) - 1; break; }
    }
    region[pt] = out;
}

__global__ __launch_bounds__(GC_THREADS) void region_boxes_kernel(const double* __restrict__ verts, const int32_t* __restrict__ ring_start,
                                                                   const int32_t* __restrict__ ring_region, int V, int R, double* __restrict__ box) {
    __shared__ double red[GC_THREADS / 64][4];
    const int g = blockIdx.x, tid = threadIdx.x;
    // the rings of region g: [first ring with region >= g, first ring with region > g)
    int lo = 0, hi = R;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (ring_region[mid] >= g) hi = mid; else lo = mid + 1; }
    const int r0 = lo;
    hi = R;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (ring_region[mid] > g) hi = mid; else lo = mid + 1; }
    const int r1 = lo;
    const double inf = __builtin_inf();
    double xmin = inf, ymin = inf, xmax = -inf, ymax = -inf;
    if (r1 > r0) {
        const int v0 = max(ring_start[r0], 0), v1 = min(ring_start[r1], V);
        for (int j = v0 + tid; j < v1; j += GC_THREADS) {
            const double2 q = make_double2(verts[2 * int64_t(j)], verts[2 * int64_t(j) + 1]);
            xmin = fmin(xmin, q.x); ymin = fmin(ymin, q.y); xmax = fmax(xmax, q.x); ymax = fmax(ymax, q.y);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        xmin = fmin(xmin, __shfl_xor(xmin, o, 64)); ymin = fmin(ymin, __shfl_xor(ymin, o, 64));
        xmax = fmax(xmax, __shfl_xor(xmax, o, 64)); ymax = fmax(ymax, __shfl_xor(ymax, o, 64));
    }
    if ((tid & 63) == 0) { red[tid >> 6][0] = xmin; red[tid >> 6][1] = ymin; red[tid >> 6][2] = xmax; red[tid >> 6][3] = ymax; }
    __syncthreads();
    if (tid < 4) {
        double v = red[0][tid];
        for (int w = 1; w < GC_THREADS / 64; ++w) v = tid < 2 ? fmin(v, red[w][tid]) : fmax(v, red[w][tid]);
        box[4 * g + tid] = v;
    }
}

struct RasterP {
    const double* points; const void* raster; int32_t* value;
    int N, H, W, dtype, has_nodata, nodata;
    double x0, dx, y0, dy;
};

__global__ __launch_bounds__(GC_THREADS) void raster_lookup_kernel(const RasterP p) {
#pragma clang fp contract(off)
    const int64_t pt = int64_t(blockIdx.x) * GC_THREADS + threadIdx.x;
    if (pt >= p.N) return;
    const double2 q = make_double2(p.points[2 * pt], p.points[2 * pt + 1]);
    const double col = floor((q.x - p.x0) / p.dx), row = floor((q.y - p.y0) / p.dy);
    int v = 0;
    if (col >= 0.0 && col < double(p.W) && row >= 0.0 && row < double(p.H)) {   // false for NaN
        const int64_t at = int64_t(row) * p.W + int64_t(col);
        if (p.dtype == NIRGAN_RASTER_U8) v = static_cast<const uint8_t*>(p.raster)[at];
        else if (p.dtype == NIRGAN_RASTER_I16) v = static_cast<const int16_t*>(p.raster)[at];
        else v = static_cast<const int32_t*>(p.raster)[at];
        if (p.has_nodata && v == p.nodata) v = 0;
    }
    p.value[pt] = v;
}

// what both polygon entries check of the layer; the optional host copies of the two ring tables are read here, the device's never
int layer_checks(const nirgan_point_regions_desc* d, const char* who) {
    NG_REQUIRE(d != nullptr, "%s: null descriptor", who);
    NG_REQUIRE(d->n_points >= 0 && d->n_verts >= 0 && d->n_rings >= 0 && d->n_regions >= 0,
               "%s: negative count (n_points %d, n_verts %d, n_rings %d, n_regions %d)", who, d->n_points, d->n_verts, d->n_rings, d->n_regions);
    NG_REQUIRE(d->slab_verts >= 0 && d->slab_verts <= GC_SLAB_MAX, "%s: slab_verts=%d must lie in 0..%d (0: the default)", who, d->slab_verts, GC_SLAB_MAX);
    if (d->ring_region_host)
        for (int r = 0; r < d->n_rings; ++r) {
            const int g = d->ring_region_host[r];
            NG_REQUIRE(g >= 0 && g < d->n_regions, "%s: ring_region[%d]=%d outside 0..%d", who, r, g, d->n_regions - 1);
            NG_REQUIRE(r == 0 || g >= d->ring_region_host[r - 1], "%s: ring_region decreases at ring %d", who, r);
        }
    if (d->ring_start_host) {
        NG_REQUIRE(d->ring_start_host[0] == 0, "%s: ring_start[0]=%d is not 0", who, d->ring_start_host[0]);
        for (int r = 0; r < d->n_rings; ++r)
            NG_REQUIRE(d->ring_start_host[r + 1] >= d->ring_start_host[r], "%s: ring_start decreases at ring %d", who, r);
        NG_REQUIRE(d->ring_start_host[d->n_rings] == d->n_verts, "%s: ring_start[%d]=%d is not n_verts=%d", who, d->n_rings,
                   d->ring_start_host[d->n_rings], d->n_verts);
    }
    return NIRGAN_OK;
}

}  // namespace

extern "C" int64_t nirgan_point_regions_ws_bytes(int n_points, int n_regions) {
    if (n_points <= 0 || n_regions <= 0) return 0;
    return int64_t(n_points) * ((n_regions + 31) / 32) * 4;
}

extern "C" int nirgan_region_boxes(const nirgan_point_regions_desc* d, void* stream) {
    const int rc = layer_checks(d, "region_boxes");
    if (rc != NIRGAN_OK) return rc;
    if (d->n_regions == 0) return NIRGAN_OK;
    NG_REQUIRE(d->region_box && d->ring_start && (d->n_rings == 0 || d->ring_region) && (d->n_verts == 0 || d->verts), "region_boxes: null pointer");
    hipLaunchKernelGGL(region_boxes_kernel, dim3(unsigned(d->n_regions)), dim3(GC_THREADS), 0, static_cast<hipStream_t>(stream),
                       d->verts, d->ring_start, d->ring_region, d->n_verts, d->n_rings, d->region_box);
    return nirgan_check_launch("region_boxes");
}

extern "C" int nirgan_point_regions(const nirgan_point_regions_desc* d, void* stream) {
    const int rc = layer_checks(d, "point_regions");
    if (rc != NIRGAN_OK) return rc;
    if (d->n_points == 0 || d->n_regions == 0) return NIRGAN_OK;
    NG_REQUIRE(d->points && d->region && d->ws && d->region_box && d->ring_start && (d->n_rings == 0 || d->ring_region) && (d->n_verts == 0 || d->verts),
               "point_regions: null pointer");
    RegionsP p;
    p.points = d->points; p.verts = d->verts;
    p.ring_start = d->ring_start; p.ring_region = d->ring_region; p.box = d->region_box;
    p.ws = d->ws; p.region = d->region;
    p.N = d->n_points; p.V = d->n_verts; p.R = d->n_rings; p.G = d->n_regions;
    p.words = (d->n_regions + 31) / 32;
    const int64_t need = nirgan_point_regions_ws_bytes(d->n_points, d->n_regions);
    NG_REQUIRE(d->ws_bytes >= need, "point_regions: workspace of %lld bytes, %lld needed (nirgan_point_regions_ws_bytes)", (long long)d->ws_bytes, (long long)need);
    p.slab = d->slab_verts > 0 ? d->slab_verts : GC_SLAB_DEFAULT;
    p.nslab = (d->n_verts + p.slab - 1) / p.slab;
    const int64_t npc = (int64_t(d->n_points) + GC_THREADS - 1) / GC_THREADS;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(d->ws, 0, size_t(need), st) != hipSuccess) return nirgan_check_launch("point_regions");
    if (p.nslab > 0 && p.R > 0) {
        int64_t nvc = (GC_TARGET_BLOCKS + npc - 1) / npc;                       // a small table: cut the vertex axis too
        if (nvc > p.nslab) nvc = p.nslab;
        p.slabs_per_chunk = int((p.nslab + nvc - 1) / nvc);
        p.nvc = (p.nslab + p.slabs_per_chunk - 1) / p.slabs_per_chunk;
        const int64_t blocks = npc * p.nvc;
        NG_REQUIRE(blocks < (int64_t(1) << 31), "point_regions: too many blocks");
        hipLaunchKernelGGL(point_regions_kernel, dim3(unsigned(blocks)), dim3(GC_THREADS), 0, st, p);
    }
    hipLaunchKernelGGL(point_regions_pick_kernel, dim3(unsigned(npc)), dim3(GC_THREADS), 0, st, d->ws, p.N, p.words, d->region);
    return nirgan_check_launch("point_regions");
}

extern "C" int nirgan_raster_lookup(const nirgan_raster_lookup_desc* d, void* stream) {
    NG_REQUIRE(d != nullptr, "raster_lookup: null descriptor");
    NG_REQUIRE(d->n_points >= 0, "raster_lookup: negative count (n_points %d)", d->n_points);
    NG_REQUIRE(d->H > 0 && d->W > 0, "raster_lookup: empty raster (%d x %d)", d->H, d->W);
    NG_REQUIRE(d->dtype == NIRGAN_RASTER_U8 || d->dtype == NIRGAN_RASTER_I16 || d->dtype == NIRGAN_RASTER_I32, "raster_lookup: unknown dtype %d", d->dtype);
    NG_REQUIRE(d->dx != 0.0 && d->dy != 0.0 && d->dx == d->dx && d->dy == d->dy && d->x0 == d->x0 && d->y0 == d->y0,
               "raster_lookup: transform (x0 %g, dx %g, y0 %g, dy %g) needs non-zero steps and no NaN", d->x0, d->dx, d->y0, d->dy);
    if (d->n_points == 0) return NIRGAN_OK;
    NG_REQUIRE(d->points && d->raster && d->value, "raster_lookup: null pointer");
    RasterP p;
    p.points = d->points; p.raster = d->raster; p.value = d->value;
    p.N = d->n_points; p.H = d->H; p.W = d->W; p.dtype = d->dtype; p.has_nodata = d->has_nodata; p.nodata = d->nodata;
    p.x0 = d->x0; p.dx = d->dx; p.y0 = d->y0; p.dy = d->dy;
    const int64_t blocks = (int64_t(d->n_points) + GC_THREADS - 1) / GC_THREADS;
    hipLaunchKernelGGL(raster_lookup_kernel, dim3(unsigned(blocks)), dim3(GC_THREADS), 0, static_cast<hipStream_t>(stream), p);
    return nirgan_check_launch("raster_lookup");
}
