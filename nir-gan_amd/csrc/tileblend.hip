// Tiled inference with cross-faded tile overlaps: nirgan_tile_count_ov / nirgan_tile_gather_ov / nirgan_tile_blend.
//
// Per axis, core = tile - 2 margin and stride = core - overlap (0 <= overlap <= core / 2): tile i reads scene rows
// i * stride - margin .. + tile - 1 (reflected at the borders) and its usable region is scene rows [i * stride, i * stride + core).
// Two neighbouring usable regions share `overlap` rows t = 0 .. overlap - 1 counted from the later tile's first usable row; there the
// later tile weighs r(t), the earlier one 1 - r(t).  With overlap <= core / 2 no row lies in more than two usable regions, so a pixel
// has at most four covering tiles and its weight for a tile is (row weight) * (column weight).  overlap = 0 is the geometry of
// nirgan_tile_gather / nirgan_tile_scatter (layout.hip).
//
// Both kernels are streaming passes over scene pixels resp. tile pixels: a thread owns four pixels consecutive in x, lanes own
// consecutive quads, addresses are 64-bit.  The blend is parallel over SCENE pixels, so no two threads of a launch write one pixel and
// there are no atomics: a pixel's covering tiles are visited in ascending tile number, the lowest-numbered one stores w * v, every
// later one does acc = fma(w, v, acc).  Whether the lowest-numbered covering tile lies before `first` follows from the geometry
// alone, which is what selects between starting from the stored value and starting fresh -- the scene needs no initialisation and the
// result does not depend on how the tiles are split into launches (ascending `first`, one stream).
#include "tile_dev.h"

namespace {

struct BlendP {
    float* scene; float* tiles;
    int B, C, H, W, tile, margin, overlap, window, core, stride, nth, ntw, first, n;
    int b0, nb, y0, ny, x0, nq;        // the blend's rectangle of scene pixels: images b0 .. b0 + nb - 1, rows y0 .. y0 + ny - 1, nq quads from column x0
    int vec;                           // 16-byte stores allowed (alignment of the written buffer and of its rows)
};

// weight of the LATER tile at band position t (0 <= t < overlap); the earlier tile gets 1 - r
__device__ __forceinline__ float band_weight(int t, int overlap, int window) {
    const float u = __fdiv_rn(float(t) + 0.5f, float(overlap));
    return window == 0 ? u : __fsub_rn(0.5f, __fmul_rn(0.5f, cosf(3.14159265358979323846f * u)));
}

// the tiles covering position h of one axis: the later one `hi` (always) with weight w_hi, and in a band the earlier one hi - 1
// with weight w_lo (has_lo)
struct Cover { int hi; float w_hi, w_lo; bool has_lo; };

__device__ __forceinline__ Cover axis_cover(int h, int stride, int nt, int overlap, int window) {
    Cover c;
    c.hi = min(h / stride, nt - 1);
    const int t = h - c.hi * stride;
    c.has_lo = c.hi >= 1 && t < overlap;
    c.w_hi = 1.0f; c.w_lo = 0.0f;
    if (c.has_lo) {
        c.w_hi = band_weight(t, overlap, window);
        c.w_lo = __fsub_rn(1.0f, c.w_hi);
    }
    return c;
}

__global__ __launch_bounds__(256) void tile_gather_ov_kernel(const BlendP p) {
    const int groups = (p.tile + 3) >> 2;
    const int64_t total = int64_t(p.n) * p.C * p.tile * groups;
    const int per = p.nth * p.ntw;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += int64_t(gridDim.x) * 256) {
        const int g = int(i % groups);
        int64_t r = i / groups;
        const int y = int(r % p.tile);
        r /= p.tile;
        const int c = int(r % p.C), k = int(r / p.C);
        const int id = p.first + k, b = id / per, t = id - b * per, ti = t / p.ntw, tj = t - ti * p.ntw;
        const int h = tb_reflect(ti * p.stride + y - p.margin, p.H);
        const float* __restrict__ src = p.scene + ((int64_t(b) * p.C + c) * p.H + h) * p.W;
        float* __restrict__ dst = p.tiles + ((int64_t(k) * p.C + c) * p.tile + y) * p.tile + 4 * g;
        const int xs = tj * p.stride + 4 * g - p.margin;
        if (p.vec) {                    // tile % 4 == 0: the quad is whole
            f32x4 v;
            v.x = src[tb_reflect(xs, p.W)];
            v.y = src[tb_reflect(xs + 1, p.W)];
            v.z = src[tb_reflect(xs + 2, p.W)];
            v.w = src[tb_reflect(xs + 3, p.W)];
            *reinterpret_cast<f32x4*>(dst) = v;
        } else {
            for (int e = 0; e < 4 && 4 * g + e < p.tile; ++e) dst[e] = src[tb_reflect(xs + e, p.W)];
        }
    }
}

__global__ __launch_bounds__(256) void tile_blend_kernel(const BlendP p) {
    const int64_t total = int64_t(p.nb) * p.C * p.ny * p.nq;
    const int per = p.nth * p.ntw;
    const int64_t last = int64_t(p.first) + p.n;              // one past the launch's tiles
    const int64_t trow = p.tile, timg = int64_t(p.tile) * p.tile;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += int64_t(gridDim.x) * 256) {
        const int q = int(i % p.nq);
        int64_t r = i / p.nq;
        const int h = p.y0 + int(r % p.ny);
        r /= p.ny;
        const int c = int(r % p.C), b = p.b0 + int(r / p.C);
        // the row's tiles and weights, once for the thread's four pixels
        const Cover cy = axis_cover(h, p.stride, p.nth, p.overlap, p.window);
        const int64_t id_hi = int64_t(b) * per + int64_t(cy.hi) * p.ntw;          // tile (b, cy.hi, 0); the earlier row of tiles is p.ntw before
        const int row_hi = h - cy.hi * p.stride + p.margin;                    // the pixel's row inside tile row cy.hi; + stride inside cy.hi - 1
        float* __restrict__ out = p.scene + ((int64_t(b) * p.C + c) * p.H + h) * p.W;
        const int xq = p.x0 + 4 * q;
        float acc[4];
        bool hit[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int x = xq + e;
            hit[e] = false;
            acc[e] = 0.0f;
            if (x >= p.W) continue;
            const Cover cx = axis_cover(x, p.stride, p.ntw, p.overlap, p.window);
            const int col_hi = x - cx.hi * p.stride + p.margin;
            const int64_t lowest = id_hi - (cy.has_lo ? p.ntw : 0) + cx.hi - (cx.has_lo ? 1 : 0);
            if (lowest >= last) continue;                                       // none of the pixel's tiles is in this launch
            bool have = lowest < p.first;                                       // an earlier launch left the sum so far in the scene
            if (have) {
                if (id_hi + cx.hi < p.first) continue;                          // all of the pixel's tiles came before this launch
                acc[e] = out[x];
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {                                       // ascending tile number: (lo, lo), (lo, hi), (hi, lo), (hi, hi)
                const bool ylo = s < 2, xlo = (s & 1) == 0;
                if ((ylo && !cy.has_lo) || (xlo && !cx.has_lo)) continue;
                const int64_t id = id_hi - (ylo ? p.ntw : 0) + cx.hi - (xlo ? 1 : 0);
                if (id < p.first || id >= last) continue;
                const float w = __fmul_rn(ylo ? cy.w_lo : cy.w_hi, xlo ? cx.w_lo : cx.w_hi);
                const int ry = row_hi + (ylo ? p.stride : 0), rx = col_hi + (xlo ? p.stride : 0);
                const float v = p.tiles[((id - p.first) * p.C + c) * timg + ry * trow + rx];
                acc[e] = have ? __fmaf_rn(w, v, acc[e]) : __fmul_rn(w, v);
                have = true;
                hit[e] = true;
            }
        }
        if (p.vec && hit[0] && hit[1] && hit[2] && hit[3]) {
            f32x4 v;
            v.x = acc[0]; v.y = acc[1]; v.z = acc[2]; v.w = acc[3];
            *reinterpret_cast<f32x4*>(out + xq) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (hit[e]) out[xq + e] = acc[e];
        }
    }
}

inline int blend_grid(int64_t items) {
    const int64_t g = (items + 255) / 256;
    return int(g < 8192 ? (g < 1 ? 1 : g) : 8192);
}

inline bool tiling_ok(int B, int H, int W, int tile, int margin, int overlap) {
    return B > 0 && H > 0 && W > 0 && tile > 0 && margin >= 0 && 2 * int64_t(margin) < tile && overlap >= 0 && 2 * int64_t(overlap) <= tile - 2 * margin;
}

int blend_params(BlendP& p, const nirgan_tile_blend_desc* d, const char* who) {
    NG_REQUIRE(d && d->scene && d->tiles, "%s: null pointer", who);
    NG_REQUIRE(d->B > 0 && d->C > 0 && d->H > 0 && d->W > 0 && d->tile > 0, "%s: bad shape", who);
    NG_REQUIRE(d->margin >= 0 && 2 * int64_t(d->margin) < d->tile, "%s: margin %d must be below tile / 2 (tile %d)", who, d->margin, d->tile);
    const int core = d->tile - 2 * d->margin;
    NG_REQUIRE(d->overlap >= 0 && 2 * int64_t(d->overlap) <= core, "%s: overlap %d outside 0 .. core / 2 (core %d)", who, d->overlap, core);
    NG_REQUIRE(d->window == NIRGAN_BLEND_LINEAR || d->window == NIRGAN_BLEND_COSINE, "%s: unknown window %d", who, d->window);
    NG_REQUIRE(d->H < (1 << 30) && d->W < (1 << 30) && int64_t(d->H) * d->W < (1ll << 31) && int64_t(d->C) * d->tile * d->tile < (1ll << 31),
               "%s: a plane of the scene or a tile has 2^31 elements or more", who);
    p.scene = d->scene; p.tiles = d->tiles;
    p.B = d->B; p.C = d->C; p.H = d->H; p.W = d->W; p.tile = d->tile; p.margin = d->margin; p.overlap = d->overlap; p.window = d->window;
    p.core = core; p.stride = core - d->overlap;
    p.nth = tiles_per_axis(d->H, core, p.stride); p.ntw = tiles_per_axis(d->W, core, p.stride);
    const int64_t count = int64_t(d->B) * p.nth * p.ntw;
    NG_REQUIRE(count < (1ll << 31), "%s: 2^31 tiles or more", who);
    NG_REQUIRE(d->first >= 0 && d->n > 0 && int64_t(d->first) + d->n <= count, "%s: tiles %d .. %lld of %lld", who, d->first, (long long)d->first + d->n - 1, (long long)count);
    p.first = d->first; p.n = d->n;
    p.b0 = p.nb = p.y0 = p.ny = p.x0 = p.nq = p.vec = 0;
    return NIRGAN_OK;
}

}  // namespace

extern "C" int64_t nirgan_tile_count_ov(int B, int H, int W, int tile, int margin, int overlap) {
    if (!tiling_ok(B, H, W, tile, margin, overlap)) return 0;
    const int core = tile - 2 * margin, stride = core - overlap;
    return int64_t(B) * tiles_per_axis(H, core, stride) * tiles_per_axis(W, core, stride);
}

extern "C" int nirgan_tile_gather_ov(const nirgan_tile_blend_desc* d, void* stream) {
    BlendP p;
    const int rc = blend_params(p, d, "tile_gather_ov");
    if (rc != NIRGAN_OK) return rc;
    p.vec = p.tile % 4 == 0 && ng_aligned16(p.tiles);
    const int64_t items = int64_t(p.n) * p.C * p.tile * ((p.tile + 3) / 4);
    hipLaunchKernelGGL(tile_gather_ov_kernel, dim3(blend_grid(items)), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return nirgan_check_launch("tile_gather_ov");
}

extern "C" int nirgan_tile_blend(const nirgan_tile_blend_desc* d, void* stream) {
    BlendP p;
    const int rc = blend_params(p, d, "tile_blend");
    if (rc != NIRGAN_OK) return rc;
    // the rectangle of scene pixels that the usable regions of tiles first .. first + n - 1 can reach: one row of tiles -> its columns,
    // several rows of one image -> their rows at full width, several images -> those images
    const int per = p.nth * p.ntw, lastid = p.first + p.n - 1;
    const int b_lo = p.first / per, b_hi = lastid / per;
    const int ti_lo = (p.first - b_lo * per) / p.ntw, ti_hi = (lastid - b_hi * per) / p.ntw;
    int y0 = 0, y1 = p.H, x0 = 0, x1 = p.W;
    if (b_lo == b_hi) {
        y0 = ti_lo * p.stride;
        y1 = ti_hi * p.stride + p.core < p.H ? ti_hi * p.stride + p.core : p.H;
        if (ti_lo == ti_hi) {
            const int tj_lo = p.first - b_lo * per - ti_lo * p.ntw, tj_hi = lastid - b_lo * per - ti_lo * p.ntw;
            x0 = (tj_lo * p.stride) & ~3;                                          // quads stay aligned with the scene's rows
            x1 = tj_hi * p.stride + p.core < p.W ? tj_hi * p.stride + p.core : p.W;
        }
    }
    p.b0 = b_lo; p.nb = b_hi - b_lo + 1; p.y0 = y0; p.ny = y1 - y0; p.x0 = x0; p.nq = (x1 - x0 + 3) / 4;
    p.vec = p.W % 4 == 0 && ng_aligned16(p.scene);
    const int64_t items = int64_t(p.nb) * p.C * p.ny * p.nq;
    hipLaunchKernelGGL(tile_blend_kernel, dim3(blend_grid(items)), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return nirgan_check_launch("tile_blend");
}
