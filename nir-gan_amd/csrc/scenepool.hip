// Training batches from device-resident scenes: nirgan_scene_invalid_prefix / nirgan_scene_sample.
//
// The pool keeps the scenes as they are stored (uint16 or float, planar, nothing aligned).  A batch is two launches:
//   draw    one thread per sample: Philox4x32-10 on (seed; draw, sample0 + b, attempt) -> a window index among all windows of all
//           scenes (the high word of a 64 x 64 bit product: no modulo bias beyond 2^-64 * total), a binary search of the running window
//           counts for the scene, the rejection test on four entries of the scene's invalid-prefix table, the view, the coords;
//   gather  one 256-thread block per 64 x 64 block of one output plane, grid-strided.  Plain views (0 .. 3) keep the lanes along the
//           output row, which is a source row read forwards or backwards: one element per lane, 128 contiguous bytes per wave for
//           uint16 whatever the address (offsets, widths and x0 are arbitrary, so nothing wider than the element is ever loaded).
//           Transposing views (4 .. 7) read the source row-wise as well, lanes along the output COLUMN, and turn the block in LDS
//           with rows padded to 65 floats as tileviews.hip does (written with stride 65, read with stride 1: no bank conflict).
//           The division happens on the way; every output element has one owner, stores are one dword per lane, 256 contiguous
//           bytes per wave, so any T >= 1 needs no tail handling.
// The prefix table of a scene is built once: a wave scans each row 64 pixels at a time with a carry, then one thread per column runs
// the sum down in place (eight rows of loads in flight).  Integers throughout: exact and order-independent, no atomics.
#include "scene_dev.h"

namespace {

template <typename T> struct Elem;
template <> struct Elem<uint16_t> {
    static __device__ __forceinline__ bool invalid(uint16_t v, int nodata) { return int(v) == nodata; }
};
template <> struct Elem<float> {
    static __device__ __forceinline__ bool invalid(float v, int) { return v != v; }
};

struct PrefixP {
    const void* scene;                   // the scene's first element
    int H, W, nodata;
    int64_t plane[4];                    // element offsets of the four selected planes inside the scene
    int32_t* prefix;
};

template <typename T>
__global__ __launch_bounds__(256) void scene_prefix_rows_kernel(const PrefixP p) {
    const T* __restrict__ src = static_cast<const T*>(p.scene);
    const int lane = threadIdx.x & 63;
    const int ld = p.W + 1;
    const int64_t waves = int64_t(gridDim.x) * 4;
    for (int64_t ty = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); ty <= p.H; ty += waves) {   // ty: wave-uniform
        int32_t* __restrict__ row = p.prefix + ty * ld;
        if (ty == 0) {
            for (int x = lane; x < ld; x += 64) row[x] = 0;
            continue;
        }
        if (lane == 0) row[0] = 0;
        const int64_t at = (ty - 1) * p.W;
        int carry = 0;
        for (int x0 = 0; x0 < p.W; x0 += 64) {
            const int x = x0 + lane;
            int v = 0;
            if (x < p.W) {
                bool bad = false;
#pragma unroll
                for (int k = 0; k < 4; ++k) bad = bad || Elem<T>::invalid(src[p.plane[k] + at + x], p.nodata);
                v = bad ? 1 : 0;
            }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(v, o, 64);
                if (lane >= o) v += u;
            }
            if (x < p.W) row[x + 1] = carry + v;
            carry += __shfl(v, 63, 64);
        }
    }
}

__global__ __launch_bounds__(256) void scene_prefix_cols_kernel(const PrefixP p) {
    const int ld = p.W + 1;
    for (int64_t x = 1 + blockIdx.x * int64_t(blockDim.x) + threadIdx.x; x <= p.W; x += int64_t(gridDim.x) * blockDim.x) {
        int run = 0;
        for (int ty = 1; ty <= p.H; ty += 8) {
            int v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = ty + k <= p.H ? p.prefix[int64_t(ty + k) * ld + x] : 0;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (ty + k <= p.H) {
                    run += v[k];
                    p.prefix[int64_t(ty + k) * ld + x] = run;
                }
        }
    }
}

struct SampleP {
    const void* pool;
    const int64_t* table;
    const int32_t* prefix;
    const double* geo;
    int64_t total;                       // windows of the whole pool
    int64_t band[4];                     // selected plane numbers
    int S, T, B, views, max_invalid, nb; // nb: blocks per tile side
    int64_t nblk;                        // B * 4 * nb * nb
    float divisor;
    uint32_t seed_lo, seed_hi, draw_lo, draw_hi, sample0;
    float* rgb; float* nir; float* coords;
    int32_t* window;
};

__global__ __launch_bounds__(256) void scene_draw_kernel(const SampleP p) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    int s = 0, y0 = 0, x0 = 0, view = 0, a = 0;
    bool ok = false;
    for (; a < NIRGAN_SCENE_ATTEMPTS; ++a) {
        uint32_t w[4];
        philox4x32_10(p.draw_lo, p.draw_hi, p.sample0 + uint32_t(b), uint32_t(a), p.seed_lo, p.seed_hi, w);
        const int64_t n = sp_attempt(w, p.table, p.prefix, p.S, p.T, p.total, p.views, s, y0, x0, view);
        if (n <= p.max_invalid) { ok = true; break; }
    }
    if (!ok) a = NIRGAN_SCENE_ATTEMPTS - 1;
    int32_t* __restrict__ o = p.window + int64_t(b) * 4;
    o[0] = s; o[1] = y0; o[2] = x0;
    o[3] = int32_t(uint32_t(view) | (uint32_t(a) << 8) | (ok ? 0u : 0x80000000u));
    if (p.geo && p.coords) sp_centre(p.geo + int64_t(s) * 4, y0, x0, p.T, p.coords + int64_t(b) * 2);
}

template <typename T>
__global__ __launch_bounds__(256) void scene_gather_kernel(const SampleP p) {
    __shared__ float lds[SP_B * SP_LD];
    const T* __restrict__ pool = static_cast<const T*>(p.pool);
    const int t = threadIdx.x, lx = t & 63, ly = t >> 6;
    const int Tt = p.T;
    const int64_t tt = int64_t(Tt) * Tt;
    for (int64_t blk = blockIdx.x; blk < p.nblk; blk += gridDim.x) {
        const int c0 = int(blk % p.nb) * SP_B;
        int64_t q = blk / p.nb;
        const int r0 = int(q % p.nb) * SP_B;
        q /= p.nb;
        const int ch = int(q & 3);
        const int64_t b = q >> 2;
        const int32_t* __restrict__ win = p.window + b * 4;
        const int s = win[0], y0 = win[1], x0 = win[2], view = win[3] & 7;
        const int64_t* __restrict__ row = p.table + int64_t(s) * TC;
        const int64_t W = row[2];
        const T* __restrict__ src = pool + row[0] + p.band[ch] * row[1] * W + int64_t(y0) * W + x0;       // the window's corner
        float* __restrict__ out = ch < 3 ? p.rgb + (b * 3 + ch) * tt : p.nir + b * tt;
        if (!(view & 4)) {
            const int j = c0 + lx, jp = (view & 1) ? Tt - 1 - j : j;
            if (j < Tt) {
#pragma unroll 4
                for (int k = 0; k < 16; ++k) {
                    const int i = r0 + ly + 4 * k;
                    if (i < Tt) {
                        const int ip = (view & 2) ? Tt - 1 - i : i;
                        out[int64_t(i) * Tt + j] = __fdiv_rn(float(src[ip * W + jp]), p.divisor);
                    }
                }
            }
        } else {
            // out[i][j] = src[f1(j)][f0(i)]: the lanes run along i, which is the source's column
            const int i = r0 + lx, jp = (view & 1) ? Tt - 1 - i : i;
            if (i < Tt) {
#pragma unroll 4
                for (int k = 0; k < 16; ++k) {
                    const int jl = ly + 4 * k, j = c0 + jl;
                    if (j < Tt) {
                        const int ip = (view & 2) ? Tt - 1 - j : j;
                        lds[lx * SP_LD + jl] = __fdiv_rn(float(src[ip * W + jp]), p.divisor);
                    }
                }
            }
            __syncthreads();
            const int j = c0 + lx;
            if (j < Tt) {
#pragma unroll 4
                for (int k = 0; k < 16; ++k) {
                    const int il = ly + 4 * k, i2 = r0 + il;
                    if (i2 < Tt) out[int64_t(i2) * Tt + j] = lds[il * SP_LD + lx];
                }
            }
            __syncthreads();                                                    // the next block of this grid-stride loop writes lds again
        }
    }
}

}  // namespace

extern "C" int nirgan_scene_invalid_prefix(const nirgan_scene_prefix_desc* d, void* stream) {
    NG_REQUIRE(d && d->pool && d->prefix, "scene_invalid_prefix: null pointer");
    NG_REQUIRE(d->dtype == NIRGAN_SCENE_U16 || d->dtype == NIRGAN_SCENE_F32, "scene_invalid_prefix: unknown dtype %d", d->dtype);
    NG_REQUIRE(d->C > 0 && d->H > 0 && d->W > 0, "scene_invalid_prefix: bad shape (C %d, H %d, W %d)", d->C, d->H, d->W);
    NG_REQUIRE((int64_t(d->H) + 1) * (int64_t(d->W) + 1) < LIM31, "scene_invalid_prefix: the table (H+1)(W+1) is 2^31 or more");
    for (int k = 0; k < 4; ++k) NG_REQUIRE(d->band[k] >= 0 && d->band[k] < d->C, "scene_invalid_prefix: band %d outside 0 .. C-1", d->band[k]);
    const int64_t plane = int64_t(d->H) * d->W;
    NG_REQUIRE(d->offset >= 0 && d->pool_elems >= 0 && d->offset <= d->pool_elems && plane * d->C <= d->pool_elems - d->offset,
               "scene_invalid_prefix: the scene lies outside the pool");
    NG_REQUIRE(d->dtype != NIRGAN_SCENE_U16 || (d->nodata >= 0 && d->nodata <= 65535), "scene_invalid_prefix: nodata %d outside 0 .. 65535", d->nodata);
    PrefixP p;
    p.H = d->H; p.W = d->W; p.nodata = d->nodata; p.prefix = d->prefix;
    for (int k = 0; k < 4; ++k) p.plane[k] = d->band[k] * plane;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int g1 = (d->H + 1 + 3) / 4, g2 = (d->W + 255) / 256;
    if (d->dtype == NIRGAN_SCENE_U16) {
        p.scene = static_cast<const uint16_t*>(d->pool) + d->offset;
        hipLaunchKernelGGL(scene_prefix_rows_kernel<uint16_t>, dim3(g1 < 8192 ? g1 : 8192), dim3(256), 0, st, p);
    } else {
        p.scene = static_cast<const float*>(d->pool) + d->offset;
        hipLaunchKernelGGL(scene_prefix_rows_kernel<float>, dim3(g1 < 8192 ? g1 : 8192), dim3(256), 0, st, p);
    }
    hipLaunchKernelGGL(scene_prefix_cols_kernel, dim3(g2 < 8192 ? g2 : 8192), dim3(256), 0, st, p);
    return nirgan_check_launch("scene_invalid_prefix");
}

extern "C" int nirgan_scene_sample(const nirgan_scene_sample_desc* d, void* stream) {
    NG_REQUIRE(d && d->pool && d->table && d->table_host && d->rgb && d->nir && d->window, "scene_sample: null pointer");
    NG_REQUIRE(d->dtype == NIRGAN_SCENE_U16 || d->dtype == NIRGAN_SCENE_F32, "scene_sample: unknown dtype %d", d->dtype);
    NG_REQUIRE(d->S > 0 && d->C >= 4, "scene_sample: bad pool (S %d, C %d; C must be at least 4)", d->S, d->C);
    NG_REQUIRE(d->views == 1 || d->views == 4 || d->views == 8, "scene_sample: views %d is not 1, 4 or 8", d->views);
    for (int k = 0; k < 4; ++k) NG_REQUIRE(d->band[k] >= 0 && d->band[k] < d->C, "scene_sample: band %d outside 0 .. C-1", d->band[k]);
    const int64_t T = d->tile;
    NG_REQUIRE(d->B > 0 && T > 0 && T * T < LIM31 && T * T * d->B < LIM31, "scene_sample: B, tile or B*tile*tile is not in 1 .. 2^31-1 (B %d, tile %d)", d->B, d->tile);
    NG_REQUIRE(d->divisor == d->divisor && d->divisor != 0.0f, "scene_sample: divisor is 0 or NaN");
    NG_REQUIRE(d->max_invalid >= 0, "scene_sample: negative max_invalid");
    NG_REQUIRE(d->pool_elems >= 0 && d->prefix_elems >= 0, "scene_sample: negative pool_elems or prefix_elems");
    int64_t total = 0;
    if (int e = sp_check_table("scene_sample", d->table_host, d->S, T, &total)) return e;
    NG_REQUIRE(total > 0, "scene_sample: no scene holds a window of tile %d", d->tile);
    if (int e = sp_check_extents("scene_sample", d->table_host, d->S, d->C, d->pool_elems, d->prefix, d->prefix_elems)) return e;
    SampleP p;
    p.pool = d->pool; p.table = d->table; p.prefix = d->prefix; p.geo = d->geo; p.total = total;
    for (int k = 0; k < 4; ++k) p.band[k] = d->band[k];
    p.S = d->S; p.T = d->tile; p.B = d->B; p.views = d->views; p.max_invalid = d->max_invalid;
    p.nb = (d->tile + SP_B - 1) / SP_B;
    p.nblk = int64_t(d->B) * 4 * p.nb * p.nb;
    p.divisor = d->divisor;
    p.seed_lo = d->seed_lo; p.seed_hi = d->seed_hi; p.draw_lo = uint32_t(d->draw); p.draw_hi = uint32_t(d->draw >> 32); p.sample0 = d->sample0;
    p.rgb = d->rgb; p.nir = d->nir; p.coords = d->geo ? d->coords : nullptr; p.window = d->window;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(scene_draw_kernel, dim3((d->B + 255) / 256), dim3(256), 0, st, p);
    const int grid = int(p.nblk < 16384 ? p.nblk : 16384);
    if (d->dtype == NIRGAN_SCENE_U16) hipLaunchKernelGGL(scene_gather_kernel<uint16_t>, dim3(grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(scene_gather_kernel<float>, dim3(grid), dim3(256), 0, st, p);
    return nirgan_check_launch("scene_sample");
}
