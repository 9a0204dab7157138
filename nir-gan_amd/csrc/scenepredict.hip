// Predicting one device-resident scene in place: nirgan_scene_tile_invalid / nirgan_scene_tile_gather /
// nirgan_scene_finish.  The scene stays as it is stored (uint16 or float, planar, nothing aligned); the tiling is that of
// tileblend.hip (tile_dev.h) and the generator's answers go through nirgan_tile_blend unchanged.
//   counts  one 256-thread workgroup per tile, grid-strided.  A wave owns every fourth row of the tile's usable region, its lanes run
//           along x: one element per lane, 128 contiguous bytes per wave for uint16 whatever the address.  Integer sums: a butterfly
//           inside the wave, four words of LDS across the waves, one store per tile -- exact and the same on every run.
//   gather  the kernel of nirgan_tile_gather_ov with the tile number read from a list and the division on the way: a thread owns four
//           pixels consecutive in x (four reflected element loads -- a wave's lanes read one contiguous span --, one 16-byte store).
//           The first n threads of the grid also write the tiles' coords.
//   finish  element-wise over the flattened H * W plane: a thread owns four consecutive pixels, loaded and stored as one vector each
//           where every address allows it, element by element otherwise (and for the last, partial quad).
// 64-bit addressing, no atomics, every output element has one owner.
#include <hip/hip_fp16.h>
#include "scene_dev.h"
#include "tile_dev.h"

namespace {

__device__ __forceinline__ bool sc_bad(uint16_t v, int nodata) { return int(v) == nodata; }
__device__ __forceinline__ bool sc_bad(float v, int) { return v != v; }

struct SceneP {
    const void* scene;
    int64_t plane[3];                    // element offsets of the three selected planes
    int64_t hw;                          // H * W
    int H, W, has_nodata, nodata;
    int tile, margin, core, stride, nth, ntw, nt;
    float divisor;
    int32_t* counts;
    const int32_t* ids; int n;
    float* tiles; const double* geo; float* coords;
    const float* blended; void* out;
    float scale, nodata_out;
    int nodata_q;                        // nodata_out as the uint16 code
    int vec;                             // finish: every plane, `blended` and `out` allow one vector access per quad
};

template <typename T>
__global__ __launch_bounds__(256) void scene_tile_invalid_kernel(const SceneP p) {
    __shared__ int part[4];
    const T* __restrict__ s0 = static_cast<const T*>(p.scene) + p.plane[0];
    const T* __restrict__ s1 = static_cast<const T*>(p.scene) + p.plane[1];
    const T* __restrict__ s2 = static_cast<const T*>(p.scene) + p.plane[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = blockIdx.x; t < p.nt; t += gridDim.x) {                         // t: uniform over the workgroup
        const int ti = t / p.ntw, tj = t - ti * p.ntw;
        const int y0 = ti * p.stride, x0 = tj * p.stride;
        const int hy = min(p.core, p.H - y0), wx = min(p.core, p.W - x0);
        int sum = 0;
        if (p.has_nodata) {
            for (int y = wave; y < hy; y += 4) {
                const int64_t at = int64_t(y0 + y) * p.W + x0;
#pragma unroll 4
                for (int x = lane; x < wx; x += 64)
                    sum += (sc_bad(s0[at + x], p.nodata) || sc_bad(s1[at + x], p.nodata) || sc_bad(s2[at + x], p.nodata)) ? 1 : 0;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (lane == 0) part[wave] = sum;
        __syncthreads();
        if (threadIdx.x == 0) p.counts[t] = (part[0] + part[1]) + (part[2] + part[3]);
        __syncthreads();                                                        // the next tile of this grid-stride loop writes part again
    }
}

template <typename T>
__global__ __launch_bounds__(256) void scene_tile_gather_kernel(const SceneP p) {
    const T* __restrict__ scene = static_cast<const T*>(p.scene);
    const int groups = p.tile >> 2;                                              // tile % 4 == 0: every quad is whole
    const int64_t total = int64_t(p.n) * 3 * p.tile * groups;
    const int64_t start = blockIdx.x * 256ll + threadIdx.x, step = int64_t(gridDim.x) * 256;
    for (int64_t i = start; i < total; i += step) {
        const int g = int(i % groups);
        int64_t r = i / groups;
        const int y = int(r % p.tile);
        r /= p.tile;
        const int c = int(r % 3), k = int(r / 3);
        const int t = p.ids[k], ti = t / p.ntw, tj = t - ti * p.ntw;
        const int h = tb_reflect(ti * p.stride + y - p.margin, p.H);
        const T* __restrict__ src = scene + p.plane[c] + int64_t(h) * p.W;
        const int xs = tj * p.stride + 4 * g - p.margin;
        f32x4 v;
        v.x = __fdiv_rn(float(src[tb_reflect(xs, p.W)]), p.divisor);
        v.y = __fdiv_rn(float(src[tb_reflect(xs + 1, p.W)]), p.divisor);
        v.z = __fdiv_rn(float(src[tb_reflect(xs + 2, p.W)]), p.divisor);
        v.w = __fdiv_rn(float(src[tb_reflect(xs + 3, p.W)]), p.divisor);
        *reinterpret_cast<f32x4*>(p.tiles + ((int64_t(k) * 3 + c) * p.tile + y) * p.tile + 4 * g) = v;
    }
    if (p.coords) {                                                             // set only together with geo
        for (int64_t k = start; k < p.n; k += step) {
            const int t = p.ids[k], ti = t / p.ntw, tj = t - ti * p.ntw;
            const int y0 = ti * p.stride, x0 = tj * p.stride;
            const double cy = double(y0 + min(p.core, p.H - y0) / 2) + 0.5, cx = double(x0 + min(p.core, p.W - x0) / 2) + 0.5;   // exact
            p.coords[2 * k] = float(sp_mul_then_add(p.geo[0], cx, p.geo[1]));
            p.coords[2 * k + 1] = float(sp_mul_then_add(p.geo[2], cy, p.geo[3]));
        }
    }
}

template <typename X> struct alignas(4 * sizeof(X)) Quad { X e[4]; };

template <int KIND> struct Out { typedef uint16_t type; };                       // the uint16 code, or the bits of a binary16
template <> struct Out<NIRGAN_SCENE_OUT_F32> { typedef float type; };

template <int KIND>
__device__ __forceinline__ typename Out<KIND>::type finish_one(float v, bool bad, const SceneP& p) {
    if constexpr (KIND == NIRGAN_SCENE_OUT_F32) {
        return bad ? p.nodata_out : v;
    } else if constexpr (KIND == NIRGAN_SCENE_OUT_F16) {
        return __half_as_ushort(__float2half_rn(bad ? p.nodata_out : v));
    } else {
        const float t = __fmul_rn(v, p.scale);
        if (bad || t != t) return uint16_t(p.nodata_q);
        int q = int(fminf(fmaxf(rintf(t), 0.0f), 65535.0f));
        if (q == p.nodata_q) q = p.nodata_q == 65535 ? 65534 : p.nodata_q + 1;   // a valid pixel is never read as nodata
        return uint16_t(q);
    }
}

template <typename T, int KIND>
__global__ __launch_bounds__(256) void scene_finish_kernel(const SceneP p) {
    typedef typename Out<KIND>::type O;
    const T* __restrict__ s0 = static_cast<const T*>(p.scene) + p.plane[0];
    const T* __restrict__ s1 = static_cast<const T*>(p.scene) + p.plane[1];
    const T* __restrict__ s2 = static_cast<const T*>(p.scene) + p.plane[2];
    O* __restrict__ out = static_cast<O*>(p.out);
    const int64_t nq = (p.hw + 3) >> 2;
    for (int64_t q = blockIdx.x * 256ll + threadIdx.x; q < nq; q += int64_t(gridDim.x) * 256) {
        const int64_t i0 = q * 4;
        const int m = int(p.hw - i0 < 4 ? p.hw - i0 : 4);                        // pixels of this quad
        Quad<T> a = {}, b = {}, c = {};
        Quad<float> v = {};
        Quad<O> o;
        const bool whole = p.vec && m == 4;
        if (whole) {
            if (p.has_nodata) {
                a = *reinterpret_cast<const Quad<T>*>(s0 + i0);
                b = *reinterpret_cast<const Quad<T>*>(s1 + i0);
                c = *reinterpret_cast<const Quad<T>*>(s2 + i0);
            }
            v = *reinterpret_cast<const Quad<float>*>(p.blended + i0);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e >= m) continue;
                if (p.has_nodata) { a.e[e] = s0[i0 + e]; b.e[e] = s1[i0 + e]; c.e[e] = s2[i0 + e]; }
                v.e[e] = p.blended[i0 + e];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool bad = p.has_nodata && (sc_bad(a.e[e], p.nodata) || sc_bad(b.e[e], p.nodata) || sc_bad(c.e[e], p.nodata));
            o.e[e] = finish_one<KIND>(v.e[e], bad, p);
        }
        if (whole) {
            *reinterpret_cast<Quad<O>*>(out + i0) = o;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < m) out[i0 + e] = o.e[e];
        }
    }
}

inline int grid_for(int64_t items) {
    const int64_t g = (items + 255) / 256;
    return int(g < 8192 ? (g < 1 ? 1 : g) : 8192);
}

inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the checks and the geometry every entry shares
int scene_params(SceneP& p, const nirgan_scene_predict_desc* d, const char* who) {
    NG_REQUIRE(d && d->scene, "%s: null pointer", who);
    NG_REQUIRE(d->dtype == NIRGAN_SCENE_U16 || d->dtype == NIRGAN_SCENE_F32, "%s: unknown dtype %d", who, d->dtype);
    NG_REQUIRE(d->C >= 3 && d->H > 0 && d->W > 0, "%s: bad scene (C %d, H %d, W %d; C must be at least 3)", who, d->C, d->H, d->W);
    const int64_t hw = int64_t(d->H) * d->W;
    NG_REQUIRE(hw < LIM31, "%s: the plane H*W is 2^31 or more", who);
    for (int k = 0; k < 3; ++k) NG_REQUIRE(d->band[k] >= 0 && d->band[k] < d->C, "%s: band %d outside 0 .. C-1", who, d->band[k]);
    NG_REQUIRE(!d->has_nodata || d->dtype != NIRGAN_SCENE_U16 || (d->nodata >= 0 && d->nodata <= 65535), "%s: nodata %d outside 0 .. 65535", who, d->nodata);
    NG_REQUIRE(d->divisor == d->divisor && d->divisor != 0.0f, "%s: divisor is 0 or NaN", who);
    NG_REQUIRE(d->tile >= 4 && d->tile % 4 == 0, "%s: tile %d is not a positive multiple of 4", who, d->tile);
    NG_REQUIRE(d->margin >= 0 && 2 * int64_t(d->margin) < d->tile, "%s: margin %d must be below tile / 2 (tile %d)", who, d->margin, d->tile);
    const int core = d->tile - 2 * d->margin;
    NG_REQUIRE(d->overlap >= 0 && 2 * int64_t(d->overlap) <= core, "%s: overlap %d outside 0 .. core / 2 (core %d)", who, d->overlap, core);
    p.scene = d->scene; p.hw = hw;
    for (int k = 0; k < 3; ++k) p.plane[k] = d->band[k] * hw;
    p.H = d->H; p.W = d->W; p.has_nodata = d->has_nodata ? 1 : 0; p.nodata = d->nodata;
    p.tile = d->tile; p.margin = d->margin; p.core = core; p.stride = core - d->overlap;
    p.nth = tiles_per_axis(d->H, core, p.stride); p.ntw = tiles_per_axis(d->W, core, p.stride);
    const int64_t nt = int64_t(p.nth) * p.ntw;
    NG_REQUIRE(nt < LIM31, "%s: 2^31 tiles or more", who);
    p.nt = int(nt);
    p.divisor = d->divisor;
    p.counts = nullptr; p.ids = nullptr; p.n = 0; p.tiles = nullptr; p.geo = nullptr; p.coords = nullptr;
    p.blended = nullptr; p.out = nullptr; p.scale = 0.0f; p.nodata_out = 0.0f; p.nodata_q = 0; p.vec = 0;
    return NIRGAN_OK;
}

template <typename T>
void launch_finish(const SceneP& p, int kind, size_t elem, hipStream_t st) {
    SceneP q = p;
    const size_t out_elem = kind == NIRGAN_SCENE_OUT_F32 ? 4 : 2;
    q.vec = aligned_to(p.blended, 16) && aligned_to(p.out, 4 * out_elem) ? 1 : 0;
    for (int k = 0; k < 3; ++k) q.vec = q.vec && aligned_to(static_cast<const char*>(p.scene) + p.plane[k] * int64_t(elem), 4 * elem);
    const int grid = grid_for((p.hw + 3) / 4);
    if (kind == NIRGAN_SCENE_OUT_U16) hipLaunchKernelGGL((scene_finish_kernel<T, NIRGAN_SCENE_OUT_U16>), dim3(grid), dim3(256), 0, st, q);
    else if (kind == NIRGAN_SCENE_OUT_F16) hipLaunchKernelGGL((scene_finish_kernel<T, NIRGAN_SCENE_OUT_F16>), dim3(grid), dim3(256), 0, st, q);
    else hipLaunchKernelGGL((scene_finish_kernel<T, NIRGAN_SCENE_OUT_F32>), dim3(grid), dim3(256), 0, st, q);
}

}  // namespace

extern "C" int nirgan_scene_tile_invalid(const nirgan_scene_predict_desc* d, void* stream) {
    SceneP p;
    if (int e = scene_params(p, d, "scene_tile_invalid")) return e;
    NG_REQUIRE(d->counts, "scene_tile_invalid: null pointer (counts)");
    p.counts = d->counts;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int grid = p.nt < 8192 ? p.nt : 8192;
    if (d->dtype == NIRGAN_SCENE_U16) hipLaunchKernelGGL(scene_tile_invalid_kernel<uint16_t>, dim3(grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(scene_tile_invalid_kernel<float>, dim3(grid), dim3(256), 0, st, p);
    return nirgan_check_launch("scene_tile_invalid");
}

extern "C" int nirgan_scene_tile_gather(const nirgan_scene_predict_desc* d, void* stream) {
    SceneP p;
    if (int e = scene_params(p, d, "scene_tile_gather")) return e;
    NG_REQUIRE(d->ids && d->ids_host && d->tiles, "scene_tile_gather: null pointer (ids, ids_host or tiles)");
    NG_REQUIRE(ng_aligned16(d->tiles), "scene_tile_gather: tiles is not 16-byte aligned");
    NG_REQUIRE(d->n > 0 && int64_t(d->n) * 3 * d->tile * d->tile < LIM31, "scene_tile_gather: n or n*3*tile*tile is not in 1 .. 2^31-1 (n %d, tile %d)", d->n, d->tile);
    for (int k = 0; k < d->n; ++k) {
        const int id = d->ids_host[k];
        NG_REQUIRE(id >= 0 && id < p.nt, "scene_tile_gather: ids[%d] = %d outside 0 .. %d", k, id, p.nt - 1);
        NG_REQUIRE(k == 0 || id > d->ids_host[k - 1], "scene_tile_gather: ids[%d] = %d is not above its predecessor", k, id);
    }
    p.ids = d->ids; p.n = d->n; p.tiles = d->tiles;
    if (d->geo && d->coords) { p.geo = d->geo; p.coords = d->coords; }
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int grid = grid_for(int64_t(p.n) * 3 * p.tile * (p.tile / 4));
    if (d->dtype == NIRGAN_SCENE_U16) hipLaunchKernelGGL(scene_tile_gather_kernel<uint16_t>, dim3(grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(scene_tile_gather_kernel<float>, dim3(grid), dim3(256), 0, st, p);
    return nirgan_check_launch("scene_tile_gather");
}

extern "C" int nirgan_scene_finish(const nirgan_scene_predict_desc* d, void* stream) {
    SceneP p;
    if (int e = scene_params(p, d, "scene_finish")) return e;
    NG_REQUIRE(d->blended && d->out, "scene_finish: null pointer (blended or out)");
    NG_REQUIRE(d->out_kind == NIRGAN_SCENE_OUT_U16 || d->out_kind == NIRGAN_SCENE_OUT_F16 || d->out_kind == NIRGAN_SCENE_OUT_F32,
               "scene_finish: unknown out_kind %d", d->out_kind);
    if (d->out_kind == NIRGAN_SCENE_OUT_U16) {
        NG_REQUIRE(d->nodata_out >= 0.0f && d->nodata_out <= 65535.0f && d->nodata_out == float(int(d->nodata_out)),
                   "scene_finish: nodata_out %g is not an integer in 0 .. 65535", double(d->nodata_out));
        p.nodata_q = int(d->nodata_out);
    }
    p.blended = d->blended; p.out = d->out; p.scale = d->scale; p.nodata_out = d->nodata_out;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->dtype == NIRGAN_SCENE_U16) launch_finish<uint16_t>(p, d->out_kind, 2, st);
    else launch_finish<float>(p, d->out_kind, 4, st);
    return nirgan_check_launch("scene_finish");
}
