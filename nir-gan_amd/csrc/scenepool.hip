// The invalid-prefix table of one device-resident scene: nirgan_scene_invalid_prefix.  The entries that draw and cut
// batches from the pool are in scenesample.hip.
//
// The table is built once per scene: a wave scans each row 64 pixels at a time with a carry, then one thread per column runs the sum
// down in place (eight rows of loads in flight).  Integers throughout: exact and order-independent, no atomics.
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
