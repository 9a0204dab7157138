// Dropout (p = 0.5) of the generator's residual blocks as a counter-based mask (include/nirgan_hip.h: nirgan_dropout_desc).
// Philox4x32-10 per channel quad, keyed by the seed, counted by (quad index of the logical tensor, stream id, call): forward and
// backward compute the same bits again, no mask tensor exists.  HBM-bound: ~60 integer operations per 32 bytes moved.
#include "common.h"
#include "philox_dev.h"

namespace {

struct DropP {
    float* buf;
    const uint32_t* state;
    int64_t total;                 // channel quads of the padded grid
    int H, W, hp, wp, q4, pad;
    uint32_t stream_id;
    int sample0;
};

__global__ __launch_bounds__(256) void dropout_halo_kernel(const DropP p) {
    const uint32_t k0 = p.state[0], k1 = p.state[1], call = p.state[2];
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < p.total; i += int64_t(gridDim.x) * blockDim.x) {
        const int cq = int(i % p.q4);
        const int64_t pix = i / p.q4;
        const int x = int(pix % p.wp);
        const int64_t t = pix / p.wp;
        const int y = int(t % p.hp);
        const int64_t b = t / p.hp;
        // the mask of a halo element is that of the interior pixel it reflects
        const int h = ng_reflect(y - p.pad, p.H), w = ng_reflect(x - p.pad, p.W);
        const uint64_t q = (((uint64_t(p.sample0) + uint64_t(b)) * uint64_t(p.H) + uint64_t(h)) * uint64_t(p.W) + uint64_t(w)) * uint64_t(p.q4) + uint64_t(cq);
        uint32_t r[4];
        philox4x32_10(uint32_t(q), uint32_t(q >> 32), p.stream_id, call, k0, k1, r);
        f32x4* e = reinterpret_cast<f32x4*>(p.buf) + i;
        const f32x4 v = *e;
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (r[k] >> 31) ? 2.0f * v[k] : 0.0f;      // a select: a dropped NaN / Inf becomes +0
        *e = o;
    }
}

__global__ void dropout_advance_kernel(uint32_t* state) {
    if (blockIdx.x == 0 && threadIdx.x == 0) state[2] += 1u;
}

}  // namespace

extern "C" int nirgan_dropout_advance(uint32_t* state, void* stream) {
    NG_REQUIRE(state, "dropout_advance: null pointer");
    hipLaunchKernelGGL(dropout_advance_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), state);
    return nirgan_check_launch("dropout_advance");
}

extern "C" int nirgan_dropout_halo(const nirgan_dropout_desc* d, void* stream) {
    NG_REQUIRE(d && d->buf && d->state, "dropout_halo: null pointer");
    NG_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->C >= 4 && d->C % 4 == 0, "dropout_halo: bad shape (C must be a multiple of 4)");
    NG_REQUIRE(d->pad >= 0 && d->pad < (d->H < d->W ? d->H : d->W), "dropout_halo: pad %d outside 0 .. min(H, W) - 1", d->pad);
    NG_REQUIRE(d->sample0 >= 0, "dropout_halo: negative sample0");
    NG_REQUIRE(ng_aligned16(d->buf), "dropout_halo: buf must be 16-byte aligned");
    const int64_t hp = int64_t(d->H) + 2 * d->pad, wp = int64_t(d->W) + 2 * d->pad;
    // (B, hp, wp, C < 2^31 each: the product is taken in steps so that it cannot wrap before the bound is applied)
    const int64_t plane = hp * wp;
    NG_REQUIRE(hp < (int64_t(1) << 31) && wp < (int64_t(1) << 31) && plane < (int64_t(1) << 40) && plane * d->C < (int64_t(1) << 40) && plane * d->C * d->B < (int64_t(1) << 40),
               "dropout_halo: B (H + 2 pad)(W + 2 pad) C must stay below 2^40");
    const int64_t elems = plane * d->C * d->B;
    NG_REQUIRE(d->buf_elems >= elems, "dropout_halo: buf holds %lld floats, %lld needed", (long long)d->buf_elems, (long long)elems);
    DropP p;
    p.buf = d->buf; p.state = d->state; p.total = elems / 4;
    p.H = d->H; p.W = d->W; p.hp = int(hp); p.wp = int(wp); p.q4 = d->C / 4; p.pad = d->pad;
    p.stream_id = d->stream_id; p.sample0 = d->sample0;
    const int64_t g = (p.total + 255) / 256;
    hipLaunchKernelGGL(dropout_halo_kernel, dim3(int(g < 4096 ? g : 4096)), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return nirgan_check_launch("dropout_halo");
}
