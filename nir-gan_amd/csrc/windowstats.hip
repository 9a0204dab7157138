// Window statistics of a date stack (the reference's NDVI time series, validation_utils/time_series_validation.py:120-132 and :243-266):
// per tile the mean and the MEDIAN, over one window inside the stored images, of nir, pred, ndvi(nir) and ndvi(pred).
//
// One workgroup per (tile, quantity), one launch, no workspace.  The median is exact selection by radix, nothing is sorted: every
// value becomes an order-preserving 32-bit key (sign bit flipped for positive floats, all bits for negative ones), four passes of
// 8 bits each count the keys that still match the selected prefix into a 256-bin integer histogram in LDS, the first wave scans the
// bins and narrows (prefix, rank).  Integer LDS atomics commute, so the selected key -- from which the float is rebuilt -- does not
// depend on the order of arrival.  The rank is (n - 1) / 2: the LOWER middle value of an even count, as torch.median; a NaN anywhere
// in the window gives NaN.
//
// A window of up to STAGE = 4096 values (the reference's 64 x 64 plot crop is its largest) is read from memory ONCE: the pass that
// sums the mean leaves the keys in LDS and the four selection passes read LDS.  A larger window is re-read from memory in every pass
// and its NDVI value recomputed.  That value is bit-identical in every pass because it comes from ONE __device__ function,
// ndvi_value (keys_dev.h).
//
// Means: thread t adds values t, t + 256, ... in order, a wave adds its lanes by the xor butterfly, the four waves are added in a
// fixed order.  The association depends on (wh, ww) only: a tile's row is bitwise the same alone and inside any stack; no float atomics.
#include "keys_dev.h"

namespace {

constexpr int THREADS = 256;
constexpr int STAGE = 4096;                    // keys staged in LDS (16 KB)
constexpr int BINS = 256;

struct WinP {
    const float* rgb; const float* nir; const float* pred;
    int H, W, y0, x0, wh, ww, nq;
    float* rows;
};

// value i (row-major inside the window) of this block's quantity; src / red point at the tile's planes, at the window's origin
__device__ __forceinline__ float value_at(const float* src, const float* red, int W, int ww, int i) {
    const int y = i / ww, x = i - y * ww;
    const size_t o = size_t(y) * W + x;
    const float v = src[o];
    return red ? ndvi_value(v, red[o]) : v;
}

__global__ __launch_bounds__(THREADS) void window_stats_kernel(const WinP p) {
    __shared__ unsigned keys[STAGE];
    __shared__ __attribute__((aligned(16))) unsigned hist[BINS];
    __shared__ float red_sum[THREADS / 64];
    __shared__ unsigned sel[2];
    const int tid = threadIdx.x;
    const int q = blockIdx.x % p.nq, t = blockIdx.x / p.nq;          // quantity: 0 nir, 1 pred, 2 ndvi(nir), 3 ndvi(pred)
    const size_t plane = size_t(p.H) * p.W, origin = size_t(p.y0) * p.W + p.x0;
    const float* src = ((q & 1) ? p.pred : p.nir) + size_t(t) * plane + origin;
    const float* red = q >= 2 ? p.rgb + size_t(t) * 3 * plane + origin : nullptr;
    const int n = p.wh * p.ww;
    const bool staged = n <= STAGE;

    float sum = 0.f;
    int nan = 0;
    for (int i = tid; i < n; i += THREADS) {
        const float v = value_at(src, red, p.W, p.ww, i);
        sum += v;
        nan |= (v != v);
        if (staged) keys[i] = key_of(v);
    }
    sum = ng_wave_sum(sum);
    if ((tid & 63) == 0) red_sum[tid >> 6] = sum;
    nan = __syncthreads_or(nan);                                      // also orders the staged keys and red_sum
    float* row = p.rows + size_t(t) * NIRGAN_WINDOW_STAT_COLS + 2 * q;
    if (tid == 0) row[0] = ((red_sum[0] + red_sum[1]) + (red_sum[2] + red_sum[3])) / float(n);
    if (nan) {
        if (tid == 0) row[1] = __uint_as_float(0x7fc00000u);
        return;
    }

    unsigned prefix = 0, k = unsigned(n - 1) >> 1;                    // keys that match `prefix` above the pass's byte; rank among them
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += THREADS) {
            const unsigned key = staged ? keys[i] : key_of(value_at(src, red, p.W, p.ww, i));
            if (shift == 24 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & (BINS - 1)], 1u);
        }
        __syncthreads();
        if (tid < 64) {                                               // lane l owns bins 4 l .. 4 l + 3
            const uint4 h = *reinterpret_cast<const uint4*>(&hist[4 * tid]);
            const unsigned s = h.x + h.y + h.z + h.w;
            unsigned inc = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned up = __shfl_up(inc, o, 64);
                if (tid >= o) inc += up;
            }
            const unsigned exc = inc - s;
            if (k >= exc && k < inc) {                                // exactly one lane: the counts add up to more than k
                unsigned r = k - exc, b = 4 * tid;
                if (r >= h.x) { r -= h.x; ++b; if (r >= h.y) { r -= h.y; ++b; if (r >= h.z) { r -= h.z; ++b; } } }
                sel[0] = b; sel[1] = r;
            }
        }
        __syncthreads();
        prefix = (prefix << 8) | sel[0];
        k = sel[1];
    }
    if (tid == 0) row[1] = value_of(prefix);
}

}  // namespace

extern "C" int nirgan_window_stats(const nirgan_window_stats_desc* d, void* stream) {
    NG_REQUIRE(d != nullptr && d->nir && d->pred && d->rows, "window_stats: null pointer");
    NG_REQUIRE(d->T > 0 && d->H > 0 && d->W > 0, "window_stats: empty problem");
    NG_REQUIRE(d->wh > 0 && d->ww > 0, "window_stats: window extent %dx%d must be positive", d->wh, d->ww);
    NG_REQUIRE(d->y0 >= 0 && d->x0 >= 0 && d->wh <= d->H - d->y0 && d->ww <= d->W - d->x0,
               "window_stats: window y0=%d x0=%d %dx%d outside the %dx%d image", d->y0, d->x0, d->wh, d->ww, d->H, d->W);
    NG_REQUIRE(int64_t(d->H) * d->W < (int64_t(1) << 31), "window_stats: image too large");
    const int nq = d->rgb ? 4 : 2;
    NG_REQUIRE(int64_t(d->T) * nq < (int64_t(1) << 31), "window_stats: too many tiles");
    WinP p;
    p.rgb = d->rgb; p.nir = d->nir; p.pred = d->pred;
    p.H = d->H; p.W = d->W; p.y0 = d->y0; p.x0 = d->x0; p.wh = d->wh; p.ww = d->ww; p.nq = nq;
    p.rows = d->rows;
    hipLaunchKernelGGL(window_stats_kernel, dim3(unsigned(d->T * nq)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), p);
    return nirgan_check_launch("window_stats");
}
