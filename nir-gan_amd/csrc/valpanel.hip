// Validation figure panels (the reference's utils/logging_helpers.py: plot_tensors_hist :68-136, plot_index :139-193, and the val_stats
// scalars of model/pix2pix.py:301-309): per tile the 100-bin histograms of the stretched nir / pred over a window, min / max / mean of
// the raw nir / pred over the full tile, the two percentiles of the tile's rgb, and the display planes of both figures.
//
// Four launches, every tile spread over many workgroups (256 threads, four consecutive values per thread and load: 16-byte loads
// where H * W is a multiple of 4 and the planes are 16-byte aligned, guarded scalar loads of the SAME four values otherwise, so the
// association of every sum is the same on both paths):
//   first_pass   grid (ceil(H W / 2048), B): reads nir, pred and rgb ONCE.  Leaves per block {min, max, sum, NaN flag} of nir and of
//                pred in the workspace, the two 100-bin histograms (ds_add_u32 in LDS, merged into the output by integer atomics),
//                the nir / pred / NDVI display planes, and the counts of the first radix digit of the rgb keys.
//   select<1>    grid (ceil(3 H W / 4096), B): every block narrows the first digit itself (2048 counts per tile: cheaper than a launch),
//   select<2>    counts the next digit of the keys that match a selected prefix; the same one digit further.
//   finish       narrows the last digit, interpolates rgb_lo / rgb_hi, block 0 of a tile folds the partials in a fixed order and writes
//                stats, and every block writes its share of rgb_disp.
// Selection: an order-preserving 32-bit key (keys_dev.h), digits of 11 / 11 / 10 bits, so the rgb is read three times for the
// percentiles.  The FOUR ranks of a tile (floor and ceil of q (n - 1) for q and 1 - q) are narrowed together: a rank whose prefix equals
// an earlier rank's shares its histogram slot, ranks that part ways (neighbours in different digits, as with a negative and a positive
// value) get slots of their own, at most four.  Counts are integers, so the selected keys do not depend on the order of arrival.
// Means: a thread adds its 8 values in index order, a wave adds its lanes by the xor butterfly, the four waves are added in a fixed
// order, and the block partials are folded the same way: the association depends on (H, W) only.  No float atomics anywhere.
#include "keys_dev.h"

namespace {

constexpr int THREADS = 256;
constexpr int PPB = 2048;                       // pixels of one tile per block of the first pass (2 x 4 per thread)
constexpr int SPB = 4096;                       // rgb values of one tile per block of a selection pass (4 x 4 per thread)
constexpr int SLOT = 2048;                      // counts of one histogram slot (digits of 11, 11 and 10 bits)
constexpr int BINS = NIRGAN_PANEL_BINS;
// per-tile integer region of the workspace (zeroed by the entry): digit 0 [SLOT], digit 1 [4][SLOT], digit 2 [4][SLOT], then
// {rgb NaN flag, .., state after digit 0 {prefix[4], rank[4]}, state after digit 1}
constexpr int OFF_CNT1 = SLOT, OFF_CNT2 = 5 * SLOT, OFF_FLAG = 9 * SLOT, OFF_ST0 = OFF_FLAG + 8, OFF_ST1 = OFF_FLAG + 16;
constexpr int TILE_INTS = 9 * SLOT + 32;
constexpr int PART = 8;                         // floats per block partial: {min, max, sum, nan} of nir, of pred

struct PanelP {
    const float* rgb; const float* nir; const float* pred;
    int H, W, y0, x0, ch, cw, vec, nblk, clamp_rgb, count_rgb;
    float gain;
    unsigned rank[4];
    double t_lo, t_hi;
    unsigned* ints; float* part;
    int* hist; float* stats;
    float* nir_disp; float* pred_disp; float* ndvi_nir_disp; float* ndvi_pred_disp; float* rgb_disp;
    float edges[BINS + 1];
};

__device__ __forceinline__ float clamp01(float v) {          // a NaN and the sign of a zero pass through, as torch.clamp
    v = v < 0.f ? 0.f : v;
    return v > 1.f ? 1.f : v;
}

__device__ __forceinline__ float ndvi_disp(float n, float r) {
#pragma clang fp contract(off)
    float v = ndvi_value(n, r);
    v = v < -1.f ? -1.f : v;
    v = v > 1.f ? 1.f : v;
    return (v + 1.f) * 0.5f;
}

// values i .. i + 3 of a plane of n values (i a multiple of 4); what lies past n is 0 and ignored by the callers
__device__ __forceinline__ float4 load4(const float* p, int i, int n, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec) {
        if (i < n) v = *reinterpret_cast<const float4*>(p + i);
    } else {
        if (i < n) v.x = p[i];
        if (i + 1 < n) v.y = p[i + 1];
        if (i + 2 < n) v.z = p[i + 2];
        if (i + 3 < n) v.w = p[i + 3];
    }
    return v;
}

// np.histogram's rule on its float32 edges: a guess from the product, corrected against the table
__device__ __forceinline__ int bin_of(float v, const float* edges) {
    int i = int(v * float(BINS));
    i = i < 0 ? 0 : (i > BINS - 1 ? BINS - 1 : i);
    if (v < edges[i]) --i;
    else if (i < BINS - 1 && v >= edges[i + 1]) ++i;
    return i;
}

__global__ __launch_bounds__(THREADS) void first_pass_kernel(const PanelP p) {
    __shared__ unsigned digit[SLOT];
    __shared__ unsigned hist[2 * BINS];
    __shared__ float edges[BINS + 1];
    __shared__ float red[THREADS / 64][PART];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int npx = p.H * p.W;
    for (int i = tid; i < SLOT; i += THREADS) digit[i] = 0;
    if (tid < 2 * BINS) hist[tid] = 0;
    if (tid <= BINS) edges[tid] = p.edges[tid];
    __syncthreads();
    const float* nir = p.nir + size_t(b) * npx;
    const float* pred = p.pred + size_t(b) * npx;
    const float* rgb = p.rgb ? p.rgb + size_t(b) * 3 * npx : nullptr;
    const size_t wbase = size_t(b) * p.ch * p.cw;
    const bool per_pixel_rgb = rgb && (p.count_rgb || p.ndvi_nir_disp || p.ndvi_pred_disp);
    float mn[2] = {INFINITY, INFINITY}, mx[2] = {-INFINITY, -INFINITY}, sm[2] = {0.f, 0.f};
    int nan_n = 0, nan_p = 0, nan_c = 0;
#pragma unroll
    for (int it = 0; it < PPB / (4 * THREADS); ++it) {
        const int i0 = blockIdx.x * PPB + it * 4 * THREADS + 4 * tid;
        const float4 n4 = load4(nir, i0, npx, p.vec), p4 = load4(pred, i0, npx, p.vec);
        float4 r4 = make_float4(0.f, 0.f, 0.f, 0.f), g4 = r4, b4 = r4;
        if (per_pixel_rgb) {
            r4 = load4(rgb, i0, npx, p.vec);
            if (p.count_rgb) { g4 = load4(rgb + npx, i0, npx, p.vec); b4 = load4(rgb + 2 * size_t(npx), i0, npx, p.vec); }
        }
        const float nv[4] = {n4.x, n4.y, n4.z, n4.w}, pv[4] = {p4.x, p4.y, p4.z, p4.w};
        const float rv[4] = {r4.x, r4.y, r4.z, r4.w}, gv[4] = {g4.x, g4.y, g4.z, g4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
        int y = i0 / p.W, x = i0 - y * p.W;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (i0 + e < npx) {
                const float n = nv[e], q = pv[e];
                mn[0] = fminf(mn[0], n); mx[0] = fmaxf(mx[0], n); sm[0] += n; nan_n |= (n != n);
                mn[1] = fminf(mn[1], q); mx[1] = fmaxf(mx[1], q); sm[1] += q; nan_p |= (q != q);
                if (p.count_rgb) {
                    const float c3[3] = {rv[e], gv[e], bv[e]};
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float v = p.clamp_rgb ? clamp01(c3[c]) : c3[c];
                        nan_c |= (v != v);
                        atomicAdd(&digit[key_of(v) >> 21], 1u);
                    }
                }
                const int wy = y - p.y0, wx = x - p.x0;
                if (wy >= 0 && wy < p.ch && wx >= 0 && wx < p.cw) {
                    const size_t o = wbase + size_t(wy) * p.cw + wx;
                    const float vn = clamp01(p.gain * n), vp = clamp01(p.gain * q);
                    if (p.nir_disp) p.nir_disp[o] = vn;
                    if (p.pred_disp) p.pred_disp[o] = vp;
                    if (p.hist) {
                        if (vn == vn) atomicAdd(&hist[bin_of(vn, edges)], 1u);
                        if (vp == vp) atomicAdd(&hist[BINS + bin_of(vp, edges)], 1u);
                    }
                    if (p.ndvi_nir_disp) p.ndvi_nir_disp[o] = ndvi_disp(n, rv[e]);
                    if (p.ndvi_pred_disp) p.ndvi_pred_disp[o] = ndvi_disp(q, rv[e]);
                }
            }
            if (++x == p.W) { x = 0; ++y; }
        }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[q] = fminf(mn[q], __shfl_xor(mn[q], o, 64));
            mx[q] = fmaxf(mx[q], __shfl_xor(mx[q], o, 64));
        }
        sm[q] = ng_wave_sum(sm[q]);
    }
    nan_n = __any(nan_n); nan_p = __any(nan_p); nan_c = __any(nan_c);
    if ((tid & 63) == 0) {
        float* r = red[tid >> 6];
        r[0] = mn[0]; r[1] = mx[0]; r[2] = sm[0]; r[3] = nan_n ? 1.f : 0.f;
        r[4] = mn[1]; r[5] = mx[1]; r[6] = sm[1]; r[7] = nan_p ? 1.f : 0.f;
        if (nan_c) atomicOr(&p.ints[size_t(b) * TILE_INTS + OFF_FLAG], 1u);
    }
    __syncthreads();
    if (tid < PART) {
        const float a = red[0][tid], c = red[1][tid], d = red[2][tid], f = red[3][tid];
        const int kind = tid & 3;
        float v;
        if (kind == 0) v = fminf(fminf(a, c), fminf(d, f));
        else if (kind == 1) v = fmaxf(fmaxf(a, c), fmaxf(d, f));
        else v = (a + c) + (d + f);
        p.part[(size_t(b) * p.nblk + blockIdx.x) * PART + tid] = v;
    }
    if (p.hist && tid < 2 * BINS && hist[tid]) atomicAdd(&p.hist[size_t(b) * 2 * BINS + tid], int(hist[tid]));
    if (p.count_rgb) {
        unsigned* cnt = p.ints + size_t(b) * TILE_INTS;
        for (int i = tid; i < SLOT; i += THREADS)
            if (digit[i]) atomicAdd(&cnt[i], digit[i]);
    }
}

// One digit of the four selections of a tile, by the whole block.  in / out (LDS, distinct): [0..3] the key prefix selected so far,
// [4..7] the rank among the keys that carry it.  cnt: the tile's counts of this digit, one slot of SLOT per DISTINCT prefix, the slot of
// a prefix being the first rank that has it.  Ends with a barrier.
template <int NBINS, int BITS>
__device__ __forceinline__ void narrow(const unsigned* cnt, const unsigned* in, unsigned* out, unsigned* wsum) {
    constexpr int PER = NBINS / THREADS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
        int s = j;
        for (int i = j - 1; i >= 0; --i)
            if (in[i] == in[j]) s = i;
        const unsigned k = in[4 + j];
        const uint4* c = reinterpret_cast<const uint4*>(cnt + s * SLOT + tid * PER);
        unsigned h[PER], own = 0;
#pragma unroll
        for (int e = 0; e < PER / 4; ++e) {
            const uint4 q = c[e];
            h[4 * e] = q.x; h[4 * e + 1] = q.y; h[4 * e + 2] = q.z; h[4 * e + 3] = q.w;
            own += (q.x + q.y) + (q.z + q.w);
        }
        unsigned inc = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        for (int w = 0; w < wave; ++w) inc += wsum[w];
        const unsigned exc = inc - own;
        if (k >= exc && k < inc) {                                    // exactly one thread: the counts add up to more than k
            unsigned r = k - exc;
            int bin = 0;
            bool done = false;
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                if (!done) {
                    if (r < h[e]) { done = true; bin = e; }
                    else r -= h[e];
                }
            }
            out[j] = (in[j] << BITS) | unsigned(tid * PER + bin);
            out[4 + j] = r;
        }
        __syncthreads();
    }
}

// LEVEL 1: narrows digit 0 (key bits 31..21), counts digit 1 (bits 20..10); LEVEL 2: narrows digit 1, counts digit 2 (bits 9..0)
template <int LEVEL>
__global__ __launch_bounds__(THREADS) void select_kernel(const PanelP p) {
    constexpr int NB = LEVEL == 1 ? 2048 : 1024;
    constexpr int SHIFT = LEVEL == 1 ? 21 : 10;
    __shared__ unsigned hist[4][NB];
    __shared__ unsigned st_in[8], st_out[8], wsum[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    unsigned* ints = p.ints + size_t(b) * TILE_INTS;
    if (tid < 8) st_in[tid] = LEVEL == 1 ? (tid < 4 ? 0u : p.rank[tid - 4]) : ints[OFF_ST0 + tid];
    for (int i = tid; i < 4 * NB; i += THREADS) (&hist[0][0])[i] = 0;
    __syncthreads();
    narrow<2048, 11>(ints + (LEVEL == 1 ? 0 : OFF_CNT1), st_in, st_out, wsum);
    if (blockIdx.x == 0 && tid < 8) ints[(LEVEL == 1 ? OFF_ST0 : OFF_ST1) + tid] = st_out[tid];
    const unsigned p0 = st_out[0], p1 = st_out[1], p2 = st_out[2], p3 = st_out[3];
    const bool u1 = p1 != p0, u2 = p2 != p1 && p2 != p0, u3 = p3 != p2 && p3 != p1 && p3 != p0;      // first rank with its prefix
    const int n = 3 * p.H * p.W;
    const float* rgb = p.rgb + size_t(b) * n;
#pragma unroll
    for (int it = 0; it < SPB / (4 * THREADS); ++it) {
        const int i0 = blockIdx.x * SPB + it * 4 * THREADS + 4 * tid;
        const float4 v4 = load4(rgb, i0, n, p.vec);
        const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (i0 + e < n) {
                const unsigned key = key_of(p.clamp_rgb ? clamp01(vv[e]) : vv[e]);
                const unsigned pre = key >> SHIFT, d = (key >> (SHIFT - (LEVEL == 1 ? 11 : 10))) & (NB - 1);
                if (pre == p0) atomicAdd(&hist[0][d], 1u);
                else if (u1 && pre == p1) atomicAdd(&hist[1][d], 1u);
                else if (u2 && pre == p2) atomicAdd(&hist[2][d], 1u);
                else if (u3 && pre == p3) atomicAdd(&hist[3][d], 1u);
            }
        }
    }
    __syncthreads();
    unsigned* cnt = ints + (LEVEL == 1 ? OFF_CNT1 : OFF_CNT2);
    for (int i = tid; i < 4 * NB; i += THREADS) {
        const unsigned c = (&hist[0][0])[i];
        if (c) atomicAdd(&cnt[(i / NB) * SLOT + (i % NB)], c);
    }
}

__global__ __launch_bounds__(THREADS) void finish_kernel(const PanelP p) {
    __shared__ unsigned st_in[8], st_out[8], wsum[4];
    __shared__ float red[THREADS / 64][PART];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int npx = p.H * p.W;
    unsigned* ints = p.ints + size_t(b) * TILE_INTS;
    float lo = 0.f, hi = 0.f;
    if (p.count_rgb) {
        if (tid < 8) st_in[tid] = ints[OFF_ST1 + tid];
        __syncthreads();
        narrow<1024, 10>(ints + OFF_CNT2, st_in, st_out, wsum);
        if (ints[OFF_FLAG]) {
            lo = hi = __uint_as_float(0x7fc00000u);
        } else {
            // torch.quantile's lerp: a + t (b - a), from the far end for t >= 0.5 (the same number; it decides what an infinite
            // neighbour gives), in double, rounded once
            const double a0 = value_of(st_out[0]), b0 = value_of(st_out[1]), a1 = value_of(st_out[2]), b1 = value_of(st_out[3]);
            lo = float(p.t_lo < 0.5 ? a0 + p.t_lo * (b0 - a0) : b0 - (b0 - a0) * (1.0 - p.t_lo));
            hi = float(p.t_hi < 0.5 ? a1 + p.t_hi * (b1 - a1) : b1 - (b1 - a1) * (1.0 - p.t_hi));
        }
    }
    if (blockIdx.x == 0 && p.stats) {
        float acc[PART];
#pragma unroll
        for (int v = 0; v < PART; ++v) acc[v] = (v & 3) == 0 ? INFINITY : ((v & 3) == 1 ? -INFINITY : 0.f);
        for (int i = tid; i < p.nblk; i += THREADS) {
            const float4* q = reinterpret_cast<const float4*>(p.part + (size_t(b) * p.nblk + i) * PART);
            const float4 u = q[0], w = q[1];
            acc[0] = fminf(acc[0], u.x); acc[1] = fmaxf(acc[1], u.y); acc[2] += u.z; acc[3] = fmaxf(acc[3], u.w);
            acc[4] = fminf(acc[4], w.x); acc[5] = fmaxf(acc[5], w.y); acc[6] += w.z; acc[7] = fmaxf(acc[7], w.w);
        }
#pragma unroll
        for (int v = 0; v < PART; ++v) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float other = __shfl_xor(acc[v], o, 64);
                acc[v] = (v & 3) == 0 ? fminf(acc[v], other) : ((v & 3) == 2 ? acc[v] + other : fmaxf(acc[v], other));
            }
            if ((tid & 63) == 0) red[tid >> 6][v] = acc[v];
        }
        __syncthreads();
        if (tid < 2) {
            const int o = 4 * tid;
            const float nan = fmaxf(fmaxf(red[0][o + 3], red[1][o + 3]), fmaxf(red[2][o + 3], red[3][o + 3]));
            const float qnan = __uint_as_float(0x7fc00000u);
            float* row = p.stats + size_t(b) * NIRGAN_PANEL_STAT_COLS + 3 * tid;
            row[0] = nan > 0.f ? qnan : fminf(fminf(red[0][o], red[1][o]), fminf(red[2][o], red[3][o]));
            row[1] = nan > 0.f ? qnan : fmaxf(fmaxf(red[0][o + 1], red[1][o + 1]), fmaxf(red[2][o + 1], red[3][o + 1]));
            row[2] = nan > 0.f ? qnan : __fdiv_rn((red[0][o + 2] + red[1][o + 2]) + (red[2][o + 2] + red[3][o + 2]), float(npx));
        }
        if (tid == 2 && p.count_rgb) {
            p.stats[size_t(b) * NIRGAN_PANEL_STAT_COLS + 6] = lo;
            p.stats[size_t(b) * NIRGAN_PANEL_STAT_COLS + 7] = hi;
        }
    }
    if (!p.rgb_disp) return;
    const int nw = p.ch * p.cw;
    const float* rgb = p.rgb + size_t(b) * 3 * npx + size_t(p.y0) * p.W + p.x0;
    float* out = p.rgb_disp + size_t(b) * nw * 3;
    const float span = hi - lo;
    for (int i = blockIdx.x * THREADS + tid; i < nw; i += gridDim.x * THREADS) {
        const int y = i / p.cw, x = i - y * p.cw;
        const size_t o = size_t(y) * p.W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = rgb[o + size_t(c) * npx];
            if (p.clamp_rgb) v = clamp01(v);
            out[size_t(i) * 3 + c] = hi == lo ? 0.f : clamp01(__fdiv_rn(v - lo, span));
        }
    }
}

}  // namespace

extern "C" int64_t nirgan_val_panel_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || int64_t(B) * 3 * H * W >= (int64_t(1) << 31)) return 0;
    const int64_t nblk = (int64_t(H) * W + PPB - 1) / PPB;
    return int64_t(B) * TILE_INTS * 4 + int64_t(B) * nblk * PART * 4;
}

extern "C" int nirgan_val_panel(const nirgan_val_panel_desc* d, void* stream) {
    NG_REQUIRE(d != nullptr && d->nir && d->pred, "val_panel: null pointer (nir and pred are required)");
    NG_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0, "val_panel: empty problem B=%d H=%d W=%d", d->B, d->H, d->W);
    NG_REQUIRE(d->ch > 0 && d->cw > 0, "val_panel: window extent %dx%d must be positive", d->ch, d->cw);
    NG_REQUIRE(d->y0 >= 0 && d->x0 >= 0 && d->ch <= d->H - d->y0 && d->cw <= d->W - d->x0,
               "val_panel: window y0=%d x0=%d %dx%d outside the %dx%d image", d->y0, d->x0, d->ch, d->cw, d->H, d->W);
    NG_REQUIRE(int64_t(d->B) * 3 * d->H * d->W < (int64_t(1) << 31), "val_panel: batch too large (B*3*H*W must stay below 2^31)");
    NG_REQUIRE(d->B <= 65535, "val_panel: B=%d exceeds 65535 tiles per call", d->B);
    NG_REQUIRE(d->perc >= 0.f && d->perc < 50.f, "val_panel: perc=%g must lie in [0, 50)", double(d->perc));
    NG_REQUIRE(d->rgb || !(d->ndvi_nir_disp || d->ndvi_pred_disp || d->rgb_disp), "val_panel: the NDVI and rgb display planes need rgb");
    NG_REQUIRE(d->ws && d->ws_bytes >= nirgan_val_panel_ws_bytes(d->B, d->H, d->W), "val_panel: workspace too small (%lld < %lld bytes)",
               (long long)d->ws_bytes, (long long)nirgan_val_panel_ws_bytes(d->B, d->H, d->W));
    NG_REQUIRE(ng_aligned16(d->ws), "val_panel: workspace must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t npx = int64_t(d->H) * d->W;
    PanelP p;
    p.rgb = d->rgb; p.nir = d->nir; p.pred = d->pred;
    p.H = d->H; p.W = d->W; p.y0 = d->y0; p.x0 = d->x0; p.ch = d->ch; p.cw = d->cw;
    p.vec = npx % 4 == 0 && ng_aligned16(d->nir) && ng_aligned16(d->pred) && (!d->rgb || ng_aligned16(d->rgb));
    p.nblk = int((npx + PPB - 1) / PPB);
    p.clamp_rgb = d->clamp_rgb != 0;
    p.count_rgb = d->rgb && (d->stats || d->rgb_disp);
    p.gain = d->gain;
    // torch.quantile: pos = q (n - 1), the order statistics of rank floor(pos) and ceil(pos), weight pos - floor(pos)
    const double n1 = double(3 * npx - 1), q = double(d->perc) / 100.0, pos[2] = {q * n1, (100.0 - double(d->perc)) / 100.0 * n1};
    double t[2];
    for (int i = 0; i < 2; ++i) {
        double lo = floor(pos[i]), hi = ceil(pos[i]);
        lo = lo < 0 ? 0 : (lo > n1 ? n1 : lo);
        hi = hi < 0 ? 0 : (hi > n1 ? n1 : hi);
        p.rank[2 * i] = unsigned(lo); p.rank[2 * i + 1] = unsigned(hi);
        t[i] = pos[i] - lo;
    }
    p.t_lo = t[0]; p.t_hi = t[1];
    p.ints = static_cast<unsigned*>(d->ws);
    p.part = reinterpret_cast<float*>(p.ints + size_t(d->B) * TILE_INTS);
    p.hist = d->hist; p.stats = d->stats;
    p.nir_disp = d->nir_disp; p.pred_disp = d->pred_disp; p.ndvi_nir_disp = d->ndvi_nir_disp; p.ndvi_pred_disp = d->ndvi_pred_disp;
    p.rgb_disp = d->rgb_disp;
    // np.linspace(0, 1, 101, dtype=float32): arange * (1 / 100) in double, the last edge set to 1, rounded to float
    for (int i = 0; i <= BINS; ++i) p.edges[i] = float(double(i) * (1.0 / double(BINS)));
    p.edges[BINS] = 1.f;

    if (hipMemsetAsync(p.ints, 0, size_t(d->B) * TILE_INTS * 4, st) != hipSuccess) return nirgan_check_launch("val_panel");
    if (d->hist && hipMemsetAsync(d->hist, 0, size_t(d->B) * 2 * BINS * 4, st) != hipSuccess) return nirgan_check_launch("val_panel");
    hipLaunchKernelGGL(first_pass_kernel, dim3(unsigned(p.nblk), unsigned(d->B)), dim3(THREADS), 0, st, p);
    if (p.count_rgb) {
        const unsigned sblk = unsigned((3 * npx + SPB - 1) / SPB);
        hipLaunchKernelGGL(select_kernel<1>, dim3(sblk, unsigned(d->B)), dim3(THREADS), 0, st, p);
        hipLaunchKernelGGL(select_kernel<2>, dim3(sblk, unsigned(d->B)), dim3(THREADS), 0, st, p);
    }
    if (d->stats || d->rgb_disp) {
        const int64_t nw = int64_t(d->ch) * d->cw;
        const unsigned fblk = d->rgb_disp ? unsigned((nw + 4 * THREADS - 1) / (4 * THREADS)) : 1u;
        hipLaunchKernelGGL(finish_kernel, dim3(fblk, unsigned(d->B)), dim3(THREADS), 0, st, p);
    }
    return nirgan_check_launch("val_panel");
}
