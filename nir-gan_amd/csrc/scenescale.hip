// Multi-scale training batches from device-resident scenes: nirgan_scene_sample_scaled; and the same gather on a list
// of windows the caller names: nirgan_scene_gather; and the draw from a table of rectangles of window origins with the
// same gather behind it: nirgan_scene_sample_origins, at the end of the file.
//
// The draw of scenepool.hip with one more decision: sample b takes its resolution factor f from the fourth Philox word of attempt 0,
// cuts a window of side L = f * T and delivers the T x T tile of the means of its f x f blocks.  Two launches, as there:
//   draw    one thread per sample; the attempts run on the table of the drawn scale and accept n <= max_invalid * f * f;
//   gather  one 256-thread block per 64 x 64 block of D, the T x T mean image of one plane BEFORE the view, grid-strided.  A wave owns
//           D row p (16 rows per wave and block).  It reads the f source rows p*f .. p*f + f-1 with the lanes ALONG the source row:
//           f chunks of 64 consecutive elements per row, one element per lane, every source element fetched once.  The loads are
//           unconditional (a lane past the block reads the block's last element and drops it), so the compiler can issue those of
//           up to four rows of D, at most 64 per lane, before the first is used.
//             uint16: each lane adds its f rows up in int32 registers first (f column sums per lane), then the wave puts the 64 f
//                     column sums into its own LDS strip and lane q adds the f sums of D column q: at most 64 * 65535 < 2^24.
//             float:  the contract fixes the ORDER of the float64 sum (row-major over the block), so a lane cannot add rows up
//                     before the columns are joined; the wave sends each source row through the strip in turn and lane q adds its
//                     f values into one float64 accumulator, row after row.
//           The strip is PERMUTED: the sum of source column c = q*f + e lives at [e][q], rows of LDQ = 64 + ceil(32 / f) dwords.
//           Lane q then reads [e][q] for e = 0 .. f-1, stride 1 across the lanes (no conflict at any f; f consecutive dwords per lane
//           would be f-way for even f).  The store of a 32-lane group covers f rows of ~32 / f consecutive q whose bank offsets
//           e * LDQ mod 32 = e * ceil(32 / f) tile the 32 banks: free of conflicts for f = 2, 4, 8, at most 2-way for the others,
//           which costs a dword store nothing.  A strip belongs to ONE wave, so a wave-level barrier orders it, not __syncthreads.
//           Plain views (0 .. 3) store from the registers, lane q -> output column q or T-1-q: 256 contiguous bytes per wave either
//           way.  Transposing views (4 .. 7) turn the block in the 64 x 65 padded LDS block of scenepool.hip.
//           f is uniform per block (one sample per block) and selects a template instance: the f x f loops unroll, nothing is
//           indexed dynamically, no scratch.  The kernel comes in two widths, factors to 4 and factors to 8, picked by the call's
//           largest factor.  Every output element has one owner, stores are one dword per lane, no atomics.
#include <type_traits>

#include "scene_dev.h"

namespace {

constexpr int MAXK = NIRGAN_SCENE_MAX_SCALES;
constexpr int MAXF = NIRGAN_SCENE_MAX_FACTOR;
constexpr int strip_ld(int F) { return SP_B + (32 + F - 1) / F; }
constexpr int STRIP = MAXF * strip_ld(MAXF);                                    // the largest F * strip_ld(F) over F = 2 .. 8
static_assert(2 * strip_ld(2) <= STRIP && 3 * strip_ld(3) <= STRIP && 4 * strip_ld(4) <= STRIP && 5 * strip_ld(5) <= STRIP &&
              6 * strip_ld(6) <= STRIP && 7 * strip_ld(7) <= STRIP, "strip too small");

struct ScaledP {
    const void* pool;
    const int64_t* table;                // [K][S][TC]
    const int32_t* prefix;
    const double* geo;
    int64_t total[MAXK];                 // windows of the whole pool at scale k
    int64_t band[4];
    int factor[MAXK];
    uint32_t cumw[MAXK], wtot;           // running weights; cumw[K-1] = wtot < 2^32
    int K, S, T, B, views, max_invalid, nb;
    int64_t nblk;                        // B * 4 * nb * nb
    float divisor;
    uint32_t seed_lo, seed_hi, draw_lo, draw_hi, sample0;
    float* rgb; float* nir; float* coords;
    int32_t* window;                     // written by the draw
    const int32_t* rows;                 // read by the gather: the draw's window, or the caller's list (nirgan_scene_gather)
};

__global__ __launch_bounds__(256) void scene_scaled_draw_kernel(const ScaledP p) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    uint32_t w[4];
    philox4x32_10(p.draw_lo, p.draw_hi, p.sample0 + uint32_t(b), 0u, p.seed_lo, p.seed_hi, w);
    const uint32_t pick = uint32_t((uint64_t(w[3]) * uint64_t(p.wtot)) >> 32);             // floor(w3 * Wtot / 2^32) < Wtot
    int k = 0, f = p.factor[0];
    int64_t total = p.total[0];
#pragma unroll
    for (int j = 1; j < MAXK; ++j)       // cumw rises: the last j with cumw[j-1] <= pick is the first with cumw[j] > pick
        if (j < p.K && p.cumw[j - 1] <= pick) { k = j; f = p.factor[j]; total = p.total[j]; }
    const int L = f * p.T;
    const int64_t* __restrict__ table = p.table + int64_t(k) * p.S * TC;
    const int64_t most = int64_t(p.max_invalid) * f * f;
    int s = 0, y0 = 0, x0 = 0, view = 0, a = 0;
    bool ok = false;
    for (; a < NIRGAN_SCENE_ATTEMPTS; ++a) {
        if (a > 0) philox4x32_10(p.draw_lo, p.draw_hi, p.sample0 + uint32_t(b), uint32_t(a), p.seed_lo, p.seed_hi, w);
        const int64_t n = sp_attempt(w, table, p.prefix, p.S, L, total, p.views, s, y0, x0, view);
        if (n <= most) { ok = true; break; }
    }
    if (!ok) a = NIRGAN_SCENE_ATTEMPTS - 1;
    int32_t* __restrict__ o = p.window + int64_t(b) * 4;
    o[0] = s; o[1] = y0; o[2] = x0;
    o[3] = int32_t(uint32_t(view) | (uint32_t(a) << 8) | (uint32_t(f - 1) << 16) | (ok ? 0u : 0x80000000u));
    if (p.geo && p.coords) sp_centre(p.geo + int64_t(s) * 4, y0, x0, L, p.coords + int64_t(b) * 2);
}

// orders the LDS traffic of ONE wave: what its lanes stored before is what its lanes load after
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float block_mean(int sum, int ff) { return __fdiv_rn(float(sum), float(ff)); }
__device__ __forceinline__ float block_mean(double sum, int ff) { return float(sum / double(ff)); }

// one 64 x 64 block of D at (dr0, dc0); src: the window's corner in the plane; W: the scene's width; strip: this wave's
template <typename T, int F>
__device__ __forceinline__ void gather_block(const T* __restrict__ src, int64_t W, float* __restrict__ out, int Tt, int view, int dr0, int dc0,
                                             float divisor, float* __restrict__ tile, int* __restrict__ strip) {
    constexpr int LDQ = strip_ld(F);
    constexpr bool INTS = sizeof(T) == 2;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const int nc = Tt - dc0 < SP_B ? Tt - dc0 : SP_B;                           // D columns of this block
    const int ncf = nc * F;                                                     // source columns of this block
    const int q = dc0 + lx, qo = (view & 1) ? Tt - 1 - q : q;                   // this lane's D column and where the view puts it
    // U rows of D per step: their U * F * F loads are issued before the first is used (a wave has nothing else to wait behind)
    constexpr int U = INTS ? (F <= 4 ? 4 : F <= 6 ? 2 : 1) : (F <= 2 ? 4 : F <= 4 ? 2 : 1);
#pragma unroll 1
    for (int k0 = 0; k0 < 16; k0 += U) {
        if (dr0 + ly + 4 * k0 >= Tt) break;                                     // wave-uniform, as every p below
        typename std::conditional<INTS, int, float>::type x[U][INTS ? 1 : F][F];   // uint16: the column sums of the F rows; float: the values
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // a row past the tile or a column past the block reads the last one instead: inside the window, never used, and the
            // loads stay unconditional, so all of them are in flight before the first wait
            const int p = dr0 + ly + 4 * (k0 + u);
            const T* __restrict__ rows = src + int64_t(p < Tt ? p : Tt - 1) * F * W + int64_t(dc0) * F;
#pragma unroll
            for (int m = 0; m < F; ++m) {
                const int c = lx + 64 * m < ncf ? lx + 64 * m : ncf - 1;
                if constexpr (INTS) x[u][0][m] = 0;
#pragma unroll
                for (int rr = 0; rr < F; ++rr) {
                    if constexpr (INTS) x[u][0][m] += int(rows[rr * W + c]);
                    else x[u][rr][m] = rows[rr * W + c];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int pl = ly + 4 * (k0 + u), p = dr0 + pl;
            if (p >= Tt) break;
            typename std::conditional<INTS, int, double>::type sum = x[u][0][0];
            if constexpr (F > 1) {
#pragma unroll
                for (int rr = 0; rr < (INTS ? 1 : F); ++rr) {                   // float: row-major over the block, from its first value
#pragma unroll
                    for (int m = 0; m < F; ++m) {
                        const int c = lx + 64 * m;
                        if (c < ncf) {
                            if constexpr (INTS) strip[(c % F) * LDQ + c / F] = x[u][0][m];
                            else strip[(c % F) * LDQ + c / F] = __float_as_int(x[u][rr][m]);
                        }
                    }
                    wave_sync();
                    if (lx < nc) {
#pragma unroll
                        for (int e = 0; e < F; ++e) {
                            if constexpr (INTS) sum = e == 0 ? strip[lx] : sum + strip[e * LDQ + lx];
                            else {
                                const double x1 = double(__int_as_float(strip[e * LDQ + lx]));
                                sum = (rr == 0 && e == 0) ? x1 : sum + x1;
                            }
                        }
                    }
                    wave_sync();                                                // the next row stores into the strip again
                }
            }
            const float v = __fdiv_rn(block_mean(sum, F * F), divisor);
            if (lx < nc) {
                if (!(view & 4)) out[int64_t((view & 2) ? Tt - 1 - p : p) * Tt + qo] = v;
                else tile[pl * SP_LD + lx] = v;
            }
        }
    }
    if (view & 4) {
        // out[i][j] = D[f2(j)][f1(i)]: the lanes run along j, which is D's row
        __syncthreads();
        const int p = dr0 + lx, j = (view & 2) ? Tt - 1 - p : p;
        if (p < Tt) {
#pragma unroll 4
            for (int k = 0; k < 16; ++k) {
                const int ql = ly + 4 * k, qq = dc0 + ql;
                if (qq < Tt) out[int64_t((view & 1) ? Tt - 1 - qq : qq) * Tt + j] = tile[lx * SP_LD + ql];
            }
        }
        __syncthreads();                                                        // the next block of the grid-stride loop writes tile again
    }
}

// FMAX: the largest factor this instance holds code for (4 or 8).  The registers of a kernel are those of its widest case, so a call
// whose factors stop at 4 -- the usual one -- runs the instance that stops there, at 4 waves per SIMD instead of 3.
template <typename T, int FMAX>
__global__ __launch_bounds__(256) void scene_scaled_gather_kernel(const ScaledP p) {
    __shared__ float tile[SP_B * SP_LD];
    __shared__ int strips[4 * STRIP];
    const T* __restrict__ pool = static_cast<const T*>(p.pool);
    int* __restrict__ strip = strips + (threadIdx.x >> 6) * STRIP;
    const int Tt = p.T;
    const int64_t tt = int64_t(Tt) * Tt;
    for (int64_t blk = blockIdx.x; blk < p.nblk; blk += gridDim.x) {
        const int dc0 = int(blk % p.nb) * SP_B;
        int64_t q = blk / p.nb;
        const int dr0 = int(q % p.nb) * SP_B;
        q /= p.nb;
        const int ch = int(q & 3);
        const int64_t b = q >> 2;
        const int32_t* __restrict__ win = p.rows + b * 4;
        const int s = win[0], y0 = win[1], x0 = win[2], view = win[3] & 7, f = ((win[3] >> 16) & 7) + 1;
        int k = 0;
#pragma unroll
        for (int j = 1; j < MAXK; ++j)
            if (j < p.K && p.factor[j] == f) k = j;
        const int64_t* __restrict__ row = p.table + (int64_t(k) * p.S + s) * TC;
        const int64_t W = row[2];
        const T* __restrict__ src = pool + row[0] + p.band[ch] * row[1] * W + int64_t(y0) * W + x0;       // the window's corner
        float* __restrict__ out = ch < 3 ? p.rgb + (b * 3 + ch) * tt : p.nir + b * tt;
        switch (f) {                                                            // uniform over the block
            case 1: gather_block<T, 1>(src, W, out, Tt, view, dr0, dc0, p.divisor, tile, strip); break;
            case 2: gather_block<T, 2>(src, W, out, Tt, view, dr0, dc0, p.divisor, tile, strip); break;
            case 3: gather_block<T, 3>(src, W, out, Tt, view, dr0, dc0, p.divisor, tile, strip); break;
            case 4: gather_block<T, 4>(src, W, out, Tt, view, dr0, dc0, p.divisor, tile, strip); break;
            default:
                if constexpr (FMAX > 4) {
                    switch (f) {
                        case 5: gather_block<T, 5>(src, W, out, Tt, view, dr0, dc0, p.divisor, tile, strip); break;
                        case 6: gather_block<T, 6>(src, W, out, Tt, view, dr0, dc0, p.divisor, tile, strip); break;
                        case 7: gather_block<T, 7>(src, W, out, Tt, view, dr0, dc0, p.divisor, tile, strip); break;
                        default: gather_block<T, 8>(src, W, out, Tt, view, dr0, dc0, p.divisor, tile, strip); break;
                    }
                }
        }
    }
}

// fmax: the largest factor among the rows the launch reads
void launch_gather(const ScaledP& p, int dtype, int fmax, hipStream_t st) {
    const int grid = int(p.nblk < 16384 ? p.nblk : 16384);
    const bool wide = fmax > 4;
    const dim3 g(grid), t(256);
    if (dtype == NIRGAN_SCENE_U16) {
        if (wide) hipLaunchKernelGGL((scene_scaled_gather_kernel<uint16_t, 8>), g, t, 0, st, p);
        else hipLaunchKernelGGL((scene_scaled_gather_kernel<uint16_t, 4>), g, t, 0, st, p);
    } else {
        if (wide) hipLaunchKernelGGL((scene_scaled_gather_kernel<float, 8>), g, t, 0, st, p);
        else hipLaunchKernelGGL((scene_scaled_gather_kernel<float, 4>), g, t, 0, st, p);
    }
}

}  // namespace

extern "C" int nirgan_scene_sample_scaled(const nirgan_scene_scaled_desc* d, void* stream) {
    static const char* who = "scene_sample_scaled";
    NG_REQUIRE(d && d->pool && d->table && d->table_host && d->rgb && d->nir && d->window, "%s: null pointer", who);
    NG_REQUIRE(d->dtype == NIRGAN_SCENE_U16 || d->dtype == NIRGAN_SCENE_F32, "%s: unknown dtype %d", who, d->dtype);
    NG_REQUIRE(d->S > 0 && d->C >= 4, "%s: bad pool (S %d, C %d; C must be at least 4)", who, d->S, d->C);
    NG_REQUIRE(d->views == 1 || d->views == 4 || d->views == 8, "%s: views %d is not 1, 4 or 8", who, d->views);
    for (int k = 0; k < 4; ++k) NG_REQUIRE(d->band[k] >= 0 && d->band[k] < d->C, "%s: band %d outside 0 .. C-1", who, d->band[k]);
    const int64_t T = d->tile;
    NG_REQUIRE(d->B > 0 && T > 0 && T * T < LIM31 && T * T * d->B < LIM31, "%s: B, tile or B*tile*tile is not in 1 .. 2^31-1 (B %d, tile %d)", who, d->B, d->tile);
    NG_REQUIRE(d->divisor == d->divisor && d->divisor != 0.0f, "%s: divisor is 0 or NaN", who);
    NG_REQUIRE(d->max_invalid >= 0, "%s: negative max_invalid", who);
    NG_REQUIRE(d->pool_elems >= 0 && d->prefix_elems >= 0, "%s: negative pool_elems or prefix_elems", who);
    NG_REQUIRE(d->K >= 1 && d->K <= MAXK, "%s: K %d outside 1 .. %d", who, d->K, MAXK);
    ScaledP p;
    uint64_t wtot = 0;
    for (int k = 0; k < d->K; ++k) {
        const int f = d->factor[k];
        NG_REQUIRE(f >= 1 && f <= MAXF, "%s: factor %d outside 1 .. %d", who, f, MAXF);
        NG_REQUIRE(k == 0 || f > d->factor[k - 1], "%s: the factors are not strictly increasing (%d after %d)", who, f, d->factor[k - 1]);
        NG_REQUIRE(d->weight[k] > 0, "%s: the weight of factor %d is 0", who, f);
        wtot += d->weight[k];
        NG_REQUIRE(wtot < (uint64_t(1) << 32), "%s: the weights sum to 2^32 or more", who);
        NG_REQUIRE(f * T * f * T < LIM31, "%s: the window of factor %d, (factor*tile)^2, is 2^31 or more", who, f);
        p.factor[k] = f;
        p.cumw[k] = uint32_t(wtot);
    }
    for (int k = 0; k < d->K; ++k) {
        const int64_t* th = d->table_host + int64_t(k) * d->S * TC;
        if (int e = sp_check_table(who, th, d->S, p.factor[k] * T, &p.total[k])) return e;
        NG_REQUIRE(p.total[k] > 0, "%s: no scene holds a window of factor %d (side %lld)", who, p.factor[k], (long long)(p.factor[k] * T));
        if (int e = sp_check_extents(who, th, d->S, d->C, d->pool_elems, d->prefix, d->prefix_elems)) return e;
    }
    p.wtot = uint32_t(wtot);
    for (int k = d->K; k < MAXK; ++k) { p.factor[k] = 0; p.cumw[k] = 0; p.total[k] = 0; }
    p.pool = d->pool; p.table = d->table; p.prefix = d->prefix; p.geo = d->geo;
    for (int k = 0; k < 4; ++k) p.band[k] = d->band[k];
    p.K = d->K; p.S = d->S; p.T = d->tile; p.B = d->B; p.views = d->views; p.max_invalid = d->max_invalid;
    p.nb = (d->tile + SP_B - 1) / SP_B;
    p.nblk = int64_t(d->B) * 4 * p.nb * p.nb;
    p.divisor = d->divisor;
    p.seed_lo = d->seed_lo; p.seed_hi = d->seed_hi; p.draw_lo = uint32_t(d->draw); p.draw_hi = uint32_t(d->draw >> 32); p.sample0 = d->sample0;
    p.rgb = d->rgb; p.nir = d->nir; p.coords = d->geo ? d->coords : nullptr; p.window = d->window; p.rows = d->window;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(scene_scaled_draw_kernel, dim3((d->B + 255) / 256), dim3(256), 0, st, p);
    launch_gather(p, d->dtype, p.factor[d->K - 1], st);                         // the factors rise: the last is the largest
    return nirgan_check_launch(who);
}

// The gather of the samplers on a list of windows the CALLER names.  The pixels are scene_scaled_gather_kernel's, the
// same instances: with K = 1 it reads table 0 for every row, whatever the row's factor, and a row's factor only picks the block
// routine.  The coords are sp_centre's, one thread per row.
namespace {

struct CentreP {
    const double* geo; const int32_t* rows; float* coords;
    int n, T;
};

__global__ __launch_bounds__(256) void scene_gather_centre_kernel(const CentreP p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    const int32_t* __restrict__ win = p.rows + int64_t(i) * 4;
    const int f = ((win[3] >> 16) & 7) + 1;
    sp_centre(p.geo + int64_t(win[0]) * 4, win[1], win[2], f * p.T, p.coords + int64_t(i) * 2);
}

}  // namespace

extern "C" int nirgan_scene_gather(const nirgan_scene_gather_desc* d, void* stream) {
    static const char* who = "scene_gather";
    NG_REQUIRE(d && d->pool && d->table && d->table_host && d->window && d->window_host && d->rgb && d->nir, "%s: null pointer", who);
    NG_REQUIRE(d->dtype == NIRGAN_SCENE_U16 || d->dtype == NIRGAN_SCENE_F32, "%s: unknown dtype %d", who, d->dtype);
    NG_REQUIRE(d->S > 0 && d->C >= 4, "%s: bad pool (S %d, C %d; C must be at least 4)", who, d->S, d->C);
    for (int k = 0; k < 4; ++k) NG_REQUIRE(d->band[k] >= 0 && d->band[k] < d->C, "%s: band %d outside 0 .. C-1", who, d->band[k]);
    const int64_t T = d->tile;
    NG_REQUIRE(d->n > 0 && T > 0 && T * T < LIM31 && T * T * d->n < LIM31, "%s: n, tile or n*tile*tile is not in 1 .. 2^31-1 (n %d, tile %d)", who, d->n, d->tile);
    NG_REQUIRE(d->first >= 0 && d->n_windows >= d->n && d->first <= d->n_windows - d->n,
               "%s: first %lld, n %d: the rows are not inside 0 .. n_windows-1 (n_windows %lld)", who, (long long)d->first, d->n, (long long)d->n_windows);
    NG_REQUIRE(d->divisor == d->divisor && d->divisor != 0.0f, "%s: divisor is 0 or NaN", who);
    for (int s = 0; s < d->S; ++s) {
        const int64_t* r = d->table_host + int64_t(s) * TC;
        NG_REQUIRE(r[1] > 0 && r[1] < LIM31 && r[2] > 0 && r[2] < LIM31, "%s: scene %d has an extent outside 1 .. 2^31-1", who, s);
    }
    if (int e = sp_check_extents(who, d->table_host, d->S, d->C, d->pool_elems, nullptr, 0, false)) return e;
    int fmax = 1;
    for (int64_t i = d->first; i < d->first + d->n; ++i) {
        const int32_t* w = d->window_host + i * 4;
        const uint32_t word = uint32_t(w[3]);
        NG_REQUIRE((word & ~0x8007FF07u) == 0, "%s: row %lld: the word 0x%08x has a bit set outside the view, attempt, factor and exhausted fields", who, (long long)i, word);
        NG_REQUIRE(w[0] >= 0 && w[0] < d->S, "%s: row %lld: scene %d outside 0 .. S-1", who, (long long)i, w[0]);
        const int f = int((word >> 16) & 7) + 1;
        const int64_t L = f * T;                                                // T * T < 2^31: L < 2^19
        NG_REQUIRE(L * L < LIM31, "%s: row %lld: the window of factor %d, (factor*tile)^2, is 2^31 or more", who, (long long)i, f);
        const int64_t* r = d->table_host + int64_t(w[0]) * TC;
        NG_REQUIRE(w[1] >= 0 && w[2] >= 0 && w[1] + L <= r[1] && w[2] + L <= r[2],
                   "%s: row %lld: the window of side %lld at (%d, %d) is not inside scene %d (%lld x %lld)", who, (long long)i, (long long)L, w[1], w[2], w[0],
                   (long long)r[1], (long long)r[2]);
        if (f > fmax) fmax = f;
    }
    ScaledP p = {};
    p.pool = d->pool; p.table = d->table;
    for (int k = 0; k < 4; ++k) p.band[k] = d->band[k];
    p.K = 1; p.S = d->S; p.T = d->tile; p.B = d->n;
    p.nb = (d->tile + SP_B - 1) / SP_B;
    p.nblk = int64_t(d->n) * 4 * p.nb * p.nb;
    p.divisor = d->divisor;
    p.rgb = d->rgb; p.nir = d->nir;
    p.rows = d->window + d->first * 4;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->geo && d->coords) {
        const CentreP c = {d->geo, p.rows, d->coords, d->n, d->tile};
        hipLaunchKernelGGL(scene_gather_centre_kernel, dim3((d->n + 255) / 256), dim3(256), 0, st, c);
    }
    launch_gather(p, d->dtype, fmax, st);
    return nirgan_check_launch(who);
}

// The draw from a table of rectangles of window origins: nirgan_scene_sample_origins.  Its own parameter block and its
// own attempt (so_attempt of scene_dev.h); the scale is picked as scene_scaled_draw_kernel picks it, the window word and the coords
// are written as there, and the pixels are scene_scaled_gather_kernel's on the rows the draw wrote, launched as nirgan_scene_gather
// launches it: K = 1, the one scene table for every row.
namespace {

struct OriginsP {
    const int64_t* table;                // [S][TC]: W_s and the prefix offset are read
    const int64_t* origins;              // [R][OC]
    const int32_t* prefix;
    const double* geo;
    int64_t total[MAXK];                 // origins of scale k: the cum of its last row
    int first[MAXK], count[MAXK];
    int factor[MAXK];
    uint32_t cumw[MAXK], wtot;
    int K, T, B, views, max_invalid;
    uint32_t seed_lo, seed_hi, draw_lo, draw_hi, sample0;
    float* coords;
    int32_t* window;
};

__global__ __launch_bounds__(256) void scene_origins_draw_kernel(const OriginsP p) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    uint32_t w[4];
    philox4x32_10(p.draw_lo, p.draw_hi, p.sample0 + uint32_t(b), 0u, p.seed_lo, p.seed_hi, w);
    const uint32_t pick = uint32_t((uint64_t(w[3]) * uint64_t(p.wtot)) >> 32);             // floor(w3 * Wtot / 2^32) < Wtot
    int f = p.factor[0], first = p.first[0], count = p.count[0];
    int64_t total = p.total[0];
#pragma unroll
    for (int j = 1; j < MAXK; ++j)       // cumw rises: the last j with cumw[j-1] <= pick is the first with cumw[j] > pick
        if (j < p.K && p.cumw[j - 1] <= pick) { f = p.factor[j]; first = p.first[j]; count = p.count[j]; total = p.total[j]; }
    const int L = f * p.T;
    const int64_t* __restrict__ rows = p.origins + int64_t(first) * OC;
    const int64_t most = int64_t(p.max_invalid) * f * f;
    int s = 0, y0 = 0, x0 = 0, view = 0, a = 0;
    bool ok = false;
    for (; a < NIRGAN_SCENE_ATTEMPTS; ++a) {
        if (a > 0) philox4x32_10(p.draw_lo, p.draw_hi, p.sample0 + uint32_t(b), uint32_t(a), p.seed_lo, p.seed_hi, w);
        const int64_t n = so_attempt(w, p.table, rows, count, p.prefix, L, total, p.views, s, y0, x0, view);
        if (n <= most) { ok = true; break; }
    }
    if (!ok) a = NIRGAN_SCENE_ATTEMPTS - 1;
    int32_t* __restrict__ o = p.window + int64_t(b) * 4;
    o[0] = s; o[1] = y0; o[2] = x0;
    o[3] = int32_t(uint32_t(view) | (uint32_t(a) << 8) | (uint32_t(f - 1) << 16) | (ok ? 0u : 0x80000000u));
    if (p.geo && p.coords) sp_centre(p.geo + int64_t(s) * 4, y0, x0, L, p.coords + int64_t(b) * 2);
}

}  // namespace

extern "C" int nirgan_scene_sample_origins(const nirgan_scene_origins_desc* d, void* stream) {
    static const char* who = "scene_sample_origins";
    NG_REQUIRE(d && d->pool && d->table && d->table_host && d->origins && d->origins_host && d->rgb && d->nir && d->window, "%s: null pointer", who);
    NG_REQUIRE(d->dtype == NIRGAN_SCENE_U16 || d->dtype == NIRGAN_SCENE_F32, "%s: unknown dtype %d", who, d->dtype);
    NG_REQUIRE(d->S > 0 && d->C >= 4, "%s: bad pool (S %d, C %d; C must be at least 4)", who, d->S, d->C);
    NG_REQUIRE(d->views == 1 || d->views == 4 || d->views == 8, "%s: views %d is not 1, 4 or 8", who, d->views);
    for (int k = 0; k < 4; ++k) NG_REQUIRE(d->band[k] >= 0 && d->band[k] < d->C, "%s: band %d outside 0 .. C-1", who, d->band[k]);
    const int64_t T = d->tile;
    NG_REQUIRE(d->B > 0 && T > 0 && T * T < LIM31 && T * T * d->B < LIM31, "%s: B, tile or B*tile*tile is not in 1 .. 2^31-1 (B %d, tile %d)", who, d->B, d->tile);
    NG_REQUIRE(d->divisor == d->divisor && d->divisor != 0.0f, "%s: divisor is 0 or NaN", who);
    NG_REQUIRE(d->max_invalid >= 0, "%s: negative max_invalid", who);
    NG_REQUIRE(d->pool_elems >= 0 && d->prefix_elems >= 0, "%s: negative pool_elems or prefix_elems", who);
    NG_REQUIRE(d->K >= 1 && d->K <= MAXK, "%s: K %d outside 1 .. %d", who, d->K, MAXK);
    OriginsP p;
    uint64_t wtot = 0;
    for (int k = 0; k < d->K; ++k) {
        const int f = d->factor[k];
        NG_REQUIRE(f >= 1 && f <= MAXF, "%s: factor %d outside 1 .. %d", who, f, MAXF);
        NG_REQUIRE(k == 0 || f > d->factor[k - 1], "%s: the factors are not strictly increasing (%d after %d)", who, f, d->factor[k - 1]);
        NG_REQUIRE(d->weight[k] > 0, "%s: the weight of factor %d is 0", who, f);
        wtot += d->weight[k];
        NG_REQUIRE(wtot < (uint64_t(1) << 32), "%s: the weights sum to 2^32 or more", who);
        NG_REQUIRE(f * T * f * T < LIM31, "%s: the window of factor %d, (factor*tile)^2, is 2^31 or more", who, f);
        p.factor[k] = f;
        p.cumw[k] = uint32_t(wtot);
    }
    for (int s = 0; s < d->S; ++s) {
        const int64_t* r = d->table_host + int64_t(s) * TC;
        NG_REQUIRE(r[1] > 0 && r[1] < LIM31 && r[2] > 0 && r[2] < LIM31, "%s: scene %d has an extent outside 1 .. 2^31-1", who, s);
    }
    if (int e = sp_check_extents(who, d->table_host, d->S, d->C, d->pool_elems, d->prefix, d->prefix_elems)) return e;
    NG_REQUIRE(d->R >= 1, "%s: R %d: the origin table has no row", who, d->R);
    int64_t next = 0;
    for (int k = 0; k < d->K; ++k) {
        NG_REQUIRE(d->count[k] >= 1, "%s: factor %d owns no row of the origin table (count %d): no admissible window of side %lld", who, p.factor[k],
                   d->count[k], (long long)(p.factor[k] * T));
        NG_REQUIRE(d->first[k] == next, "%s: first / count do not tile 0 .. R-1 in order (scale %d starts at row %d, not %lld)", who, k, d->first[k], (long long)next);
        next += d->count[k];
        NG_REQUIRE(next <= d->R, "%s: first / count do not tile 0 .. R-1 in order (scale %d ends past R %d)", who, k, d->R);
    }
    NG_REQUIRE(next == d->R, "%s: first / count do not tile 0 .. R-1 in order (they end at row %lld, R %d)", who, (long long)next, d->R);
    for (int k = 0; k < d->K; ++k) {
        const int64_t L = p.factor[k] * T;
        int64_t total = 0;
        for (int i = d->first[k]; i < d->first[k] + d->count[k]; ++i) {
            const int64_t* o = d->origins_host + int64_t(i) * OC;
            NG_REQUIRE(o[0] >= 0 && o[0] < d->S, "%s: row %d: scene %lld outside 0 .. S-1", who, i, (long long)o[0]);
            const int64_t* r = d->table_host + o[0] * TC;
            const int64_t ny = r[1] - L + 1, nx = r[2] - L + 1;                   // origins of the whole scene; not positive if it holds no window
            NG_REQUIRE(o[3] >= 1 && o[4] >= 1, "%s: row %d: an extent (oh %lld, ow %lld) below 1", who, i, (long long)o[3], (long long)o[4]);
            NG_REQUIRE(o[1] >= 0 && o[2] >= 0, "%s: row %d: a negative origin (oy %lld, ox %lld)", who, i, (long long)o[1], (long long)o[2]);
            NG_REQUIRE(o[1] <= ny && o[3] <= ny - o[1] && o[2] <= nx && o[4] <= nx - o[2],
                       "%s: row %d: windows of side %lld from origins (%lld, %lld) + (%lld, %lld) are not inside scene %lld (%lld x %lld)", who, i, (long long)L,
                       (long long)o[1], (long long)o[2], (long long)o[3], (long long)o[4], (long long)o[0], (long long)r[1], (long long)r[2]);
            total += o[3] * o[4];                                                 // each term below 2^62: the sum cannot wrap before the bound
            NG_REQUIRE(total < (int64_t(1) << 62), "%s: factor %d has 2^62 origins or more", who, p.factor[k]);
            NG_REQUIRE(o[5] == total, "%s: row %d: cum is not the running sum of oh*ow of factor %d", who, i, p.factor[k]);
        }
        p.total[k] = total;
        p.first[k] = d->first[k];
        p.count[k] = d->count[k];
    }
    p.wtot = uint32_t(wtot);
    for (int k = d->K; k < MAXK; ++k) { p.factor[k] = 0; p.cumw[k] = 0; p.total[k] = 0; p.first[k] = 0; p.count[k] = 0; }
    p.table = d->table; p.origins = d->origins; p.prefix = d->prefix; p.geo = d->geo;
    p.K = d->K; p.T = d->tile; p.B = d->B; p.views = d->views; p.max_invalid = d->max_invalid;
    p.seed_lo = d->seed_lo; p.seed_hi = d->seed_hi; p.draw_lo = uint32_t(d->draw); p.draw_hi = uint32_t(d->draw >> 32); p.sample0 = d->sample0;
    p.coords = d->geo ? d->coords : nullptr; p.window = d->window;
    ScaledP g = {};                                                             // the gather's block, as nirgan_scene_gather fills it
    g.pool = d->pool; g.table = d->table;
    for (int k = 0; k < 4; ++k) g.band[k] = d->band[k];
    g.K = 1; g.S = d->S; g.T = d->tile; g.B = d->B;
    g.nb = (d->tile + SP_B - 1) / SP_B;
    g.nblk = int64_t(d->B) * 4 * g.nb * g.nb;
    g.divisor = d->divisor;
    g.rgb = d->rgb; g.nir = d->nir;
    g.rows = d->window;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(scene_origins_draw_kernel, dim3((d->B + 255) / 256), dim3(256), 0, st, p);
    launch_gather(g, d->dtype, p.factor[d->K - 1], st);                         // the factors rise: the last is the largest
    return nirgan_check_launch(who);
}
