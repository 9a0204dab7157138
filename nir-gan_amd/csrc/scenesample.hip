// Batches drawn and cut from device-resident scenes, four entries on one draw and one gather:
//   nirgan_scene_sample            the draw over whole scenes with the one factor 1;
//   nirgan_scene_sample_scaled     the draw over whole scenes, one table per factor;
//   nirgan_scene_gather            no draw: the gather on a list of windows the caller names;
//   nirgan_scene_sample_origins    the draw over a table of rectangles of window origins.
//
// The pool keeps the scenes as they are stored (uint16 or float, planar, nothing aligned).  Sample b takes its resolution factor f
// from the fourth Philox word of attempt 0, cuts a window of side L = f * T and delivers the T x T tile of the means of its f x f
// blocks.  Two launches:
//   draw    one thread per sample: Philox4x32-10 on (seed; draw, sample0 + b, attempt) -> an index among all windows of the drawn
//           scale (the high word of a 64 x 64 bit product: no modulo bias beyond 2^-64 * total), which the SOURCE of the draw turns
//           into (scene, y0, x0) -- a binary search of running counts either way, sp_attempt / so_attempt of scene_dev.h -- then the
//           rejection test n <= max_invalid * f * f on four entries of the scene's invalid-prefix table, the view, the coords;
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
//           way.  Transposing views (4 .. 7) turn the block in LDS with rows padded to 65 floats, as tileviews.hip does (written
//           with stride 65, read with stride 1: no bank conflict).
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

// A source of the draw names what it draws from at scale k (`scale`, asked with a constant k only: the scale differs from lane to
// lane) and turns the words of one attempt there into a window of side L and its invalid count.
struct Scenes {                          // every window of every scene: one table per scale
    const int64_t* table;                // [K][S][TC]
    int S;
    struct Scale { const int64_t* table; };
    __device__ __forceinline__ Scale scale(int k) const { return {table + int64_t(k) * S * TC}; }
    __device__ __forceinline__ int64_t attempt(const uint32_t w[4], const Scale& at, const int32_t* __restrict__ prefix, int L, int64_t total,
                                               int views, int& s, int& y0, int& x0, int& view) const {
        return sp_attempt(w, at.table, prefix, S, L, total, views, s, y0, x0, view);
    }
};
struct Origins {                         // the windows whose origins the rows list: scale k owns rows first[k] .. first[k] + count[k] - 1
    int first[MAXK], count[MAXK];
    const int64_t* table;                // [S][TC]: W_s and the prefix offset are read
    const int64_t* origins;              // [R][OC]
    struct Scale { const int64_t* rows; int count; };
    __device__ __forceinline__ Scale scale(int k) const { return {origins + int64_t(first[k]) * OC, count[k]}; }
    __device__ __forceinline__ int64_t attempt(const uint32_t w[4], const Scale& at, const int32_t* __restrict__ prefix, int L, int64_t total,
                                               int views, int& s, int& y0, int& x0, int& view) const {
        return so_attempt(w, table, at.rows, at.count, prefix, L, total, views, s, y0, x0, view);
    }
};

// The draw, whatever its windows are drawn from.
struct DrawCommon {
    const int32_t* prefix;
    const double* geo;
    int64_t total[MAXK];                 // windows of scale k
    int factor[MAXK];
    uint32_t cumw[MAXK], wtot;           // running weights; cumw[K-1] = wtot < 2^32
    int K, T, B, views, max_invalid;
    uint32_t seed_lo, seed_hi, draw_lo, draw_hi, sample0;
    float* coords;
    int32_t* window;
};

// The draw's one argument: the common block and the source's few fields.  The kernel is ONE wave that waits for every 64-byte line
// of its arguments that it reads with scalar loads, so the order of the two is not free, and it is the measured one for each source
// (DESIGN 3.13): with the common block in front, nirgan_scene_sample_origins took 0.26 us more per call than with it behind
// (22.18 against 21.92 us); with it behind, nirgan_scene_sample_scaled took 0.2 us more than with it in front.
template <typename Source> struct DrawP;
template <> struct DrawP<Scenes> : DrawCommon, Scenes {};
template <> struct DrawP<Origins> : Origins, DrawCommon {};

template <typename Source>
__global__ __launch_bounds__(256) void scene_draw_kernel(const DrawP<Source> p) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= p.B) return;
    uint32_t w[4];
    philox4x32_10(p.draw_lo, p.draw_hi, p.sample0 + uint32_t(b), 0u, p.seed_lo, p.seed_hi, w);
    const uint32_t pick = uint32_t((uint64_t(w[3]) * uint64_t(p.wtot)) >> 32);             // floor(w3 * Wtot / 2^32) < Wtot
    int f = p.factor[0];
    int64_t total = p.total[0];
    typename Source::Scale at = p.scale(0);
#pragma unroll
    for (int j = 1; j < MAXK; ++j)       // cumw rises: the last j with cumw[j-1] <= pick is the first with cumw[j] > pick
        if (j < p.K && p.cumw[j - 1] <= pick) { f = p.factor[j]; total = p.total[j]; at = p.scale(j); }
    const int L = f * p.T;
    const int64_t most = int64_t(p.max_invalid) * f * f;
    int s = 0, y0 = 0, x0 = 0, view = 0, a = 0;
    bool ok = false;
    for (; a < NIRGAN_SCENE_ATTEMPTS; ++a) {
        if (a > 0) philox4x32_10(p.draw_lo, p.draw_hi, p.sample0 + uint32_t(b), uint32_t(a), p.seed_lo, p.seed_hi, w);
        const int64_t n = p.attempt(w, at, p.prefix, L, total, p.views, s, y0, x0, view);
        if (n <= most) { ok = true; break; }
    }
    if (!ok) a = NIRGAN_SCENE_ATTEMPTS - 1;
    int32_t* __restrict__ o = p.window + int64_t(b) * 4;
    o[0] = s; o[1] = y0; o[2] = x0;
    o[3] = int32_t(uint32_t(view) | (uint32_t(a) << 8) | (uint32_t(f - 1) << 16) | (ok ? 0u : 0x80000000u));
    if (p.geo && p.coords) sp_centre(p.geo + int64_t(s) * 4, y0, x0, L, p.coords + int64_t(b) * 2);
}

// The gather: the rows it cuts and what it cuts them from.
struct GatherP {
    const void* pool;
    const int64_t* table;                // [K][S][TC]; with K = 1 the one table serves every row, whatever its factor
    int64_t band[4];                     // selected plane numbers
    int factor[MAXK];                    // of table k (not read with K = 1)
    int K, S, T, nb;                     // nb: blocks per tile side
    int64_t nblk;                        // rows * 4 * nb * nb
    float divisor;
    float* rgb; float* nir;
    const int32_t* rows;                 // the draw's window, or the caller's list (nirgan_scene_gather)
};

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
__global__ __launch_bounds__(256) void scene_scaled_gather_kernel(const GatherP p) {
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
void launch_gather(const GatherP& p, int dtype, int fmax, hipStream_t st) {
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

// the coords of nirgan_scene_gather's rows, one thread per row (the samplers' draw writes its own)
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

// ---- the host side: what the four descriptors share is checked and filled once; D is the entry's descriptor type ----

template <typename D> constexpr bool names_rows = std::is_same<D, nirgan_scene_gather_desc>::value;    // no draw: n rows, not B samples

// The checks every entry opens with, in the order every entry has always made them.  own_ptrs: the entry's pointers beyond those
// of all four.  nirgan_scene_gather has no views, max_invalid or prefix_elems, and places its rows among its window list here.
template <typename D>
int check_common(const char* who, const D* d, bool own_ptrs) {
    NG_REQUIRE(d && d->pool && d->table && d->table_host && d->rgb && d->nir && d->window && own_ptrs, "%s: null pointer", who);
    NG_REQUIRE(d->dtype == NIRGAN_SCENE_U16 || d->dtype == NIRGAN_SCENE_F32, "%s: unknown dtype %d", who, d->dtype);
    NG_REQUIRE(d->S > 0 && d->C >= 4, "%s: bad pool (S %d, C %d; C must be at least 4)", who, d->S, d->C);
    if constexpr (!names_rows<D>) NG_REQUIRE(d->views == 1 || d->views == 4 || d->views == 8, "%s: views %d is not 1, 4 or 8", who, d->views);
    for (int k = 0; k < 4; ++k) NG_REQUIRE(d->band[k] >= 0 && d->band[k] < d->C, "%s: band %d outside 0 .. C-1", who, d->band[k]);
    const int64_t T = d->tile;
    int n;
    if constexpr (names_rows<D>) n = d->n; else n = d->B;
    const char* nn = names_rows<D> ? "n" : "B";
    NG_REQUIRE(n > 0 && T > 0 && T * T < LIM31 && T * T * n < LIM31, "%s: %s, tile or %s*tile*tile is not in 1 .. 2^31-1 (%s %d, tile %d)", who, nn, nn, nn, n, d->tile);
    if constexpr (names_rows<D>)
        NG_REQUIRE(d->first >= 0 && d->n_windows >= d->n && d->first <= d->n_windows - d->n,
                   "%s: first %lld, n %d: the rows are not inside 0 .. n_windows-1 (n_windows %lld)", who, (long long)d->first, d->n, (long long)d->n_windows);
    NG_REQUIRE(d->divisor == d->divisor && d->divisor != 0.0f, "%s: divisor is 0 or NaN", who);
    if constexpr (!names_rows<D>) {
        NG_REQUIRE(d->max_invalid >= 0, "%s: negative max_invalid", who);
        NG_REQUIRE(d->pool_elems >= 0 && d->prefix_elems >= 0, "%s: negative pool_elems or prefix_elems", who);
    }
    return NIRGAN_OK;
}

// K factors and their weights into the draw's block: factor, cumw, wtot, K
int check_scales(const char* who, int K, const int* factor, const uint32_t* weight, int64_t T, DrawCommon& p) {
    NG_REQUIRE(K >= 1 && K <= MAXK, "%s: K %d outside 1 .. %d", who, K, MAXK);
    uint64_t wtot = 0;
    for (int k = 0; k < K; ++k) {
        const int f = factor[k];
        NG_REQUIRE(f >= 1 && f <= MAXF, "%s: factor %d outside 1 .. %d", who, f, MAXF);
        NG_REQUIRE(k == 0 || f > factor[k - 1], "%s: the factors are not strictly increasing (%d after %d)", who, f, factor[k - 1]);
        NG_REQUIRE(weight[k] > 0, "%s: the weight of factor %d is 0", who, f);
        wtot += weight[k];
        NG_REQUIRE(wtot < (uint64_t(1) << 32), "%s: the weights sum to 2^32 or more", who);
        NG_REQUIRE(f * T * f * T < LIM31, "%s: the window of factor %d, (factor*tile)^2, is 2^31 or more", who, f);
        p.factor[k] = f;
        p.cumw[k] = uint32_t(wtot);
    }
    p.K = K;
    p.wtot = uint32_t(wtot);
    return NIRGAN_OK;
}

// the gather of n rows on the entry's ONE [S][TC] table (K = 1); nirgan_scene_sample_scaled then names its K tables
template <typename D>
GatherP gather_one_table(const D* d, int n, const int32_t* rows) {
    GatherP g = {};
    g.pool = d->pool; g.table = d->table;
    for (int k = 0; k < 4; ++k) g.band[k] = d->band[k];
    g.K = 1; g.S = d->S; g.T = d->tile;
    g.nb = (d->tile + SP_B - 1) / SP_B;
    g.nblk = int64_t(n) * 4 * g.nb * g.nb;
    g.divisor = d->divisor;
    g.rgb = d->rgb; g.nir = d->nir;
    g.rows = rows;
    return g;
}

// The two launches of a sampler.  p holds the source's fields, the scales and their totals; the rest of the draw comes from the
// descriptor.
template <typename D, typename Source>
int launch_sampler(const char* who, const D* d, DrawP<Source>& p, const GatherP& g, void* stream) {
    p.prefix = d->prefix; p.geo = d->geo;
    p.T = d->tile; p.B = d->B; p.views = d->views; p.max_invalid = d->max_invalid;
    p.seed_lo = d->seed_lo; p.seed_hi = d->seed_hi; p.draw_lo = uint32_t(d->draw); p.draw_hi = uint32_t(d->draw >> 32); p.sample0 = d->sample0;
    p.coords = d->geo ? d->coords : nullptr; p.window = d->window;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(scene_draw_kernel<Source>, dim3((d->B + 255) / 256), dim3(256), 0, st, p);
    launch_gather(g, d->dtype, p.factor[p.K - 1], st);                          // the factors rise: the last is the largest
    return nirgan_check_launch(who);
}

}  // namespace

extern "C" int nirgan_scene_sample(const nirgan_scene_sample_desc* d, void* stream) {
    static const char* who = "scene_sample";
    static const int factor[1] = {1};
    static const uint32_t weight[1] = {1};
    if (int e = check_common(who, d, true)) return e;
    DrawP<Scenes> p = {};
    p.table = d->table; p.S = d->S;
    if (int e = check_scales(who, 1, factor, weight, d->tile, p)) return e;
    if (int e = sp_check_table(who, d->table_host, d->S, d->tile, &p.total[0])) return e;
    NG_REQUIRE(p.total[0] > 0, "%s: no scene holds a window of tile %d", who, d->tile);
    if (int e = sp_check_extents(who, d->table_host, d->S, d->C, d->pool_elems, d->prefix, d->prefix_elems)) return e;
    return launch_sampler(who, d, p, gather_one_table(d, d->B, d->window), stream);
}

extern "C" int nirgan_scene_sample_scaled(const nirgan_scene_scaled_desc* d, void* stream) {
    static const char* who = "scene_sample_scaled";
    if (int e = check_common(who, d, true)) return e;
    const int64_t T = d->tile;
    DrawP<Scenes> p = {};
    p.table = d->table; p.S = d->S;
    if (int e = check_scales(who, d->K, d->factor, d->weight, T, p)) return e;
    for (int k = 0; k < d->K; ++k) {
        const int64_t* th = d->table_host + int64_t(k) * d->S * TC;
        if (int e = sp_check_table(who, th, d->S, p.factor[k] * T, &p.total[k])) return e;
        NG_REQUIRE(p.total[k] > 0, "%s: no scene holds a window of factor %d (side %lld)", who, p.factor[k], (long long)(p.factor[k] * T));
        if (int e = sp_check_extents(who, th, d->S, d->C, d->pool_elems, d->prefix, d->prefix_elems)) return e;
    }
    GatherP g = gather_one_table(d, d->B, d->window);
    g.K = d->K;
    for (int k = 0; k < d->K; ++k) g.factor[k] = p.factor[k];
    return launch_sampler(who, d, p, g, stream);
}

// The gather on a list of windows the CALLER names: K = 1, table 0 for every row, and a row's factor only picks the
// block routine.
extern "C" int nirgan_scene_gather(const nirgan_scene_gather_desc* d, void* stream) {
    static const char* who = "scene_gather";
    if (int e = check_common(who, d, d && d->window_host)) return e;
    const int64_t T = d->tile;
    if (int e = sp_check_sides(who, d->table_host, 0, d->S)) return e;
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
    const GatherP g = gather_one_table(d, d->n, d->window + d->first * 4);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->geo && d->coords) {
        const CentreP c = {d->geo, g.rows, d->coords, d->n, d->tile};
        hipLaunchKernelGGL(scene_gather_centre_kernel, dim3((d->n + 255) / 256), dim3(256), 0, st, c);
    }
    launch_gather(g, d->dtype, fmax, st);
    return nirgan_check_launch(who);
}

// The draw from a table of rectangles of window origins; the gather runs on the rows the draw wrote as
// nirgan_scene_gather runs it: the one scene table for every row.
extern "C" int nirgan_scene_sample_origins(const nirgan_scene_origins_desc* d, void* stream) {
    static const char* who = "scene_sample_origins";
    if (int e = check_common(who, d, d && d->origins && d->origins_host)) return e;
    const int64_t T = d->tile;
    DrawP<Origins> p = {};
    p.table = d->table; p.origins = d->origins;
    if (int e = check_scales(who, d->K, d->factor, d->weight, T, p)) return e;
    if (int e = sp_check_sides(who, d->table_host, 0, d->S)) return e;
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
    return launch_sampler(who, d, p, gather_one_table(d, d->B, d->window), stream);
}

