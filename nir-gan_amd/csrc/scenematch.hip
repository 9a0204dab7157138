// Matching a uint16 plane's histogram to a reference band: nirgan_scene_hist / nirgan_scene_match_lut /
// nirgan_scene_lut_apply.  Integer-exact: a count pass, a 65 536-entry table, a lookup pass.
//   count   grid-stride over 16-byte loads (eight codes); the up to seven codes in front of the first 16-byte boundary and the up to
//           seven behind the last whole vector go element-wise.  A workgroup keeps 32-bit counters for a WINDOW of HW_BINS adjacent
//           codes in LDS (128 KiB, dynamic; one workgroup of 1024 threads per CU) and adds every other code straight to the 64-bit
//           global table; at the end it flushes its non-zero counters with one 64-bit global add each.  Where the window lies is chosen per workgroup from the first vector of each of its
//           threads (a 64-bin coarse count, the best run of HW_BINS / 1024 bins): a choice of speed only -- every element is added
//           exactly once, in the window or outside it.
//   table   64 workgroups of 1024 threads, one code per thread, a wave = one block of 64 adjacent codes.  Every workgroup sums the
//           1024 blocks of both tables (a wave reads one block as 512 contiguous bytes), scans them in LDS, and then holds the
//           inclusive count, the rounded quantile and the last present reference code at every block's end.  A thread forms x_v from a
//           wave scan of its block, finds the first block whose rounded quantile exceeds x_v (binary search in LDS) and walks that
//           block's 64 reference counts to the crossing.  float64 with every operation rounded on its own.
//   apply   a thread owns eight consecutive codes (one 16-byte load, eight table loads, one 16-byte store) where plane and out
//           share their position in a 16-byte line, single codes otherwise and at the ends.  The table is read from global memory.
// 64-bit addressing; the only atomics are the count's integer adds.
#include "common.h"

namespace {

constexpr int64_t LIM31 = int64_t(1) << 31;
constexpr int CODES = NIRGAN_SCENE_CODES;
constexpr int HW_BINS = 32768;           // the count's LDS window: 128 KiB of 32-bit counters, one workgroup per CU
constexpr int HW_THREADS = 1024;
constexpr int HW_GRID = 256;
constexpr int HW_COARSE = 1024;          // codes per bin of the sampled coarse count

typedef unsigned long long u64;
struct alignas(16) Codes8 { uint16_t e[8]; };

struct MatchP {
    const uint16_t* plane;
    int64_t n, head, nvec;               // [0, head) single codes, then nvec vectors of eight, then the rest single
    int has_nodata, nodata;
    u64* hist;
    const int64_t* src; const int64_t* ref; int64_t* totals;
    uint16_t* lut; uint16_t* out;
};

__device__ __forceinline__ void hist_add(uint32_t* win, u64* hist, int base, int code) {
    const unsigned r = unsigned(code - base);
    if (r < unsigned(HW_BINS)) atomicAdd(win + r, 1u);
    else __hip_atomic_fetch_add(hist + code, u64(1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// LDS (dynamic: more than 64 KiB): BINS window counters, then the NB coarse counters, then the window's first code
constexpr size_t HW_LDS = size_t(HW_BINS) * 4 + (CODES / HW_COARSE) * 4 + 16;

__global__ __launch_bounds__(HW_THREADS) void scene_hist_kernel(const MatchP p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int BINS = HW_BINS, THREADS = HW_THREADS, RUN = BINS / HW_COARSE, NB = CODES / HW_COARSE;
    uint32_t* win = reinterpret_cast<uint32_t*>(smem_raw);
    uint32_t* coarse = win + BINS;
    int* base_s = reinterpret_cast<int*>(coarse + NB);
    const uint16_t* plane = p.plane;
    const int skip = p.has_nodata ? p.nodata : -1;
    const Codes8* vecs = reinterpret_cast<const Codes8*>(plane + p.head);
    const int64_t first = blockIdx.x * int64_t(THREADS) + threadIdx.x, step = int64_t(gridDim.x) * THREADS;
    Codes8 v = {};
    if (first < p.nvec) v = vecs[first];
    for (int i = threadIdx.x; i < BINS; i += THREADS) win[i] = 0;
    if (threadIdx.x < NB) coarse[threadIdx.x] = 0;
    __syncthreads();
    if (first < p.nvec) {                                                        // the sample: this thread's first vector
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (int(v.e[e]) != skip) atomicAdd(coarse + (v.e[e] / HW_COARSE), 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                                      // the run of RUN coarse bins that holds most of the sample
        uint32_t sum = 0;
        for (int b = 0; b < RUN; ++b) sum += coarse[b];
        uint32_t best = sum;
        int at = 0;
        for (int b = 1; b + RUN <= NB; ++b) {
            sum += coarse[b + RUN - 1] - coarse[b - 1];
            if (sum > best) { best = sum; at = b; }
        }
        *base_s = at * HW_COARSE;
    }
    __syncthreads();
    const int base = *base_s;
    for (int64_t i = first; i < p.nvec; i += step) {
        if (i != first) v = vecs[i];
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (int(v.e[e]) != skip) hist_add(win, p.hist, base, v.e[e]);
    }
    const int64_t tail0 = p.head + 8 * p.nvec;
    for (int64_t i = first; i < p.head + (p.n - tail0); i += step) {            // the ends, one code per thread
        const int c = plane[i < p.head ? i : tail0 + (i - p.head)];
        if (c != skip) hist_add(win, p.hist, base, c);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BINS; i += THREADS) {
        const uint32_t c = win[i];
        if (c) __hip_atomic_fetch_add(p.hist + base + i, u64(c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the table
constexpr int LT_THREADS = 1024, LT_BLOCKS = CODES / 64;                         // 1024 blocks of 64 codes

__device__ __forceinline__ double quantile(int64_t c, double total) {
    return __ddiv_rn(double(c), total);
}

// t_j + ((t_n - t_j) / (q_n - q_j)) * (x - q_j), four differences / quotients / products / sums, each rounded on its own
__device__ __forceinline__ double interp_between(double x, double qj, double tj, double qn, double tn) {
#pragma clang fp contract(off)
    const double slope = (tn - tj) / (qn - qj);
    const double rise = slope * (x - qj);
    return rise + tj;
}

__device__ __forceinline__ int64_t wave_sum64(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(LT_THREADS) void scene_match_lut_kernel(const MatchP p) {
    __shared__ int64_t cum[2][LT_BLOCKS];                                        // inclusive counts at every block's end: source, reference
    __shared__ int64_t tmp[2][LT_BLOCKS];
    __shared__ double qend[LT_BLOCKS];                                           // the rounded reference quantile at every block's end
    __shared__ int lastp[2][LT_BLOCKS];                                          // the last present reference code at or before it, or -1
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int WAVES = LT_THREADS / 64, AHEAD = 8;
    for (int r = 0; r < LT_BLOCKS / WAVES; r += AHEAD) {                         // this wave's blocks, eight blocks' loads in flight
        int64_t hs[AHEAD], hr[AHEAD];
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) {
            const int b = (r + k) * WAVES + wave;                                // uniform over the wave
            hs[k] = p.src[b * 64 + lane];
            hr[k] = p.ref[b * 64 + lane];
        }
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) {
            const int b = (r + k) * WAVES + wave;
            const int64_t ss = wave_sum64(hs[k]), sr = wave_sum64(hr[k]);
            const u64 present = __ballot(hr[k] > 0);
            if (lane == 0) {
                cum[0][b] = ss;
                cum[1][b] = sr;
                lastp[0][b] = present ? b * 64 + 63 - __clzll(present) : -1;
            }
        }
    }
    __syncthreads();
    int cur = 0;                                                                 // lastp's current half; cum / tmp swap roles with it
    int64_t (*a)[LT_BLOCKS] = cum, (*b2)[LT_BLOCKS] = tmp;
    for (int o = 1; o < LT_BLOCKS; o <<= 1) {                                    // an inclusive scan over the 1024 blocks, one per thread
        const int t = threadIdx.x;
        b2[0][t] = a[0][t] + (t >= o ? a[0][t - o] : 0);
        b2[1][t] = a[1][t] + (t >= o ? a[1][t - o] : 0);
        lastp[cur ^ 1][t] = t >= o ? max(lastp[cur][t], lastp[cur][t - o]) : lastp[cur][t];
        __syncthreads();
        int64_t (*s)[LT_BLOCKS] = a; a = b2; b2 = s;
        cur ^= 1;
    }
    const int64_t ns = a[0][LT_BLOCKS - 1], nr = a[1][LT_BLOCKS - 1];
    if (blockIdx.x == 0 && threadIdx.x == 0 && p.totals) { p.totals[0] = ns; p.totals[1] = nr; }
    const int v = blockIdx.x * LT_THREADS + threadIdx.x, blk = v >> 6;           // blk: this wave's block
    if (ns == 0 || nr == 0) {                                                    // uniform over the grid
        p.lut[v] = uint16_t(v);
        return;
    }
    const double dns = double(ns), dnr = double(nr);
    qend[threadIdx.x] = quantile(a[1][threadIdx.x], dnr);
    __syncthreads();
    int64_t cs = p.src[v];                                                       // the inclusive count of the source up to v
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t up = __shfl_up(cs, o, 64);
        if (lane >= o) cs += up;
    }
    if (blk > 0) cs += a[0][blk - 1];
    const double x = quantile(cs, dns);
    int lo = 0, hi = LT_BLOCKS;                                                  // the first block whose end quantile exceeds x
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (qend[mid] > x) hi = mid; else lo = mid + 1;
    }
    double y;
    if (lo == LT_BLOCKS) {
        y = double(lastp[cur][LT_BLOCKS - 1]);                                   // x >= q_{m-1}
    } else {
        int tj = lo > 0 ? lastp[cur][lo - 1] : -1, tn = -1;
        double qj = lo > 0 ? qend[lo - 1] : 0.0, qn = 0.0;
        int64_t c = lo > 0 ? a[1][lo - 1] : 0;
        for (int u0 = lo * 64; u0 < lo * 64 + 64 && tn < 0; u0 += 16) {          // the crossing lies in this block; 16 counts in flight
            int64_t h[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) h[k] = p.ref[u0 + k];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (tn >= 0 || h[k] <= 0) continue;
                c += h[k];
                const double q = quantile(c, dnr);
                if (q > x) { tn = u0 + k; qn = q; }
                else { tj = u0 + k; qj = q; }
            }
        }
        if (tj < 0) y = double(tn);                                              // x < q_0
        else if (x == qj || tn < 0) y = double(tj);
        else y = interp_between(x, qj, double(tj), qn, double(tn));
    }
    int r = int(fmin(fmax(rint(y), 0.0), 65535.0));
    if (p.has_nodata && r == p.nodata) r = p.nodata == 65535 ? 65534 : p.nodata + 1;
    p.lut[v] = uint16_t(r);
}

// ---------------------------------------------------------------------------------------------------------------- the apply
__device__ __forceinline__ uint16_t lut_one(const uint16_t* __restrict__ lut, uint16_t c, int skip) {
    return int(c) == skip ? c : lut[c];
}

__global__ __launch_bounds__(256) void scene_lut_apply_kernel(const MatchP p) {
    const uint16_t* in = p.plane;                                                // may be `out` itself: no __restrict__
    uint16_t* out = p.out;
    const uint16_t* __restrict__ lut = p.lut;
    const int skip = p.has_nodata ? p.nodata : -1;
    const int64_t first = blockIdx.x * 256ll + threadIdx.x, step = int64_t(gridDim.x) * 256;
    const Codes8* vin = reinterpret_cast<const Codes8*>(in + p.head);
    Codes8* vout = reinterpret_cast<Codes8*>(out + p.head);
    for (int64_t i = first; i < p.nvec; i += step) {
        const Codes8 v = vin[i];
        Codes8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.e[e] = lut_one(lut, v.e[e], skip);
        vout[i] = o;
    }
    const int64_t tail0 = p.head + 8 * p.nvec;
    for (int64_t i = first; i < p.head + (p.n - tail0); i += step) {
        const int64_t at = i < p.head ? i : tail0 + (i - p.head);
        out[at] = lut_one(lut, in[at], skip);
    }
}

inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// codes in front of the first 16-byte boundary of a 2-byte aligned address
inline int64_t codes_to_line(const void* p) { return int64_t((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / 2; }

int plane_params(MatchP& p, const nirgan_scene_match_desc* d, const char* who) {
    NG_REQUIRE(d && d->plane, "%s: null pointer (d or plane)", who);
    NG_REQUIRE(d->n >= 1 && d->n < LIM31, "%s: n %lld outside 1 .. 2^31-1", who, (long long)d->n);
    NG_REQUIRE(!d->has_nodata || (d->nodata >= 0 && d->nodata <= 65535), "%s: nodata %d outside 0 .. 65535", who, d->nodata);
    NG_REQUIRE(aligned_to(d->plane, 2), "%s: the plane is not 2-byte aligned", who);
    p = MatchP{};
    p.plane = static_cast<const uint16_t*>(d->plane);
    p.n = d->n;
    p.has_nodata = d->has_nodata ? 1 : 0;
    p.nodata = d->nodata;
    p.head = codes_to_line(d->plane) < d->n ? codes_to_line(d->plane) : d->n;
    p.nvec = (d->n - p.head) / 8;
    return NIRGAN_OK;
}

}  // namespace

extern "C" int nirgan_scene_hist(const nirgan_scene_match_desc* d, void* stream) {
    MatchP p;
    if (int e = plane_params(p, d, "scene_hist")) return e;
    NG_REQUIRE(d->hist, "scene_hist: null pointer (hist)");
    NG_REQUIRE(aligned_to(d->hist, 8), "scene_hist: hist is not 8-byte aligned");
    p.hist = reinterpret_cast<u64*>(d->hist);
    static bool once = [] { return hipFuncSetAttribute(reinterpret_cast<const void*>(scene_hist_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(HW_LDS)) == hipSuccess; }();
    (void)once;
    const int64_t items = p.nvec > 14 ? p.nvec : 14;                             // the ends hold up to 14 codes
    const int64_t g = (items + HW_THREADS - 1) / HW_THREADS;
    hipLaunchKernelGGL(scene_hist_kernel, dim3(int(g < HW_GRID ? g : HW_GRID)), dim3(HW_THREADS), HW_LDS, static_cast<hipStream_t>(stream), p);
    return nirgan_check_launch("scene_hist");
}

extern "C" int nirgan_scene_match_lut(const nirgan_scene_match_desc* d, void* stream) {
    NG_REQUIRE(d && d->src_hist && d->ref_hist && d->lut, "scene_match_lut: null pointer (d, src_hist, ref_hist or lut)");
    NG_REQUIRE(!d->has_nodata || (d->nodata >= 0 && d->nodata <= 65535), "scene_match_lut: nodata %d outside 0 .. 65535", d->nodata);
    NG_REQUIRE(aligned_to(d->src_hist, 8) && aligned_to(d->ref_hist, 8) && aligned_to(d->lut, 8) && aligned_to(d->totals, 8),
               "scene_match_lut: src_hist, ref_hist, lut or totals is not 8-byte aligned");
    MatchP p = {};
    p.has_nodata = d->has_nodata ? 1 : 0;
    p.nodata = d->nodata;
    p.src = d->src_hist; p.ref = d->ref_hist; p.totals = d->totals; p.lut = d->lut;
    hipLaunchKernelGGL(scene_match_lut_kernel, dim3(CODES / LT_THREADS), dim3(LT_THREADS), 0, static_cast<hipStream_t>(stream), p);
    return nirgan_check_launch("scene_match_lut");
}

extern "C" int nirgan_scene_lut_apply(const nirgan_scene_match_desc* d, void* stream) {
    MatchP p;
    if (int e = plane_params(p, d, "scene_lut_apply")) return e;
    NG_REQUIRE(d->lut && d->out, "scene_lut_apply: null pointer (lut or out)");
    NG_REQUIRE(aligned_to(d->out, 2), "scene_lut_apply: out is not 2-byte aligned");
    NG_REQUIRE(aligned_to(d->lut, 8), "scene_lut_apply: lut is not 8-byte aligned");
    const uintptr_t a = reinterpret_cast<uintptr_t>(d->plane), b = reinterpret_cast<uintptr_t>(d->out), bytes = uintptr_t(d->n) * 2;
    NG_REQUIRE(a == b || a + bytes <= b || b + bytes <= a, "scene_lut_apply: out overlaps the plane without being the plane");
    p.lut = d->lut;
    p.out = static_cast<uint16_t*>(d->out);
    if (((a ^ b) & 15) != 0) { p.head = p.n; p.nvec = 0; }                       // no common 16-byte phase: single codes throughout
    const int64_t items = p.nvec > p.n - 8 * p.nvec ? p.nvec : p.n - 8 * p.nvec;
    const int64_t g = (items + 255) / 256;
    hipLaunchKernelGGL(scene_lut_apply_kernel, dim3(int(g < 8192 ? g : 8192)), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return nirgan_check_launch("scene_lut_apply");
}
