// Device pieces and table checks of the scene entries (scenesample.hip: nirgan_scene_sample, nirgan_scene_sample_scaled,
// nirgan_scene_gather, nirgan_scene_sample_origins; scenepredict.hip takes the unfused product and sum): the padded 64 x 64 LDS block
// of the gather, the prefix count of a window, one attempt of the draw on the words of one Philox call (over whole scenes: sp_attempt;
// over a table of origin rectangles: so_attempt; each is its own index -> (s, y0, x0) step), and the coords.
#pragma once
#include "common.h"
#include "philox_dev.h"

constexpr int SP_B = 64;                 // side of the gather's block
constexpr int SP_LD = SP_B + 1;          // padded LDS row
constexpr int TC = NIRGAN_SCENE_TABLE_COLS;
constexpr int64_t LIM31 = int64_t(1) << 31;

// a + x * y as one rounded float64 product and one rounded float64 sum.  __dmul_rn / __dadd_rn are plain operators in the compiler's
// header and carry its default contraction with them when inlined, so the two operations stand here under the pragma instead.
__device__ __forceinline__ double sp_mul_then_add(double a, double x, double y) {
#pragma clang fp contract(off)
    const double m = x * y;
    return a + m;
}

// the number of invalid pixels in the T x T window at (y0, x0) of the scene with table row `scene`; 0 where the scene has no prefix
// table or prefix is null (the row is then not read: a draw without tables waits for one load less)
__device__ __forceinline__ int64_t sp_invalid(const int32_t* __restrict__ prefix, const int64_t* __restrict__ scene, int y0, int x0, int T) {
    if (!prefix || scene[4] < 0) return 0;
    const int32_t* __restrict__ P = prefix + scene[4];
    const int64_t ld = scene[2] + 1;
    return int64_t(P[(y0 + T) * ld + x0 + T]) - P[y0 * ld + x0 + T] - P[(y0 + T) * ld + x0] + P[y0 * ld + x0];
}

// One attempt: the window that the words w name among the `total` windows of side T of table [S][TC], and the number of invalid
// pixels it holds (0 without a prefix table).
__device__ __forceinline__ int64_t sp_attempt(const uint32_t w[4], const int64_t* __restrict__ table, const int32_t* __restrict__ prefix,
                                              int S, int T, int64_t total, int views, int& s, int& y0, int& x0, int& view) {
    const uint64_t u = uint64_t(w[0]) | (uint64_t(w[1]) << 32);
    const int64_t idx = int64_t(__umul64hi(u, uint64_t(total)));                // < total
    int lo = 0, hi = S - 1;                                                     // the first scene with cum > idx (cum[S-1] = total > idx)
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (table[int64_t(mid) * TC + 3] > idx) hi = mid; else lo = mid + 1;
    }
    s = lo;
    const int64_t* __restrict__ row = table + int64_t(s) * TC;
    const int64_t r = idx - (s > 0 ? row[3 - TC] : 0);
    const int64_t W = row[2], nx = W - T + 1;
    y0 = int(r / nx);
    x0 = int(r % nx);
    view = int(w[2] & uint32_t(views - 1));
    return sp_invalid(prefix, row, y0, x0, T);
}

constexpr int OC = NIRGAN_SCENE_ORIGIN_COLS;

// One attempt of nirgan_scene_sample_origins: the window of side T that the words w name among the `total` origins of the `count`
// rows {scene, oy, ox, oh, ow, cum} at `rows` (the rows of ONE scale, cum running from its first row), and the number of invalid
// pixels it holds (0 without a prefix table).  table: the [S][TC] scene table (W_s and the prefix offset are read).
__device__ __forceinline__ int64_t so_attempt(const uint32_t w[4], const int64_t* __restrict__ table, const int64_t* __restrict__ rows, int count,
                                              const int32_t* __restrict__ prefix, int T, int64_t total, int views, int& s, int& y0, int& x0, int& view) {
    const uint64_t u = uint64_t(w[0]) | (uint64_t(w[1]) << 32);
    const int64_t idx = int64_t(__umul64hi(u, uint64_t(total)));                // < total
    int lo = 0, hi = count - 1;                                                 // the first row with cum > idx (cum[count-1] = total > idx)
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (rows[int64_t(mid) * OC + 5] > idx) hi = mid; else lo = mid + 1;
    }
    const int64_t* __restrict__ row = rows + int64_t(lo) * OC;
    const int64_t r = idx - (lo > 0 ? row[5 - OC] : 0);
    const int64_t ow = row[4];
    s = int(row[0]);
    y0 = int(row[1] + r / ow);
    x0 = int(row[2] + r % ow);
    view = int(w[2] & uint32_t(views - 1));
    return sp_invalid(prefix, table + int64_t(s) * TC, y0, x0, T);
}

// coords[b] of a window of side T at (y0, x0) of a scene with geotransform g = (lon0, dlon, lat0, dlat)
__device__ __forceinline__ void sp_centre(const double* __restrict__ g, int y0, int x0, int T, float* __restrict__ out) {
    const double cx = double(x0 + T / 2) + 0.5, cy = double(y0 + T / 2) + 0.5;  // exact
    out[0] = float(sp_mul_then_add(g[0], cx, g[1]));
    out[1] = float(sp_mul_then_add(g[2], cy, g[3]));
}

// the extents of scenes s0 .. s1-1 of a [S][TC] host table: sp_check_table asks scene by scene, between its other checks; an entry
// that reads no cum_windows asks for all S at once
static inline int sp_check_sides(const char* who, const int64_t* table_host, int s0, int s1) {
    for (int s = s0; s < s1; ++s) {
        const int64_t* r = table_host + int64_t(s) * TC;
        NG_REQUIRE(r[1] > 0 && r[1] < LIM31 && r[2] > 0 && r[2] < LIM31, "%s: scene %d has an extent outside 1 .. 2^31-1", who, s);
    }
    return NIRGAN_OK;
}

// the argument checks of one [S][TC] host table for windows of side T; on success *total_out = cum_windows[S-1] (which may be 0)
static inline int sp_check_table(const char* who, const int64_t* table_host, int S, int64_t T, int64_t* total_out) {
    int64_t total = 0;
    for (int s = 0; s < S; ++s) {
        const int64_t* r = table_host + int64_t(s) * TC;
        if (int e = sp_check_sides(who, table_host, s, s + 1)) return e;
        if (r[1] >= T && r[2] >= T) total += (r[1] - T + 1) * (r[2] - T + 1);   // each term below 2^62: the sum cannot wrap before the bound
        NG_REQUIRE(total < (int64_t(1) << 62), "%s: the pool has 2^62 windows or more", who);
        NG_REQUIRE(r[3] == total, "%s: cum_windows of scene %d is not the running window count for tile %lld", who, s, (long long)T);
    }
    *total_out = total;
    return NIRGAN_OK;
}

// ... and, once a table is known to hold a window, where its scenes and prefix tables lie (with_prefix = false: column 4 is not read)
static inline int sp_check_extents(const char* who, const int64_t* table_host, int S, int C, int64_t pool_elems, const void* prefix,
                                   int64_t prefix_elems, bool with_prefix = true) {
    for (int s = 0; s < S; ++s) {
        const int64_t* r = table_host + int64_t(s) * TC;
        NG_REQUIRE(r[0] >= 0 && r[0] <= pool_elems && r[1] * r[2] <= (pool_elems - r[0]) / C, "%s: scene %d lies outside the pool", who, s);
        if (with_prefix && r[4] >= 0) {
            NG_REQUIRE(prefix, "%s: scene %d names a prefix table but prefix is null", who, s);
            NG_REQUIRE(r[4] <= prefix_elems && (r[1] + 1) * (r[2] + 1) <= prefix_elems - r[4], "%s: the prefix table of scene %d lies outside prefix_elems", who, s);
        }
    }
    return NIRGAN_OK;
}
