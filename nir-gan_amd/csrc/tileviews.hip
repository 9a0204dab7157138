// Dihedral test-time augmentation of tiles: nirgan_tile_views_expand / nirgan_tile_views_merge.
//
// View g of an H x W plane x (bit 0 mirrors columns, bit 1 mirrors rows, bit 2 transposes; the header states it in full):
//     view_g(x)[i][j] = x[i'][j'],  (a, b) = bit 2 ? (j, i) : (i, j),  i' = bit 1 ? H-1-a : a,  j' = bit 0 ? W-1-b : b.
// Source element (p, q) therefore lands at (f1(p), f0(q)) of a plain view and at (f0(q), f1(p)) of a transposing one, with
// f1(p) = bit 1 ? H-1-p : p and f0(q) = bit 0 ? W-1-q : q.
//
// Both kernels give one 256-thread block a TV_B x TV_B block of one plane, grid-strided.  The plain views (0 .. 3) never leave the
// registers: a thread owns four pixels consecutive in x ("quad") of four rows, a mirrored row is the same quads stored (loaded) at
// W-4-q with their elements reversed, so global access stays row-contiguous and 16 bytes wide where the host found the base
// addresses and W to allow it.  The transposing views (4 .. 7) go through LDS with a row padded to TV_B + 1 floats: the quad side
// touches it row-wise, the other side column-wise with one dword per lane, lanes along the view's row (256 contiguous bytes per wave,
// ascending or descending), and neither side has a bank conflict -- row-wise because the 32 lanes of a half wave are laid out as
// 4 rows x 8 quads (bank = row + 4 quad + e mod 32 is then a bijection), column-wise because 65 is odd.
// Expand reads a source block once and writes it k times; merge reads the k view blocks once, sums them in registers in the fixed
// tree ((v0+v1)+(v2+v3))+((v4+v5)+(v6+v7)) with plain fp32 adds, multiplies by 1/k (exact) and stores once.  No atomics; every
// destination element has one owner, so neither destination needs initialisation.
#include "common.h"

namespace {

constexpr int TV_B = 64;                 // side of the staged block
constexpr int TV_LD = TV_B + 1;          // padded LDS row

struct ViewsP {
    const float* src; float* dst;
    int C, H, W, k, bh, bw;              // bh x bw blocks per plane
    int64_t nblk;                        // n * C * bh * bw
    int vec_src, vec_dst;                // 16-byte accesses allowed on that side (alignment of the base and of every row)
};

// the quad side: thread -> (row inside a 16-row pass, quad of the block's 16); a half wave is 4 rows x 8 quads
__device__ __forceinline__ int tv_quad_col(int t) { return (t & 7) + (((t & 63) >> 5) << 3); }
__device__ __forceinline__ int tv_quad_row(int t) { return ((t >> 6) << 2) + ((t & 31) >> 3); }

__device__ __forceinline__ f32x4 tv_reverse(f32x4 v) {
    f32x4 u;
    u.x = v.w; u.y = v.z; u.z = v.y; u.w = v.x;
    return u;
}

// the quad x[row][q .. q+3] of a plain view's plane as the source quad (q .. q+3): mirrored columns sit at W-1-q-e
__device__ __forceinline__ f32x4 tv_load_quad(const float* __restrict__ row, int q, int W, bool mirror, bool vec) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (vec) {                                                                  // W % 4 == 0: the quad is whole, W-4-q is a multiple of 4
        v = *reinterpret_cast<const f32x4*>(row + (mirror ? W - 4 - q : q));
        return mirror ? tv_reverse(v) : v;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (q + e < W) v[e] = row[mirror ? W - 1 - q - e : q + e];
    return v;
}

__device__ __forceinline__ void tv_store_quad(float* __restrict__ row, int q, int W, bool mirror, bool vec, f32x4 v) {
    if (vec) {
        *reinterpret_cast<f32x4*>(row + (mirror ? W - 4 - q : q)) = mirror ? tv_reverse(v) : v;
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (q + e < W) row[mirror ? W - 1 - q - e : q + e] = v[e];
}

struct BlockAt { int64_t plane_id; int r0, c0; };                               // plane_id = image * C + c

__device__ __forceinline__ BlockAt tv_block(const ViewsP& p, int64_t blk) {
    BlockAt b;
    b.c0 = int(blk % p.bw) * TV_B;
    int64_t r = blk / p.bw;
    b.r0 = int(r % p.bh) * TV_B;
    b.plane_id = r / p.bh;
    return b;
}

__global__ __launch_bounds__(256) void tile_views_expand_kernel(const ViewsP p) {
    __shared__ float lds[TV_B * TV_LD];
    const int t = threadIdx.x;
    const int qc = tv_quad_col(t), qr = tv_quad_row(t);
    const int64_t plane = int64_t(p.H) * p.W, vstride = int64_t(p.C) * plane;   // view g of an image starts g * vstride after view 0
    for (int64_t blk = blockIdx.x; blk < p.nblk; blk += gridDim.x) {
        const BlockAt b = tv_block(p, blk);
        const int64_t img = b.plane_id / p.C;
        const int c = int(b.plane_id - img * p.C);
        const float* __restrict__ src = p.src + b.plane_id * plane;
        float* __restrict__ dst = p.dst + (img * p.k * p.C + c) * plane;
        const int q = b.c0 + 4 * qc;
        f32x4 v[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = b.r0 + qr + 16 * s;
            v[s] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (row < p.H && q < p.W) {
                v[s] = tv_load_quad(src + int64_t(row) * p.W, q, p.W, false, p.vec_src);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (g >= p.k) break;
                    const int i = (g & 2) ? p.H - 1 - row : row;
                    tv_store_quad(dst + g * vstride + int64_t(i) * p.W, q, p.W, (g & 1) != 0, p.vec_dst, v[s]);
                }
            }
        }
        if (p.k == 8) {                                                         // H == W
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int e = 0; e < 4; ++e) lds[(qr + 16 * s) * TV_LD + 4 * qc + e] = v[s][e];
            __syncthreads();
            const int lp = t & 63, pp = b.r0 + lp;                              // the lane's source row = the views' column
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
                const int lq = (t >> 6) + 4 * s, qq = b.c0 + lq;                // source column = the views' row
                if (pp < p.H && qq < p.W) {
                    const float val = lds[lp * TV_LD + lq];
#pragma unroll
                    for (int g = 4; g < 8; ++g) {
                        const int i = (g & 1) ? p.W - 1 - qq : qq, j = (g & 2) ? p.H - 1 - pp : pp;
                        dst[g * vstride + int64_t(i) * p.W + j] = val;
                    }
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void tile_views_merge_kernel(const ViewsP p) {
    __shared__ float lds[2][TV_B * TV_LD];
    const int t = threadIdx.x;
    const int qc = tv_quad_col(t), qr = tv_quad_row(t);
    const int64_t plane = int64_t(p.H) * p.W, vstride = int64_t(p.C) * plane;
    const float inv = 1.0f / float(p.k);
    for (int64_t blk = blockIdx.x; blk < p.nblk; blk += gridDim.x) {
        const BlockAt b = tv_block(p, blk);
        const int64_t img = b.plane_id / p.C;
        const int c = int(b.plane_id - img * p.C);
        const float* __restrict__ src = p.src + (img * p.k * p.C + c) * plane;
        float* __restrict__ dst = p.dst + b.plane_id * plane;
        const int q = b.c0 + 4 * qc;
        f32x4 acc[4], t45[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = b.r0 + qr + 16 * s;
            acc[s] = t45[s] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (row < p.H && q < p.W) {
                f32x4 v[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    v[g] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    if (g < p.k) {
                        const int i = (g & 2) ? p.H - 1 - row : row;
                        v[g] = tv_load_quad(src + g * vstride + int64_t(i) * p.W, q, p.W, (g & 1) != 0, p.vec_src);
                    }
                }
                acc[s] = v[0];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (p.k >= 2) acc[s][e] = __fadd_rn(v[0][e], v[1][e]);
                    if (p.k >= 4) acc[s][e] = __fadd_rn(acc[s][e], __fadd_rn(v[2][e], v[3][e]));
                }
            }
        }
        if (p.k == 8) {                                                         // H == W
            const int lp = t & 63, pp = b.r0 + lp;
            for (int half = 0; half < 2; ++half) {
                __syncthreads();                                                // the previous pair has been read
#pragma unroll 4
                for (int s = 0; s < 16; ++s) {
                    const int lq = (t >> 6) + 4 * s, qq = b.c0 + lq;
                    if (pp < p.H && qq < p.W) {
#pragma unroll
                        for (int z = 0; z < 2; ++z) {
                            const int g = 4 + 2 * half + z;
                            const int i = (g & 1) ? p.W - 1 - qq : qq, j = (g & 2) ? p.H - 1 - pp : pp;
                            lds[z][lp * TV_LD + lq] = src[g * vstride + int64_t(i) * p.W + j];
                        }
                    }
                }
                __syncthreads();
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int at = (qr + 16 * s) * TV_LD + 4 * qc + e;      // past the plane's edge: stale values, never stored
                        const float pair = __fadd_rn(lds[0][at], lds[1][at]);
                        if (half == 0) t45[s][e] = pair;
                        else acc[s][e] = __fadd_rn(acc[s][e], __fadd_rn(t45[s][e], pair));
                    }
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = b.r0 + qr + 16 * s;
            if (row < p.H && q < p.W) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = __fmul_rn(acc[s][e], inv);
                tv_store_quad(dst + int64_t(row) * p.W, q, p.W, false, p.vec_dst, o);
            }
        }
    }
}

int views_params(ViewsP& p, const nirgan_tile_views_desc* d, const char* who) {
    NG_REQUIRE(d && d->src && d->dst, "%s: null pointer", who);
    NG_REQUIRE(d->views == 1 || d->views == 2 || d->views == 4 || d->views == 8, "%s: views %d is not 1, 2, 4 or 8", who, d->views);
    NG_REQUIRE(d->n > 0 && d->C > 0 && d->H > 0 && d->W > 0, "%s: bad shape (n %d, C %d, H %d, W %d)", who, d->n, d->C, d->H, d->W);
    NG_REQUIRE(d->views != 8 || d->H == d->W, "%s: views 8 needs a square plane, got %d x %d", who, d->H, d->W);
    NG_REQUIRE(int64_t(d->H) * d->W < (1ll << 31) && int64_t(d->n) * d->views * d->C < (1ll << 31),
               "%s: a plane or the plane count (n * views * C) is 2^31 or more", who);
    p.src = d->src; p.dst = d->dst;
    p.C = d->C; p.H = d->H; p.W = d->W; p.k = d->views;
    p.bh = (d->H + TV_B - 1) / TV_B; p.bw = (d->W + TV_B - 1) / TV_B;
    p.nblk = int64_t(d->n) * d->C * p.bh * p.bw;
    p.vec_src = d->W % 4 == 0 && ng_aligned16(d->src);
    p.vec_dst = d->W % 4 == 0 && ng_aligned16(d->dst);
    return NIRGAN_OK;
}

inline int views_grid(int64_t nblk) { return int(nblk < 4096 ? nblk : 4096); }

}  // namespace

extern "C" int nirgan_tile_views_expand(const nirgan_tile_views_desc* d, void* stream) {
    ViewsP p;
    const int rc = views_params(p, d, "tile_views_expand");
    if (rc != NIRGAN_OK) return rc;
    hipLaunchKernelGGL(tile_views_expand_kernel, dim3(views_grid(p.nblk)), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return nirgan_check_launch("tile_views_expand");
}

extern "C" int nirgan_tile_views_merge(const nirgan_tile_views_desc* d, void* stream) {
    ViewsP p;
    const int rc = views_params(p, d, "tile_views_merge");
    if (rc != NIRGAN_OK) return rc;
    hipLaunchKernelGGL(tile_views_merge_kernel, dim3(views_grid(p.nblk)), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return nirgan_check_launch("tile_views_merge");
}
