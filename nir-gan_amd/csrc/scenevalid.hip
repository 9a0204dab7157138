// Valid-pixel masks of scene-pool windows:
//   nirgan_scene_valid   the mask that belongs to a list of window rows, from the scenes' invalid-prefix tables: one launch;
//   nirgan_valid_count   how many elements of a mask are set: the common divisor of the masked pixel losses (losses_masked.hip).
// The mask kernel has the shape of the gather of scenesample.hip: 64 x 64 blocks of D, a wave per row of D with its lanes along the
// source row, transposing views turned through the padded LDS tile.  A lane reads the four corners of its own f x f block -- its
// right corners are its neighbour's left ones and come out of the same cache lines -- with clamped addresses and no predicate.
#include "scene_dev.h"

namespace {

struct ValidP {
    const int64_t* table;                // [S][TC]: columns 1, 2, 4 are read on the device
    const int32_t* prefix;               // or null: every window inside its scene is all ones
    const int32_t* rows;                 // the first row of the call
    float* valid;                        // [n][1][T][T]
    int S, T, nb;                        // nb: blocks per tile side
    int64_t nblk;                        // n * nb * nb
};

__global__ __launch_bounds__(256) void scene_valid_kernel(const ValidP p) {
    __shared__ float tile[SP_B * SP_LD];
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    const int Tt = p.T;
    const int64_t tt = int64_t(Tt) * Tt;
    for (int64_t blk = blockIdx.x; blk < p.nblk; blk += gridDim.x) {
        const int dc0 = int(blk % p.nb) * SP_B;
        int64_t r = blk / p.nb;
        const int dr0 = int(r % p.nb) * SP_B;
        const int64_t b = r / p.nb;
        const int32_t* __restrict__ win = p.rows + b * 4;
        const int s = win[0], y0 = win[1], x0 = win[2], view = win[3] & 7, f = ((win[3] >> 16) & 7) + 1;
        float* __restrict__ out = p.valid + b * tt;
        // Everything up to the loop is uniform over the block.  A row that does not lie inside a scene reads nothing of the tables
        // and gives zeros; a scene without a table gives ones.
        const int32_t* __restrict__ P = nullptr;
        int64_t ld = 0;
        float flat = 0.f;
        if (s >= 0 && s < p.S && y0 >= 0 && x0 >= 0) {
            const int64_t* __restrict__ row = p.table + int64_t(s) * TC;
            const int64_t L = int64_t(f) * Tt;
            if (y0 + L <= row[1] && x0 + L <= row[2]) {
                flat = 1.f;
                if (p.prefix && row[4] >= 0) {
                    P = p.prefix + row[4];
                    ld = row[2] + 1;
                }
            }
        }
        const int nc = Tt - dc0 < SP_B ? Tt - dc0 : SP_B;                       // D columns of this block
        const int qc = dc0 + (lx < nc ? lx : nc - 1);                           // a lane past the block reads the last column instead
        const int q = dc0 + lx, qo = (view & 1) ? Tt - 1 - q : q;
#pragma unroll 1
        for (int k0 = 0; k0 < 16; k0 += 4) {
            if (dr0 + ly + 4 * k0 >= Tt) break;                                 // wave-uniform, as every pr below
            float v[4] = {flat, flat, flat, flat};
            if (P) {
                int c[4][4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {                                   // sixteen loads in flight; a row past the tile reads the last one
                    const int pr = dr0 + ly + 4 * (k0 + u);
                    const int32_t* __restrict__ top = P + (int64_t(y0) + int64_t(pr < Tt ? pr : Tt - 1) * f) * ld + x0 + int64_t(qc) * f;
                    c[u][0] = top[0];
                    c[u][1] = top[f];
                    c[u][2] = top[int64_t(f) * ld];
                    c[u][3] = top[int64_t(f) * ld + f];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = (c[u][3] - c[u][1] - c[u][2] + c[u][0]) == 0 ? 1.f : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int pl = ly + 4 * (k0 + u), pr = dr0 + pl;
                if (pr >= Tt) break;
                if (lx < nc) {
                    if (!(view & 4)) out[int64_t((view & 2) ? Tt - 1 - pr : pr) * Tt + qo] = v[u];
                    else tile[pl * SP_LD + lx] = v[u];
                }
            }
        }
        if (view & 4) {
            // out[i][j] = D[f2(j)][f1(i)]: the lanes run along j, which is D's row
            __syncthreads();
            const int pr = dr0 + lx, j = (view & 2) ? Tt - 1 - pr : pr;
            if (pr < Tt) {
#pragma unroll 4
                for (int k = 0; k < 16; ++k) {
                    const int ql = ly + 4 * k, qq = dc0 + ql;
                    if (qq < Tt) out[int64_t((view & 1) ? Tt - 1 - qq : qq) * Tt + j] = tile[lx * SP_LD + ql];
                }
            }
            __syncthreads();                                                    // the next block of the grid-stride loop writes tile again
        }
    }
}

// Integer counts: exact in any order.  A thread counts sixteen elements per trip, the block adds its count once.
__global__ __launch_bounds__(256) void valid_count_kernel(const float* __restrict__ valid, int64_t n, int32_t* __restrict__ count) {
    __shared__ int part[4];
    int c = 0;
    const int64_t stride = int64_t(gridDim.x) * 256 * 16;
    for (int64_t i0 = int64_t(blockIdx.x) * 256 * 16 + threadIdx.x; i0 < n; i0 += stride) {
        float x[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int64_t i = i0 + j * 256;
            x[j] = i < n ? valid[i] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) c += x[j] != 0.f ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = part[0] + part[1] + part[2] + part[3];
        if (t) atomicAdd(count, t);
    }
}

}  // namespace

extern "C" int nirgan_scene_valid(const nirgan_scene_valid_desc* d, void* stream) {
    static const char* who = "scene_valid";
    NG_REQUIRE(d && d->table && d->table_host && d->window && d->valid, "%s: null pointer", who);
    NG_REQUIRE(d->S > 0, "%s: bad pool (S %d)", who, d->S);
    const int64_t T = d->tile;
    NG_REQUIRE(d->n > 0 && T > 0 && T * T < LIM31 && T * T * d->n < LIM31, "%s: n, tile or n*tile*tile is not in 1 .. 2^31-1 (n %d, tile %d)", who, d->n, d->tile);
    NG_REQUIRE(d->first >= 0 && d->n_windows >= d->n && d->first <= d->n_windows - d->n,
               "%s: first %lld, n %d: the rows are not inside 0 .. n_windows-1 (n_windows %lld)", who, (long long)d->first, d->n, (long long)d->n_windows);
    NG_REQUIRE(d->prefix_elems >= 0, "%s: negative prefix_elems", who);
    if (int e = sp_check_sides(who, d->table_host, 0, d->S)) return e;
    if (d->prefix)
        for (int s = 0; s < d->S; ++s) {
            const int64_t* r = d->table_host + int64_t(s) * TC;
            NG_REQUIRE(r[4] < 0 || (r[4] <= d->prefix_elems && (r[1] + 1) * (r[2] + 1) <= d->prefix_elems - r[4]),
                       "%s: the prefix table of scene %d lies outside prefix_elems", who, s);
        }
    if (d->window_host)
        for (int64_t i = d->first; i < d->first + d->n; ++i) {
            const int32_t* w = d->window_host + i * 4;
            const uint32_t word = uint32_t(w[3]);
            NG_REQUIRE((word & ~0x8007FF07u) == 0, "%s: row %lld: the word 0x%08x has a bit set outside the view, attempt, factor and exhausted fields", who, (long long)i, word);
            NG_REQUIRE(w[0] >= 0 && w[0] < d->S, "%s: row %lld: scene %d outside 0 .. S-1", who, (long long)i, w[0]);
            const int f = int((word >> 16) & 7) + 1;
            const int64_t L = f * T;
            NG_REQUIRE(L * L < LIM31, "%s: row %lld: the window of factor %d, (factor*tile)^2, is 2^31 or more", who, (long long)i, f);
            const int64_t* r = d->table_host + int64_t(w[0]) * TC;
            NG_REQUIRE(w[1] >= 0 && w[2] >= 0 && w[1] + L <= r[1] && w[2] + L <= r[2],
                       "%s: row %lld: the window of side %lld at (%d, %d) is not inside scene %d (%lld x %lld)", who, (long long)i, (long long)L, w[1], w[2], w[0],
                       (long long)r[1], (long long)r[2]);
        }
    ValidP p = {};
    p.table = d->table; p.prefix = d->prefix; p.rows = d->window + d->first * 4; p.valid = d->valid;
    p.S = d->S; p.T = d->tile;
    p.nb = (d->tile + SP_B - 1) / SP_B;
    p.nblk = int64_t(d->n) * p.nb * p.nb;
    const int grid = int(p.nblk < 16384 ? p.nblk : 16384);
    hipLaunchKernelGGL(scene_valid_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return nirgan_check_launch(who);
}

extern "C" int nirgan_valid_count(const float* valid, int64_t n, int32_t* count, void* stream) {
    static const char* who = "valid_count";
    NG_REQUIRE(valid && count, "%s: null pointer", who);
    NG_REQUIRE(n > 0 && n < LIM31, "%s: n %lld is not in 1 .. 2^31-1", who, (long long)n);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    (void)hipMemsetAsync(count, 0, sizeof(int32_t), st);                        // a failure is the last error that the check below reads
    const int64_t blocks = (n + 4095) / 4096;
    hipLaunchKernelGGL(valid_count_kernel, dim3(int(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, valid, n, count);
    return nirgan_check_launch(who);
}
