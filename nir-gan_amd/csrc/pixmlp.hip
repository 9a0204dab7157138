// Per-pixel baseline models (reference model/baseline_models.py: Linear_NIR :17-30, MLP_NIR :80-100) as fused kernels.
//
//   hidden = 0   y = w . x + b                                         (nn.Linear(3, 1))
//   hidden = 64  y = W3 . relu(W2 . relu(W1 . x + b1) + b2) + b3       (nn.Sequential(Linear(3,64), ReLU, Linear(64,64), ReLU, Linear(64,1)))
//
// on the boundary tensors as they are (rgb [B][3][H][W], nir / pred [B][1][H][W], fp32 NCHW): a pixel's inputs are three plane
// reads at one offset.  Parameters are read in place from the network's flat fp32 range (nirgan_hip/flat.py: state_dict order, every
// tensor padded to 4 floats); gradients leave in the same layout.
//
// The hidden = 64 train kernel walks 32-pixel tiles, one wave per tile, persistent workgroups of four waves (one per CU, up to 512
// registers per lane).  Per tile, everything between the 16 input bytes and the gradient sums stays on chip:
//   * z2 = h1 . W2^T            v_mfma_f32_32x32x2_f32, M = pixel, N = j, K = k.  The A operand h1[p][k] is COMPUTED by the lane that
//                               feeds it (its pixel's three colours are in its registers, W1 row k is an LDS broadcast read); the B
//                               operand is a W2 fragment held in registers for the whole kernel.
//   * y, dy, relu masks, dW3, db2, db3, loss: VALU on the accumulator layout (a lane owns one j per 32-column tile and 16 pixels).
//   * dW2 += dz2^T . h1         M = j, N = k, K = pixel.  The K slot (step r, lane half) is mapped to the pixel that accumulator
//                               register r of that half holds, so dz2 IS the A operand as it stands; the B operand h1[p][k] is computed
//                               again, now for the lane's two k and the 16 pixels of its half (colours from a 512-byte LDS tile).
//   * dh1 = dz2 . W2            M = pixel, N = k, K = j: the one real layout change.  dz2 goes through a per-wave LDS tile
//                               [32 pixels][64 + 4] (row pad 4: the 16-byte reads of 16 lanes cover all 64 banks once) and comes back as
//                               the A operand; B is the second W2 fragment set.
//   * dz1, dW1, db1: VALU on the accumulator layout of dh1 (the mask is the recomputed h1).
// A wave keeps its gradient sums in registers for its whole walk; at the end the four waves add theirs into one LDS record in wave
// order and the workgroup writes record [P + 4] (flat gradient layout, then the squared-error sum) to the workspace.  A second launch
// adds the records in workgroup order.  No float atomics; the grid depends on the shape only: two runs are bitwise equal.
#include "common.h"

namespace {

constexpr int PT = NIRGAN_PIXMLP_TILE;          // pixels per wave tile (hidden = 64)
constexpr int MLP_GRID = 256;                   // persistent workgroups: one per CU of the MI355X -- a CONSTANT of this gfx950-only
                                                // library, not a device query: the entries keep no state and ws_elems needs no device
constexpr int MLP_P = 4484;                     // flat range: W1 192, b1 64, W2 4096, b2 64, W3 64, b3 1 (+3)
constexpr int MLP_REC = MLP_P + 4;              // + squared-error sum, padded
constexpr int O_W1 = 0, O_B1 = 192, O_W2 = 256, O_B2 = 4352, O_W3 = 4416, O_B3 = 4480;
constexpr int LIN_GRID = 2048, LIN_BLOCK = 256;
constexpr int LIN_P = 8;                        // w 3 (+1), b 1 (+3)
constexpr int LIN_REC = LIN_P + 4;
constexpr int TS = 68;                          // row stride of the dz2 transposition tile

struct PixP {
    const float* rgb; const float* tgt; const float* params;
    float* pred; float* ws;
    unsigned n; int HW; int ntiles;
    int from_dpred;                             // tgt holds d loss / d pred instead of the target
    float scale;                                // 2 / n
};

__device__ __forceinline__ void wave_sync() {   // LDS written by some lanes of this wave, read by others: program order, no reordering
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float hidden1(const f32x4 w, float x0, float x1, float x2) {     // relu(W1[k] . x + b1[k]), one association everywhere
    return fmaxf(fmaf(w.z, x2, fmaf(w.y, x1, fmaf(w.x, x0, w.w))), 0.f);
}

// pixel of accumulator register r in lane half `half` of a 32 x 32 MFMA tile whose rows are the tile's pixels
__device__ __forceinline__ int acc_pixel(int r, int half) { return 8 * (r >> 2) + 4 * half + (r & 3); }

template <bool TRAIN>
struct TileIn {                                 // what a wave fetches from HBM for one tile
    float x0, x1, x2;                           // colours of pixel base + (lane & 31)
    float tq[TRAIN ? 16 : 1];                   // target (or d loss / d pred) of the 16 pixels this half's accumulator registers hold
};

template <bool TRAIN>
__device__ __forceinline__ void fetch_tile(const PixP& p, int tile, int l32, int half, TileIn<TRAIN>& t) {
    const unsigned base = unsigned(tile) * PT;
    const unsigned i = base + l32;
    t.x0 = t.x1 = t.x2 = 0.f;
    if (tile < p.ntiles && i < p.n) {
        const unsigned b = i / unsigned(p.HW), px = i - b * unsigned(p.HW);
        const float* q = p.rgb + size_t(b) * 3 * p.HW + px;
        t.x0 = q[0];
        t.x1 = q[p.HW];
        t.x2 = q[2 * size_t(p.HW)];
    }
    if constexpr (TRAIN) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned ir = base + acc_pixel(r, half);
            t.tq[r] = (tile < p.ntiles && ir < p.n) ? p.tgt[ir] : 0.f;
        }
    }
}

template <bool TRAIN>
__global__ __launch_bounds__(256) void pixmlp64_kernel(const PixP p) {
    __shared__ f32x4 w1tab[64];                                 // (W1[k][0..2], b1[k])
    __shared__ f32x4 xs[TRAIN ? 4 : 1][PT];                     // per wave: the tile's colours
    __shared__ __attribute__((aligned(16))) float tr[TRAIN ? 4 : 1][TRAIN ? PT * TS : 4];
    __shared__ float rec[TRAIN ? MLP_REC : 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l32 = lane & 31;
    const float* __restrict__ prm = p.params;
    if (threadIdx.x < 64) {
        const int k = threadIdx.x;
        w1tab[k] = f32x4{prm[O_W1 + 3 * k], prm[O_W1 + 3 * k + 1], prm[O_W1 + 3 * k + 2], prm[O_B1 + k]};
    }
    float w2a[2][32];                                           // B of z2: W2[j = l32 + 32 nt][k = 2 s + half]
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int s = 0; s < 32; ++s) w2a[nt][s] = prm[O_W2 + (l32 + 32 * nt) * 64 + 2 * s + half];
    float w2b[2][TRAIN ? 32 : 1];                               // B of dh1: W2[j = 8 (s / 4) + 4 half + s % 4][k = l32 + 32 nt]
    if constexpr (TRAIN) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int s = 0; s < 32; ++s) w2b[nt][s] = prm[O_W2 + acc_pixel(s, half) * 64 + l32 + 32 * nt];
    }
    const float b2v[2] = {prm[O_B2 + l32], prm[O_B2 + l32 + 32]};
    const float w3v[2] = {prm[O_W3 + l32], prm[O_W3 + l32 + 32]};
    const float b3v = prm[O_B3];
    __syncthreads();
    const f32x4 w1k[2] = {w1tab[l32], w1tab[l32 + 32]};

    f32x16 dW2[2][2];
    float dW1[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, db1[2] = {0.f, 0.f}, db2[2] = {0.f, 0.f}, dW3[2] = {0.f, 0.f}, db3 = 0.f, loss = 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) dW2[a][b][r] = 0.f;

    const int stride = gridDim.x * 4;
    TileIn<TRAIN> nxt;
    fetch_tile<TRAIN>(p, blockIdx.x * 4 + wave, l32, half, nxt);
    for (int tile = blockIdx.x * 4 + wave; tile < p.ntiles; tile += stride) {
        const unsigned base = unsigned(tile) * PT;
        const TileIn<TRAIN> cur = nxt;
        fetch_tile<TRAIN>(p, tile + stride, l32, half, nxt);    // the next tile's 16 bytes per pixel are in flight under this tile's MFMAs
        const float x0 = cur.x0, x1 = cur.x1, x2 = cur.x2;
        if constexpr (TRAIN) {
            if (half == 0) xs[wave][l32] = f32x4{x0, x1, x2, 0.f};
        }
        // ---- z2 = h1 . W2^T + b2
        f32x16 acc[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[0][r] = b2v[0];
            acc[1][r] = b2v[1];
        }
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            const float h = hidden1(w1tab[2 * s + half], x0, x1, x2);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(h, w2a[0][s], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(h, w2a[1][s], acc[1], 0, 0, 0);
        }
        // ---- y = W3 . relu(z2) + b3: the lane's two j, then the 32 lanes of the half (every lane ends with the same bits)
        float y[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = fmaf(w3v[1], fmaxf(acc[1][r], 0.f), w3v[0] * fmaxf(acc[0][r], 0.f));
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            y[r] = v + b3v;
        }
        if (p.pred) {
            float ysel = y[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) ysel = l32 == r ? y[r] : ysel;
            const unsigned ip = base + acc_pixel(l32 & 15, half);
            if (l32 < 16 && ip < p.n) p.pred[ip] = ysel;
        }
        if constexpr (TRAIN) {
            float dy[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned ir = base + acc_pixel(r, half);
                if (p.from_dpred) {
                    dy[r] = cur.tq[r];
                } else {
                    const float d = ir < p.n ? y[r] - cur.tq[r] : 0.f;
                    loss = fmaf(d, d, loss);
                    dy[r] = d * p.scale;
                }
                db3 += dy[r];
            }
            // ---- dz2 (accumulator layout), dW3, db2
            f32x16 dz[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool on = acc[nt][r] > 0.f;
                    dW3[nt] = fmaf(dy[r], on ? acc[nt][r] : 0.f, dW3[nt]);
                    const float g = on ? dy[r] * w3v[nt] : 0.f;
                    dz[nt][r] = g;
                    db2[nt] += g;
                }
            wave_sync();                                        // xs is written
            // ---- h1 again, as the B operand of dW2 and the mask of dz1: k = l32 + 32 nt, the pixel of accumulator register r
            float hB[2][16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const f32x4 xr = xs[wave][acc_pixel(r, half)];
                hB[0][r] = hidden1(w1k[0], xr.x, xr.y, xr.z);
                hB[1][r] = hidden1(w1k[1], xr.x, xr.y, xr.z);
            }
            // ---- dW2 += dz2^T . h1
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
                        dW2[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(dz[mt][r], hB[nt][r], dW2[mt][nt], 0, 0, 0);
            // ---- dz2 to the operand layout of dh1 = dz2 . W2
            float* t = tr[wave];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) t[acc_pixel(r, half) * TS + l32 + 32 * nt] = dz[nt][r];
            wave_sync();
            f32x16 dh[2];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                dh[0][r] = 0.f;
                dh[1][r] = 0.f;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(&t[l32 * TS + 8 * q + 4 * half]);      // j = acc_pixel(4 q + c, half)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    dh[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c], w2b[0][4 * q + c], dh[0], 0, 0, 0);
                    dh[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[c], w2b[1][4 * q + c], dh[1], 0, 0, 0);
                }
            }
            // ---- dz1 = dh1 . [h1 > 0]; dW1, db1
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const f32x4 xr = xs[wave][acc_pixel(r, half)];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const float g = hB[nt][r] > 0.f ? dh[nt][r] : 0.f;
                    db1[nt] += g;
                    dW1[nt][0] = fmaf(g, xr.x, dW1[nt][0]);
                    dW1[nt][1] = fmaf(g, xr.y, dW1[nt][1]);
                    dW1[nt][2] = fmaf(g, xr.z, dW1[nt][2]);
                }
            }
            wave_sync();                                        // the next tile overwrites xs and the transposition tile
        }
    }

    if constexpr (TRAIN) {
        // the four waves add their sums into the record in wave order
        for (int w = 0; w < 4; ++w) {
            if (wave == w) {
                const bool first = w == 0;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int idx = O_W2 + (32 * mt + acc_pixel(r, half)) * 64 + l32 + 32 * nt;
                            rec[idx] = (first ? 0.f : rec[idx]) + dW2[mt][nt][r];
                        }
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const int k = l32 + 32 * nt;
                    float v[6] = {dW1[nt][0], dW1[nt][1], dW1[nt][2], db1[nt], db2[nt], dW3[nt]};
#pragma unroll
                    for (int e = 0; e < 6; ++e) v[e] += __shfl_xor(v[e], 32, 64);        // the two halves hold different pixels
                    if (half == 0) {
                        rec[O_W1 + 3 * k + 0] = (first ? 0.f : rec[O_W1 + 3 * k + 0]) + v[0];
                        rec[O_W1 + 3 * k + 1] = (first ? 0.f : rec[O_W1 + 3 * k + 1]) + v[1];
                        rec[O_W1 + 3 * k + 2] = (first ? 0.f : rec[O_W1 + 3 * k + 2]) + v[2];
                        rec[O_B1 + k] = (first ? 0.f : rec[O_B1 + k]) + v[3];
                        rec[O_B2 + k] = (first ? 0.f : rec[O_B2 + k]) + v[4];
                        rec[O_W3 + k] = (first ? 0.f : rec[O_W3 + k]) + v[5];
                    }
                }
                const float sb = db3 + __shfl_xor(db3, 32, 64), sl = loss + __shfl_xor(loss, 32, 64);
                if (lane == 0) {
                    rec[O_B3] = (first ? 0.f : rec[O_B3]) + sb;
                    rec[MLP_P] = (first ? 0.f : rec[MLP_P]) + sl;
                    if (first) {
                        rec[O_B3 + 1] = rec[O_B3 + 2] = rec[O_B3 + 3] = 0.f;
                        rec[MLP_P + 1] = rec[MLP_P + 2] = rec[MLP_P + 3] = 0.f;
                    }
                }
            }
            __syncthreads();
        }
        float* dst = p.ws + size_t(blockIdx.x) * MLP_REC;
        for (int e = threadIdx.x; e < MLP_REC; e += 256) dst[e] = rec[e];
    }
}

template <bool TRAIN>
__global__ __launch_bounds__(LIN_BLOCK) void pixlin_kernel(const PixP p) {
    const float w0 = p.params[0], w1 = p.params[1], w2 = p.params[2], b = p.params[4];
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};                   // dw0, dw1, dw2, db, squared error
    for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const unsigned i = unsigned(tile) * LIN_BLOCK + threadIdx.x;
        if (i >= p.n) continue;
        const unsigned bi = i / unsigned(p.HW), px = i - bi * unsigned(p.HW);
        const float* q = p.rgb + size_t(bi) * 3 * p.HW + px;
        const float x0 = q[0], x1 = q[p.HW], x2 = q[2 * size_t(p.HW)];
        const float y = fmaf(w2, x2, fmaf(w1, x1, fmaf(w0, x0, b)));
        if (p.pred) p.pred[i] = y;
        if constexpr (TRAIN) {
            float dy;
            if (p.from_dpred) {
                dy = p.tgt[i];
            } else {
                const float d = y - p.tgt[i];
                acc[4] = fmaf(d, d, acc[4]);
                dy = d * p.scale;
            }
            acc[0] = fmaf(dy, x0, acc[0]);
            acc[1] = fmaf(dy, x1, acc[1]);
            acc[2] = fmaf(dy, x2, acc[2]);
            acc[3] += dy;
        }
    }
    if constexpr (TRAIN) {
        __shared__ float part[LIN_BLOCK / 64][5];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int e = 0; e < 5; ++e) {
            const float s = ng_wave_sum(acc[e]);
            if (lane == 0) part[wave][e] = s;
        }
        __syncthreads();
        if (threadIdx.x < LIN_REC) {
            const int e = threadIdx.x;                          // record: dw 0..2, pad, db 4, pad 5..7, squared error 8, pad
            const int src = e < 3 ? e : (e == 4 ? 3 : (e == 8 ? 4 : -1));
            float t = 0.f;
            if (src >= 0)
                for (int w = 0; w < LIN_BLOCK / 64; ++w) t += part[w][src];
            p.ws[size_t(blockIdx.x) * LIN_REC + e] = t;
        }
    }
}

// records [rows][rec] -> grads[0..P) (overwritten) and loss_out[0] += record[P] sum / n, every sum in row order
__global__ __launch_bounds__(256) void pixmlp_merge_kernel(const float* __restrict__ ws, int rows, int rec, int P, float* grads,
                                                           float* loss_out, float inv_n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e > P) return;
    float t = 0.f;
    for (int r = 0; r < rows; ++r) t += ws[size_t(r) * rec + e];
    if (e < P) grads[e] = t;
    else if (loss_out) loss_out[0] += t * inv_n;
}

struct Geo {
    int64_t n;
    int ntiles, grid, rec, P;
};

bool geometry(int B, int H, int W, int hidden, Geo& g) {
    if (B <= 0 || H <= 0 || W <= 0 || (hidden != 0 && hidden != 64)) return false;
    g.n = int64_t(B) * H * W;
    if (g.n > 2147483647LL) return false;
    if (hidden == 64) {
        g.ntiles = int((g.n + PT - 1) / PT);
        const int wg = (g.ntiles + 3) / 4;
        g.grid = wg < MLP_GRID ? wg : MLP_GRID;
        g.rec = MLP_REC;
        g.P = MLP_P;
    } else {
        g.ntiles = int((g.n + LIN_BLOCK - 1) / LIN_BLOCK);
        g.grid = g.ntiles < LIN_GRID ? g.ntiles : LIN_GRID;
        g.rec = LIN_REC;
        g.P = LIN_P;
    }
    return true;
}

}  // namespace

extern "C" int64_t nirgan_pixmlp_ws_elems(int B, int H, int W, int hidden) {
    Geo g;
    if (!geometry(B, H, W, hidden, g)) return 0;
    return int64_t(g.grid) * g.rec;
}

extern "C" int nirgan_pixmlp_fwd(const nirgan_pixmlp_desc* d, void* stream) {
    NG_REQUIRE(d && d->rgb && d->params && d->pred, "pixmlp_fwd: null pointer (rgb, params, pred)");
    NG_REQUIRE(d->hidden == 0 || d->hidden == 64, "pixmlp_fwd: hidden must be 0 (Linear_NIR) or 64 (MLP_NIR), got %d", d->hidden);
    Geo g;
    NG_REQUIRE(geometry(d->B, d->H, d->W, d->hidden, g), "pixmlp_fwd: bad shape %d x %d x %d (extents >= 1, B*H*W < 2^31)", d->B, d->H, d->W);
    PixP p{d->rgb, nullptr, d->params, d->pred, nullptr, unsigned(g.n), d->H * d->W, g.ntiles, 0, 0.f};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->hidden == 64) hipLaunchKernelGGL(pixmlp64_kernel<false>, dim3(g.grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(pixlin_kernel<false>, dim3(g.grid), dim3(LIN_BLOCK), 0, st, p);
    return nirgan_check_launch("pixmlp_fwd");
}

extern "C" int nirgan_pixmlp_train(const nirgan_pixmlp_desc* d, void* stream) {
    NG_REQUIRE(d && d->rgb && d->params && d->grads && d->ws, "pixmlp_train: null pointer (rgb, params, grads, ws)");
    NG_REQUIRE((d->nir && d->loss_out) || d->dpred, "pixmlp_train: needs nir and loss_out, or dpred");
    NG_REQUIRE(d->hidden == 0 || d->hidden == 64, "pixmlp_train: hidden must be 0 (Linear_NIR) or 64 (MLP_NIR), got %d", d->hidden);
    Geo g;
    NG_REQUIRE(geometry(d->B, d->H, d->W, d->hidden, g), "pixmlp_train: bad shape %d x %d x %d (extents >= 1, B*H*W < 2^31)", d->B, d->H, d->W);
    NG_REQUIRE(d->ws_elems >= int64_t(g.grid) * g.rec, "pixmlp_train: workspace of %lld floats required (nirgan_pixmlp_ws_elems), got %lld",
               (long long)(int64_t(g.grid) * g.rec), (long long)d->ws_elems);
    const bool from_dpred = d->dpred != nullptr;
    PixP p{d->rgb, from_dpred ? d->dpred : d->nir, d->params, d->pred, d->ws, unsigned(g.n), d->H * d->W, g.ntiles, from_dpred ? 1 : 0,
           2.f / float(g.n)};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->hidden == 64) hipLaunchKernelGGL(pixmlp64_kernel<true>, dim3(g.grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(pixlin_kernel<true>, dim3(g.grid), dim3(LIN_BLOCK), 0, st, p);
    int rc = nirgan_check_launch("pixmlp_train");
    if (rc != NIRGAN_OK) return rc;
    hipLaunchKernelGGL(pixmlp_merge_kernel, dim3((g.P + 1 + 255) / 256), dim3(256), 0, st, (const float*)d->ws, g.grid, g.rec, g.P, d->grads,
                       from_dpred ? nullptr : d->loss_out, 1.f / float(g.n));
    return nirgan_check_launch("pixmlp_train (merge)");
}
