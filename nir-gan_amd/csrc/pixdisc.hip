// The pixel discriminator (reference model/networks.py:587-616, PixelDiscriminator with norm = 'instance') as fused per-pixel kernels.
//
//   x[4] = cat(rgb, nir | pred)      z1 = W1 x + b1 (64)      h1 = lrelu_0.2(z1)      z2 = W2 h1 (128; b2 is DROPPED, see below)
//   xh = (z2 - mean_nc) * rstd_nc    (per sample and channel over H*W, biased variance, eps 1e-5, no affine)
//   h2 = lrelu_0.2(xh)               out = w3 . h2 + b3
//
// on x [B][H][W][4] (16 bytes per pixel in, 4 out).  Parameters are read in place from the network's flat fp32 range (nirgan_hip/flat.py:
// state_dict order, every tensor padded to 4 floats: 8772 floats); gradients leave in the same layout.  net.2.bias feeds the InstanceNorm:
// the mean subtraction removes it exactly, so the forward never adds it and its gradient is written as exact zeros.
//
// ONE device function, z2_tile, produces the z2 tile [32 pixels][128 channels] of a 32-pixel group from x: the K = 4 layer on the VALU by
// the lane that needs h1[p][k] as the A operand, then 128 v_mfma_f32_32x32x2_f32 against W2 (B operand: an LDS copy [128][64 + 1], the K
// slot (step s, lane half) is k = s + 32 half so that the two halves read disjoint banks).  Four passes call it with different epilogues;
// no per-pixel hidden activation is stored in HBM in either direction:
//   F1  statistics     per tile (count, mean, M2) of every channel, merged into the wave's running triple with Chan's formula
//   F2  output         normalise, LeakyReLU, dot with w3 (VALU on the accumulator layout + 5 shuffles per pixel), + b3
//   B1  backward sums  S1 = sum dxh, S2 = sum dxh xh (dxh = dout w3 lrelu'(xh)), dw3 = sum dout h2, db3 = sum dout
//   B2  gradients      dz2 = rstd (dxh - S1/n - xh S2/n), then by mode
//         PARAMS  dW2 += dz2^T . h1 (M = j, N = k, K = pixel: dz2 IS the A operand as it stands, h1 is computed again as B),
//                 dh1 = dz2 . W2 (M = pixel, N = k, K = j: dz2 goes through a per-wave LDS tile [32][128 + 4]), dz1 = dh1 lrelu'(z1),
//                 dW1 = sum dz1 (x) x, db1 = sum dz1
//         INPUT   gx[p][0..3] = W1^T dz1       PRED   channel 3 of that (the same expression: bitwise equal)
//
// z2 is taken relative to a PIVOT per (sample, channel): z2 of the sample's first pixel, which every wave computes again (one more
// z2_tile per work unit) and feeds, negated, as the C input of every tile's MFMA chain.  `stats` holds (mean of z2 - pivot, rstd): the mean
// is then of the size of the channel's spread and fp32 holds it to 2^-24 of THAT, however far the channel's level lies from zero.
//
// Work unit = (sample, chunk of consecutive tiles of that sample): a tile never straddles two samples, the last tile of every sample is
// partial and predicated.  One wave walks one unit at a time; a workgroup is four waves; the grid is a function of the shape only.
// Reductions, all in index order, no float atomics (two runs are bitwise equal):
//   per-unit records [388] in the workspace (F1: mean, M2; B1: S1, S2, dw3, db3) -> one thread per (sample, channel) merges the chunks of
//   its sample in chunk order (F1: Chan's formula -> stats (mean, rstd); B1: plain sums -> per-sample S1/n, S2/n, dw3, db3);
//   PARAMS: a wave keeps dW1, db1, dW2 in registers for its whole walk, the four waves add theirs into one LDS record in wave order,
//   the workgroup stores record [8512]; the merge kernel adds the records in workgroup order, the per-sample dw3 / db3 in sample order,
//   and writes zeros to net.2.bias and the padding elements.
#include "common.h"

namespace {

constexpr int PT = NIRGAN_PIXDISC_TILE;         // pixels per wave tile
constexpr int C2 = 128;                         // channels of z2 (2 ndf)
constexpr int W2S = 65;                         // row stride of the W2 LDS copy
constexpr int TS = 132;                         // row stride of the dz2 transposition tile
constexpr int O_W1 = 0, O_B1 = 256, O_W2 = 320, O_B2 = 8512, O_W3 = 8640, O_B3 = 8768, P_ALL = 8772;
constexpr int GREC = O_B2;                      // per-workgroup gradient record: dW1, db1, dW2
constexpr int UREC = 3 * C2 + 4;                // per-unit / per-sample record
constexpr int NC_MAX = 64;                      // chunks per sample at most
constexpr int GRID_MAX = 256;                   // workgroups at most: one per CU of the MI355X -- a CONSTANT of this gfx950-only library
constexpr float EPS = 1e-5f, SLOPE = 0.2f;

enum { F1 = 0, F2 = 1, B1 = 2, B2P = 3, B2I = 4, B2R = 5 };

struct PdP {
    const float* x; const float* params; const float* stats; const float* dout;
    float* out; float* gx;
    float* urec; float* srec; float* grec;      // workspace: per-unit records, per-sample records, per-workgroup gradient records
    int HW, T, CH, NC;                          // pixels, tiles, tiles per chunk, chunks of one sample
    long long units;                            // B * NC
};

__device__ __forceinline__ void wave_sync() {   // LDS written by some lanes of this wave, read by others: program order, no reordering
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : SLOPE * v; }

__device__ __forceinline__ float hidden1(const f32x4 w, float b, const f32x4 x) {     // lrelu(W1[k] . x + b1[k]), one association everywhere
    return lrelu(fmaf(w.w, x.w, fmaf(w.z, x.z, fmaf(w.y, x.y, fmaf(w.x, x.x, b)))));
}

// pixel of accumulator register r in lane half `half` of a 32 x 32 MFMA tile whose rows are the tile's pixels
__device__ __forceinline__ int acc_pixel(int r, int half) { return 8 * (r >> 2) + 4 * half + (r & 3); }

// z2[p][j] = sum_k h1[p][k] W2[j][k] of the 32 pixels whose inputs the lanes hold (lane: pixel l32, both halves the same pixel);
// acc[nt][r] = z2[acc_pixel(r, half)][l32 + 32 nt] + c0[nt]: the fma chains start from c0 (0, or minus the channel's pivot)
__device__ __forceinline__ void z2_tile(const f32x4 x, const f32x4* w1tab, const float* b1tab, const float* w2s, int l32, int half,
                                        const float (&c0)[4], f32x16 (&acc)[4]) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = c0[nt];
#pragma unroll
    for (int s = 0; s < 32; ++s) {
        const int k = s + 32 * half;
        const float h = hidden1(w1tab[k], b1tab[k], x);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
            acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(h, w2s[(l32 + 32 * nt) * W2S + k], acc[nt], 0, 0, 0);
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void pixdisc_kernel(const PdP p) {
    constexpr bool BWD2 = MODE == B2P || MODE == B2I || MODE == B2R;
    __shared__ f32x4 w1tab[64];
    __shared__ float b1tab[64];
    __shared__ float w2s[C2 * W2S];
    __shared__ f32x4 xs[BWD2 ? 4 : 1][PT];                      // per wave: the tile's inputs
    __shared__ __attribute__((aligned(16))) float tr[BWD2 ? 4 : 1][BWD2 ? PT * TS : 4];
    __shared__ float rec[MODE == B2P ? GREC : 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l32 = lane & 31;
    const float* __restrict__ prm = p.params;
    if (threadIdx.x < 64) {
        const int k = threadIdx.x;
        w1tab[k] = f32x4{prm[O_W1 + 4 * k], prm[O_W1 + 4 * k + 1], prm[O_W1 + 4 * k + 2], prm[O_W1 + 4 * k + 3]};
        b1tab[k] = prm[O_B1 + k];
    }
    for (int e = threadIdx.x; e < C2 * 64; e += 256) w2s[(e >> 6) * W2S + (e & 63)] = prm[O_W2 + e];
    float w3v[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) w3v[nt] = prm[O_W3 + l32 + 32 * nt];
    const float b3v = prm[O_B3];
    __syncthreads();
    const f32x4 w1k[2] = {w1tab[l32], w1tab[l32 + 32]};
    const float b1k[2] = {b1tab[l32], b1tab[l32 + 32]};

    // PARAMS: the wave's gradient sums over its whole walk
    f32x16 dW2[MODE == B2P ? 4 : 1][2];
    float dW1[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, db1[2] = {0.f, 0.f};
    if constexpr (MODE == B2P) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) dW2[a][b][r] = 0.f;
    }

    const int HW = p.HW;
    for (long long u = (long long)blockIdx.x * 4 + wave; u < p.units; u += (long long)gridDim.x * 4) {
        const long long b = u / p.NC;
        const int c = int(u - b * p.NC);
        const int t0 = c * p.CH, t1 = min(p.T, t0 + p.CH);
        const size_t pix0 = size_t(b) * HW;                     // the sample's first pixel
        // ---- the pivot of (b, l32 + 32 nt): z2 of the sample's first pixel, computed again by every unit of the sample with the same
        // chain.  Every tile's chain starts from minus the pivot, so z2 - pivot comes out of the MFMAs without a rounding at the size of
        // the mean, and the statistics, the centring and the backward sums work on numbers of the size of the channel's spread.
        float npiv[4];
        {
            const float zero[4] = {0.f, 0.f, 0.f, 0.f};
            f32x16 acc[4];
            asm volatile("" ::: "memory");
            z2_tile(*reinterpret_cast<const f32x4*>(p.x + pix0 * 4), w1tab, b1tab, w2s, l32, half, zero, acc);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) npiv[nt] = -acc[nt][0];
        }
        // ---- per-unit state
        float mean[4], rstd[4], m1[4], m2[4];                   // F2, B1, B2: the statistics of (b, l32 + 32 nt); B2: S1 / n, S2 / n
        float a0[4], a1[4], a2[4], a3 = 0.f;                    // F1: running mean, M2; B1: S1, S2, dw3, db3
        int nrun = 0;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            a0[nt] = a1[nt] = a2[nt] = 0.f;
            mean[nt] = rstd[nt] = m1[nt] = m2[nt] = 0.f;
            if constexpr (MODE != F1) {
                const size_t q = (size_t(b) * C2 + l32 + 32 * nt) * 2;
                mean[nt] = p.stats[q];
                rstd[nt] = p.stats[q + 1];
            }
            if constexpr (BWD2) {
                m1[nt] = p.srec[size_t(b) * UREC + l32 + 32 * nt];
                m2[nt] = p.srec[size_t(b) * UREC + C2 + l32 + 32 * nt];
            }
        }
        for (int t = t0; t < t1; ++t) {
            const int px0 = t * PT;
            const int cnt = min(PT, HW - px0);                  // the sample's last tile is partial
            asm volatile("" ::: "memory");                      // keeps the W1 / W2 LDS reads inside the tile loop: hoisted, the 288
                                                                // values do not fit beside the accumulators and the running sums
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (l32 < cnt) x = *reinterpret_cast<const f32x4*>(p.x + (pix0 + px0 + l32) * 4);
            if constexpr (BWD2) {
                if (half == 0) xs[wave][l32] = x;
            }
            f32x16 acc[4];
            z2_tile(x, w1tab, b1tab, w2s, l32, half, npiv, acc);

            if constexpr (MODE == F1) {
                const float fc = float(cnt), fn = float(nrun), ft = float(nrun + cnt);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    float s = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) s += acc_pixel(r, half) < cnt ? acc[nt][r] : 0.f;
                    s += __shfl_xor(s, 32, 64);
                    const float mt = s / fc;
                    float q = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float d = acc_pixel(r, half) < cnt ? acc[nt][r] - mt : 0.f;
                        q = fmaf(d, d, q);
                    }
                    q += __shfl_xor(q, 32, 64);
                    if (nrun == 0) {
                        a0[nt] = mt;
                        a1[nt] = q;
                    } else {                                    // Chan: (n, mean, M2) of the walk so far with the tile's
                        const float d = mt - a0[nt];
                        a0[nt] = fmaf(d, fc / ft, a0[nt]);
                        a1[nt] += fmaf(d * d, fn * fc / ft, q);
                    }
                }
                nrun += cnt;
            }
            if constexpr (MODE == F2) {
                float ysel = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = 0.f;
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) v = fmaf(w3v[nt], lrelu((acc[nt][r] - mean[nt]) * rstd[nt]), v);
#pragma unroll
                    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);      // the 32 lanes of the half: every lane ends with the same bits
                    ysel = l32 == r ? v + b3v : ysel;
                }
                const int ip = acc_pixel(l32 & 15, half);
                if (l32 < 16 && ip < cnt) p.out[pix0 + px0 + ip] = ysel;
            }
            if constexpr (MODE == B1 || BWD2) {
                float dy[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ip = acc_pixel(r, half);
                    dy[r] = ip < cnt ? p.dout[pix0 + px0 + ip] : 0.f;
                }
                if constexpr (MODE == B1) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) a3 += dy[r];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float xh = (acc[nt][r] - mean[nt]) * rstd[nt];
                            const float g = dy[r] * w3v[nt];
                            const float dxh = xh > 0.f ? g : SLOPE * g;
                            a0[nt] += dxh;
                            a1[nt] = fmaf(dxh, xh, a1[nt]);
                            a2[nt] = fmaf(dy[r], lrelu(xh), a2[nt]);
                        }
                } else {
                    // ---- dz2 (accumulator layout), in place of z2
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const float xh = (acc[nt][r] - mean[nt]) * rstd[nt];
                            const float g = dy[r] * w3v[nt];
                            const float dxh = xh > 0.f ? g : SLOPE * g;
                            const float dz = rstd[nt] * fmaf(-xh, m2[nt], dxh - m1[nt]);
                            acc[nt][r] = acc_pixel(r, half) < cnt ? dz : 0.f;
                        }
                    wave_sync();                                // xs is written
                    // ---- h1 again, as the B operand of dW2 and the mask of dz1: k = l32 + 32 nt, the pixel of accumulator register r
                    float hB[2][16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const f32x4 xr = xs[wave][acc_pixel(r, half)];
                        hB[0][r] = hidden1(w1k[0], b1k[0], xr);
                        hB[1][r] = hidden1(w1k[1], b1k[1], xr);
                    }
                    if constexpr (MODE == B2P) {
#pragma unroll
                        for (int r = 0; r < 16; ++r)
#pragma unroll
                            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                                for (int nt = 0; nt < 2; ++nt)
                                    dW2[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[mt][r], hB[nt][r], dW2[mt][nt], 0, 0, 0);
                    }
                    // ---- dz2 to the operand layout of dh1 = dz2 . W2
                    float* tt = tr[wave];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) tt[acc_pixel(r, half) * TS + l32 + 32 * nt] = acc[nt][r];
                    wave_sync();
                    f32x16 dh[2];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        dh[0][r] = 0.f;
                        dh[1][r] = 0.f;
                    }
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const f32x4 a = *reinterpret_cast<const f32x4*>(&tt[l32 * TS + 8 * q + 4 * half]);     // j = acc_pixel(4 q + c, half)
#pragma unroll
                        for (int cc = 0; cc < 4; ++cc) {
                            const int j = 8 * q + 4 * half + cc;
                            dh[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cc], w2s[j * W2S + l32], dh[0], 0, 0, 0);
                            dh[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cc], w2s[j * W2S + l32 + 32], dh[1], 0, 0, 0);
                        }
                    }
                    // ---- dz1 = dh1 . lrelu'(z1) on the accumulator layout of dh1 (pixel acc_pixel(r, half), k = l32 + 32 nt)
                    f32x4 gsel = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float g0 = hB[0][r] > 0.f ? dh[0][r] : SLOPE * dh[0][r];
                        const float g1 = hB[1][r] > 0.f ? dh[1][r] : SLOPE * dh[1][r];
                        if constexpr (MODE == B2P) {
                            const f32x4 xr = xs[wave][acc_pixel(r, half)];
                            db1[0] += g0;
                            db1[1] += g1;
#pragma unroll
                            for (int ch = 0; ch < 4; ++ch) {
                                dW1[0][ch] = fmaf(g0, xr[ch], dW1[0][ch]);
                                dW1[1][ch] = fmaf(g1, xr[ch], dW1[1][ch]);
                            }
                        } else {
                            // gx[p][ch] = sum_k W1[k][ch] dz1[p][k]: the lane's two k, then the 32 lanes of the half
#pragma unroll
                            for (int ch = (MODE == B2R ? 3 : 0); ch < 4; ++ch) {
                                float v = fmaf(w1k[1][ch], g1, w1k[0][ch] * g0);
#pragma unroll
                                for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                                gsel[ch] = l32 == r ? v : gsel[ch];
                            }
                        }
                    }
                    if constexpr (MODE != B2P) {
                        const int ip = acc_pixel(l32 & 15, half);
                        if (l32 < 16 && ip < cnt) {
                            if constexpr (MODE == B2I) *reinterpret_cast<f32x4*>(p.gx + (pix0 + px0 + ip) * 4) = gsel;
                            else p.gx[pix0 + px0 + ip] = gsel[3];
                        }
                    }
                    wave_sync();                                // the next tile overwrites xs and the transposition tile
                }
            }
        }
        // ---- the unit's record
        if constexpr (MODE == F1 || MODE == B1) {
            float* dst = p.urec + size_t(u) * UREC;
            if constexpr (MODE == B1) {
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {                // the two halves hold different pixels
                    a0[nt] += __shfl_xor(a0[nt], 32, 64);
                    a1[nt] += __shfl_xor(a1[nt], 32, 64);
                    a2[nt] += __shfl_xor(a2[nt], 32, 64);
                }
                a3 += __shfl_xor(a3, 32, 64);
            }
            if (half == 0) {
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    dst[l32 + 32 * nt] = a0[nt];
                    dst[C2 + l32 + 32 * nt] = a1[nt];
                    dst[2 * C2 + l32 + 32 * nt] = a2[nt];
                }
                if (l32 < 4) dst[3 * C2 + l32] = l32 == 0 ? a3 : 0.f;
            }
        }
    }

    if constexpr (MODE == B2P) {
        // the four waves add their sums into the record in wave order
        for (int w = 0; w < 4; ++w) {
            if (wave == w) {
                const bool first = w == 0;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
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
                    float v[5] = {dW1[nt][0], dW1[nt][1], dW1[nt][2], dW1[nt][3], db1[nt]};
#pragma unroll
                    for (int e = 0; e < 5; ++e) v[e] += __shfl_xor(v[e], 32, 64);        // the two halves hold different pixels
                    if (half == 0) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) rec[O_W1 + 4 * k + e] = (first ? 0.f : rec[O_W1 + 4 * k + e]) + v[e];
                        rec[O_B1 + k] = (first ? 0.f : rec[O_B1 + k]) + v[4];
                    }
                }
            }
            __syncthreads();
        }
        float* dst = p.grec + size_t(blockIdx.x) * GREC;
        for (int e = threadIdx.x; e < GREC; e += 256) dst[e] = rec[e];
    }
}

// F1 records -> stats[b][j] = (mean, rstd): the chunks of sample b in chunk order, Chan's formula
__global__ __launch_bounds__(256) void pixdisc_stats_kernel(const float* __restrict__ urec, long long rows, int NC, int CH, int HW,
                                                            float* __restrict__ stats) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const long long b = i / C2;
    const int j = int(i - b * C2);
    float mean = 0.f, M2 = 0.f;
    int n = 0;
    for (int c = 0; c < NC; ++c) {
        const float* r = urec + size_t(b * NC + c) * UREC;
        const int lo = c * CH * PT, cnt = min(HW, lo + CH * PT) - lo;
        const float mc = r[j], qc = r[C2 + j];
        if (n == 0) {
            mean = mc;
            M2 = qc;
        } else {
            const float d = mc - mean, fc = float(cnt), fn = float(n), ft = float(n + cnt);
            mean = fmaf(d, fc / ft, mean);
            M2 += fmaf(d * d, fn * fc / ft, qc);
        }
        n += cnt;
    }
    stats[2 * i] = mean;
    stats[2 * i + 1] = 1.f / sqrtf(M2 / float(HW) + EPS);
}

// B1 records -> per-sample record: S1 / n, S2 / n, dw3 of (b, j), db3 of b, the chunks of sample b in chunk order
__global__ __launch_bounds__(256) void pixdisc_sums_kernel(const float* __restrict__ urec, long long rows, int NC, int HW, float* __restrict__ srec) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const long long b = i / (C2 + 1);
    const int j = int(i - b * (C2 + 1));
    float* dst = srec + size_t(b) * UREC;
    if (j == C2) {
        float t = 0.f;
        for (int c = 0; c < NC; ++c) t += urec[size_t(b * NC + c) * UREC + 3 * C2];
        dst[3 * C2] = t;
        dst[3 * C2 + 1] = dst[3 * C2 + 2] = dst[3 * C2 + 3] = 0.f;
        return;
    }
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int c = 0; c < NC; ++c) {
        const float* r = urec + size_t(b * NC + c) * UREC;
        s1 += r[j];
        s2 += r[C2 + j];
        s3 += r[2 * C2 + j];
    }
    dst[j] = s1 / float(HW);
    dst[C2 + j] = s2 / float(HW);
    dst[2 * C2 + j] = s3;
}

// grads[0..8772) (overwritten): dW1, db1, dW2 from the workgroup records in workgroup order, dw3 / db3 from the per-sample records in
// sample order, net.2.bias and the padding elements exact zeros
__global__ __launch_bounds__(256) void pixdisc_merge_kernel(const float* __restrict__ grec, int rows, const float* __restrict__ srec, long long B,
                                                            float* __restrict__ grads) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P_ALL) return;
    float t = 0.f;
    if (e < GREC) {
        for (int r = 0; r < rows; ++r) t += grec[size_t(r) * GREC + e];
    } else if (e >= O_W3 && e <= O_B3) {
        const int o = 2 * C2 + (e - O_W3);                      // dw3 at [256 .. 384), db3 at 384
        for (long long b = 0; b < B; ++b) t += srec[size_t(b) * UREC + o];
    }
    grads[e] = t;
}

struct Geo {
    int64_t n, units;
    int HW, T, CH, NC, grid;
    int64_t ws;
};

bool geometry(int B, int H, int W, int ndf, Geo& g) {
    if (B <= 0 || H <= 0 || W <= 0 || ndf != 64) return false;
    const int64_t hw = int64_t(H) * W;
    g.n = int64_t(B) * hw;
    if (hw < 2 || g.n > 2147483647LL) return false;
    g.HW = int(hw);
    g.T = (g.HW + PT - 1) / PT;
    const int nc = g.T < NC_MAX ? g.T : NC_MAX;
    g.CH = (g.T + nc - 1) / nc;
    g.NC = (g.T + g.CH - 1) / g.CH;
    g.units = int64_t(B) * g.NC;
    const int64_t wg = (g.units + 3) / 4;
    g.grid = int(wg < GRID_MAX ? wg : GRID_MAX);
    g.ws = (g.units + B) * UREC + int64_t(g.grid) * GREC;
    return true;
}

PdP make_params(const nirgan_pixdisc_desc* d, const Geo& g) {
    PdP p;
    p.x = d->x; p.params = d->params; p.stats = d->stats; p.dout = d->dout; p.out = d->out; p.gx = d->gx;
    p.urec = d->ws;
    p.srec = d->ws + g.units * UREC;
    p.grec = p.srec + int64_t(d->B) * UREC;
    p.HW = g.HW; p.T = g.T; p.CH = g.CH; p.NC = g.NC; p.units = g.units;
    return p;
}

}  // namespace

extern "C" int64_t nirgan_pixdisc_ws_elems(int B, int H, int W, int ndf) {
    Geo g;
    if (!geometry(B, H, W, ndf, g)) return 0;
    return g.ws;
}

extern "C" int nirgan_pixdisc_fwd(const nirgan_pixdisc_desc* d, void* stream) {
    NG_REQUIRE(d && d->x && d->params && d->stats && d->out && d->ws, "pixdisc_fwd: null pointer (x, params, stats, out, ws)");
    NG_REQUIRE(d->ndf == 64, "pixdisc_fwd: ndf must be 64, got %d", d->ndf);
    Geo g;
    NG_REQUIRE(geometry(d->B, d->H, d->W, d->ndf, g), "pixdisc_fwd: bad shape %d x %d x %d (extents >= 1, H*W >= 2, B*H*W < 2^31)", d->B, d->H, d->W);
    NG_REQUIRE(d->ws_elems >= g.ws, "pixdisc_fwd: workspace of %lld floats required (nirgan_pixdisc_ws_elems), got %lld", (long long)g.ws,
               (long long)d->ws_elems);
    NG_REQUIRE(ng_aligned16(d->x), "pixdisc_fwd: x must be 16-byte aligned");
    const PdP p = make_params(d, g);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pixdisc_kernel<F1>, dim3(g.grid), dim3(256), 0, st, p);
    int rc = nirgan_check_launch("pixdisc_fwd (statistics)");
    if (rc != NIRGAN_OK) return rc;
    const long long rows = (long long)d->B * C2;
    hipLaunchKernelGGL(pixdisc_stats_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, (const float*)p.urec, rows, g.NC, g.CH, g.HW,
                       d->stats);
    rc = nirgan_check_launch("pixdisc_fwd (statistics merge)");
    if (rc != NIRGAN_OK) return rc;
    hipLaunchKernelGGL(pixdisc_kernel<F2>, dim3(g.grid), dim3(256), 0, st, p);
    return nirgan_check_launch("pixdisc_fwd (output)");
}

extern "C" int nirgan_pixdisc_bwd(const nirgan_pixdisc_desc* d, void* stream) {
    NG_REQUIRE(d && d->x && d->params && d->stats && d->dout && d->ws, "pixdisc_bwd: null pointer (x, params, stats, dout, ws)");
    NG_REQUIRE(d->mode == NIRGAN_PIXDISC_PARAMS || d->mode == NIRGAN_PIXDISC_INPUT || d->mode == NIRGAN_PIXDISC_PRED,
               "pixdisc_bwd: mode must be PARAMS (0), INPUT (1) or PRED (2), got %d", d->mode);
    NG_REQUIRE(d->mode == NIRGAN_PIXDISC_PARAMS ? d->grads != nullptr : d->gx != nullptr,
               "pixdisc_bwd: null pointer (grads for mode PARAMS, gx for INPUT / PRED)");
    NG_REQUIRE(d->ndf == 64, "pixdisc_bwd: ndf must be 64, got %d", d->ndf);
    Geo g;
    NG_REQUIRE(geometry(d->B, d->H, d->W, d->ndf, g), "pixdisc_bwd: bad shape %d x %d x %d (extents >= 1, H*W >= 2, B*H*W < 2^31)", d->B, d->H, d->W);
    NG_REQUIRE(d->ws_elems >= g.ws, "pixdisc_bwd: workspace of %lld floats required (nirgan_pixdisc_ws_elems), got %lld", (long long)g.ws,
               (long long)d->ws_elems);
    NG_REQUIRE(ng_aligned16(d->x) && (d->mode != NIRGAN_PIXDISC_INPUT || ng_aligned16(d->gx)), "pixdisc_bwd: x and gx must be 16-byte aligned");
    const PdP p = make_params(d, g);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pixdisc_kernel<B1>, dim3(g.grid), dim3(256), 0, st, p);
    int rc = nirgan_check_launch("pixdisc_bwd (sums)");
    if (rc != NIRGAN_OK) return rc;
    const long long rows = (long long)d->B * (C2 + 1);
    hipLaunchKernelGGL(pixdisc_sums_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, (const float*)p.urec, rows, g.NC, g.HW, p.srec);
    rc = nirgan_check_launch("pixdisc_bwd (sums merge)");
    if (rc != NIRGAN_OK) return rc;
    if (d->mode == NIRGAN_PIXDISC_INPUT) {
        hipLaunchKernelGGL(pixdisc_kernel<B2I>, dim3(g.grid), dim3(256), 0, st, p);
        return nirgan_check_launch("pixdisc_bwd (input)");
    }
    if (d->mode == NIRGAN_PIXDISC_PRED) {
        hipLaunchKernelGGL(pixdisc_kernel<B2R>, dim3(g.grid), dim3(256), 0, st, p);
        return nirgan_check_launch("pixdisc_bwd (pred)");
    }
    hipLaunchKernelGGL(pixdisc_kernel<B2P>, dim3(g.grid), dim3(256), 0, st, p);
    rc = nirgan_check_launch("pixdisc_bwd (params)");
    if (rc != NIRGAN_OK) return rc;
    hipLaunchKernelGGL(pixdisc_merge_kernel, dim3((P_ALL + 255) / 256), dim3(256), 0, st, (const float*)p.grec, g.grid, (const float*)p.srec,
                       (long long)d->B, d->grads);
    return nirgan_check_launch("pixdisc_bwd (merge)");
}
