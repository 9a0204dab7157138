// LDS-staged separable Gaussian of the SSIM map as device functions, used by the per-tile entries (tilemetrics.hip,
// classmetrics.hip).  It is the scheme of metrics.hip (batch means), which keeps its own in-kernel statement: built from these
// functions its block partial sums came out different in the last bit (another instruction selection of the same expressions), and
// nirgan_image_metrics must not change.  The host-side taps (ng_ssim_taps) are shared by all of them and by ssimloss.hip.
//
// Per 32x32 output tile: the (32+2r)^2 input patches of both images go to LDS (reflect indexing at the border of the
// REFLECT DOMAIN, an Hd x Wd rectangle whose rows lie `stride` floats apart: the evaluation window inside a stored image --
// nothing outside the domain is read), a horizontal pass produces the five filtered moments
// x, y, x^2, y^2, xy for the (32+2r) x 32 strip, a vertical pass finishes them at one output pixel.
#pragma once
#include <math.h>
#include "common.h"

constexpr int NG_SSIM_TILE = 32;
constexpr int NG_SSIM_MAXR = 5;                                  // window <= 11
constexpr int NG_SSIM_PW = NG_SSIM_TILE + 2 * NG_SSIM_MAXR;      // patch width

struct NgSsimLds {
    float sa[NG_SSIM_PW][NG_SSIM_PW + 1], sb[NG_SSIM_PW][NG_SSIM_PW + 1];
    float hm[5][NG_SSIM_PW][NG_SSIM_TILE + 1];
};

// normalised 1-D Gaussian of `window` taps (kornia: exp(-x^2 / (2 sigma^2)) / sum), zero beyond the window
static inline void ng_ssim_taps(int window, float sigma, float* k) {
    const int r = window / 2;
    double sum = 0.0, kv[2 * NG_SSIM_MAXR + 1];
    for (int t = 0; t < window; ++t) {
        const double x = double(t - r);
        kv[t] = exp(-(x * x) / (2.0 * double(sigma) * double(sigma)));
        sum += kv[t];
    }
    for (int t = 0; t < 2 * NG_SSIM_MAXR + 1; ++t) k[t] = t < window ? float(kv[t] / sum) : 0.f;
}

// patches of A and B around the tile whose first output pixel is (h0 + r, w0 + r) of the domain; 256 threads; ends with a barrier
__device__ __forceinline__ void ng_ssim_stage(NgSsimLds& s, const float* A, const float* B, int Hd, int Wd, int stride,
                                              int h0, int w0, int r, int tid) {
    const int pw = NG_SSIM_TILE + 2 * r;
    for (int i = tid; i < pw * pw; i += 256) {
        const int y = i / pw, x = i - y * pw;
        // reflect without edge repeat (domain larger than the window radius: checked on the host).  Patch positions past
        // the domain's last partial tile feed no output: clamp them into the reflectable band first.
        const int ph = h0 + y < Hd + r ? h0 + y : Hd - 1 + r, pwc = w0 + x < Wd + r ? w0 + x : Wd - 1 + r;
        const int hh = ng_reflect(ph, Hd), ww = ng_reflect(pwc, Wd);
        s.sa[y][x] = A[size_t(hh) * stride + ww];
        s.sb[y][x] = B[size_t(hh) * stride + ww];
    }
    __syncthreads();
}

// horizontal pass over the staged patches; ends with a barrier
__device__ __forceinline__ void ng_ssim_hpass(NgSsimLds& s, const float* k, int r, int tid) {
    const int pw = NG_SSIM_TILE + 2 * r;
    for (int i = tid; i < pw * NG_SSIM_TILE; i += 256) {
        const int y = i / NG_SSIM_TILE, x = i - y * NG_SSIM_TILE;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
        for (int t = 0; t <= 2 * r; ++t) {
            const float wv = k[t], u = s.sa[y][x + t], v = s.sb[y][x + t];
            m0 += wv * u; m1 += wv * v; m2 += wv * u * u; m3 += wv * v * v; m4 += wv * u * v;
        }
        s.hm[0][y][x] = m0; s.hm[1][y][x] = m1; s.hm[2][y][x] = m2; s.hm[3][y][x] = m3; s.hm[4][y][x] = m4;
    }
    __syncthreads();
}

// vertical pass + SSIM at output pixel (y, x) of the tile
__device__ __forceinline__ float ng_ssim_at(const NgSsimLds& s, const float* k, int r, int y, int x, float c1, float c2, float eps) {
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
    for (int t = 0; t <= 2 * r; ++t) {
        const float wv = k[t];
        m0 += wv * s.hm[0][y + t][x]; m1 += wv * s.hm[1][y + t][x]; m2 += wv * s.hm[2][y + t][x];
        m3 += wv * s.hm[3][y + t][x]; m4 += wv * s.hm[4][y + t][x];
    }
    const float mu1_sq = m0 * m0, mu2_sq = m1 * m1, mu12 = m0 * m1;
    const float s1 = m2 - mu1_sq, s2 = m3 - mu2_sq, s12 = m4 - mu12;
    const float num = (2.f * mu12 + c1) * (2.f * s12 + c2);
    const float den = (mu1_sq + mu2_sq + c1) * (s1 + s2 + c2);
    return num / (den + eps);
}
