// Per-tile validation metrics (the reference's results table: validation_utils/get_results_table.py:59-94,
// validation_utils/spider_validation_callback.py:28-64): ONE row per tile of a batch -- mean |d|, mean d^2, mean of the SSIM map, PSNR,
// the NDVI / NDWI / EVI L1 errors and the nir / pred means of a centred patch -- over an evaluation window inside each stored image.
// The window is applied by indexing (the reference copies a centre crop first): the SSIM filter reflects at the WINDOW's border and
// nothing outside the window is read.
//
// HBM-bound: five planes are read once (+ the SSIM halo of nir and pred).  Launch 1: one block per (tile, 32x32 block of the window);
// nir and pred go through the LDS-staged separable Gaussian of ssim_dev.h, each thread reads rgb at its four output pixels straight
// from memory (issued before the staging so that the loads overlap it), eight partial sums per block go to the workspace.  Launch 2:
// one block per tile adds that tile's partials in block order.  A tile's association depends only on (ch, cw): bitwise the same
// alone and inside any batch, no float atomics.
#include "ssim_dev.h"

namespace {

constexpr int TILE = NG_SSIM_TILE;
constexpr int MAXR = NG_SSIM_MAXR;
constexpr int NV = 8;                          // block partials: l1, l2, ssim, ndvi, ndwi, evi, patch nir, patch pred
constexpr int FOLD = 32;                       // strided chains of the per-tile fold

struct TileP {
    const float* rgb; const float* nir; const float* pred;
    int H, W, y0, x0, ch, cw, r;
    int py0, px0, patch;
    float k[2 * MAXR + 1];
    float c1, c2, eps;
    float* partials;                           // [B][tiles_y * tiles_x][NV]
    int tiles_x, tiles_y;
};

__global__ __launch_bounds__(256) void tile_metrics_kernel(const TileP p) {
    __shared__ NgSsimLds s;
    __shared__ float red[4][NV];
    const int tid = threadIdx.x;
    int bid = blockIdx.x;
    const int tx = bid % p.tiles_x; bid /= p.tiles_x;
    const int ty = bid % p.tiles_y;
    const int b = bid / p.tiles_y;
    const int r = p.r;
    const size_t plane = size_t(p.H) * p.W, origin = size_t(p.y0) * p.W + p.x0;
    // the four output pixels of this thread: rows (tid >> 5) + 8 j, column tid & 31 (a wave reads two 128-byte row segments)
    const int x = tid & 31, ow = tx * TILE + x;
    float R[4], G[4], Bl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int oh = ty * TILE + (tid >> 5) + 8 * j;
        R[j] = G[j] = Bl[j] = 0.f;
        if (p.rgb && oh < p.ch && ow < p.cw) {
            const float* q = p.rgb + size_t(b) * 3 * plane + origin + size_t(oh) * p.W + ow;
            R[j] = q[0]; G[j] = q[plane]; Bl[j] = q[2 * plane];
        }
    }
    ng_ssim_stage(s, p.nir + size_t(b) * plane + origin, p.pred + size_t(b) * plane + origin, p.ch, p.cw, p.W,
                  ty * TILE - r, tx * TILE - r, r, tid);
    ng_ssim_hpass(s, p.k, r, tid);
    float acc[NV] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = (tid >> 5) + 8 * j, oh = ty * TILE + y;
        if (oh >= p.ch || ow >= p.cw) continue;
        acc[2] += ng_ssim_at(s, p.k, r, y, x, p.c1, p.c2, p.eps);
        const float n = s.sa[y + r][x + r], f = s.sb[y + r][x + r];       // nir, pred
        const float d = f - n;
        acc[0] += fabsf(d);
        acc[1] += d * d;
        if (p.rgb) {                           // the formulas and epsilons of pix_loss_kernel (losses.hip), criterion l1
            acc[3] += fabsf((f - R[j]) / (f + R[j] + 1e-6f) - (n - R[j]) / (n + R[j] + 1e-6f));
            acc[4] += fabsf((f - G[j]) / (f + G[j] + 1e-6f) - (n - G[j]) / (n + G[j] + 1e-6f));
            const float c = (R[j] - 7.5f) * (Bl[j] + 1.f);
            acc[5] += fabsf(2.5f * ((f - R[j]) / ((f + 6.f) * c + 1e-6f)) - 2.5f * ((n - R[j]) / ((n + 6.f) * c + 1e-6f)));
        }
        if (unsigned(oh - p.py0) < unsigned(p.patch) && unsigned(ow - p.px0) < unsigned(p.patch)) { acc[6] += n; acc[7] += f; }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float v = ng_wave_sum(acc[i]);
        if ((tid & 63) == 0) red[tid >> 6][i] = v;
    }
    __syncthreads();
    if (tid < NV) p.partials[size_t(blockIdx.x) * NV + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// one block per tile: value j of chain c adds blocks c, c + FOLD, ... in order, then the chains are added in order
__global__ __launch_bounds__(256) void tile_metrics_fold_kernel(const float* __restrict__ partials, int nblk, float inv_n, float inv_patch,
                                                                float max_val, int has_rgb, float* __restrict__ rows) {
    __shared__ float part[FOLD][NV];
    const int j = threadIdx.x & (NV - 1), c = threadIdx.x >> 3;
    const float* src = partials + size_t(blockIdx.x) * nblk * NV;
    float v = 0.f;
    for (int i = c; i < nblk; i += FOLD) v += src[size_t(i) * NV + j];
    part[c][j] = v;
    __syncthreads();
    if (threadIdx.x >= NV) return;
    float t = 0.f;
    for (int i = 0; i < FOLD; ++i) t += part[i][j];
    float* row = rows + size_t(blockIdx.x) * NIRGAN_TILE_METRIC_COLS;
    if (j < 3) {
        const float m = t * inv_n;
        row[j] = m;
        if (j == 1) row[3] = m > 0.f ? 10.f * log10f(max_val * max_val / m) : __builtin_inff();
    } else if (j < 6) {
        if (has_rgb) row[j + 1] = t * inv_n;
    } else if (inv_patch > 0.f) {
        row[j + 1] = t * inv_patch;
    }
}

}  // namespace

extern "C" int64_t nirgan_tile_metrics_ws_elems(int B, int ch, int cw) {
    if (B <= 0 || ch <= 0 || cw <= 0) return 0;
    return int64_t(B) * ((ch + TILE - 1) / TILE) * ((cw + TILE - 1) / TILE) * NV;
}

extern "C" int nirgan_tile_metrics(const nirgan_tile_metrics_desc* d, void* stream) {
    NG_REQUIRE(d != nullptr && d->nir && d->pred && d->ws && d->rows, "tile_metrics: null pointer");
    NG_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0, "tile_metrics: empty problem");
    NG_REQUIRE(d->window >= 1 && d->window <= 2 * MAXR + 1 && (d->window & 1), "tile_metrics: window=%d must be odd and <= %d", d->window, 2 * MAXR + 1);
    const int r = d->window / 2;
    NG_REQUIRE(d->ch > 0 && d->cw > 0 && d->y0 >= 0 && d->x0 >= 0 && d->ch <= d->H - d->y0 && d->cw <= d->W - d->x0,
               "tile_metrics: evaluation window y0=%d x0=%d %dx%d outside the %dx%d image", d->y0, d->x0, d->ch, d->cw, d->H, d->W);
    NG_REQUIRE(d->ch > r && d->cw > r, "tile_metrics: evaluation window smaller than the SSIM window radius (reflect border)");
    NG_REQUIRE(d->sigma > 0.f && d->max_val > 0.f, "tile_metrics: sigma and max_val must be positive");
    NG_REQUIRE(d->patch >= 0 && d->patch <= d->ch && d->patch <= d->cw, "tile_metrics: patch=%d larger than the evaluation window", d->patch);
    NG_REQUIRE(int64_t(d->H) * d->W < (int64_t(1) << 31), "tile_metrics: image too large");
    TileP p;
    p.rgb = d->rgb; p.nir = d->nir; p.pred = d->pred;
    p.H = d->H; p.W = d->W; p.y0 = d->y0; p.x0 = d->x0; p.ch = d->ch; p.cw = d->cw; p.r = r;
    p.patch = d->patch; p.py0 = d->ch / 2 - d->patch / 2; p.px0 = d->cw / 2 - d->patch / 2;
    ng_ssim_taps(d->window, d->sigma, p.k);
    p.c1 = (0.01f * d->max_val) * (0.01f * d->max_val);
    p.c2 = (0.03f * d->max_val) * (0.03f * d->max_val);
    p.eps = d->eps;
    p.tiles_x = (d->cw + TILE - 1) / TILE; p.tiles_y = (d->ch + TILE - 1) / TILE;
    const int64_t per_tile = int64_t(p.tiles_x) * p.tiles_y, blocks = per_tile * d->B;
    NG_REQUIRE(blocks < (int64_t(1) << 31), "tile_metrics: too many blocks");
    NG_REQUIRE(d->ws_elems >= blocks * NV, "tile_metrics: workspace too small (nirgan_tile_metrics_ws_elems)");
    p.partials = d->ws;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tile_metrics_kernel, dim3(unsigned(blocks)), dim3(256), 0, st, p);
    const float inv_n = 1.f / (float(d->ch) * float(d->cw));
    const float inv_patch = d->patch > 0 ? 1.f / (float(d->patch) * float(d->patch)) : 0.f;
    hipLaunchKernelGGL(tile_metrics_fold_kernel, dim3(unsigned(d->B)), dim3(256), 0, st, d->ws, int(per_tile), inv_n, inv_patch,
                       d->max_val, d->rgb ? 1 : 0, d->rows);
    return nirgan_check_launch("tile_metrics");
}
