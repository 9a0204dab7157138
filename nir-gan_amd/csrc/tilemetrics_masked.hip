// Per-tile validation metrics over the VALID pixels of each tile (nirgan_tile_metrics_masked): the rows of tilemetrics.hip with a
// [B][1][H][W] fp32 mask (!= 0.f is valid, the convention of nirgan_pix_loss_masked / nirgan_valid_count).  l1, l2, psnr, the three
// index errors and the patch means are means over the valid pixels of the evaluation window; ssim is the mean of the SSIM map over the
// SUPPORT-CLEAN pixels, those whose whole reflected (2r+1)^2 filter support is valid -- there the map has exactly its unmasked value.
// Two count columns, n_valid and n_ssim, follow the nine of the unmasked entry.
//
// The launch shape is tile_metrics_kernel's: one block of 256 threads per (tile, 32x32 block of the window), then one fold block per
// tile.  Beside the patches of nir and pred (ssim_dev.h, used as it is) the mask's patch is staged as byte flags with the same
// reflect / clamp indexing; the horizontal pass is joined by an integer count of valid taps per strip position, and an output pixel is
// support-clean iff the 2r+1 strip counts above and below it add up to (2r+1)^2.  A dropped pixel is branched around: whatever lies in
// nir / pred / rgb at an invalid pixel (NaN, Inf, nodata) may be staged in LDS, where it can only reach filter outputs that are not
// support-clean, and those are never added.  For a kept pixel the arithmetic, the wave sums, the combination of the four waves and
// the fold are tile_metrics_kernel's and tile_metrics_fold_kernel's operation for operation, so that under a mask of ones the sums
// take the same path.  Counts are fp32 partials, exact up to 2^24 (checked on the host).  No atomics: a tile's row depends only on
// (ch, cw) and its own planes.
#include "ssim_dev.h"

namespace {

constexpr int TILE = NG_SSIM_TILE;
constexpr int MAXR = NG_SSIM_MAXR;
constexpr int PW = NG_SSIM_PW;
constexpr int NV = 11;                         // block partials: l1, l2, ssim, ndvi, ndwi, evi, patch nir, patch pred, n_valid, n_ssim, patch count
constexpr int FOLD = 32;                       // strided chains of the per-tile fold
constexpr int FOLD_THREADS = FOLD * NV;

struct MaskLds {
    unsigned char sv[PW][PW + 1];              // 1 = valid, staged like sa / sb
    unsigned char hc[PW][TILE];                // valid taps among the 2r+1 to the right of strip position (y, x): <= 11
};

struct TileMP {
    const float* rgb; const float* nir; const float* pred; const float* valid;
    int H, W, y0, x0, ch, cw, r;
    int py0, px0, patch;
    float k[2 * MAXR + 1];
    float c1, c2, eps;
    float* partials;                           // [B][tiles_y * tiles_x][NV]
    int tiles_x, tiles_y;
};

__global__ __launch_bounds__(256) void tile_metrics_masked_kernel(const TileMP p) {
    __shared__ NgSsimLds s;
    __shared__ MaskLds m;
    __shared__ float red[4][NV];
    const int tid = threadIdx.x;
    int bid = blockIdx.x;
    const int tx = bid % p.tiles_x; bid /= p.tiles_x;
    const int ty = bid % p.tiles_y;
    const int b = bid / p.tiles_y;
    const int r = p.r;
    const size_t plane = size_t(p.H) * p.W, origin = size_t(p.y0) * p.W + p.x0;
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
    {   // the mask's patch: the indexing of ng_ssim_stage, whose barrier ends this staging too
        const float* V = p.valid + size_t(b) * plane + origin;
        // the flat loop of ng_ssim_stage (a wave per patch row and a lane per column, without the division, was measured slower:
        // 7.0 us of the call against 4.1 us)
        const int pw = TILE + 2 * r, h0 = ty * TILE - r, w0 = tx * TILE - r;
        for (int i = tid; i < pw * pw; i += 256) {
            const int y = i / pw, xx = i - y * pw;
            const int ph = h0 + y < p.ch + r ? h0 + y : p.ch - 1 + r, pwc = w0 + xx < p.cw + r ? w0 + xx : p.cw - 1 + r;
            const int hh = ng_reflect(ph, p.ch), ww = ng_reflect(pwc, p.cw);
            m.sv[y][xx] = V[size_t(hh) * p.W + ww] != 0.f ? 1 : 0;
        }
    }
    ng_ssim_stage(s, p.nir + size_t(b) * plane + origin, p.pred + size_t(b) * plane + origin, p.ch, p.cw, p.W,
                  ty * TILE - r, tx * TILE - r, r, tid);
    {   // valid taps per strip position; ng_ssim_hpass's barrier ends this pass too
        const int pw = TILE + 2 * r;
        for (int i = tid; i < pw * TILE; i += 256) {
            const int y = i / TILE, xx = i - y * TILE;
            // a fixed trip count: the eleven byte reads are issued together (xx + t <= 41 lies inside the row for every t; with the
            // trip count 2r+1 the loop became a chain of unaligned two-byte reads, each waited for, and cost 14 us of a 53 us call)
            int c = 0;
#pragma unroll
            for (int t = 0; t < 2 * MAXR + 1; ++t) c += t <= 2 * r ? m.sv[y][xx + t] : 0;
            m.hc[y][xx] = (unsigned char)c;
        }
    }
    ng_ssim_hpass(s, p.k, r, tid);
    const int full = (2 * r + 1) * (2 * r + 1);
    float acc[NV] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = (tid >> 5) + 8 * j, oh = ty * TILE + y;
        if (oh >= p.ch || ow >= p.cw) continue;
        if (!m.sv[y + r][x + r]) continue;     // a dropped pixel: nothing of it is added (its support is not clean either)
        acc[8] += 1.f;
        int taps = 0;
#pragma unroll
        for (int t = 0; t < 2 * MAXR + 1; ++t) taps += t <= 2 * r ? m.hc[y + t][x] : 0;       // y + t <= 41: inside the plane
        if (taps == full) {
            acc[2] += ng_ssim_at(s, p.k, r, y, x, p.c1, p.c2, p.eps);
            acc[9] += 1.f;
        }
        const float n = s.sa[y + r][x + r], f = s.sb[y + r][x + r];       // nir, pred
        const float d = f - n;
        acc[0] += fabsf(d);
        acc[1] += d * d;
        if (p.rgb) {                           // the formulas and epsilons of tile_metrics_kernel
            acc[3] += fabsf((f - R[j]) / (f + R[j] + 1e-6f) - (n - R[j]) / (n + R[j] + 1e-6f));
            acc[4] += fabsf((f - G[j]) / (f + G[j] + 1e-6f) - (n - G[j]) / (n + G[j] + 1e-6f));
            const float c = (R[j] - 7.5f) * (Bl[j] + 1.f);
            acc[5] += fabsf(2.5f * ((f - R[j]) / ((f + 6.f) * c + 1e-6f)) - 2.5f * ((n - R[j]) / ((n + 6.f) * c + 1e-6f)));
        }
        if (unsigned(oh - p.py0) < unsigned(p.patch) && unsigned(ow - p.px0) < unsigned(p.patch)) { acc[6] += n; acc[7] += f; acc[10] += 1.f; }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float v = ng_wave_sum(acc[i]);
        if ((tid & 63) == 0) red[tid >> 6][i] = v;
    }
    __syncthreads();
    if (tid < NV) p.partials[size_t(blockIdx.x) * NV + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// one block per tile: value j of chain c adds blocks c, c + FOLD, ... in order, then the chains are added in order (the association of
// tile_metrics_fold_kernel); the means divide by the folded counts
__global__ __launch_bounds__(FOLD_THREADS) void tile_metrics_masked_fold_kernel(const float* __restrict__ partials, int nblk, int patch,
                                                                                 float max_val, int has_rgb, float* __restrict__ rows) {
    __shared__ float part[FOLD][NV];
    __shared__ float tot[NV];
    const int j = threadIdx.x % NV, c = threadIdx.x / NV;
    const float* src = partials + size_t(blockIdx.x) * nblk * NV;
    float v = 0.f;
    for (int i = c; i < nblk; i += FOLD) v += src[size_t(i) * NV + j];
    part[c][j] = v;
    __syncthreads();
    if (threadIdx.x < NV) {
        float t = 0.f;
        for (int i = 0; i < FOLD; ++i) t += part[i][j];
        tot[j] = t;
    }
    __syncthreads();
    if (threadIdx.x >= NV) return;
    const float nan = __builtin_nanf("");
    const float t = tot[j], n_valid = tot[8], n_ssim = tot[9], n_patch = tot[10];
    float* row = rows + size_t(blockIdx.x) * NIRGAN_TILE_METRIC_MASKED_COLS;
    if (j < 2) {
        const float mean = n_valid > 0.f ? t * (1.f / n_valid) : nan;
        row[j] = mean;
        if (j == 1) row[3] = n_valid > 0.f ? (mean > 0.f ? 10.f * log10f(max_val * max_val / mean) : __builtin_inff()) : nan;
    } else if (j == 2) {
        row[2] = n_ssim > 0.f ? t * (1.f / n_ssim) : nan;
    } else if (j < 6) {
        if (has_rgb) row[j + 1] = n_valid > 0.f ? t * (1.f / n_valid) : nan;
    } else if (j < 8) {
        if (patch > 0) row[j + 1] = n_patch > 0.f ? t * (1.f / n_patch) : nan;
    } else if (j < 10) {
        row[j + 1] = t;                        // n_valid, n_ssim
    }
}

}  // namespace

extern "C" int64_t nirgan_tile_metrics_masked_ws_elems(int B, int ch, int cw) {
    if (B <= 0 || ch <= 0 || cw <= 0) return 0;
    return int64_t(B) * ((ch + TILE - 1) / TILE) * ((cw + TILE - 1) / TILE) * NV;
}

extern "C" int nirgan_tile_metrics_masked(const nirgan_tile_metrics_masked_desc* d, void* stream) {
    NG_REQUIRE(d != nullptr && d->nir && d->pred && d->valid && d->ws && d->rows, "tile_metrics_masked: null pointer");
    NG_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0, "tile_metrics_masked: empty problem");
    NG_REQUIRE(d->window >= 1 && d->window <= 2 * MAXR + 1 && (d->window & 1), "tile_metrics_masked: window=%d must be odd and <= %d", d->window,
               2 * MAXR + 1);
    const int r = d->window / 2;
    NG_REQUIRE(d->ch > 0 && d->cw > 0 && d->y0 >= 0 && d->x0 >= 0 && d->ch <= d->H - d->y0 && d->cw <= d->W - d->x0,
               "tile_metrics_masked: evaluation window y0=%d x0=%d %dx%d outside the %dx%d image", d->y0, d->x0, d->ch, d->cw, d->H, d->W);
    NG_REQUIRE(d->ch > r && d->cw > r, "tile_metrics_masked: evaluation window smaller than the SSIM window radius (reflect border)");
    NG_REQUIRE(d->sigma > 0.f && d->max_val > 0.f, "tile_metrics_masked: sigma and max_val must be positive");
    NG_REQUIRE(d->patch >= 0 && d->patch <= d->ch && d->patch <= d->cw, "tile_metrics_masked: patch=%d larger than the evaluation window", d->patch);
    NG_REQUIRE(int64_t(d->H) * d->W < (int64_t(1) << 31), "tile_metrics_masked: image too large");
    NG_REQUIRE(int64_t(d->ch) * d->cw <= (int64_t(1) << 24), "tile_metrics_masked: %dx%d pixels in the evaluation window, more than 2^24 (counts are exact fp32)",
               d->ch, d->cw);
    TileMP p;
    p.rgb = d->rgb; p.nir = d->nir; p.pred = d->pred; p.valid = d->valid;
    p.H = d->H; p.W = d->W; p.y0 = d->y0; p.x0 = d->x0; p.ch = d->ch; p.cw = d->cw; p.r = r;
    p.patch = d->patch; p.py0 = d->ch / 2 - d->patch / 2; p.px0 = d->cw / 2 - d->patch / 2;
    ng_ssim_taps(d->window, d->sigma, p.k);
    p.c1 = (0.01f * d->max_val) * (0.01f * d->max_val);
    p.c2 = (0.03f * d->max_val) * (0.03f * d->max_val);
    p.eps = d->eps;
    p.tiles_x = (d->cw + TILE - 1) / TILE; p.tiles_y = (d->ch + TILE - 1) / TILE;
    const int64_t per_tile = int64_t(p.tiles_x) * p.tiles_y, blocks = per_tile * d->B;
    NG_REQUIRE(blocks < (int64_t(1) << 31), "tile_metrics_masked: too many blocks");
    NG_REQUIRE(d->ws_elems >= blocks * NV, "tile_metrics_masked: workspace too small (nirgan_tile_metrics_masked_ws_elems)");
    p.partials = d->ws;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tile_metrics_masked_kernel, dim3(unsigned(blocks)), dim3(256), 0, st, p);
    hipLaunchKernelGGL(tile_metrics_masked_fold_kernel, dim3(unsigned(d->B)), dim3(FOLD_THREADS), 0, st, d->ws, int(per_tile), d->patch,
                       d->max_val, d->rgb ? 1 : 0, d->rows);
    return nirgan_check_launch("tile_metrics_masked");
}
