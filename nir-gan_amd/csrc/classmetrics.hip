// Land-cover-stratified validation metrics: the rows of nirgan_tile_metrics (tilemetrics.hip) split by the class id of a uint8 mask
// (the five-class CLC legend of the reference's utils/plot_clc_utils.py / plot_clc_pred.py).  Per tile and class c, over the pixels
// of the evaluation window whose mask value equals c: their count, mean |d|, mean d^2, the mean over THOSE pixels of the SSIM map of
// the whole window (the filter crosses class borders and reflects at the window's border), PSNR from that l2, and the NDVI / NDWI /
// EVI L1 errors.  Nothing outside the window is read, of the images or of the mask.
//
// The scheme of tilemetrics.hip.  Launch 1: one block per (tile, 32x32 block of the window); the mask bytes and rgb of a thread's four
// output pixels are loaded before the LDS staging of nir and pred (ssim_dev.h), so that they are in flight under it; per class, in
// class order, the six per-pixel terms go through the wave shuffle sum as (m == c ? v : 0) and the count through a ballot; the
// block's [classes][8] partials (slot 0: the count as an int32) go to the workspace.  Launch 2: one block per tile adds that tile's
// partials in block order and finishes the rows.  A tile's association depends only on (ch, cw, classes): bitwise the same alone and
// inside any batch, counts are integers, no float atomics.
#include "ssim_dev.h"

namespace {

constexpr int TILE = NG_SSIM_TILE;
constexpr int MAXR = NG_SSIM_MAXR;
constexpr int NV = 8;                          // per class: count (int32), l1, l2, ssim, ndvi, ndwi, evi, unused
constexpr int NT = 6;                          // float terms per pixel
constexpr int CHAINS = 4;                      // strided chains of the per-tile fold
constexpr int NOCLASS = 0xFF;                  // mask value of a thread's pixel past the window: no class (classes <= 8)

struct ClassP {
    const float* rgb; const float* nir; const float* pred; const uint8_t* mask;
    int H, W, y0, x0, ch, cw, r, classes;
    float k[2 * MAXR + 1];
    float c1, c2, eps;
    float* partials;                           // [B][tiles_y * tiles_x][classes][NV]
    int tiles_x, tiles_y;
};

__global__ __launch_bounds__(256) void class_metrics_kernel(const ClassP p) {
    __shared__ NgSsimLds s;
    __shared__ float red[4][NIRGAN_CLASS_MAX][NT];
    __shared__ int redn[4][NIRGAN_CLASS_MAX];
    const int tid = threadIdx.x;
    int bid = blockIdx.x;
    const int tx = bid % p.tiles_x; bid /= p.tiles_x;
    const int ty = bid % p.tiles_y;
    const int b = bid / p.tiles_y;
    const int r = p.r;
    const size_t plane = size_t(p.H) * p.W, origin = size_t(p.y0) * p.W + p.x0;
    // the four output pixels of this thread: rows (tid >> 5) + 8 j, column tid & 31 (a wave reads two 32-byte segments of the mask)
    const int x = tid & 31, ow = tx * TILE + x;
    float R[4], G[4], Bl[4];
    int m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int oh = ty * TILE + (tid >> 5) + 8 * j;
        R[j] = G[j] = Bl[j] = 0.f;
        m[j] = NOCLASS;
        if (oh < p.ch && ow < p.cw) {
            const size_t at = origin + size_t(oh) * p.W + ow;
            m[j] = p.mask[size_t(b) * plane + at];
            if (p.rgb) {
                const float* q = p.rgb + size_t(b) * 3 * plane + at;
                R[j] = q[0]; G[j] = q[plane]; Bl[j] = q[2 * plane];
            }
        }
    }
    ng_ssim_stage(s, p.nir + size_t(b) * plane + origin, p.pred + size_t(b) * plane + origin, p.ch, p.cw, p.W,
                  ty * TILE - r, tx * TILE - r, r, tid);
    ng_ssim_hpass(s, p.k, r, tid);
    float e[NT][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < NT; ++i) e[i][j] = 0.f;
        if (m[j] == NOCLASS) continue;
        const int y = (tid >> 5) + 8 * j;
        e[2][j] = ng_ssim_at(s, p.k, r, y, x, p.c1, p.c2, p.eps);
        const float n = s.sa[y + r][x + r], f = s.sb[y + r][x + r];       // nir, pred
        const float d = f - n;
        e[0][j] = fabsf(d);
        e[1][j] = d * d;
        if (p.rgb) {                           // the formulas and epsilons of pix_loss_kernel (losses.hip), criterion l1
            e[3][j] = fabsf((f - R[j]) / (f + R[j] + 1e-6f) - (n - R[j]) / (n + R[j] + 1e-6f));
            e[4][j] = fabsf((f - G[j]) / (f + G[j] + 1e-6f) - (n - G[j]) / (n + G[j] + 1e-6f));
            const float c = (R[j] - 7.5f) * (Bl[j] + 1.f);
            e[5][j] = fabsf(2.5f * ((f - R[j]) / ((f + 6.f) * c + 1e-6f)) - 2.5f * ((n - R[j]) / ((n + 6.f) * c + 1e-6f)));
        }
    }
    // per class, in class order: a select (not a product: a NaN of another class's pixel stays out) through the wave sum
    for (int c = 0; c < p.classes; ++c) {
        float a[NT] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = m[j] == c;
            cnt += __popcll(__ballot(in));
#pragma unroll
            for (int i = 0; i < NT; ++i) a[i] += in ? e[i][j] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const float v = ng_wave_sum(a[i]);
            if ((tid & 63) == 0) red[tid >> 6][c][i] = v;
        }
        if ((tid & 63) == 0) redn[tid >> 6][c] = cnt;
    }
    __syncthreads();
    if (tid < p.classes * NV) {
        const int c = tid >> 3, j = tid & (NV - 1);
        float* dst = p.partials + (size_t(blockIdx.x) * p.classes + c) * NV + j;
        if (j == 0) *reinterpret_cast<int*>(dst) = (redn[0][c] + redn[1][c]) + (redn[2][c] + redn[3][c]);
        else if (j <= NT) *dst = (red[0][c][j - 1] + red[1][c][j - 1]) + (red[2][c][j - 1] + red[3][c][j - 1]);
        else *dst = 0.f;
    }
}

// one block per tile; thread = (chain, class, value): value j of class c in chain q adds blocks q, q + CHAINS, ... in order, then the
// chains are added in order.  Slot 0 (the count) is added as int32.
__global__ __launch_bounds__(256) void class_metrics_fold_kernel(const float* __restrict__ partials, int nblk, int classes, float max_val,
                                                                 int has_rgb, float* __restrict__ rows) {
    __shared__ float part[CHAINS][NIRGAN_CLASS_MAX][NV];
    __shared__ int partn[CHAINS][NIRGAN_CLASS_MAX];
    __shared__ int total[NIRGAN_CLASS_MAX];
    const int j = threadIdx.x & (NV - 1), c = (threadIdx.x >> 3) & (NIRGAN_CLASS_MAX - 1), q = threadIdx.x >> 6;
    const float* src = partials + size_t(blockIdx.x) * nblk * classes * NV;
    if (c < classes) {
        if (j == 0) {
            int n = 0;
            for (int i = q; i < nblk; i += CHAINS) n += *reinterpret_cast<const int*>(src + (size_t(i) * classes + c) * NV);
            partn[q][c] = n;
        } else {
            float v = 0.f;
            for (int i = q; i < nblk; i += CHAINS) v += src[(size_t(i) * classes + c) * NV + j];
            part[q][c][j] = v;
        }
    }
    __syncthreads();
    if (q == 0 && c < classes && j == 0) {
        int n = 0;
        for (int i = 0; i < CHAINS; ++i) n += partn[i][c];
        total[c] = n;
    }
    __syncthreads();
    if (q != 0 || c >= classes || j > NT) return;
    float* row = rows + (size_t(blockIdx.x) * classes + c) * NIRGAN_CLASS_METRIC_COLS;
    const int n = total[c];
    if (j == 0) { row[0] = float(n); return; }                            // exact: ch * cw < 2^24
    float t = 0.f;
    for (int i = 0; i < CHAINS; ++i) t += part[i][c][j];
    const float nan = __builtin_nanf("");
    const float mean = n > 0 ? t / float(n) : nan;
    if (j <= 3) {
        row[j] = mean;
        if (j == 2) row[4] = n > 0 ? (mean > 0.f ? 10.f * log10f(max_val * max_val / mean) : __builtin_inff()) : nan;
    } else if (has_rgb) {
        row[j + 1] = mean;
    }
}

}  // namespace

extern "C" int64_t nirgan_class_metrics_ws_elems(int B, int ch, int cw, int classes) {
    if (B <= 0 || ch <= 0 || cw <= 0 || classes < 1 || classes > NIRGAN_CLASS_MAX) return 0;
    return int64_t(B) * ((ch + TILE - 1) / TILE) * ((cw + TILE - 1) / TILE) * classes * NV;
}

extern "C" int nirgan_class_metrics(const nirgan_class_metrics_desc* d, void* stream) {
    NG_REQUIRE(d != nullptr && d->nir && d->pred && d->mask && d->ws && d->rows, "class_metrics: null pointer");
    NG_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0, "class_metrics: empty problem");
    NG_REQUIRE(d->classes >= 1 && d->classes <= NIRGAN_CLASS_MAX, "class_metrics: classes=%d must lie in 1..%d", d->classes, NIRGAN_CLASS_MAX);
    NG_REQUIRE(d->window >= 1 && d->window <= 2 * MAXR + 1 && (d->window & 1), "class_metrics: window=%d must be odd and <= %d", d->window, 2 * MAXR + 1);
    const int r = d->window / 2;
    NG_REQUIRE(d->ch > 0 && d->cw > 0 && d->y0 >= 0 && d->x0 >= 0 && d->ch <= d->H - d->y0 && d->cw <= d->W - d->x0,
               "class_metrics: evaluation window y0=%d x0=%d %dx%d outside the %dx%d image", d->y0, d->x0, d->ch, d->cw, d->H, d->W);
    NG_REQUIRE(d->ch > r && d->cw > r, "class_metrics: evaluation window smaller than the SSIM window radius (reflect border)");
    NG_REQUIRE(d->sigma > 0.f && d->max_val > 0.f, "class_metrics: sigma and max_val must be positive");
    NG_REQUIRE(int64_t(d->H) * d->W < (int64_t(1) << 31), "class_metrics: image too large");
    NG_REQUIRE(int64_t(d->ch) * d->cw < (int64_t(1) << 24), "class_metrics: evaluation window of %dx%d pixels: the counts are exact as floats below 2^24 only", d->ch, d->cw);
    ClassP p;
    p.rgb = d->rgb; p.nir = d->nir; p.pred = d->pred; p.mask = d->mask;
    p.H = d->H; p.W = d->W; p.y0 = d->y0; p.x0 = d->x0; p.ch = d->ch; p.cw = d->cw; p.r = r; p.classes = d->classes;
    ng_ssim_taps(d->window, d->sigma, p.k);
    p.c1 = (0.01f * d->max_val) * (0.01f * d->max_val);
    p.c2 = (0.03f * d->max_val) * (0.03f * d->max_val);
    p.eps = d->eps;
    p.tiles_x = (d->cw + TILE - 1) / TILE; p.tiles_y = (d->ch + TILE - 1) / TILE;
    const int64_t per_tile = int64_t(p.tiles_x) * p.tiles_y, blocks = per_tile * d->B;
    NG_REQUIRE(blocks < (int64_t(1) << 31), "class_metrics: too many blocks");
    NG_REQUIRE(d->ws_elems >= blocks * d->classes * NV, "class_metrics: workspace too small (nirgan_class_metrics_ws_elems)");
    p.partials = d->ws;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(class_metrics_kernel, dim3(unsigned(blocks)), dim3(256), 0, st, p);
    hipLaunchKernelGGL(class_metrics_fold_kernel, dim3(unsigned(d->B)), dim3(256), 0, st, d->ws, int(per_tile), d->classes, d->max_val,
                       d->rgb ? 1 : 0, d->rows);
    return nirgan_check_launch("class_metrics");
}
