/*
 * nirgan_hip.h -- C ABI of libnirgan_hip.so (gfx950 / MI355X).
 *
 * The drop-in boundary for the NIR-GAN Pix2Pix hot path.  The reference implements the path
 * with stock torch.nn layers (Python only, no FFI of its own); the entry points below are
 * what a binding of that path binds instead.  Each one cites the reference call site(s) it
 * replaces (paths relative to the reference repository).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch); the library never
 *     allocates, frees or retains device memory;
 *   - `stream` is a hipStream_t passed as void*; every launch goes to that stream, no hidden
 *     synchronisation, safe for hipGraph capture;
 *   - activations are fp32 "NHWC with halo": [B][Hp][Wp][cs] floats, cs % 4 == 0, base 16-byte
 *     aligned.  Convolutions are *valid* convolutions over such buffers; the producer of a
 *     buffer writes the halo (reflect copies, or zeros that are set once at allocation);
 *   - weights are consumed in a packed layout [N][ntaps*run] (K contiguous) produced by
 *     nirgan_pack_rows from the reference layouts (Conv2d Cout,Cin,kh,kw; ConvTranspose2d
 *     Cin,Cout,kh,kw; Linear out,in) through an int32 index map;
 *   - every function returns 0 on success, a negative code on error (message from
 *     nirgan_last_error()); descriptors are validated (alignment, extents) before launch.
 */
#ifndef NIRGAN_HIP_H
#define NIRGAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NIRGAN_MAX_TAPS 16

#define NIRGAN_OK 0
#define NIRGAN_ERR_ARG (-1)      /* invalid descriptor / argument */
#define NIRGAN_ERR_LAUNCH (-2)   /* HIP launch error */

#define NIRGAN_ACT_NONE 0
#define NIRGAN_ACT_RELU 1
#define NIRGAN_ACT_LRELU 2
#define NIRGAN_ACT_TANH 3

#define NIRGAN_BORDER_KEEP 0     /* halo untouched (zero halo set once by the owner) */
#define NIRGAN_BORDER_REFLECT 1  /* halo = reflection of the interior (nn.ReflectionPad2d) */

int nirgan_version(void);
const char* nirgan_last_error(void);

/* ---------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on the MFMA pipe (v_mfma_f32_32x32x2_f32, exact fp32).
 *   out[b][oh*out_stride+out_oh][ow*out_stride+out_ow][n] (+bias[n]) =
 *       sum_{t<ntaps} sum_{c<run} in[b][oh*in_stride+in_oh+tap_dh[t]][ow*in_stride+in_ow+tap_dw[t]][c] * w[n][t*run+c]
 * `run` floats are read contiguously from the tap's pixel (run may span several pixels:
 * run = kw*cs packs a kernel row).  One descriptor covers: forward of Conv2d (stride 1/2),
 * data-gradient of Conv2d (flipped weights; stride-2 as 4 sub-pixel phases), forward and
 * data-gradient of ConvTranspose2d (4 phases / strided), the 1x1 "tap-plane" products of the
 * single-output-channel 7x7 / 4x4 layers, and nn.Linear.
 * Replaces: nn.Conv2d / nn.ConvTranspose2d forward+backward at model/networks.py:342,349,
 * 360-363,367,405-427,559,566,574,579; nn.Linear at model/generator_inject.py:90,110.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const float* in;  int64_t in_elems;   /* input buffer and its size in floats */
    int in_hp, in_wp, in_cs;              /* halo'd height, width, floats per pixel */
    int run;                              /* contiguous floats per tap (multiple of 4) */
    int in_stride, in_oh, in_ow;          /* input step per output pixel, origin */
    int ntaps;
    int tap_dh[NIRGAN_MAX_TAPS], tap_dw[NIRGAN_MAX_TAPS];
    const float* w;   int64_t w_elems;    /* packed weights [N][ntaps*run] */
    const float* bias;                    /* [N] or NULL */
    float* out;       int64_t out_elems;
    int out_hp, out_wp, out_cs;
    int out_stride, out_oh, out_ow;
    int B, OH, OW, N;
    const float* zero_page;               /* >= 64 zero bytes, 16-byte aligned */
    /* optional split-K for problems with few output tiles (< 1 tile per CU slot): the K-steps are divided over
     * `ksplit` blocks per tile, partial tiles go to split_ws [ksplit][B*OH*OW][N] and are summed (fixed order,
     * + bias) into `out` by a second small launch.  ksplit <= 1: off. */
    int ksplit; float* split_ws; int64_t split_ws_elems;
    /* operand precision of the contraction: 0 = fp32 (default; the parity path), 1 = both operands rounded to bf16
     * (round-to-nearest-even) as they enter the matrix pipe, fp32 accumulate (BASELINE.json configs[4] "bf16 MFMA"),
     * 2 = fp32 operands split into two bf16 terms each, three bf16 products per fp32 product (error <= ~2^-16 relative
     * per product), fp32 accumulate.  Buffers stay fp32 in every mode. */
    int precision;
    /* 1: `w` points to bf16 values (same [N][ntaps*run] layout, written by nirgan_pack_rows_bf16; w_elems counts bf16
     * elements).  Only with precision == 1 and run % 8 == 0: the weights are rounded once when packed instead of at every
     * fragment read -- identical values, 25 % fewer operand bytes per K-step. */
    int w_bf16;
    /* 1: `in` points to bf16 values (a producer's out_bf16 / dy_bf16 twin: same halo'd geometry, in_elems counts bf16
     * elements).  Only together with w_bf16 (precision 1, run % 8 == 0, in_cs % 8 == 0): both operands are then read as
     * stored, half the bytes and LDS-DMA pieces per K-step, no conversion in the K loop. */
    int in_bf16;
    /* optional: partial sums for the instance norm that follows (nirgan_instnorm_fwd with stats_chunks / stats_shift).  Every 64 output
     * pixels x N channels held by a wave leave FOUR values per channel in stats_ws[b][stats_chunk0 + chunk][4][N]: a shift k (the
     * chunk's first pixel, WITHOUT the bias), sum (v - k), sum (v - k)^2, and the count 64 -- sums about a value of the data itself carry
     * no cancellation, nirgan_instnorm_fwd re-bases the chunks onto one shift.  chunk = (tile within the sample) * 2 + the wave's row
     * half.  The problem then has OH * OW % 128 == 0 (a tile does not cross samples) and no split-K; it contributes OH * OW / 64 chunks
     * per sample, a launch of several problems over one output (the sub-pixel phases of a transposed convolution) numbers them with
     * stats_chunk0, and stats_chunks is the total per sample (the row stride of stats_ws).  stats_ws >= B * stats_chunks * 4 * N floats. */
    float* stats_ws; int64_t stats_ws_elems; int stats_chunk0, stats_chunks;
    /* optional: the launch writes the gradient wrt the OUTPUT of a convolution + instance-norm (+ReLU / LeakyReLU) layer (it is the data
     * gradient of that layer's consumer); the first pass of that layer's backward (nirgan_instnorm_bwd: sums of g_z = g * act'(z) and of
     * g_z * z, z = (y - mean) * rstd) is then taken in the epilogue, next to the store of g: every 128-pixel tile leaves its sums in
     * fuse_part[b][fuse_chunk0 + tile within the sample][2][N] (fixed order, no atomics) and nirgan_instnorm_bwd runs with
     * sums_chunks = fuse_chunks (its first pass is not launched).  fuse_y: the layer's pre-normalisation output, dense
     * [B][fuse_h][fuse_w][N]; the launch's output pixel (oh, ow) is y pixel (oh * out_stride + fuse_oh, ow * out_stride + fuse_ow).
     * Needs OH * OW % 128 == 0, N % 4 == 0, no split-K, no bias.  fuse_part >= B * fuse_chunks * 2 * N floats. */
    const float* fuse_y; const float* fuse_mean; const float* fuse_rstd;
    int fuse_h, fuse_w, fuse_oh, fuse_ow, fuse_act; float fuse_slope;
    float* fuse_part; int64_t fuse_part_elems; int fuse_chunk0, fuse_chunks;
    /* bf16 operand mode: `out` points to bf16 elements (same geometry, out_elems counts them) -- the convolution's output in front of an
     * instance norm is stored rounded to nearest even while the statistics (stats_ws) come from the fp32 accumulators; the norm's launches
     * read it with y_bf16 = 1.  Needs N % 4 == 0, out_cs % 4 == 0, no split-K.  fuse_y_bf16: fuse_y points to such a tensor. */
    int out_bf16, fuse_y_bf16;
    /* kernel choice where more than one applies (A/B measurements, tests): 0 = default -- problems with both operands stored as bf16,
     * N % 256 == 0, run % 64 == 0 and rounds of 256 x 256 tiles that fill at least 62 % of the CUs run on the 256 x 256 x 64 eight-phase tile (one workgroup of
     * eight waves per CU, LDS-DMA in flight across the barriers), everything else on the 128-row tile; NIRGAN_CONV_TILE128 = always the
     * 128-row tile (results differ by fp32 summation order only); NIRGAN_CONV_X3_R4 as below.  Any other value fails with NIRGAN_ERR_ARG. */
    int algo;
    /* precision 3 -- fp32-EQUIVALENT on the bf16 matrix pipe (round 5): every fp32 operand is split into three bf16 terms h + m + l (exact)
     * and a product is contracted as the six bf16 products down to 2^-16 of the leading one (dropped: <= 2^-24 |a b|), fp32 accumulate;
     * buffers and results are those of precision 0; measured against float64 the convolutions sit at 0.7-1.0 x the exact tile's error, the weight
     * gradients at up to 1.65 x (max) / 2.4 x (rms) of it (twice the pixels per split in one fp32 chain at N = 128).  The activations are split inside the kernel (fp32 `in` as in every
     * mode); the packed weights come as three bf16 planes written by nirgan_split3 from `w`: w_x3 = plane h, planes m and l follow
     * w_x3_plane bf16 elements apart.  Problems the split tile does not cover (run % 32, N % 64, split-K, no w_x3) run as precision 0. */
    const void* w_x3; int64_t w_x3_plane;
    /* out_span = 2 (precision 3 only; 0 / 1 = one pixel per row): a GEMM row writes TWO horizontally adjacent output pixels -- N = 2 C
     * columns, column n = channel n % C of pixel (oh out_stride + out_oh, ow out_stride + out_ow + n / C); needs out_cs == C (dense pixels)
     * and out_stride >= 2.  Two sub-pixel phases of one output row of a stride-2 transposed convolution / data gradient with C = 64 become
     * ONE problem of 128-column tiles over the union of their taps (zero weight rows where a phase has no tap): the staged activation
     * rows serve both phases and the launch's two problems (output-row parities) balance over the persistent workgroups.  bias holds N
     * values (the layer's C twice).  The instance-norm partial sums and the fused backward sums keep their per-channel records: a chunk
     * of rows leaves two records (pixel parity 0, then 1) of C columns -- stats_chunk0 + 2 OH OW / 64 <= stats_chunks, stats_ws and
     * fuse_part sized with C; fuse_mean / fuse_rstd / fuse_y are those of the C-channel tensor.
     * Second form, out_cs == N: the caller already describes the output in pixel pairs (out_wp = W / 2, any out_stride; no fuse_y) --
     * the generator's first convolution with two adjacent outputs per GEMM row; out_span then only shapes the statistics' records. */
    int out_span;
} nirgan_conv_desc;
#define NIRGAN_CONV_TILE128 1
#define NIRGAN_CONV_X3_R4 4     /* precision 3, N % 128 == 0: the four-wave register-fed tile of igemm_x3r.h instead of the eight-wave tile (A/B; same output bits).
                                 * Taken where it applies: OW >= 16, B OH OW < 2^24 and out_elems <= 2^30 (its stores address the output with 32-bit byte
                                 * offsets; for the Winograd plane batches, per plane); other launches run on the eight-wave tile. */

int nirgan_conv_igemm(const nirgan_conv_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * Implicit-GEMM weight gradient (MFMA, split over pixels into deterministic slabs).
 *   slab[s][n][t*run+c] = sum_{m in split s}
 *       p[b][oh+p_oh][ow+p_ow][n] * q[b][oh*q_stride+q_oh+tap_dh[t]][ow*q_stride+q_ow+tap_dw[t]][c]
 * with m = (b,oh,ow) over B*OH*OW.  Conv2d: p = dY (n = cout), q = X (c = cin).
 * ConvTranspose2d: p = X (n = cin), q = dY (c = cout).  nirgan_reduce_rows then sums the
 * slabs into the reference-layout gradient.  Replaces autograd's weight gradient of the same
 * layers as nirgan_conv_igemm.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const float* p;   int64_t p_elems;
    int p_hp, p_wp, p_cs, p_oh, p_ow;
    const float* q;   int64_t q_elems;
    int q_hp, q_wp, q_cs, q_stride, q_oh, q_ow;
    int run, ntaps;
    int tap_dh[NIRGAN_MAX_TAPS], tap_dw[NIRGAN_MAX_TAPS];
    int B, OH, OW, N;                     /* N: rows of the gradient; round_up(N,4) <= p_cs */
    float* slabs;     int64_t slab_elems; /* [nsplit][N][ntaps*run] */
    int nsplit, rows_per_split;           /* rows_per_split % 32 == 0, nsplit*rows_per_split >= B*OH*OW */
    const float* zero_page;
    int precision;                        /* as in nirgan_conv_desc */
    int nplanes; int64_t p_plane, q_plane;/* > 1: that many independent problems of this geometry in one grid; plane i reads
                                           * p + i*p_plane, q + i*q_plane (floats) and writes slabs [i][nsplit][N][K] (fp32 tile only) */
    int pq_bf16;                          /* 1: p and q point to bf16 twins (same geometry; the producers' out_bf16 / dy_bf16);
                                           * precision 1, N > 64, and N, run, p_cs, q_cs multiples of 8 */
    int algo;                             /* kernel choice where more than one applies (A/B measurements, tests): 0 = default (plane-matrix
                                           * problems walk their units as persistent workgroups); NIRGAN_WGRAD_ONE_UNIT = one unit per workgroup;
                                           * NIRGAN_WGRAD_TILE128 as below.  Any other value fails with NIRGAN_ERR_ARG. */
} nirgan_wgrad_desc;
#define NIRGAN_WGRAD_ONE_UNIT 1
#define NIRGAN_WGRAD_TILE128 2   /* bf16 twins: never the 256 x 256 x 64 eight-phase tile (persistent workgroups, one per CU), which is the
                                  * default for N % 256 == 0, ntaps * run % 256 == 0, OW % 64 == 0 or 64 % OW == 0, rows_per_split % 64 == 0 */

int nirgan_wgrad_igemm(const nirgan_wgrad_desc* d, void* stream);

/* Up to 4 independent descriptors of the same tile width (all N <= 64 or all N > 64) in one launch: the four
 * sub-pixel phases of a stride-2 data gradient or of a ConvTranspose2d forward (model/networks.py:349,360-363). */
int nirgan_conv_igemm_group(const nirgan_conv_desc* const* descs, int n, void* stream);

/* Horizontally fused launch of a data-gradient convolution and the weight gradient of the same layer (both
 * read the same dY): one grid holds the tiles of both, so the partly filled last round of one problem is
 * filled by the other.  Semantics = nirgan_conv_igemm(c) followed by nirgan_wgrad_igemm(w). */
int nirgan_conv_wgrad_pair(const nirgan_conv_desc* c, const nirgan_wgrad_desc* w, void* stream);

/* names of the kernels the three launchers above pick for a descriptor (what a profile of the launch shows; NULL for an invalid
 * descriptor): the 128-row tiles or, in the bf16 operand mode, the 256 x 256 x 64 eight-phase tiles */
const char* nirgan_conv_kernel_name(const nirgan_conv_desc* d);
const char* nirgan_wgrad_kernel_name(const nirgan_wgrad_desc* d);
const char* nirgan_conv_wgrad_pair_kernel_name(const nirgan_conv_desc* c, const nirgan_wgrad_desc* w);

/* dst[n*dst_row_stride + map[k]] (= | +=) sum_s slabs[s][n][k]  for map[k] >= 0.
 * K % 4 == 0, 1 <= N <= 65535, slabs 16-byte aligned.  dst_elems clamps: a store whose index n*dst_row_stride + map[k] is >= dst_elems
 * is DROPPED (no error; nothing at or behind dst + dst_elems is read or written).  The same holds for nirgan_reduce_rows_part and for the
 * taps = 0 jobs of nirgan_reduce_rows_batch; its taps = T jobs store whole runs and rely on dst_row_stride >= Cin * T instead. */
int nirgan_reduce_rows(const float* slabs, int nsplit, int N, int K, const int32_t* map,
                       float* dst, int64_t dst_elems, int dst_row_stride, int accumulate, void* stream);
/* The same over a BAND of the slabs' rows: dst[n*dst_row_stride + map[k]] (= | +=) sum_s slabs[s][row0 + n][k] for n < rows (slabs of
 * N rows).  The weight gradient of the generator's first convolution, taken with two adjacent output pixels per GEMM row (its slab rows
 * are (pixel parity, output channel)), folds its two bands into the one weight tensor with two calls, the second accumulating
 * (model/networks.py:342 through autograd). */
int nirgan_reduce_rows_part(const float* slabs, int nsplit, int N, int row0, int rows, int K, const int32_t* map,
                            float* dst, int64_t dst_elems, int dst_row_stride, int accumulate, void* stream);

/* The slab sums of several weight gradients in one launch (a network's layers: launch latency for up to 31 MB each otherwise).
 * jobs_device: njobs x 10 int64 in DEVICE memory: {slabs, dst, map, nsplit, N, K, dst_elems, dst_row_stride | (accumulate ? 1 << 32 : 0),
 * first_block, taps}.  taps = 0: job j owns N_j * ceil(K_j / 256) blocks and scatters through map, the arithmetic and association of
 * nirgan_reduce_rows.  taps = T > 0: the caller asserts map[t * Cin + c] == c * T + t (K = T * Cin, Cin % 64 == 0, T <= 16: the Conv2d
 * weight's own layout [N][Cin][kh][kw], dst_row_stride >= Cin * T): job j owns N_j * Cin / 64 blocks which store 64 * T contiguous
 * floats each (same sums, no 4-byte scatter).  total_blocks = the sum; K % 4 == 0, slabs 16-byte aligned. */
int nirgan_reduce_rows_batch(const int64_t* jobs_device, int njobs, int total_blocks, void* stream);

/* dst[n][k] = map[k] >= 0 ? src[n*src_row_stride + map[k]] : 0   (weight packing).
 * K % 4 == 0, 1 <= N <= 65535, dst 16-byte aligned.  src_elems clamps: a source index n*src_row_stride + map[k] that is >= src_elems
 * reads as 0 (no error; nothing at or behind src + src_elems is read).  The same holds for nirgan_pack_rows_bf16 and for every job of
 * nirgan_pack_rows_batch. */
int nirgan_pack_rows(const float* src, int64_t src_elems, int src_row_stride, const int32_t* map,
                     float* dst, int N, int K, void* stream);

/* nirgan_pack_rows with the destination in bf16 (round to nearest even), K % 8 == 0 */
int nirgan_pack_rows_bf16(const float* src, int64_t src_elems, int src_row_stride, const int32_t* map,
                          void* dst_bf16, int N, int K, void* stream);
/* All weight packs of a step in one launch.  jobs_device: njobs x 10 int64 in DEVICE memory:
 * {src, dst, map, src_elems, N, K, src_row_stride | (bf16 destination ? 1 << 32 : 0), first_block, w_x3, w_x3_plane}; job j owns blocks
 * [first_block_j, first_block_j + N_j * ceil(K_j / 1024)); total_blocks = their sum.  w_x3 != 0 (fp32 destination only): the job also
 * writes the three bf16 planes of nirgan_split3 for its packed values (plane stride w_x3_plane bf16 elements). */
int nirgan_pack_rows_batch(const int64_t* jobs_device, int njobs, int total_blocks, void* stream);

/* precision 3 (nirgan_conv_desc.w_x3): n fp32 values -> three bf16 planes dst[0..n), dst[plane..), dst[2 plane..) with
 * src = h + m + l exactly, each term the round-to-nearest-even bf16 of what the previous ones left.  n % 8 == 0, plane >= n, plane % 8 == 0.
 * Runs once per optimizer step on the packed weights of the layers that take the split tile (model/networks.py:349,360-363,559-574). */
int nirgan_split3(const float* src, void* dst_bf16, int64_t n, int64_t plane, void* stream);

/* ---------------------------------------------------------------------------------------
 * InstanceNorm2d(affine=False, eps) + activation + residual + halo write, forward.
 *   z = norm ? (y - mean_bc) * rstd_bc : y ;  a = act(z) + residual ;  out interior = a,
 *   reflect halo of width o_pad written when border == NIRGAN_BORDER_REFLECT.
 * Biased variance over H*W per (b,c); mean/rstd saved for backward.
 * Replaces: nn.InstanceNorm2d + nn.ReLU / nn.LeakyReLU(0.2) / residual add / the
 * nn.ReflectionPad2d of the next layer, model/networks.py:30,343-344,350-351,364-365,
 * 405-433,559,567-568,575-576.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const float* y;                       /* [B][H][W][C] dense */
    int B, H, W, C;
    int norm; float eps;
    float* mean; float* rstd;             /* [B][C] */
    int act; float slope;
    const float* residual; int r_hp, r_wp, r_pad;   /* optional [B][r_hp][r_wp][C], interior at r_pad */
    float* out; int o_hp, o_wp, o_pad; int border;   /* out = NULL and out_bf16 = NULL (with norm): statistics only; out = NULL with
                                                      * out_bf16: only the twin is stored (every consumer reads bf16) */
    float* ws; int64_t ws_elems;          /* >= B * nchunk * 2 * C floats, see nirgan_instnorm_ws_elems */
    void* out_bf16;                       /* optional twin of `out` (same geometry, bf16 elements): every store is mirrored, rounded
                                           * to nearest even -- the operand the bf16 mode's convolutions read (in_bf16) */
    int stats_chunks;                     /* > 0 (with norm): the producer of y already left per-chunk partial sums in ws as
                                           * [B][stats_chunks][4][C] = {k, sum (v - k), sum (v - k)^2, count} with v = y - stats_shift and k a
                                           * value of the chunk itself (nirgan_wino6_output / nirgan_conv_igemm with stats_ws): the pass
                                           * over y that would form them is skipped, the chunks are re-based onto one shift in a fixed order */
    const float* stats_shift;             /* [C], what the producer left out of v (the convolution's bias); NULL = 0 */
    int y_bf16;                           /* 1: y points to bf16 elements (a convolution launch with out_bf16) */
} nirgan_in_fwd_desc;

int64_t nirgan_instnorm_ws_elems(int B, int H, int W, int C);
int nirgan_instnorm_fwd(const nirgan_in_fwd_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * Backward of the same block.  Incoming gradient g_a = gather(g) (+ g2):
 *   g is a halo'd buffer [B][g_hp][g_wp][C]; g_fold = 1 folds a reflect halo of width g_pad
 *   back onto the interior (adjoint of ReflectionPad2d), g_fold = 0 reads the interior only;
 *   g2 is an optional dense [B][H][W][C] term (skip connection).
 *   g_z = g_a * act'(z), z = norm ? (y - mean)*rstd : y;  dy = norm ? rstd*(g_z - mean(g_z) - z*mean(g_z*z)) : g_z.
 * dy is written to the interior (d_pad) of a zero-halo buffer that feeds the data- and
 * weight-gradient GEMMs; gsum_out (optional, dense) receives g_a; dbias (optional, [C])
 * accumulates sum dy when norm == 0 (it needs ws >= B * nchunk * C floats, one row of channel
 * sums per block, added in a fixed order).  With norm == 1 the sum of dy over a sample is
 * exactly 0 (a bias in front of an instance norm has no gradient): dbias is neither read nor
 * written.  With norm == 1 the two means mean(g_z), mean(g_z * z) of sample b stay in
 * ws[B * chunks * 2 * C + b * 2 * C ..) as [2][C] (chunks = sums_chunks, or the library's own
 * count: nirgan_instnorm_ws_elems sizes for it).
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const float* g; int g_hp, g_wp, g_pad, g_fold;
    const float* g2;
    const float* a; int a_hp, a_wp, a_pad;   /* unused (kept for ABI stability): the mask is the sign of z recomputed from y */
    int act; float slope;
    const float* y; const float* mean; const float* rstd; int norm;
    int B, H, W, C;
    float* dy; int d_hp, d_wp, d_pad;     /* dy = NULL (with norm): the two reductions only, their means stay in ws for a consumer that
                                             evaluates dy on the fly (nirgan_wino6_input_dy_norm) */
    float* gsum_out;
    float* dbias;
    float* ws; int64_t ws_elems;
    void* dy_bf16;                        /* optional twin of `dy` (same geometry, bf16), as out_bf16; with norm and dy = NULL only the twin is
                                           * stored (dy = NULL and dy_bf16 = NULL: the two reductions only) */
    int sums_chunks;                      /* > 0 (with norm): the first pass is done -- the producer of the gradient left the partial sums of g_z
                                             and g_z * z in ws as [B][sums_chunks][2][C].  Either nirgan_wino6_output with fuse_gz (the folded
                                             gradient g_a then sits in gsum_out; g / g2 are not read), or a convolution launch with
                                             nirgan_conv_desc.fuse_* (gsum_out NULL: the second pass reads g itself, which then has no fold
                                             and no g2).  ws >= B * sums_chunks * 2 * C + B * 2 * C floats */
    int y_bf16;                           /* 1: y points to bf16 elements (as nirgan_in_fwd_desc.y_bf16) */
    int g_bf16;                           /* 1: g points to bf16 elements (same halo'd geometry): the data-gradient launch that produced it stored
                                           * it with nirgan_conv_desc.out_bf16 (bf16 operand mode; g2 and gsum_out stay fp32) */
} nirgan_in_bwd_desc;

int nirgan_instnorm_bwd(const nirgan_in_bwd_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * Layout / halo helpers at the NCHW boundary.
 * ------------------------------------------------------------------------------------- */
/* dst[b][hh][ww][c0+c] = src[b][c][rh(hh)][rw(ww)], c < Cs.  pad_mode REFLECT: the halo of
 * width pad1+pad2 is the composition reflect(pad1) then reflect(pad2) (Px2Px_PL.forward's
 * F.pad(...,'reflect') model/pix2pix.py:91-93 followed by ReflectionPad2d(3) networks.py:341).
 * pad_mode KEEP: only the interior (offset pad1+pad2) is written (torch.cat + zero padding,
 * model/pix2pix.py:197,202,216 + networks.py:559). */
int nirgan_nchw_to_halo(const float* src, int B, int Cs, int H, int W,
                        float* dst, int dst_cs, int c0, int pad1, int pad2, int pad_mode, void* stream);

/* Data gradient of a Conv2d wrt ONE input channel (the generator step only needs dD/dpred, channel 3 of
 * cat(rgb, pred): model/pix2pix.py:216-221 through networks.py:559):
 *   out[b][h][w] = sum_{kh,kw,co} dY[b][(h+pad-kh)/stride][(w+pad-kw)/stride][co] * W[co][channel][kh][kw]
 * dY is a halo'd NHWC buffer [B][OH+2dy_pad][OW+2dy_pad][C]; W is in the reference layout [C][cin][k][k].  The halo of dY is never read.
 * Two kernels: k == 4, stride == 2, pad == 1, H == 2 OH, W == 2 OW and (16 C + 1600) floats of LDS <= 64 KB (C <= 924) take the
 * output-stationary k4s2 kernel; every other layer the generic one, which needs C % 4 == 0, k <= 7 and k*k*C floats <= 64 KB. */
typedef struct {
    const float* dy; int dy_hp, dy_wp, dy_pad, C;
    const float* w; int cin, k, stride, pad, channel;
    int B, H, W;
    float* out;                           /* [B][H][W] */
} nirgan_chan_dgrad_desc;
int nirgan_conv_channel_dgrad(const nirgan_chan_dgrad_desc* d, void* stream);

/* Single-output-channel convolution tail: out[b][oh][ow] = act(bias + sum_t Q[b][oh+tap_dh[t]][ow+tap_dw[t]][t])
 * restricted to the crop window (crop pixels removed on every side); dst is NCHW [B][1][OH-2crop][OW-2crop].
 * With the 1x1 tap-plane product this is Conv2d(C,1,k) (+Tanh, + crop of pix2pix.py:107-108):
 * model/networks.py:367-368, :579.  Planes t >= ntaps of Q are never added.
 * Two kernels: a full k x k tap list in row-major order (tap t = (t / k, t % k)) on a cropped map of >= 4096 outputs takes the rows
 * kernel (one kernel row of planes in LDS at a time); every other list or map the window kernel, whose all-planes window of
 * (8 + kh - 1) x (32 + kw - 1) records of (q_cs | 1) floats (kh, kw = 1 + the largest dh, dw) must fit 160 KB of LDS. */
typedef struct {
    const float* q; int q_hp, q_wp, q_cs;
    int ntaps; int tap_dh[64], tap_dw[64];
    const float* bias;                    /* 1 float on device, or NULL */
    int act;
    int B, OH, OW, crop;
    float* dst;                           /* [B][OH-2crop][OW-2crop] */
} nirgan_tap_gather_desc;
int nirgan_tap_gather(const nirgan_tap_gather_desc* d, void* stream);

/* Adjoint: dq[b][hh][ww][t] = dz[b][hh-tap_dh[t]][ww-tap_dw[t]], dz = dout*act'(out) inside
 * the crop window and 0 elsewhere; channels t >= ntaps of dq are zeroed; dbias (optional)
 * accumulates sum dz (fp32, fixed order); when the float64 sum of the same terms is exactly
 * 0 (terms of one magnitude and opposite signs: the two halves of a wgangp discriminator
 * batch) nothing is added. */
typedef struct {
    const float* dout; const float* out;  /* [B][OH-2crop][OW-2crop] each; out may be NULL when act == NONE */
    int act;
    int B, OH, OW, crop;
    int ntaps; int tap_dh[64], tap_dw[64];
    float* dq; int q_hp, q_wp, q_cs;
    float* dbias;
} nirgan_tap_scatter_desc;
int nirgan_tap_scatter(const nirgan_tap_scatter_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * The generator's last layer as direct kernels: Conv2d(64, 1, 7) + bias + tanh (+ crop) over the
 * reflect-padded halo'd NHWC input, and its backward (model/networks.py:366-368 -- ReflectionPad2d(3),
 * Conv2d(ngf, output_nc, kernel_size=7, padding=0), Tanh; the crop is model/pix2pix.py:101-110).
 * A wave's 64 lanes are the 64 input channels; C must be 64 and k 7 (other widths keep the
 * tap-plane route above).  Same results as nirgan_conv_igemm + nirgan_tap_gather /
 * nirgan_tap_scatter + nirgan_wgrad_igemm + nirgan_conv_igemm up to fp32 summation order.
 *   forward : out[b][y][x] = act(bias + sum_{ka,kb,c} x[b][y+crop+ka][x+crop+kb][c] * w[ka*7+kb][c])
 *   dz      : zero-bordered image of dout * act'(out) (workspace shared by the two gradients), [B][OH + 12][S] with
 *             S = (OW + 12 + 3) / 4 * 4 + 8: nirgan_endconv_dz_elems = B * (OH + 12) * S; gbias (optional) accumulates sum dz
 *   dgrad   : gx over the whole halo'd grid [B][x_hp][x_wp][64]
 *   wgrad   : gw[c*49 + t] (the Conv2d weight's own [1][64][7][7] layout), overwritten; fixed
 *             summation order (bitwise reproducible)
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const float* x; int x_hp, x_wp;       /* [B][x_hp][x_wp][C], x_hp = OH + k - 1 */
    int B, OH, OW, crop, C, k;
    const float* w;                       /* [k*k][C] tap-major (the tap-plane forward pack) */
    const float* bias; int act;
    float* out;                           /* [B][OH-2crop][OW-2crop] */
    const float* dout;                    /* gradient wrt out */
    float* dz; int64_t dz_elems;          /* >= nirgan_endconv_dz_elems(B, OH, OW) floats, 16-byte aligned */
    float* gx;
    float* gw; float* gbias;
    float* ws; int64_t ws_elems;          /* >= nirgan_endconv_ws_elems(B, OH, OW) floats */
} nirgan_endconv_desc;
int64_t nirgan_endconv_dz_elems(int B, int OH, int OW);
int64_t nirgan_endconv_ws_elems(int B, int OH, int OW);
int nirgan_endconv_fwd(const nirgan_endconv_desc* d, void* stream);
int nirgan_endconv_dz(const nirgan_endconv_desc* d, void* stream);
int nirgan_endconv_dgrad(const nirgan_endconv_desc* d, void* stream);
int nirgan_endconv_wgrad(const nirgan_endconv_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * Losses (forward value + gradient in one pass).
 * ------------------------------------------------------------------------------------- */
/* LSGAN: loss_out[0] += weight * mean((pred - target)^2); grad = weight * 2 (pred-target)/n.
 * GANLoss('lsgan') with MSELoss, model/networks.py:233,258-276.  One workgroup (patch maps are a few 10^4 values): the sum is
 * bitwise reproducible. */
int nirgan_lsgan(const float* pred, int64_t n, float target, float weight,
                 float* loss_out, float* grad, void* stream);

/* The other two objectives of GANLoss (model/networks.py:210-276), value and gradient in one pass like nirgan_lsgan: loss_out[0] is
 * accumulated (one add per launch), grad [n] is overwritten and may be NULL (forward only).  One workgroup; the terms are summed in
 * float64 in a fixed order, so two runs give the same bits.  pred needs no alignment, n >= 1 is any.
 *   NIRGAN_GAN_VANILLA  BCEWithLogitsLoss against the label, x = pred[i], t = target (any float: checkpoints may carry smoothed labels):
 *                       loss_out[0] += weight * mean(max(x, 0) - x t + log1p(exp(-|x|)))
 *                       grad[i]      = weight * (sigmoid(x) - t) * (1.f / (float)n),  sigmoid from exp(-|x|): 1 / (1 + e) for x >= 0,
 *                                      e / (1 + e) below; precise expf / log1pf, no exp of a positive argument
 *   NIRGAN_GAN_WGANGP   s = target > 0.5f ? -1 : +1 (the label only picks the side, as target_is_real does):
 *                       loss_out[0] += weight * s * mean(x)
 *                       grad[i]      = (s * weight) * (1.f / (float)n), both operations in fp32
 * Any other mode (lsgan keeps nirgan_lsgan), n <= 0, a NULL pred or loss_out: NIRGAN_ERR_ARG before any launch.
 * cal_gradient_penalty (networks.py:279-313) is not part of the entry. */
#define NIRGAN_GAN_VANILLA 1
#define NIRGAN_GAN_WGANGP 2
int nirgan_gan_loss(const float* pred, int64_t n, int mode, float target, float weight,
                    float* loss_out, float* grad, void* stream);

/* L1 + spectral-index losses on NCHW tiles (rgb [B][3][H][W], nir/pred [B][1][H][W]).
 *   sums[0..6] += sum|pred-nir|, then the per-index sums of criterion(idx(nir), idx(pred))
 *   for ndvi, ndwi, gndvi, savi, msavi, evi (all divided by n by the caller);
 *   grad_pred = extra_scale*extra[...][extra_c] + w_l1*sign(pred-nir)/n + sum_i w_i * d crit_i / d pred
 * criterion 0 = l1, 1 = l2.  torch.nn.L1Loss model/pix2pix.py:60,222;
 * RemoteSensingIndices utils/remote_sensing_indices.py:23-71,84-319. */
typedef struct {
    const float* rgb;                     /* [B][3][H][W]; NULL = plain L1 on (pred, nir): every index weight 0, log_all 0 */
    const float* nir; const float* pred;
    int B, H, W;
    float w_l1, w_ndvi, w_ndwi, w_gndvi, w_savi, w_msavi, w_evi;  /* already multiplied by lambda_rs */
    int criterion;
    int log_all;                          /* 1: evaluate all six indices (logging_dict); 0: only those with weight != 0 */
    const float* extra; int extra_cs, extra_c; float extra_scale;  /* optional NHWC gradient term */
    float* sums;                          /* 7 floats, accumulated */
    float* grad_pred;                     /* [B][1][H][W] or NULL (forward only) */
    float* ws; int64_t ws_elems;          /* >= NIRGAN_PIX_LOSS_WS_ELEMS floats: per-block partial sums, added up in block order
                                             (no float atomics: the seven sums are bitwise reproducible); not shared between streams */
} nirgan_pix_loss_desc;
#define NIRGAN_PIX_LOSS_WS_ELEMS 8192
int nirgan_pix_loss(const nirgan_pix_loss_desc* d, void* stream);

/* The same losses over the pixels a mask keeps (csrc/losses_masked.hip; the mask of a scene-pool batch is nirgan_scene_valid's, the
 * last section of this header).  Every field up to ws_elems is nirgan_pix_loss_desc's, with the same meaning and the same checks.
 *   valid  float [B][1][H][W], device.  A pixel i takes part iff valid[i] != 0.f (-0.f drops it; any other value, NaN included, keeps it).
 *   count  int32 [1], DEVICE memory, read by the kernel: the divisor of the mean, normally nirgan_valid_count of `valid` -- or of the
 *          mask of a larger batch this call is one part of, whose parts then share one divisor.  Nothing is read back to the host.
 * Per kept pixel the arithmetic is nirgan_pix_loss's, operation for operation, with
 *     inv = count[0] > 0 ? 1.f / (float)count[0] : 0.f        in the place of 1.f / (float)n.
 * A dropped pixel adds nothing to any of the seven sums, and grad_pred there is exactly extra_scale * extra[...][extra_c], or +0.0f
 * without `extra`.  Its rgb, nir and pred are NOT LOADED: NaN, Inf or nodata / divisor at a dropped pixel reach no output.
 * Same grid, same per-block partial sums in `ws`, same fixed-order finish: with valid all ones and count[0] = n the sums and the
 * gradient are BITWISE those of nirgan_pix_loss.  With count[0] <= 0 the sums still accumulate over the kept pixels and the loss
 * part of the gradient is 0.  The caller divides the sums by the count.
 * Everything nirgan_pix_loss refuses, and a NULL valid or count, return NIRGAN_ERR_ARG before any launch. */
typedef struct {
    const float* rgb;
    const float* nir; const float* pred;
    int B, H, W;
    float w_l1, w_ndvi, w_ndwi, w_gndvi, w_savi, w_msavi, w_evi;
    int criterion;
    int log_all;
    const float* extra; int extra_cs, extra_c; float extra_scale;
    float* sums;
    float* grad_pred;
    float* ws; int64_t ws_elems;
    const float* valid;                   /* [B][1][H][W] */
    const int32_t* count;                 /* device [1] */
} nirgan_pix_loss_masked_desc;
int nirgan_pix_loss_masked(const nirgan_pix_loss_masked_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * Per-pixel baseline models, fused (csrc/pixmlp.hip).  rgb [B][3][H][W], nir / pred / dpred [B][1][H][W], fp32 NCHW, contiguous.
 *   hidden = 0   Linear_NIR: y = w . x + b                                    model/baseline_models.py:17-30
 *   hidden = 64  MLP_NIR:    y = W3 . relu(W2 . relu(W1 . x + b1) + b2) + b3   model/baseline_models.py:80-100
 * `params` / `grads` are the network's flat fp32 ranges (state_dict order, every tensor padded to a multiple of 4 floats:
 * 8 floats for hidden = 0, 4484 for hidden = 64), read and written in place.
 *   fwd:   pred = model(rgb).
 *   train: ONE pass over the pixels: prediction (stored when `pred` is set, bitwise the forward entry's), then
 *            loss_out[0] += mean((pred - nir)^2)            (ACCUMULATED, like the sums of the pixel-loss entry: the caller zeroes it)
 *            grads[0..P)  = d mean((pred - nir)^2) / d params   (OVERWRITTEN, padding elements = 0)
 *          (F.mse_loss + backward, baseline_models.py:28, :98).  With `dpred` set (the autograd bridge: an upstream gradient with
 *          respect to the prediction) dy is read from it instead of 2 (pred - nir) / n; nir and loss_out are then not touched.
 *          Persistent workgroups leave one record [P + 4] each in `ws`; a second launch adds the records in workgroup order.  No
 *          float atomics, the grid is a function of the shape only: two runs are bitwise equal.  The grid's cap is a CONSTANT of this
 *          gfx950-only library (hidden = 64: 256 workgroups, one per CU of the MI355X; hidden = 0: 2048), not a device query: the
 *          entries keep no state and the ws_elems query needs no device.  The hidden activations never
 *          reach HBM.  `ws` holds grid x record floats, independent of the pixel count once the tiles outnumber the grid.
 * Any B, H, W >= 1 with B*H*W < 2^31 (partial tiles are predicated).
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const float* rgb;
    const float* nir;                     /* train: the target; NULL with dpred, and for fwd */
    const float* dpred;                   /* train: NULL, or d loss / d pred given from outside */
    int B, H, W;
    int hidden;                           /* 0 or 64; anything else fails with NIRGAN_ERR_ARG */
    const float* params;
    float* grads;                         /* train; NULL for fwd */
    float* pred;                          /* fwd: required; train: optional */
    float* loss_out;                      /* train without dpred: one float, accumulated */
    float* ws; int64_t ws_elems;          /* train: >= the ws_elems query below; not shared between streams */
} nirgan_pixmlp_desc;
#define NIRGAN_PIXMLP_TILE 32             /* pixels per wave tile of the hidden = 64 kernels (hidden = 0: 256 per workgroup) */
int nirgan_pixmlp_fwd(const nirgan_pixmlp_desc* d, void* stream);
int nirgan_pixmlp_train(const nirgan_pixmlp_desc* d, void* stream);
int64_t nirgan_pixmlp_ws_elems(int B, int H, int W, int hidden);

/* ---------------------------------------------------------------------------------------
 * The pixel discriminator (1x1 PatchGAN, model/networks.py:587-616 with norm = 'instance'), fused per pixel (csrc/pixdisc.hip):
 *   z1 = W1 x + b1 (ndf)   h1 = lrelu_0.2(z1)   z2 = W2 h1 (2 ndf)   xh = (z2 - mean_nc) * rstd_nc   out = w3 . lrelu_0.2(xh) + b3
 * with mean / rstd per sample and channel over H*W (biased variance, eps 1e-5, no affine).  fp32 throughout (fp32 MFMA).
 * x [B][H][W][4] = cat(rgb, nir | pred), NHWC without halo, 16-byte aligned; out / dout [B][H][W].
 * `params` / `grads` are the network's flat fp32 ranges (state_dict order net.0.weight, net.0.bias, net.2.weight, net.2.bias,
 * net.5.weight, net.5.bias, every tensor padded to a multiple of 4 floats: 8772 floats).  net.2.bias feeds the InstanceNorm, which
 * removes it exactly: the forward does not read it and its gradient is written as exact zeros.
 *   fwd:  stats[B][2 ndf][2] = (mean of z2 - pivot, rstd), then out.  Two passes over x; z2 is recomputed, never stored.  The pivot of
 *         (sample, channel) is z2 of the sample's first pixel: it is computed again wherever it is needed and enters the matrix
 *         products as their starting value, so no rounding at the size of the mean reaches xh.
 *   bwd:  needs the `stats` the forward of the same x and params left.  Two passes over x and dout:
 *           mode PARAMS  grads[0..8772) = d (sum dout . out) / d params     (OVERWRITTEN, padding elements and net.2.bias = 0)
 *           mode INPUT   gx[B][H][W][4] = d (sum dout . out) / d x           (16-byte aligned)
 *           mode PRED    gx[B][H][W]    = channel 3 of that, bitwise
 * A 32-pixel tile never straddles two samples; the last tile of a sample is predicated.  Statistics are merged as (count, mean, M2)
 * with Chan's formula; every reduction runs in index order over records in `ws` (per (sample, chunk of tiles), per sample, per
 * workgroup), no float atomics, the grid is a function of the shape only (at most 256 workgroups, a CONSTANT of this gfx950-only
 * library): two runs are bitwise equal.
 * ndf == 64 only; B, H, W >= 1 with H*W >= 2 (InstanceNorm needs more than one spatial element) and B*H*W < 2^31.  Argument errors
 * (null pointer, ndf, shape, workspace, mode) return NIRGAN_ERR_ARG before any launch.
 * ------------------------------------------------------------------------------------- */
#define NIRGAN_PIXDISC_PARAMS 0
#define NIRGAN_PIXDISC_INPUT 1
#define NIRGAN_PIXDISC_PRED 2
typedef struct {
    const float* x;
    int B, H, W;
    int ndf;                              /* 64; anything else fails with NIRGAN_ERR_ARG */
    const float* params;
    float* stats;                         /* [B][2 ndf][2]: written by fwd, read by bwd */
    float* out;                           /* fwd */
    const float* dout;                    /* bwd */
    float* grads;                         /* bwd, mode PARAMS */
    float* gx;                            /* bwd, mode INPUT / PRED */
    int mode;                             /* bwd: NIRGAN_PIXDISC_PARAMS / _INPUT / _PRED */
    float* ws; int64_t ws_elems;          /* >= the ws_elems query below; not shared between streams; fwd and bwd may share it */
} nirgan_pixdisc_desc;
#define NIRGAN_PIXDISC_TILE 32            /* pixels per wave tile */
int64_t nirgan_pixdisc_ws_elems(int B, int H, int W, int ndf);      /* 0 for a problem the entries refuse */
int nirgan_pixdisc_fwd(const nirgan_pixdisc_desc* d, void* stream);
int nirgan_pixdisc_bwd(const nirgan_pixdisc_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * Adam (torch.optim.Adam, amsgrad=False, weight_decay=0) on a flat fp32 range.
 * model/pix2pix.py:486-487.  `step` is the 1-based count after increment.
 * ------------------------------------------------------------------------------------- */
int nirgan_adam(float* p, const float* g, float* m, float* v, int64_t n,
                float lr, float beta1, float beta2, float eps, int step, void* stream);

/* -------------------------------------------------------------------------------------
 * Image-quality metrics of the train / validation loop, one pass on the device instead of the
 * reference's `.cpu()` round trip every 10th batch (model/pix2pix.py:183-186, :281):
 * utils/calculate_metrics.py:5-36 = F.l1_loss, F.mse_loss, kornia.metrics.psnr(pred, target, 1.0),
 * kornia.metrics.ssim(pred, target, window_size=5, max_val=1.).mean(); utils/losses.py:11-30 ssim_loss (window 11).
 * means[0] = mean |pred - target|, means[1] = mean (pred - target)^2, means[2] = mean of the SSIM map
 * (Gaussian window `window` x `window`, sigma, reflect border, output size = input size:
 *   ssim = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2) + eps), C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2);
 * PSNR = 10 log10(max_val^2 / means[1]) is left to the caller.  pred/target: `planes` = B*C dense H x W images.
 * ws: nirgan_image_metrics_ws_elems(planes, H, W) floats.  Deterministic (fixed-order partial sums).
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const float* pred; const float* target;
    int planes, H, W;
    int window; float sigma, max_val, eps;   /* kornia: sigma 1.5, eps 1e-12; window odd, <= 11, H, W > window/2 */
    float* ws; int64_t ws_elems;
    float* means;                            /* 3 floats on device */
} nirgan_metrics_desc;

int64_t nirgan_image_metrics_ws_elems(int planes, int H, int W);
int nirgan_image_metrics(const nirgan_metrics_desc* d, void* stream);

/* -------------------------------------------------------------------------------------
 * Per-tile validation metrics: the rows of the reference's results table (validation_utils/get_results_table.py:59-94 and
 * validation_utils/spider_validation_callback.py:28-64, batch size 1 on CPU copies there), ONE device pass for a whole batch.
 * Per tile b, over the evaluation window [y0, y0+ch) x [x0, x0+cw) of the stored images (the reference's
 * crop_center(.., 240), validation_utils/val_utils.py:20-42, by indexing instead of by copying):
 *   rows[b][0] l1    = mean |nir - pred|                      rows[b][1] l2 = mean (nir - pred)^2
 *   rows[b][2] ssim  = mean of the SSIM map of (nir, pred), formula above; the Gaussian filter reflects at the border of the
 *                      WINDOW (kornia pads the crop), pixels outside the window are never read
 *   rows[b][3] psnr  = 10 log10(max_val^2 / l2), +inf where l2 == 0 (kornia.metrics.psnr)
 *   rows[b][4..6]    = mean |idx(pred) - idx(nir)| for NDVI, NDWI, EVI: the 'logging_dict' errors of RemoteSensingIndices with
 *                      criterion l1, formulas and epsilons of the pixel-loss entry above.  rgb == NULL: these three stay untouched
 *   rows[b][7..8]    = mean of nir / of pred over the patch x patch square at (ch/2 - patch/2, cw/2 - patch/2) of the window
 *                      (validation_utils/time_series_validation.py:120-132).  patch == 0: these two stay untouched
 * Every computed column is OVERWRITTEN.  ws: at least the _ws_elems count of floats.  Deterministic: a tile's reduction order depends
 * only on (ch, cw), so its row is bitwise the same alone and inside any batch (fixed-order partial sums, no float atomics).
 * Argument errors (null pointer, window outside the image, ch or cw <= window/2, even window or > 11, patch > ch or cw,
 * workspace too small) return NIRGAN_ERR_ARG before any launch.
 * ------------------------------------------------------------------------------------- */
#define NIRGAN_TILE_METRIC_COLS 9   /* l1, l2, ssim, psnr, l1_ndvi, l1_ndwi, l1_evi, patch_mean_nir, patch_mean_pred */
typedef struct {
    const float* rgb;          /* [B][3][H][W] fp32 NCHW, may be NULL: index columns are then not computed */
    const float* nir;          /* [B][1][H][W] */
    const float* pred;         /* [B][1][H][W] */
    int B, H, W;
    int y0, x0, ch, cw;        /* evaluation window inside each image (crop_center: y0 = (H-ch)/2, x0 = (W-cw)/2) */
    int window; float sigma, max_val, eps;   /* SSIM: odd window <= 11, kornia defaults 1.5 / 1.0 / 1e-12 */
    int patch;                 /* side of the centred patch whose nir / pred means are reported; 0 = none */
    float* ws; int64_t ws_elems;
    float* rows;               /* [B][NIRGAN_TILE_METRIC_COLS] on device, OVERWRITTEN */
} nirgan_tile_metrics_desc;
int64_t nirgan_tile_metrics_ws_elems(int B, int ch, int cw);
int nirgan_tile_metrics(const nirgan_tile_metrics_desc* d, void* stream);

/* -------------------------------------------------------------------------------------
 * Per-tile validation metrics over the VALID pixels of each tile: the rows of nirgan_tile_metrics under a mask.
 * valid: [B][1][H][W] fp32, an element != 0.f is valid (-0.f is not; the convention of nirgan_pix_loss_masked / nirgan_valid_count).
 * Per tile b, over the evaluation window (y0, x0, ch, cw):
 *   rows[b][9]  n_valid = the number of window pixels with valid != 0
 *   rows[b][10] n_ssim  = the number of SUPPORT-CLEAN window pixels: those whose (2r+1)^2 filter taps, r = window/2, reflected at the
 *                         window's border like the filter itself, are all valid (the centre is a tap: n_ssim <= n_valid)
 *   rows[b][0], [1], [4..6]  l1, l2, l1_ndvi, l1_ndwi, l1_evi: sums over the valid pixels times 1.f / n_valid
 *   rows[b][3]  psnr from the masked l2 (+inf where that is 0).  n_valid == 0: these six columns are NaN
 *   rows[b][2]  ssim = sum of the SSIM map over the support-clean pixels times 1.f / n_ssim (there the map has exactly its unmasked
 *               value); n_ssim == 0: NaN
 *   rows[b][7..8]  means of nir / pred over the valid pixels of the centred patch, NaN when the patch holds none
 * rgb == NULL: the index columns stay untouched; patch == 0: the patch columns stay untouched; every other column is OVERWRITTEN.
 * A dropped pixel is branched around, not multiplied by zero: NaN, +-Inf or nodata values in nir / pred / rgb at an invalid pixel reach
 * no output.  Nothing outside the window is read, from any plane, the mask included.  Counts are exact: ch * cw <= 2^24 is required.
 * Under a mask of ones the sums take the path of nirgan_tile_metrics (same operations, same order, 1.f / n_valid == its divisor).
 * ws: at least the _ws_elems count of floats (11 partials per 32x32 block).  Deterministic, no atomics: a tile's row depends only on
 * (ch, cw) and its own planes.  Argument errors: those of nirgan_tile_metrics, valid == NULL and ch * cw > 2^24, NIRGAN_ERR_ARG
 * before any launch.
 * ------------------------------------------------------------------------------------- */
#define NIRGAN_TILE_METRIC_MASKED_COLS 11   /* the nine of NIRGAN_TILE_METRIC_COLS, n_valid, n_ssim */
typedef struct {
    const float* rgb;          /* [B][3][H][W] fp32 NCHW, may be NULL: index columns are then not computed */
    const float* nir;          /* [B][1][H][W] */
    const float* pred;         /* [B][1][H][W] */
    int B, H, W;
    int y0, x0, ch, cw;
    int window; float sigma, max_val, eps;
    int patch;
    float* ws; int64_t ws_elems;
    float* rows;               /* [B][NIRGAN_TILE_METRIC_MASKED_COLS] on device */
    const float* valid;        /* [B][1][H][W] fp32, != 0.f is valid */
} nirgan_tile_metrics_masked_desc;
int64_t nirgan_tile_metrics_masked_ws_elems(int B, int ch, int cw);
int nirgan_tile_metrics_masked(const nirgan_tile_metrics_masked_desc* d, void* stream);

/* -------------------------------------------------------------------------------------
 * Window statistics of a date stack: the numbers of the reference's NDVI time series (validation_utils/time_series_validation.py:
 * centroid patch means :120-132, window medians of the NDVI :243-266; per date on CPU copies there), ONE launch for the whole stack.
 * Per tile t, over the window [y0, y0+wh) x [x0, x0+ww) of the stored images:
 *   rows[t][0], rows[t][1]   mean, median of nir              rows[t][2], rows[t][3]   mean, median of pred
 *   rows[t][4], rows[t][5]   mean, median of ndvi(nir)        rows[t][6], rows[t][7]   mean, median of ndvi(pred)
 * with ndvi(n) = (n - R) / ((n + R) + 1e-6f), R = rgb[t][0] (the association of the pixel-loss entry above).  rgb == NULL: columns
 * 4 to 7 stay untouched.  Every computed column is OVERWRITTEN.
 * Median = torch.median of the flattened window: one of the window's values (exact radix selection on the device, no interpolation),
 * the LOWER of the two middle values of an even count, NaN with a NaN anywhere in the window; the sign of a zero is unspecified.
 * Means are fixed-order partial sums whose association depends only on (wh, ww): a tile's row is bitwise the same alone and inside
 * any stack, and two calls are bitwise equal (no float atomics).  Any T, H, W >= 1 and any window inside the image; no workspace.
 * Argument errors (null nir, pred or rows, window outside the image, non-positive extent) return NIRGAN_ERR_ARG before any launch.
 * ------------------------------------------------------------------------------------- */
#define NIRGAN_WINDOW_STAT_COLS 8   /* mean_nir, median_nir, mean_pred, median_pred, mean_ndvi_nir, median_ndvi_nir, mean_ndvi_pred, median_ndvi_pred */
typedef struct {
    const float* rgb;          /* [T][3][H][W] fp32 NCHW, may be NULL: the NDVI columns are then not computed */
    const float* nir;          /* [T][1][H][W] */
    const float* pred;         /* [T][1][H][W] */
    int T, H, W;
    int y0, x0, wh, ww;        /* the window inside each image */
    float* rows;               /* [T][NIRGAN_WINDOW_STAT_COLS] on device, OVERWRITTEN */
} nirgan_window_stats_desc;
int nirgan_window_stats(const nirgan_window_stats_desc* d, void* stream);

/* -------------------------------------------------------------------------------------
 * Validation figure panels: the numbers and display planes behind the reference's two validation figures (utils/logging_helpers.py:
 * plot_tensors_hist :68-136, plot_index :139-193) and the per-tile parts of its val_stats scalars (model/pix2pix.py:301-309); per image on CPU
 * copies there, ONE entry call for a whole batch here.  Per tile b, with v(x) = clamp(gain * x, 0, 1) in fp32 and the window
 * [y0, y0+ch) x [x0, x0+cw) of the stored images:
 *   hist[b][0][100], hist[b][1][100]   counts of v(nir), v(pred) over the window: bit-exactly np.histogram(v, bins=100, range=(0, 1))[0] on
 *                      float32 input, i.e. the edges are np.linspace(0, 1, 101, dtype=float32), a value goes to the bin i with
 *                      edge[i] <= v < edge[i+1], the last bin is closed at 1 and a NaN is counted nowhere
 *   stats[b][0..2]     min, max, mean of raw nir over the FULL tile;   stats[b][3..5] the same of raw pred
 *   stats[b][6..7]     rgb_lo, rgb_hi: the perc-th and the (100 - perc)-th percentile of all 3*H*W values of the tile's rgb (clamped to
 *                      [0, 1] first when clamp_rgb = 1, raw when 0), as torch.quantile(x.flatten(), q) with linear interpolation:
 *                      pos = q (n - 1) in double on the host, a + t (b - a) on the order statistics of rank floor(pos) and ceil(pos)
 *                      (taken from b's end for t >= 0.5, as torch's lerp), evaluated in double and rounded once.  The order statistics are EXACT (radix selection on the sign-corrected bit
 *                      pattern: no sort, no sampling).  rgb == NULL: these two stay untouched
 *   nir_disp, pred_disp [b][ch][cw]             v(nir), v(pred) over the window
 *   ndvi_nir_disp, ndvi_pred_disp [b][ch][cw]   (clip(ndvi(n), -1, 1) + 1) / 2 with ndvi(n) = (n - R) / ((n + R) + 1e-6f) from RAW values,
 *                      R = rgb[b][0] (the association and IEEE division of the pixel-loss entry above)
 *   rgb_disp [b][ch][cw][3] (channel last)      clamp((c - rgb_lo) / (rgb_hi - rgb_lo), 0, 1), c clamped to [0, 1] first when clamp_rgb = 1;
 *                      0 where rgb_hi == rgb_lo
 * The reference's minmax_percentile lives in data/normalise_s2.py, which it does not ship: the percentile stretch above is THIS project's
 * reading of it.  It is per image, so a tile's output does not depend on its batch neighbours.
 * A NaN anywhere in a tile's nir, pred or rgb gives NaN in that tile's affected columns only (torch.min / max / mean / quantile).
 * Every output pointer may be NULL: that output is not computed.  Every computed output is OVERWRITTEN.  ws: at least _ws_bytes bytes.
 * Deterministic: means are fixed-order partial sums whose association depends only on (H, W), counts are integer atomics (they commute),
 * no float atomics: a tile's every output is bitwise the same alone and inside any batch, and two calls are bitwise equal.
 * Argument errors (null nir or pred, a non-positive extent, a window outside the image, perc outside [0, 50), ndvi_*_disp or rgb_disp without
 * rgb, workspace too small, B*3*H*W >= 2^31) return NIRGAN_ERR_ARG before any launch.
 * ------------------------------------------------------------------------------------- */
#define NIRGAN_PANEL_BINS 100
#define NIRGAN_PANEL_STAT_COLS 8    /* min_nir, max_nir, mean_nir, min_pred, max_pred, mean_pred, rgb_lo, rgb_hi */
typedef struct {
    const float* rgb;          /* [B][3][H][W] fp32 NCHW, may be NULL */
    const float* nir;          /* [B][1][H][W] */
    const float* pred;         /* [B][1][H][W] */
    int B, H, W;
    int y0, x0, ch, cw;        /* the window inside each image */
    float gain;                /* stretch of nir and pred before the histogram and the display (the reference's figure: 1.5f) */
    float perc;                /* percentile of the rgb stretch, in [0, 50) (the reference: 2) */
    int clamp_rgb;             /* 1: rgb is clamped to [0, 1] before the percentiles and the stretch (plot_tensors_hist); 0: raw (plot_index) */
    void* ws; int64_t ws_bytes;
    int32_t* hist;             /* [B][2][NIRGAN_PANEL_BINS] */
    float* stats;              /* [B][NIRGAN_PANEL_STAT_COLS] */
    float* nir_disp;           /* [B][ch][cw] */
    float* pred_disp;          /* [B][ch][cw] */
    float* ndvi_nir_disp;      /* [B][ch][cw], needs rgb */
    float* ndvi_pred_disp;     /* [B][ch][cw], needs rgb */
    float* rgb_disp;           /* [B][ch][cw][3], needs rgb */
} nirgan_val_panel_desc;
int64_t nirgan_val_panel_ws_bytes(int B, int H, int W);
int nirgan_val_panel(const nirgan_val_panel_desc* d, void* stream);

/* -------------------------------------------------------------------------------------
 * Land-cover-stratified validation metrics: the per-tile rows above split by the class id of a mask (the five-class CLC legend of the
 * reference's utils/plot_clc_utils.py / utils/plot_clc_pred.py: 0 none, 1 agricultural, 2 natural vegetation, 3 water, 4 artificial),
 * ONE device pass for a whole batch.  Per tile b and class c < classes, over the pixels of the evaluation window
 * [y0, y0+ch) x [x0, x0+cw) whose mask value equals c:
 *   rows[b][c][0] count  = their number, exact (ch * cw < 2^24), stored as a float
 *   rows[b][c][1] l1     = mean |nir - pred|                  rows[b][c][2] l2 = mean (nir - pred)^2
 *   rows[b][c][3] ssim   = mean over those pixels of the SSIM map of the WHOLE window: the Gaussian filter crosses class borders and
 *                          reflects at the window's border, exactly as in the per-tile entry
 *   rows[b][c][4] psnr   = 10 log10(max_val^2 / l2), +inf where l2 == 0
 *   rows[b][c][5..7]     = mean |idx(pred) - idx(nir)| for NDVI, NDWI, EVI, formulas and epsilons of the per-tile entry.
 *                          rgb == NULL: these three stay untouched
 * count == 0: every other computed column of that row is NaN.  Mask ids >= classes belong to no class.  No pixel outside the window is
 * read, of the images or of the mask.  Every computed column is OVERWRITTEN.  ws: at least the _ws_elems count of floats.
 * Deterministic: counts are added as integers, the float partial sums in a fixed order that depends only on (ch, cw, classes), so a
 * tile's rows are bitwise the same alone and inside any batch and two calls are bitwise equal (no float atomics).
 * Argument errors (everything the per-tile entry rejects, a null mask, classes outside 1..NIRGAN_CLASS_MAX, ch * cw >= 2^24, workspace
 * too small) return NIRGAN_ERR_ARG before any launch.
 * ------------------------------------------------------------------------------------- */
#define NIRGAN_CLASS_MAX 8
#define NIRGAN_CLASS_METRIC_COLS 8   /* count, l1, l2, ssim, psnr, l1_ndvi, l1_ndwi, l1_evi */
typedef struct {
    const float* rgb;            /* [B][3][H][W], may be NULL: index columns untouched */
    const float* nir; const float* pred;   /* [B][1][H][W] */
    const uint8_t* mask;         /* [B][H][W] class ids */
    int B, H, W; int y0, x0, ch, cw;
    int window; float sigma, max_val, eps; /* as nirgan_tile_metrics_desc */
    int classes;                 /* 1..NIRGAN_CLASS_MAX */
    float* ws; int64_t ws_elems;
    float* rows;                 /* [B][classes][NIRGAN_CLASS_METRIC_COLS], OVERWRITTEN */
} nirgan_class_metrics_desc;
int64_t nirgan_class_metrics_ws_elems(int B, int ch, int cw, int classes);
int nirgan_class_metrics(const nirgan_class_metrics_desc* d, void* stream);

/* -------------------------------------------------------------------------------------
 * SSIM term of the generator objective, value AND gradient: model/pix2pix.py:233-237 adds
 * lambda_ssim * ssim_loss(pred, nir); utils/losses.py:10-30: 1 - kornia.metrics.ssim(img1, img2, window_size=11).mean()
 * (Gaussian window sigma 1.5, reflect border, max_val 1, eps 1e-12 in the denominator).
 *   *loss      += weight * (1 - mean SSIM)                (atomic add; NULL = skip)
 *   *value      = 1 - mean SSIM                            (NULL = skip)
 *   grad_pred  += weight * d(1 - mean SSIM) / d pred       (dense [planes][H][W]; NULL = value only)
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const float* pred; const float* target;  /* dense [planes][H][W] */
    int planes, H, W;
    int window; float sigma, max_val, eps;
    float weight;
    float* ws; int64_t ws_elems;             /* nirgan_ssim_loss_ws_elems(planes, H, W, window) floats */
    float* loss; float* value; float* grad_pred;
} nirgan_ssim_loss_desc;

int64_t nirgan_ssim_loss_ws_elems(int planes, int H, int W, int window);
int nirgan_ssim_loss(const nirgan_ssim_loss_desc* d, void* stream);

/* emd_loss of utils/losses.py:64-78, value and gradient wrt pred: mean | cumsum(softmax(pred.reshape(B,-1),1),1) -
 * cumsum(softmax(target.reshape(B,-1),1),1) | over the B*N elements; scans in double (as torch's CPU cumsum accumulates).
 * *loss += weight * emd (atomic; NULL = skip), *value = emd (NULL = skip), grad_pred += weight * d emd / d pred (NULL = value only). */
typedef struct {
    const float* pred; const float* target;  /* dense [B][N] */
    int B; int64_t N;                        /* N = C*H*W < 2^24 */
    float weight;
    void* ws; int64_t ws_bytes;              /* nirgan_emd_loss_ws_bytes(B, N, grad_pred != NULL), 8-byte aligned */
    float* loss; float* value; float* grad_pred;
} nirgan_emd_loss_desc;

int64_t nirgan_emd_loss_ws_bytes(int B, int64_t N, int with_grad);
int nirgan_emd_loss(const nirgan_emd_loss_desc* d, void* stream);

/* -------------------------------------------------------------------------------------
 * SatCLIP location encoder, fp64 like the reference (model/satclip/load_lightweight.py:29,
 * satclip_wrapper.py:30-35; called from model/pix2pix.py:481-484 once per batch):
 * positional_encoding/spherical_harmonics.py:26-42 + spherical_harmonics_closed_form.py:8-40 (real spherical
 * harmonics of degree < L at phi = deg2rad(lon + 180), theta = deg2rad(lat + 90); feature (l, m) at index l*l+l+m),
 * then SirenNet (location_encoder.py:73-151): x <- sin(w0_i * (W_i x + b_i)) for every layer with w0_i != 0,
 * x <- W_i x + b_i where w0_i == 0 (the last layer's Identity).  Evaluation mode (dropout off), forward only.
 * sh_norm[l*l+l+m] = [sqrt 2 if m != 0] * sqrt((2l+1)(l-|m|)!/(4 pi (l+|m|)!)) is supplied by the host.
 * weights[i]: [dims[i+1]][dims[i]] row-major (nn.Linear layout), biases[i] may be NULL; all device pointers,
 * the pointer tables themselves live on the host.  features (optional): [B][L*L] copy of the harmonics.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const double* lonlat; int B;             /* [B][2] = (lon, lat) in degrees */
    int L; const double* sh_norm;            /* legendre_polys; [L*L] on device */
    int nlayers;                             /* linear layers incl. the last one, <= 8 */
    const double* const* weights; const double* const* biases;
    const int* dims;                         /* host: nlayers+1 widths, dims[0] = L*L, each <= 2048 */
    const double* w0;                        /* host: nlayers sine frequencies (30, 1, ..., 0) */
    double* out;                             /* [B][dims[nlayers]] */
    double* features;                        /* optional */
} nirgan_locenc_desc;

int nirgan_location_encoder(const nirgan_locenc_desc* d, void* stream);

/* -------------------------------------------------------------------------------------
 * Histogram matching of predicted tiles to a reference band: create_synthetic_dataset.py:34-47
 * `match_histograms(img_np, ref_np, channel_axis=None)` per tile (scikit-image, float path
 * `_match_cumulative_cdf`): out = interp(cumsum(src_counts)/n, cumsum(tmpl_counts)/n, tmpl_values)[src_lookup]
 * with (values, counts) = unique(...) of each plane.  image/reference/out: [B][N] dense planes of equal size
 * (the script resizes the reference to the tile first).  ws: nirgan_hist_match_ws_bytes(B, N) bytes, 8-byte aligned.
 * Finite inputs (no NaN); -0.0 and +0.0 are one value, as in numpy.  Deterministic.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const float* image; const float* reference;
    int B, N;
    void* ws; int64_t ws_bytes;
    float* out;
} nirgan_hist_match_desc;

int64_t nirgan_hist_match_ws_bytes(int B, int N);
int nirgan_hist_match(const nirgan_hist_match_desc* d, void* stream);

/* Output-gradient side of a Winograd layer's backward (used by nirgan_wino6_dy / nirgan_wino6_input_dy): Yt = A dY A^T per tile. */
typedef struct {
    const float* dy; int dy_hp, dy_wp, dy_pad;   /* halo'd [B][H+2pad][W+2pad][K] */
    int B, H, W, K;
    float* Yt; int64_t Yt_elems;                 /* [planes][tiles][K] */
    int r;                                       /* variant code of the layer (nirgan_wino6_desc.r) */
} nirgan_wino_dy_desc;

/* -------------------------------------------------------------------------------------
 * Winograd F(4x4, 3x3) for the same layers (nn.Conv2d(C, K, 3, stride 1) over a halo of 1, model/networks.py:405-427): 36 products
 * per 4x4 outputs (F(2x2,3x3): 64, direct: 144).  The 16 outputs of a tile do not fit the register file next to the product, so
 * the stages are separate launches and the transform-domain product M goes through HBM once:
 *   nirgan_wino6_input   V[f][t][c] = (B^T d B)[f]   6x6 patches at stride 4 of x; T = B*ceil(H/4)*ceil(W/4) tiles, f = 6 f1 + f2
 *   nirgan_wino6_gemm    M[f][t][k] = sum_c V[f][t][c] U[f][k][c]   36 GEMMs in one grid on the direct 128x128 MFMA tile
 *   nirgan_wino6_output  y[b][4ty+i][4tx+j][k] = (A^T M A)[i][j] + bias[k]
 * Cook-Toom points 0, 1, -1, 2, -1/2, inf (matrices in csrc/wino6.hip); exact fp32 products, the result differs from the direct
 * contraction by fp32 rounding only (measured 4e-6 of the output's maximum).  U = nirgan_wino6_weights(W) is [36][K][C].
 * C % 4 == 0, K % 4 == 0, K > 64; extents that are no multiple of 4 cost one partly used tile row / column.
 * Data gradient: the same calls with x = dY (zero halo 2), transpose_flip weights, H x W = the padded input extent.
 * Weight gradient: dU[f][k][c] = sum_t Yt[f][t][k] V[f][t][c] with Yt = A dY A^T (nirgan_wino6_dy / nirgan_wino6_input_dy) and V of
 * the forward input -- ONE nirgan_wgrad_igemm launch with nplanes = 36 -- then nirgan_wino6_wgrad_finish: dW = G^T (sum of the
 * split slabs, in order) G in the reference layout [K][C][3][3].
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const float* x; int x_hp, x_wp;       /* [B][H+2][W+2][C] */
    int B, H, W, C, K;
    const float* U; const float* bias;    /* [36][K][C]; [K] or NULL */
    float* V; int64_t V_elems;            /* [36][T][C] */
    float* M; int64_t M_elems;            /* [36][T][K] */
    float* y;                             /* dense [B][H][W][K] */
    const float* zero_page;
    int r;                                /* filter size: 0 or 3 = F(4x4,3x3) above; 4 = F(4x4,4x4): nn.Conv2d(C, K, 4, stride 1) of the PatchGAN
                                             (model/networks.py:573-579): x is [B][H+3][W+3][C] for H x W outputs, 7x7 patches, 49 planes in
                                             U / V / M / Yt; Cook-Toom over 0, 1, -1, 2, -2, 1/2, inf; fp32 error 1e-5 of the output's maximum;
                                             6 = F(6x6,3x3): 3x3 filters as above with 6x6 outputs per tile, 8x8 patches at stride 6, 64 planes,
                                             T = B * ceil(H/6) * ceil(W/6) (nirgan_wino6_tiles_r); Cook-Toom over 0, 1, -1, 2, -2, 1/2, -1/2, inf;
                                             fp32 error 1.7e-5 of the output's maximum.  The same code goes into nirgan_wino_dy_desc.r,
                                             nirgan_wino6_weights_r and nirgan_wino6_wgrad_finish_r for the layer */
    float* stats_ws; int64_t stats_ws_elems;   /* optional (nirgan_wino6_output): per-tile partial sums of the output for the instance norm that
                                             follows, [B][tiles per image][4][K] = T * 4 * K floats: {k, sum (o - k), sum (o - k)^2, count} over the
                                             tile's stored outputs o WITHOUT the bias, k = the tile's first output; feed nirgan_instnorm_fwd with
                                             ws = stats_ws, stats_chunks = tiles per image, stats_shift = bias */
    /* optional (nirgan_wino6_output of a DATA GRADIENT over the padded extent, 3x3 filters): the first pass of the instance-norm backward
       of the layer that consumes this gradient, in the same kernel.  H x W here is the padded extent (interior (H-2) x (W-2), reflect halo
       of 1): the tile's outputs are folded onto the interior in registers (adjoint of ReflectionPad2d(1); the far halo line and its
       partner must fall in one tile: (H-3) / m == (H-1) / m for tile size m, same for W), fuse_g2 (optional, dense) is added, the
       result g_a goes to fuse_gz (dense [B][H-2][W-2][K]) INSTEAD of y (which is not written and may be NULL), and the tile's partial sums
       of g_z = g_a * act'(z) and g_z * z, z = (fuse_y - mean) * rstd, go to fuse_part as [B][tiles per image][2][K].  Feed
       nirgan_instnorm_bwd with gsum_out = fuse_gz, ws = fuse_part, sums_chunks = tiles per image. */
    const float* fuse_y; const float* fuse_mean; const float* fuse_rstd; const float* fuse_g2;
    float* fuse_gz; float* fuse_part; int64_t fuse_part_elems; int fuse_act; float fuse_slope;
    int algo;                             /* plane-GEMM kernel choice (nirgan_wino6_gemm, nirgan_wino6_gemm_wgrad_pair) where more than one
                                             applies: 0 = default (persistent workgroups on 32-k stages for C = 256 / 512);
                                             NIRGAN_W6_ONE_TILE = one tile per workgroup (16-k stages); NIRGAN_W6_DIRECT_TILE = the direct
                                             convolution tile (32-k stages, one tile per workgroup); NIRGAN_W6_X3_R4, NIRGAN_W6_PATCH_PER_* as
                                             below.  All compute the same products; kept for A/B measurements and the kernel tests.  Any other
                                             value fails with NIRGAN_ERR_ARG (the transforms check the field too). */
    const void* U3;                       /* optional (precision 3, as nirgan_conv_desc.w_x3): U as three bf16 planes h, m, l, each [planes][K][C],
                                             written by nirgan_wino6_weights_x3 next to U.  With it (and C % 32 == 0, K % 64 == 0) the plane
                                             GEMMs run on the bf16 matrix pipe as six bf16 products per fp32 product, V split inside the
                                             kernel: fp32-equivalent results.  U itself may then be NULL (nirgan_wino6_weights_x3 with U = NULL
                                             writes the planes only: 6 instead of 10 bytes per transformed weight); a launch the split tile
                                             does not take fails without U.  nirgan_wino6_gemm_wgrad_pair then runs its two halves as two
                                             launches (the weight-gradient planes take nirgan_wgrad_desc.precision = 3 on their own). */
} nirgan_wino6_desc;
#define NIRGAN_W6_ONE_TILE 1
#define NIRGAN_W6_DIRECT_TILE 3
#define NIRGAN_W6_X3_R4 5                   /* nirgan_wino6_gemm with U3, K % 128 == 0: the plane GEMMs on the four-wave register-fed split tile (A/B; same bits) */
#define NIRGAN_W6_PATCH_PER_THREAD 16      /* nirgan_wino6_input*: F(6x6,3x3) patches one per thread (A/B; default for the plain / dY transforms: a wave per patch x 32 channels) */
#define NIRGAN_W6_PATCH_PER_LANES 17       /* ... and the lane-spread form also for the normalising variant (default there: one per thread) */
/* names of the kernels the two launchers above pick for a descriptor (what a profile of the launch shows) */
const char* nirgan_wino6_gemm_kernel_name(const nirgan_wino6_desc* d);
const char* nirgan_wino6_pair_kernel_name(const nirgan_wino6_desc* d, const nirgan_wgrad_desc* w);
/* ... and of the kernel a transform stage picks, from the fields its routing reads alone (r, C or K, algo, fuse_gz): pointers, extents and
 * workspace sizes are NOT validated.  "" for a NULL descriptor, an unknown variant, stage or algo, and a stage the variant does not have
 * (the normalising input of F(4x4,4x4); the dY-norm input and the fused output outside F(6x6,3x3), the former also needs C % 32 == 0).
 * nirgan_wino6_dy has one kernel per variant, wino6_dy_kernel<r>. */
#define NIRGAN_W6_STAGE_INPUT 0            /* nirgan_wino6_input and nirgan_wino6_input_dy: the same kernel */
#define NIRGAN_W6_STAGE_INPUT_NORM 1       /* nirgan_wino6_input_norm */
#define NIRGAN_W6_STAGE_INPUT_DY_NORM 2    /* nirgan_wino6_input_dy_norm */
#define NIRGAN_W6_STAGE_OUTPUT 3           /* nirgan_wino6_output: the fused mode where d->fuse_gz is set */
const char* nirgan_wino6_transform_kernel_name(const nirgan_wino6_desc* d, int stage);

int64_t nirgan_wino6_tiles(int B, int H, int W);                   /* T of the 4x4-output variants */
int64_t nirgan_wino6_tiles_r(int B, int H, int W, int r);          /* T of variant r (0 / 3, 4, 6); 0 for an unknown variant */
int nirgan_wino6_weights(const float* w, int K, int C, int transpose_flip, float* U, void* stream);   /* transpose_flip = 0: U of the forward filter, w = [K][C][3][3]; 1: U of the DATA GRADIENT's filter g'[k][c][i][j] = w[c][k][2-i][2-j] with w = [C][K][3][3] the forward weight */
int nirgan_wino6_weights_r(const float* w, int K, int C, int r, int transpose_flip, float* U, void* stream);   /* w = [K][C][r][r], U = [(r+3)^2][K][C] */
/* nirgan_wino6_weights_r that also leaves U as three bf16 planes (nirgan_split3's rule; U3 = 3 x (r+3)^2 x K x C bf16 elements); U may be
 * NULL: the planes only */
int nirgan_wino6_weights_x3(const float* w, int K, int C, int r, int transpose_flip, float* U, void* U3_bf16, void* stream);
/* all weight transforms of a step in one launch: njobs x 8 int64 {w, U, K, C, transpose_flip, first_block, r, U3 (or 0)} in device memory,
 * first_block = running sum of ceil(K*C/256) */
int nirgan_wino6_weights_batch(const int64_t* jobs_device, int njobs, int total_blocks, void* stream);
int nirgan_wino6_input(const nirgan_wino6_desc* d, void* stream);
/* V straight from a convolution's raw output y (dense [B][H][W][C], d->x unused): x = act((y - mean) * rstd) under a REFLECT halo of 1,
 * evaluated on the fly: nirgan_instnorm_fwd with out = NULL (statistics only) then this call replace the apply pass + the transform */
int nirgan_wino6_input_norm(const nirgan_wino6_desc* d, const float* y, const float* mean, const float* rstd, int act, float slope, void* stream);
int nirgan_wino6_gemm(const nirgan_wino6_desc* d, void* stream);
/* the data gradient's plane GEMMs (c: x = dY, transpose_flip weights; its V written by nirgan_wino6_input_dy) and the layer's 36
 * transform-domain weight-gradient problems (w: nplanes = 36) in ONE grid, like nirgan_conv_wgrad_pair: the long weight-gradient
 * blocks first, the GEMM blocks pack behind them.  Semantics = nirgan_wino6_gemm(c) followed by nirgan_wgrad_igemm(w). */
int nirgan_wino6_gemm_wgrad_pair(const nirgan_wino6_desc* c, const nirgan_wgrad_desc* w, void* stream);
int nirgan_wino6_output(const nirgan_wino6_desc* d, void* stream);
int nirgan_wino6_conv3x3(const nirgan_wino6_desc* d, void* stream);   /* input + gemm + output */
/* Yt [(r+3)^2][B*ceil(H/4)*ceil(W/4)][K]; the descriptor's r field selects the filter size (0 / 3 or 4) */
int nirgan_wino6_dy(const nirgan_wino_dy_desc* d, void* stream);
/* nirgan_wino6_input(c) and nirgan_wino6_dy(y) of the SAME output-gradient buffer (c->x == y->dy, zero halo 2) in one pass: the 4x4
 * block of tile (ty, tx) is the lower-right corner of data-gradient patch (ty, tx) */
int nirgan_wino6_input_dy(const nirgan_wino6_desc* c, const nirgan_wino_dy_desc* y, void* stream);
/* the same pass with dY NOT read from memory but evaluated on the fly as the instance-norm backward's result (F(6x6,3x3), C % 32 == 0): n
 * describes the block (g / g2 / gsum_out, y, mean, rstd, act, ws as given to nirgan_instnorm_bwd with dy = NULL, which leaves the two
 * reduction passes' means in ws); every patch element is rstd * (g_z - mean(g_z) - z * mean(g_z * z)), bitwise what the second pass would
 * have stored into c->x -- that buffer is neither written nor read (c->x / y->dy only describe its geometry: zero halo 2) */
int nirgan_wino6_input_dy_norm(const nirgan_wino6_desc* c, const nirgan_wino_dy_desc* y, const nirgan_in_bwd_desc* n, void* stream);
int nirgan_wino6_wgrad_finish(const float* slabs, int nsplit, int K, int C, float* grad, int accumulate, void* stream);
int nirgan_wino6_wgrad_finish_r(const float* slabs, int nsplit, int K, int C, int r, float* grad, int accumulate, void* stream);   /* [K][C][r][r] */
/* the same for n <= 16 layers of one geometry in ONE grid (host arrays of device pointers; every layer then keeps its own slabs until the
 * call): a single layer's finish is launch latency for 33 MB, twelve of them in one launch run at the memory rate */
int nirgan_wino6_wgrad_finish_batch(const float* const* slabs, float* const* grads, int n, int nsplit, int K, int C, int r, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------
 * SatCLIP injection (model/generator_inject.py:110-127).
 * ------------------------------------------------------------------------------------- */
/* F.interpolate(e.view(B,1,S,S), size=(OH,OW), mode='bilinear', align_corners=False) */
int nirgan_bilinear_fwd(const float* src, int B, int SH, int SW, float* dst, int OH, int OW, void* stream);
int nirgan_bilinear_bwd(const float* ddst, int B, int OH, int OW, float* dsrc, int SH, int SW, void* stream);

/* a = relu(z * (1 + s*e)) ('multiply' with the scale parameter, generator_inject.py:124-125), relu(z * e) ('multiply' with
 * scale == NULL, :126-127) or relu(z + s*e) ('add', :122-123; s = 1 when scale == NULL); z dense [B][H][W][C], e [B][H][W],
 * a written to the interior of a halo'd buffer (the halo is left as it is). */
typedef struct {
    const float* z; const float* e; const float* scale;   /* scale: 1 float on device, or NULL: no scale parameter */
    int style;                                            /* 0 multiply, 1 add */
    int B, H, W, C;
    float* out; int o_hp, o_wp, o_pad;
} nirgan_inject_fwd_desc;
int nirgan_inject_fwd(const nirgan_inject_fwd_desc* d, void* stream);

/* backward: g (dense, wrt a) -> dz (dense), de [B][H][W], dscale (1 float, accumulated) */
typedef struct {
    const float* g; const float* a; int a_hp, a_wp, a_pad;
    const float* z; const float* e; const float* scale;
    int style;
    int B, H, W, C;
    float* dz; float* de; float* dscale;
    float* ws; int64_t ws_elems;          /* >= 2048 floats when dscale is set: per-block partial sums of dscale (fixed-order finish) */
} nirgan_inject_bwd_desc;
int nirgan_inject_bwd(const nirgan_inject_bwd_desc* d, void* stream);

/* column sums: out[c] (+)= sum_r x[r][c]  (bias gradients of Linear) */
int nirgan_colsum(const float* x, int64_t rows, int cols, float* out, int accumulate, void* stream);

/* misc stream-ordered helpers */
/* ResnetGenerator_inject's optional post-correction (model/generator_inject.py:97-100,133-134: `x = x * self.post_correction_param`, a
 * learnable 0-dim parameter): out[i] = x[i] * (*param); the parameter is read from device memory (it changes with every optimizer step).
 * Backward: gx[i] = gout[i] * (*param) and *dparam += sum_i gout[i] * x[i] (x = the UNcorrected output; per-block partial sums in ws --
 * at least min(1024, ceil(n / 256)) floats -- added in block order: bitwise reproducible; the caller zeroes dparam first). */
int nirgan_param_scale_fwd(const float* x, const float* param, float* out, int64_t n, void* stream);
int nirgan_param_scale_bwd(const float* gout, const float* x, const float* param, float* gx, float* dparam, float* ws, int64_t ws_elems,
                           int64_t n, void* stream);
int nirgan_fill(float* dst, int64_t n, float value, void* stream);
int nirgan_axpy(float* y, const float* x, int64_t n, float alpha, void* stream);   /* y += alpha*x */

/* ---------------------------------------------------------------------------------------
 * Dropout of the generator's residual blocks (model/networks.py:415-416: nn.Dropout(0.5) behind the first InstanceNorm + ReLU of a
 * ResnetBlock) as a COUNTER-BASED mask: no mask tensor is stored, forward and backward compute the same bits again.
 *
 * Generator: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85) with
 *     key     = (seed_lo, seed_hi)
 *     counter = (q_lo, q_hi, stream_id, call)
 *     q       = (((sample0 + b) * H + h) * W + w) * (C / 4) + c / 4      -- the channel-quad index of the LOGICAL, un-padded tensor, 64 bits
 * The four output words belong to channels 4 (c / 4) + 0 .. 3; an element is kept iff the top bit of its word is 1 (p = 0.5, the only
 * rate the reference can reach), and
 *     out = keep ? 2.0f * x : 0.0f
 * a select, not a product: a dropped NaN or Inf becomes +0; the multiplication by 2 is exact.
 *
 * state: uint32_t[4] = {seed_lo, seed_hi, call, 0} in DEVICE memory, read by the kernels (plans stay static and graph-capturable).
 * The advance entry sets call += 1 on the stream (one thread, a vector store); the forward plan of a network runs it first, and the
 * backward plan reads the call the forward left.
 *
 * The halo entry works IN PLACE on a halo'd NHWC buffer [B][H + 2 pad][W + 2 pad][C]: every element of the padded grid is replaced by
 * the select above with the mask of its REFLECTED SOURCE PIXEL (ReflectionPad2d index rule).  On an activation whose halo is a
 * reflection the result is again the reflection of the masked interior; on a gradient over the padded grid, fold(g * m_pad) =
 * fold(g) * m, so the instance norm's backward with g_fold = 1 that follows needs no change.  pad = 0: a dense tensor.
 * One thread per channel quad (16-byte loads and stores), grid-stride, 64-bit indexing; deterministic, no atomics.
 * Argument errors (null pointer, a non-positive extent, C % 4 != 0, pad < 0, pad >= min(H, W), sample0 < 0, buf not 16-byte aligned,
 * buf_elems below B (H + 2 pad)(W + 2 pad) C, that count at 2^40 or more) return NIRGAN_ERR_ARG before any launch.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    float* buf; int64_t buf_elems;        /* the halo'd buffer and its size in floats */
    int B, H, W, C, pad;
    const uint32_t* state;                /* device: {seed_lo, seed_hi, call, 0} */
    uint32_t stream_id;                   /* which mask of the call: the residual block's index */
    int sample0;                          /* index of this buffer's first sample in the logical batch (micro-batches) */
} nirgan_dropout_desc;
int nirgan_dropout_advance(uint32_t* state, void* stream);
int nirgan_dropout_halo(const nirgan_dropout_desc* d, void* stream);

/* run a pre-built list of descriptors back to back (one host call per phase) */
#define NIRGAN_OP_CONV 1
#define NIRGAN_OP_WGRAD 2
#define NIRGAN_OP_IN_FWD 3
#define NIRGAN_OP_IN_BWD 4
typedef struct { int op; const void* desc; } nirgan_plan_entry;
int nirgan_run_plan(const nirgan_plan_entry* entries, int n, void* stream);

/* ---------------------------------------------------------------------------------------
 * Tiled inference on large scenes (create_synthetic_dataset.py:100-118 runs model(hr) per tile; model/pix2pix.py:91-93,107-108 hides
 * tile-edge artefacts with reflect-pad / crop): scene [B][C][H][W] -> n overlapping tiles [n][C][tile][tile] (tile (b, ti, tj), b-major,
 * covers rows ti*core - margin ..., core = tile - 2*margin, reflected at the scene's borders like F.pad(mode='reflect')), and the
 * tiles' cores back into a scene (pixels past H x W dropped).  One launch per batch of tiles [first, first + n).
 * ------------------------------------------------------------------------------------- */
int64_t nirgan_tile_count(int B, int H, int W, int tile, int margin);      /* B * ceil(H/core) * ceil(W/core) */
int nirgan_tile_gather(const float* scene, int B, int C, int H, int W, int tile, int margin, int first, int n, float* tiles, void* stream);
int nirgan_tile_scatter(const float* tiles, int B, int C, int H, int W, int tile, int margin, int first, int n, float* scene, void* stream);

/* ---------------------------------------------------------------------------------------
 * The same tiling with OVERLAPPING usable regions that are cross-faded (every layer of the generator is followed by an instance norm,
 * so a tile's prediction carries that tile's own per-channel statistics and two neighbours differ by an offset along their border).
 * Per axis, core = tile - 2*margin and stride = core - overlap with 0 <= overlap <= core/2 (no pixel in more than two usable regions
 * per axis; overlap = 0 is the tiling above):
 *   tile i reads scene rows i*stride - margin .. + tile - 1, reflected at the borders (the index rule of the gather above, continued
 *   with period 2*(H-1) for rows more than one reflection away: a scene may be smaller than a tile);
 *   its usable region is scene rows [i*stride, i*stride + core) = tile rows [margin, tile - margin);
 *   tiles per axis: 1 if H <= core, else ceil((H - core) / stride) + 1; numbering b-major, then ti, then tj.
 * Where two usable regions overlap, band position t = 0 .. overlap-1 counts from the LATER tile's first usable row: the later tile
 * weighs r(t), the earlier one 1 - r(t); NIRGAN_BLEND_LINEAR: r = (t + 0.5) / overlap, NIRGAN_BLEND_COSINE:
 * r = 0.5 - 0.5*cos(pi*(t + 0.5) / overlap).  Outside the bands the weight is 1; a pixel's weight for a tile is the product of its row
 * and column weights, at most four tiles cover a pixel, and their weights sum to 1.
 *
 * The gather cuts tiles [first, first + n) out of the scene into tiles [n][C][tile][tile].  The blend adds the usable regions of tiles
 * [first, first + n) ([n][C][tile][tile]) into scene [B][C][H][W]; pixels past H x W are dropped.  The scene needs NO initialisation:
 * for each pixel its lowest-numbered covering tile stores w*v and every later covering tile does acc = fma(w, v, acc) in ascending
 * tile number, one thread per pixel, no atomics.  Launches must come in ascending `first` on one stream and together cover every tile
 * once; the result is then bitwise independent of how the tiles are split into launches.
 * Argument errors (null pointer, overlap outside 0 .. core/2, margin >= tile/2, first / n outside the count, unknown window, a plane
 * of the scene or a tile or the tile count at 2^31 or more) return NIRGAN_ERR_ARG before any launch.
 * ------------------------------------------------------------------------------------- */
#define NIRGAN_BLEND_LINEAR 0
#define NIRGAN_BLEND_COSINE 1
typedef struct {
    int B, C, H, W;                       /* the scene */
    int tile, margin, overlap;
    int window;                           /* NIRGAN_BLEND_LINEAR or NIRGAN_BLEND_COSINE (the gather checks it too) */
    int first, n;                         /* this launch's tiles */
    float* scene;                         /* [B][C][H][W]: read by the gather, accumulated into by the blend */
    float* tiles;                         /* [n][C][tile][tile]: written by the gather, read by the blend */
} nirgan_tile_blend_desc;
int64_t nirgan_tile_count_ov(int B, int H, int W, int tile, int margin, int overlap);      /* 0 for a bad tiling */
int nirgan_tile_gather_ov(const nirgan_tile_blend_desc* d, void* stream);
int nirgan_tile_blend(const nirgan_tile_blend_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * Dihedral test-time augmentation of tiles: the generator's prediction depends on a tile's orientation, so the k = 1, 2, 4 or 8
 * mirrored / transposed views of every tile are predicted, placed back and averaged (self-ensembling over a subgroup of D4).
 * View g (0 <= g < k) of an H x W plane x is built from three bits -- bit 0 mirrors columns, bit 1 mirrors rows, bit 2 transposes:
 *     view_g(x)[i][j] = x[i'][j']   with   (a, b) = (j, i) if bit 2 is set, else (i, j);
 *                                          i' = H-1-a if bit 1 is set, else a;   j' = W-1-b if bit 0 is set, else b.
 * k = 2 is {identity, column mirror}, k = 4 the four flips, k = 8 all of D4 (needs H == W).  Views 0 .. 3 are involutions; so are
 * 4 and 7 (the two diagonal reflections), while 5 and 6 (the quarter turns) are each other's inverse.
 *
 * Expand copies:  src [n][C][H][W] -> dst [n][k][C][H][W],  dst[t][g][c] = view_g(src[t][c]).  A pure permutation, bitwise exact
 * (NaN payloads included).
 * Merge undoes and averages:  src [n][k][C][H][W] -> dst [n][C][H][W],  dst[t][c] = (1/k) * sum over g of v_g with
 * v_g = view_g^-1(src[t][g][c]) (v_g[i'][j'] = src[t][g][c][i][j] in the terms above).  The additions are plain fp32 adds (no fma) in
 * the fixed pairwise tree ((v0+v1)+(v2+v3))+((v4+v5)+(v6+v7)), or its prefix v0, v0+v1, (v0+v1)+(v2+v3) for k = 1, 2, 4, followed by
 * ONE multiply by 1/k (a power of two: exact).  k equal inputs therefore give exactly that value, and merge(expand(x)) == x
 * bitwise for finite x.
 * No atomics; every destination element is written by one thread, so neither dst needs initialisation.  One launch per call.
 * Argument errors (null pointer, views not 1 / 2 / 4 / 8, views == 8 with H != W, a non-positive extent, a plane H*W or the plane
 * count n*views*C at 2^31 or more) return NIRGAN_ERR_ARG before any launch.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    int n, C, H, W;                       /* n images of C planes of H x W */
    int views;                            /* k = 1, 2, 4 or 8; k = 8 needs H == W */
    const float* src;
    float* dst;
} nirgan_tile_views_desc;
int nirgan_tile_views_expand(const nirgan_tile_views_desc* d, void* stream);      /* src [n][C][H][W] -> dst [n][k][C][H][W] */
int nirgan_tile_views_merge(const nirgan_tile_views_desc* d, void* stream);       /* src [n][k][C][H][W] -> dst [n][C][H][W] */

/* ---------------------------------------------------------------------------------------
 * The geo-context join of the validation table (validation_utils/geo_ablation.py:18-53 of the reference: gpd.sjoin of every tile's
 * lon / lat with a country layer, a point query of a Koeppen raster): n_points points against a polygon layer, and against a raster.
 * Planar coordinates, float64 throughout; no antimeridian wrapping, no geodesic edges.
 *
 * The layer: verts [n_verts][2] (x, y); ring r owns vertices ring_start[r] .. ring_start[r+1]-1 (ring_start[0] = 0,
 * ring_start[n_rings] = n_verts) and the closing edge from its last vertex to its first -- a ring that repeats its first vertex at
 * the end is legal too, the zero-length edge never counts; ring_region[r] in 0 .. n_regions-1, NON-DECREASING, names the region
 * (feature) of ring r: holes and the parts of a multipolygon are further rings of the same region.  region_box [n_regions][4] =
 * (xmin, ymin, xmax, ymax) over the region's vertices, (+inf, +inf, -inf, -inf) for a region without vertices:
 * nirgan_region_boxes WRITES it (once per layer), nirgan_point_regions reads it.
 *
 * nirgan_point_regions: region[i] = the LOWEST region index whose rings are crossed an odd number of times in total by the ray from
 * point i towards +x, or -1 (the even-odd rule: a point in a hole is outside; an enclave listed after the country around it is found
 * through that country's hole; where regions overlap the lowest index wins).  An edge (x0,y0) -> (x1,y1) is crossed by (px,py) iff
 *     straddles = (y0 > py) != (y1 > py)
 *     d         = (x1 - x0) * (py - y0) - (px - x0) * (y1 - y0)
 *     crossing  = straddles && (y1 > y0 ? d > 0 : d < 0)
 * with every operation an individually rounded float64 operation (four subtractions, two products, one subtraction; no fused
 * multiply-add, no division): the result is bitwise that statement's, for every point.  A point exactly on an edge (d == 0) does not
 * cross that edge; its membership is whatever follows and is UNSPECIFIED.  Finite vertices are assumed; a point with a NaN gets -1.
 * The parities are combined with integer XOR in a uint32 bitset ws [n_points][ceil(n_regions / 32)] which the entry zeroes itself:
 * the result does not depend on slab_verts (vertices per LDS slab, 0 = the default, at most NIRGAN_GEO_SLAB_MAX; the edge axis is
 * cut at slab boundaries, also across blocks when there are few points), nor on the order of anything.  No float atomics.
 * n_points == 0 or n_regions == 0 returns NIRGAN_OK without a launch (n_regions == 0 leaves `region` untouched: fill it with -1).
 * Argument errors return NIRGAN_ERR_ARG before any launch: a null pointer, a negative count, slab_verts out of range, a workspace
 * below nirgan_point_regions_ws_bytes, and -- where the optional HOST copies ring_start_host / ring_region_host are given (device
 * memory is not read for checks) -- a decreasing ring_region or ring_start, a region id outside the layer, ring_start[0] != 0 or
 * ring_start[n_rings] != n_verts.  Without them a malformed table gives garbage but reads and writes nothing out of range.
 * ------------------------------------------------------------------------------------- */
#define NIRGAN_GEO_SLAB_MAX 2048
typedef struct {
    const double* points;                 /* [n_points][2]; not read by nirgan_region_boxes */
    int n_points;
    int n_verts;
    const double* verts;                  /* [n_verts][2] */
    const int32_t* ring_start;            /* [n_rings + 1] */
    const int32_t* ring_region;           /* [n_rings] */
    int n_rings, n_regions;
    double* region_box;                   /* [n_regions][4] */
    const int32_t* ring_start_host;       /* optional HOST copies of the two tables, checked before any launch */
    const int32_t* ring_region_host;
    int slab_verts;                       /* 0 = the default; 1 .. NIRGAN_GEO_SLAB_MAX */
    uint32_t* ws;                         /* nirgan_point_regions_ws_bytes(n_points, n_regions) bytes, zeroed by the entry */
    int64_t ws_bytes;
    int32_t* region;                      /* [n_points], OVERWRITTEN (unless n_regions == 0) */
} nirgan_point_regions_desc;
int64_t nirgan_point_regions_ws_bytes(int n_points, int n_regions);      /* n_points * ceil(n_regions / 32) * 4; 0 for an empty problem */
int nirgan_region_boxes(const nirgan_point_regions_desc* d, void* stream);
int nirgan_point_regions(const nirgan_point_regions_desc* d, void* stream);

/* value[i] = raster[row][col] with col = floor((x - x0) / dx), row = floor((y - y0) / dy) in float64 (a north-up affine transform,
 * dy may be negative): the cell that CONTAINS the point, no interpolation.  0 outside the raster, for a NaN coordinate, or where the
 * cell equals `nodata` (has_nodata != 0) -- the reference's "Unknown" id.  dx or dy of 0, a NaN in the transform, an empty raster, an
 * unknown dtype, a negative count or a null pointer return NIRGAN_ERR_ARG before any launch; n_points == 0 launches nothing. */
#define NIRGAN_RASTER_U8 0
#define NIRGAN_RASTER_I16 1
#define NIRGAN_RASTER_I32 2
typedef struct {
    const double* points;                 /* [n_points][2] */
    int n_points;
    int H, W, dtype;                      /* NIRGAN_RASTER_* */
    const void* raster;                   /* [H][W] */
    double x0, dx, y0, dy;
    int has_nodata, nodata;
    int32_t* value;                       /* [n_points], OVERWRITTEN */
} nirgan_raster_lookup_desc;
int nirgan_raster_lookup(const nirgan_raster_lookup_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * Training batches from device-resident scenes (data/SR_dataset_RGB.py:24-56 of the reference: a rasterio stack, .astype(float32) /
 * 10000, bands 0..2 = RGB, band 3 = NIR, coords = lon / lat of the centre pixel).  The training set stays in device memory as it is
 * stored; a batch is cut, normalised, mirrored / rotated and georeferenced in one pass, and WHICH windows a batch holds is a pure
 * function of (seed, draw, sample index): Philox4x32-10 as in the dropout section above, no generator state anywhere.
 *
 * The pool: ONE device buffer of uint16_t (NIRGAN_SCENE_U16) or float (NIRGAN_SCENE_F32) elements holding S scenes, scene s planar
 * [C][H_s][W_s] from element table[s][0].  Nothing is aligned: offsets, widths and windows are arbitrary, every load is one element.
 * table: int64 [S][NIRGAN_SCENE_TABLE_COLS] =
 *     { element offset of the scene, H_s, W_s, cum_windows, element offset of the scene's invalid-prefix table in `prefix` or -1 }
 * cum_windows[s] = sum over scenes 0 .. s of (H-T+1)*(W-T+1), a scene smaller than the tile T in either extent adding 0: the table
 * belongs to one tile size.  table_host is the same table in HOST memory: every check reads it, device memory is not read for checks.
 * geo: double [S][4] = (lon0, dlon, lat0, dlat), the outer corner of pixel [0][0] and the per-pixel steps of an axis-aligned
 * EPSG:4326 grid; NULL = no coords are produced (coords is then not touched).
 *
 * nirgan_scene_invalid_prefix, for ONE scene: prefix [(H+1)][(W+1)] int32,
 *     prefix[y][x] = number of invalid pixels (r, c) with r < y and c < x          (first row and first column 0)
 * a pixel being invalid iff any of its four selected planes band[0..3] equals `nodata` (uint16 pool; compared as integers) or is NaN
 * (float pool; nodata is ignored).  Integer arithmetic: exact, independent of any order.  Two launches, no atomics: a scan along
 * every row (one wave per row, 64 pixels per step with a carry), then a running sum down every column in place.
 * Argument errors (null pointer, unknown dtype, non-positive extent, (H+1)*(W+1) at 2^31 or more, a band outside 0 .. C-1, the scene
 * outside the pool, nodata outside 0 .. 65535 for a uint16 pool) return NIRGAN_ERR_ARG before any launch.
 *
 * nirgan_scene_sample: TWO launches on the stream, no host synchronisation, no atomics.
 *   Draw, one thread per sample b = 0 .. B-1.  Attempt a = 0 .. NIRGAN_SCENE_ATTEMPTS-1:
 *     (w0, w1, w2, w3) = Philox4x32-10(key = (seed_lo, seed_hi), counter = (draw_lo, draw_hi, sample0 + b mod 2^32, a))
 *     u    = w0 | w1 << 32;   idx = floor(u * total / 2^64)   with total = cum_windows[S-1]     (the high word of the 128-bit product)
 *     s    = the first scene with cum_windows[s] > idx;   r = idx - cum_windows[s-1] (0 for s = 0);   nx = W_s - T + 1
 *     y0   = r / nx;   x0 = r % nx;   view = w2 & (views - 1)
 *     n    = P[y0+T][x0+T] - P[y0][x0+T] - P[y0+T][x0] + P[y0][x0]   with P the scene's prefix table; 0 where the scene has none
 *            (table[s][4] < 0) or prefix is NULL
 *   The first attempt with n <= max_invalid is taken; if none is, the LAST attempt is taken and `exhausted` is set.
 *     window[b] = { s, y0, x0, view | a << 8 | exhausted << 31 }
 *     coords[b] = { (float)(lon0 + ((x0 + T/2) + 0.5) * dlon), (float)(lat0 + ((y0 + T/2) + 0.5) * dlat) }
 *   T/2 an integer division; the sum in the parentheses is exact; then ONE float64 product and ONE float64 sum, each rounded on its
 *   own (no fused multiply-add), then one conversion to float: the centre of the centre pixel (SR_dataset_RGB.py:32).
 *   Gather:  out[b][ch][i][j] = (float)src_s[band[ch]][y0 + i'][x0 + j'] / divisor      (one correctly rounded float32 division)
 *   with (i', j') from (i, j) by the view rule of nirgan_tile_views_expand on the T x T window (bit 0 mirrors columns, bit 1 mirrors
 *   rows, bit 2 transposes); ch 0..2 go to rgb [B][3][T][T], ch 3 to nir [B][1][T][T].  A float pool takes the same path with the
 *   value as it is.  Every output element is written by one thread; the outputs need no initialisation.
 * Argument errors return NIRGAN_ERR_ARG before any launch: a null pointer (d, pool, table, table_host, rgb, nir, window); unknown
 * dtype; S or C non-positive, C < 4; views not 1, 4 or 8; a band outside 0 .. C-1; B, T or B*T*T non-positive or at 2^31 or more;
 * divisor == 0 or NaN; max_invalid < 0; a table row with a negative offset, an extent outside 1 .. 2^31-1, a scene outside the pool,
 * a cum_windows that is not the running sum for this T, a prefix offset without `prefix` or a prefix table outside prefix_elems; no
 * scene holding a window (total == 0); total at 2^62 or more.
 * ------------------------------------------------------------------------------------- */
#define NIRGAN_SCENE_ATTEMPTS 8
#define NIRGAN_SCENE_TABLE_COLS 5
#define NIRGAN_SCENE_U16 0
#define NIRGAN_SCENE_F32 1
typedef struct {
    const void* pool; int64_t pool_elems; /* the whole pool and its size in elements */
    int dtype;                            /* NIRGAN_SCENE_U16 or NIRGAN_SCENE_F32 */
    int64_t offset;                       /* element offset of the scene */
    int C, H, W;
    int band[4];
    int nodata;                           /* uint16 pool: 0 .. 65535 */
    int32_t* prefix;                      /* [(H+1)][(W+1)], OVERWRITTEN */
} nirgan_scene_prefix_desc;
typedef struct {
    const void* pool; int64_t pool_elems;
    int dtype;
    int S, C;
    const int64_t* table;                 /* device [S][NIRGAN_SCENE_TABLE_COLS] */
    const int64_t* table_host;            /* the same table in HOST memory */
    const int32_t* prefix; int64_t prefix_elems;   /* device: the scenes' invalid-prefix tables, or NULL */
    const double* geo;                    /* device [S][4], or NULL */
    int band[4];                          /* source planes of R, G, B, NIR */
    int tile, B, views;                   /* views: 1, 4 or 8 */
    float divisor;
    uint32_t seed_lo, seed_hi;
    uint64_t draw;
    uint32_t sample0;                     /* index of this call's first sample in the logical batch (ranks, micro-batches) */
    int max_invalid;
    float* rgb;                           /* [B][3][T][T] */
    float* nir;                           /* [B][1][T][T] */
    float* coords;                        /* [B][2], or NULL */
    int32_t* window;                      /* [B][4] */
} nirgan_scene_sample_desc;
int nirgan_scene_invalid_prefix(const nirgan_scene_prefix_desc* d, void* stream);
int nirgan_scene_sample(const nirgan_scene_sample_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * Multi-scale training batches from device-resident scenes (README.md:54 of the reference: "In order to make the model
 * scale-agnostic, we randomly sample a derivative resolution from the datasets"; its datamodule is not part of the reference, so the
 * behaviour is fixed HERE).  nirgan_scene_sample_scaled is nirgan_scene_sample with one more decision per sample: a resolution
 * factor f out of K given ones.  The sample is a window of side L = f * T of the source, delivered as the T x T tile of the means of
 * its f x f blocks -- the sensor's degradation for an integer factor, a box filter and nothing else.
 *
 * Pool, prefix, geo, band, views, divisor, seed, draw, sample0, rgb, nir, coords: as in nirgan_scene_sample_desc.
 * factor[0 .. K-1]: strictly increasing, each in 1 .. NIRGAN_SCENE_MAX_FACTOR; weight[k] > 0 the integer weight of factor[k],
 * Wtot = sum of the weights < 2^32; entries from K on are ignored.
 * table / table_host: int64 [K][S][NIRGAN_SCENE_TABLE_COLS]; table k is EXACTLY the table nirgan_scene_sample wants for the tile side
 * L_k = factor[k] * tile (same format; cum_windows the running sum for L_k), and is checked as that entry checks its own.
 *
 * TWO launches on the stream, no host synchronisation, no atomics.
 *   Draw, one thread per sample b = 0 .. B-1.  With (v0, v1, v2, v3) = Philox4x32-10(key = (seed_lo, seed_hi), counter = (draw_lo,
 *   draw_hi, sample0 + b mod 2^32, 0)), the call of attempt 0:
 *     k    = the first k with weight[0] + .. + weight[k] > floor(v3 * Wtot / 2^32);   f = factor[k];   L = f * T
 *   The scale is drawn ONCE per sample, from a word nirgan_scene_sample does not use: rejected attempts cannot move the mix of
 *   scales towards those that reject less.  Then attempts a = 0 .. NIRGAN_SCENE_ATTEMPTS-1 run as in nirgan_scene_sample on table k
 *   with T replaced by L (attempt 0 on the words above): u, idx with total = cum_windows_k[S-1], s, r, nx = W_s - L + 1, y0, x0,
 *   view, and n the prefix-table count of the L x L window.  A window is accepted iff n <= (int64)max_invalid * f * f: max_invalid
 *   counts invalid SOURCE pixels per output pixel's worth of area, the same invalid fraction at every scale.
 *     window[b] = { s, y0, x0, view | a << 8 | (f - 1) << 16 | exhausted << 31 }          y0, x0 in SOURCE pixels
 *     coords[b] = { (float)(lon0 + ((x0 + L/2) + 0.5) * dlon), (float)(lat0 + ((y0 + L/2) + 0.5) * dlat) }
 *   L/2 an integer division, then ONE float64 product and ONE float64 sum, not fused, as there.
 *   Gather:  D[ch][p][q] = the mean of src_s[band[ch]][y0 + p*f + rr][x0 + q*f + e], rr, e = 0 .. f-1:
 *     uint16 pool:  S = the exact integer sum (at most 64 * 65535 < 2^24);   m = (float)S / (float)(f*f)     (one rounded division)
 *     float pool:   S = a float64 sum, the f*f values added one after another in row-major order of the block (rr outer, e inner),
 *                   starting from the first value;   m = (float)(S / (double)(f*f));   NaN propagates
 *     out[b][ch][i][j] = D[ch][i'][j'] / divisor                                           (one correctly rounded float32 division)
 *   with (i', j') from (i, j) by the view rule of nirgan_tile_views_expand on the T x T tile.  A nodata value inside an accepted
 *   window is averaged like any other value: rejection bounds how many there are, nothing masks them.
 *   For f = 1 every step is nirgan_scene_sample's arithmetic: with factor = {1} the window words, coords and pixels are bitwise its.
 * Argument errors return NIRGAN_ERR_ARG before any launch: everything nirgan_scene_sample refuses, each table against its own L_k;
 * K outside 1 .. NIRGAN_SCENE_MAX_SCALES; a factor outside 1 .. NIRGAN_SCENE_MAX_FACTOR or not above the one before it; a weight of
 * 0; Wtot at 2^32 or more; L_k * L_k at 2^31 or more; a scale of which no scene holds a window (the message names the factor).
 * ------------------------------------------------------------------------------------- */
#define NIRGAN_SCENE_MAX_SCALES 8
#define NIRGAN_SCENE_MAX_FACTOR 8
typedef struct {
    const void* pool; int64_t pool_elems;
    int dtype;
    int S, C;
    const int64_t* table;                 /* device [K][S][NIRGAN_SCENE_TABLE_COLS] */
    const int64_t* table_host;            /* the same tables in HOST memory */
    const int32_t* prefix; int64_t prefix_elems;
    const double* geo;
    int band[4];
    int tile, B, views;                   /* tile: the side T of the DELIVERED tile */
    float divisor;
    uint32_t seed_lo, seed_hi;
    uint64_t draw;
    uint32_t sample0;
    int max_invalid;                      /* invalid source pixels allowed per f x f block's worth of window area */
    float* rgb;                           /* [B][3][T][T] */
    float* nir;                           /* [B][1][T][T] */
    float* coords;                        /* [B][2], or NULL */
    int32_t* window;                      /* [B][4] */
    int K;                                /* 1 .. NIRGAN_SCENE_MAX_SCALES */
    int factor[8];
    uint32_t weight[8];
} nirgan_scene_scaled_desc;
int nirgan_scene_sample_scaled(const nirgan_scene_scaled_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * An explicit list of windows cut from device-resident scenes: the gather of the two samplers above without their draw.  It serves
 * fixed validation sets (a grid of windows cut the same way at every epoch) and gives back the tiles behind a batch: the `window`
 * rows a sampler wrote can be fed in as they are.
 *
 * Pool, geo, band, divisor, rgb, nir, coords: as in nirgan_scene_sample_desc.
 * table / table_host: int64 [S][NIRGAN_SCENE_TABLE_COLS] in the format of nirgan_scene_sample; columns 0 .. 2 (offset, H_s, W_s) are
 * read, columns 3 and 4 (cum_windows, prefix offset) are IGNORED: the table of any tile size will do, nothing is drawn or rejected.
 * window / window_host: int32 [n_windows][4], on the device and the same words in HOST memory; every check reads the host copy.
 *   row = { s, y0, x0, word }     view = word & 7;   f = ((word >> 16) & 7) + 1;   L = f * T;   y0, x0 in SOURCE pixels
 * exactly what the two samplers write.  Bits 8 .. 15 (attempt) and bit 31 (exhausted) of the word are ignored; any other set bit is
 * an argument error.  One call cuts rows first .. first + n - 1; sample i of the call is row first + i.
 *
 * At most TWO launches on the stream (the coords, if asked for; the pixels), no host synchronisation, no atomics.
 *   coords[i] = { (float)(lon0 + ((x0 + L/2) + 0.5) * dlon), (float)(lat0 + ((y0 + L/2) + 0.5) * dlat) }
 *   L/2 an integer division, then ONE float64 product and ONE float64 sum, not fused, as in nirgan_scene_sample; written only when
 *   both geo and coords are set.
 *   Pixels: the Gather of nirgan_scene_sample_scaled, word for word.  D[ch][p][q] = the mean of src_s[band[ch]][y0 + p*f + rr][x0 +
 *   q*f + e], rr, e = 0 .. f-1: a uint16 pool the exact integer sum and one rounded float32 division by f*f, a float pool the float64
 *   sum in row-major order of the block from its first value and one rounded float64 division by f*f, converted to float; then
 *     out[i][ch][j1][j2] = D[ch][j1'][j2'] / divisor                                       (one correctly rounded float32 division)
 *   with (j1', j2') by the view rule of nirgan_tile_views_expand on the T x T tile; ch 0..2 go to rgb [n][3][T][T], ch 3 to nir
 *   [n][1][T][T].  For f = 1 this is nirgan_scene_sample's arithmetic.  The result is therefore BITWISE what either sampler
 *   delivered for the same row.  A call may mix factors and views freely; the kernel (factors to 4, or to 8) is picked from the
 *   largest factor among the call's rows, read from window_host.  Every output element is written by one thread, the outputs need
 *   no initialisation, nothing outside them is written.
 * Argument errors return NIRGAN_ERR_ARG before any launch: a null pointer (d, pool, table, table_host, window, window_host, rgb,
 * nir); unknown dtype; S <= 0 or C < 4; a band outside 0 .. C-1; tile, n or n*tile*tile outside 1 .. 2^31-1; first < 0 or first + n >
 * n_windows; divisor == 0 or NaN; a table row with an extent outside 1 .. 2^31-1 or a scene outside the pool; a row in [first,
 * first + n) with s outside 0 .. S-1, with (f*T)^2 at 2^31 or more, with y0 < 0, x0 < 0, y0 + L > H_s or x0 + L > W_s, or with a stray
 * bit in its word (the message names the row).
 * ------------------------------------------------------------------------------------- */
typedef struct {
    const void* pool; int64_t pool_elems;
    int dtype;                            /* NIRGAN_SCENE_U16 or NIRGAN_SCENE_F32 */
    int S, C;
    const int64_t* table;                 /* device [S][NIRGAN_SCENE_TABLE_COLS]; columns 0..2 (offset, H, W) are read, 3 and 4 are ignored */
    const int64_t* table_host;            /* the same table in HOST memory: every check reads it */
    const double* geo;                    /* device [S][4] or NULL */
    int band[4];
    int tile;                             /* side T of the DELIVERED tile */
    float divisor;
    const int32_t* window;                /* device [n_windows][4] */
    const int32_t* window_host;           /* the same words in HOST memory: every check reads them */
    int64_t n_windows;
    int64_t first; int n;                 /* this launch cuts windows [first, first + n) */
    float* rgb;                           /* [n][3][T][T] */
    float* nir;                           /* [n][1][T][T] */
    float* coords;                        /* [n][2], or NULL */
} nirgan_scene_gather_desc;
int nirgan_scene_gather(const nirgan_scene_gather_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * Training batches from the part of a pool that is NOT held out: nirgan_scene_sample_scaled with the window drawn from a table of
 * rectangles of admissible window ORIGINS instead of from whole scenes.  What the draw can name is what the table lists, so a
 * sample never touches a region the caller left out of the table -- also a sample that runs out of its nodata attempts, which
 * rejection alone could not promise -- and the draw stays exactly uniform over the windows the table lists.
 *
 * pool, pool_elems, dtype, S, C, prefix, prefix_elems, geo, band, tile, B, views, divisor, seed, draw, sample0, max_invalid, rgb,
 * nir, coords, window, K, factor[8], weight[8]: as in nirgan_scene_scaled_desc, with one exception:
 * table / table_host: ONE int64 [S][NIRGAN_SCENE_TABLE_COLS] table in the format of nirgan_scene_sample.  Columns 0, 1, 2 and 4
 * (offset, H_s, W_s, prefix offset) are read; column 3 (cum_windows) is IGNORED, as nirgan_scene_gather ignores it: the table of any
 * tile size will do.
 * origins / origins_host: int64 [R][NIRGAN_SCENE_ORIGIN_COLS] on the device and the same rows in HOST memory (every check reads the
 * host copy, device memory is not read for checks):
 *     row = { scene, oy, ox, oh, ow, cum }
 * the windows of side L_k = factor[k] * tile of `scene` whose origin (y0, x0) lies in [oy, oy + oh) x [ox, ox + ow).  Scale k owns
 * the rows first[k] .. first[k] + count[k] - 1; the scales tile [0, R) in order of k.  cum is the running sum of oh * ow over the
 * rows of ONE scale: it RESTARTS at every scale, total_k = cum of the last row of scale k.  With one row { s, 0, 0, H_s - L_k + 1,
 * W_s - L_k + 1, . } per scene that holds a window (scenes too small for L_k left out) the entry is arithmetically
 * nirgan_scene_sample_scaled, bitwise in rgb, nir, coords and window; with factor = {1} it is nirgan_scene_sample.
 * Rectangles that OVERLAP are not refused and not looked for: a window under several rectangles is simply drawn that many times as
 * often.  nirgan_hip.data builds disjoint ones.
 *
 * TWO launches on the stream, no host synchronisation, no atomics.
 *   Draw, one thread per sample b.  The scale k is picked exactly as nirgan_scene_sample_scaled picks it (word 3 of attempt 0, once
 *   per sample);  f = factor[k];  L = f * T.  Attempt a = 0 .. NIRGAN_SCENE_ATTEMPTS-1, on the words (w0, w1, w2, w3) of that entry:
 *     u    = w0 | w1 << 32;   idx = floor(u * total_k / 2^64)
 *     i    = the first row of scale k with cum > idx;   r = idx - cum[i-1], cum[i-1] being 0 for the FIRST row of the scale (not the
 *            last cum of scale k-1)
 *     s    = scene_i;   y0 = oy_i + r / ow_i;   x0 = ox_i + r % ow_i;   view = w2 & (views - 1)
 *     n    = the prefix-table count of the L x L window at (y0, x0) of scene s; 0 where the scene has no table or prefix is NULL
 *   accepted iff n <= (int64)max_invalid * f * f; if no attempt is, the LAST one is taken and `exhausted` is set.
 *     window[b] = { s, y0, x0, view | a << 8 | (f - 1) << 16 | exhausted << 31 }          y0, x0 in SOURCE pixels of the scene
 *     coords[b] = { (float)(lon0 + ((x0 + L/2) + 0.5) * dlon), (float)(lat0 + ((y0 + L/2) + 0.5) * dlat) }      as there
 *   Gather: the Gather of nirgan_scene_sample_scaled, the same kernel, on the rows the draw wrote: nirgan_scene_gather replays a
 *   batch bitwise from its window rows.
 * Argument errors return NIRGAN_ERR_ARG before any launch: everything nirgan_scene_sample_scaled refuses that still applies (a null
 * pointer -- also origins, origins_host --, dtype, S, C, views, band, B, tile, divisor, max_invalid, negative pool_elems or
 * prefix_elems, K, factor, weight, Wtot, L_k * L_k at 2^31 or more, a table row with an extent outside 1 .. 2^31-1, a scene outside
 * the pool, a prefix offset without `prefix` or a prefix table outside prefix_elems); R < 1; a count[k] < 1 (the message names the
 * factor); first / count not tiling [0, R) in order of k; a row with scene outside 0 .. S-1, oh < 1 or ow < 1, oy < 0 or ox < 0,
 * oy + oh > H_s - L_k + 1 or ox + ow > W_s - L_k + 1, or a cum that is not the running sum of its scale (the message names the row);
 * a total_k at 2^62 or more.  These checks are what keeps every window inside its scene.
 * ------------------------------------------------------------------------------------- */
#define NIRGAN_SCENE_ORIGIN_COLS 6
typedef struct {
    const void* pool; int64_t pool_elems;
    int dtype;
    int S, C;
    const int64_t* table;                 /* device [S][NIRGAN_SCENE_TABLE_COLS]; columns 0, 1, 2, 4 are read, 3 is ignored */
    const int64_t* table_host;            /* the same table in HOST memory */
    const int32_t* prefix; int64_t prefix_elems;
    const double* geo;
    int band[4];
    int tile, B, views;                   /* tile: the side T of the DELIVERED tile */
    float divisor;
    uint32_t seed_lo, seed_hi;
    uint64_t draw;
    uint32_t sample0;
    int max_invalid;                      /* invalid source pixels allowed per f x f block's worth of window area */
    float* rgb;                           /* [B][3][T][T] */
    float* nir;                           /* [B][1][T][T] */
    float* coords;                        /* [B][2], or NULL */
    int32_t* window;                      /* [B][4] */
    int K;                                /* 1 .. NIRGAN_SCENE_MAX_SCALES */
    int factor[8];
    uint32_t weight[8];
    const int64_t* origins;               /* device [R][NIRGAN_SCENE_ORIGIN_COLS] = { scene, oy, ox, oh, ow, cum } */
    const int64_t* origins_host;          /* the same rows in HOST memory: every check reads them */
    int R;                                /* rows of all scales together */
    int first[8], count[8];               /* scale k owns rows first[k] .. first[k] + count[k] - 1 */
} nirgan_scene_origins_desc;
int nirgan_scene_sample_origins(const nirgan_scene_origins_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * Predicting the NIR band of ONE device-resident scene in place: the scene stays as it is stored (uint16 reflectance or float32,
 * planar [C][H][W], C >= 3, nothing aligned), the three entries below stand around the generator and nirgan_tile_blend:
 *   counts   which tiles hold nothing but nodata (they are skipped: the generator never sees them),
 *   gather   the listed tiles, cut and normalised on the way, plus each tile's lon / lat,
 *   finish   the blended float scene -> the stored band (uint16 / float16 / float32), nodata pixels marked.
 * One descriptor serves all three; every entry checks the COMMON fields and its OWN, and reads nothing else.
 *
 * Geometry: exactly that of nirgan_tile_count_ov with B = 1.  core = tile - 2*margin, stride = core - overlap, 0 <= overlap <= core/2,
 * nth / ntw tiles per axis (1 if H <= core, else ceil((H - core)/stride) + 1), nt = nth*ntw tiles numbered t = ti*ntw + tj.  Tile
 * (ti, tj) reads scene rows ti*stride - margin .. + tile - 1 (columns alike), reflected with period 2*(H-1) as nirgan_tile_gather_ov
 * reflects; its usable region is rows [ti*stride, ti*stride + core) x columns [tj*stride, tj*stride + core), clipped to the scene:
 * hy = min(core, H - ti*stride) rows, wx = min(core, W - tj*stride) columns (both >= 1).
 *
 * Validity: with has_nodata set, a pixel is INVALID iff any of the planes band[0..2] equals `nodata` there (NIRGAN_SCENE_U16) or is
 * NaN (NIRGAN_SCENE_F32; `nodata` is not read).  With has_nodata == 0 no pixel is invalid.
 *
 * nirgan_scene_tile_invalid   counts[t] = the number of invalid pixels in the clipped usable region of tile t, for all nt tiles.
 *   One launch, one workgroup per tile (grid-strided), lanes along x; integer sums through a wave reduction and LDS: exact and
 *   independent of scheduling.  A tile can be skipped iff counts[t] == hy*wx.
 * nirgan_scene_tile_gather    tiles[k][c][y][x] = (float)scene[band[c]][r(ti*stride - margin + y)][r(tj*stride - margin + x)] / divisor
 *   for the tile t = ids[k], k = 0 .. n-1: ONE correctly rounded float32 division, so the tile is BITWISE what
 *   nirgan_tile_gather_ov cuts from the host-converted float scene a[band].astype(float32) / float32(divisor).  Nodata pixels enter as
 *   nodata / divisor.  ids / ids_host: int32 [n] on the device and the same words in HOST memory; every check reads the host copy:
 *   strictly ascending, inside 0 .. nt-1.  tile % 4 == 0 and `tiles` 16-byte aligned: a thread stores four pixels at once.
 *   With geo AND coords set the same launch writes
 *     coords[k] = { (float)(lon0 + cx*dlon), (float)(lat0 + cy*dlat) },   cx = tj*stride + wx/2 + 0.5,   cy = ti*stride + hy/2 + 0.5
 *   (integer divisions; then ONE rounded float64 product and ONE rounded float64 sum per axis, not fused, as in nirgan_scene_sample):
 *   the centre of the tile's clipped usable region.  geo = device { lon0, dlon, lat0, dlat }.  One launch.
 * nirgan_scene_finish         out[y][x] from v = blended[y][x] and the scene.  An invalid pixel (the rule above, recomputed from the
 *   three planes) gets nodata_out.  Otherwise
 *     NIRGAN_SCENE_OUT_U16   t = v * scale (one rounded float32 product); t NaN -> nodata_out; else q = rint(t) (ties to even) clamped to
 *                            0 .. 65535; q == nodata_out moves to nodata_out + 1, or to 65534 where nodata_out is 65535: a valid
 *                            pixel is never read as nodata.  nodata_out must be an integer in 0 .. 65535.
 *     NIRGAN_SCENE_OUT_F16   v rounded to binary16 (nearest even); nodata_out is rounded the same way.
 *     NIRGAN_SCENE_OUT_F32   v; nodata_out as it is (any float, NaN included).
 *   One launch; a thread owns four consecutive pixels (vector loads and stores where every address allows, element-wise otherwise).
 * 64-bit addressing throughout, no atomics, no host synchronisation, every output element has one owner, nothing outside the
 * outputs is written and they need no initialisation.
 *
 * With skipped tiles the nirgan_tile_blend launches no longer cover every tile.  Only invalid pixels can then miss a covering tile (a
 * pixel inside a skipped tile's usable region is itself invalid), a scene that was zeroed first makes what they hold deterministic,
 * and the finish overwrites them; every valid pixel sees all of its covering tiles in ascending order as before.
 *
 * Argument errors return NIRGAN_ERR_ARG before any launch, the message names the entry.  Common: a null d or scene; unknown dtype;
 * C < 3; H or W < 1, H*W at 2^31 or more; a band outside 0 .. C-1; has_nodata with a uint16 nodata outside 0 .. 65535; divisor 0 or
 * NaN; tile < 4 or tile % 4 != 0; margin < 0 or margin >= tile/2; overlap < 0 or past core/2; 2^31 tiles or more.  Counts: null
 * counts.  Gather: null ids, ids_host or tiles, tiles not 16-byte aligned; n < 1 or n*3*tile*tile at 2^31 or more; an id outside
 * 0 .. nt-1 or not above its predecessor (the message names the position).  Finish: null blended or out; unknown out_kind;
 * NIRGAN_SCENE_OUT_U16 with a nodata_out that is not an integer in 0 .. 65535.
 * ------------------------------------------------------------------------------------- */
#define NIRGAN_SCENE_OUT_U16 0
#define NIRGAN_SCENE_OUT_F16 1
#define NIRGAN_SCENE_OUT_F32 2
typedef struct {
    /* common */
    const void* scene;                    /* device [C][H][W], the first element of plane 0 */
    int dtype;                            /* NIRGAN_SCENE_U16 or NIRGAN_SCENE_F32 */
    int C, H, W;
    int band[3];                          /* the planes of R, G, B */
    int has_nodata, nodata;               /* nodata: the uint16 value; not read for a float scene */
    float divisor;
    int tile, margin, overlap;
    /* nirgan_scene_tile_invalid */
    int32_t* counts;                      /* [nt] */
    /* nirgan_scene_tile_gather */
    const int32_t* ids;                   /* device [n], strictly ascending tile numbers */
    const int32_t* ids_host;              /* the same words in HOST memory: every check reads them */
    int n;
    float* tiles;                         /* [n][3][tile][tile], 16-byte aligned */
    const double* geo;                    /* device { lon0, dlon, lat0, dlat }, or NULL */
    float* coords;                        /* [n][2], or NULL */
    /* nirgan_scene_finish */
    const float* blended;                 /* [H][W] */
    int out_kind;                         /* NIRGAN_SCENE_OUT_* */
    float scale, nodata_out;
    void* out;                            /* [H][W] uint16, binary16 or float32 */
} nirgan_scene_predict_desc;
int nirgan_scene_tile_invalid(const nirgan_scene_predict_desc* d, void* stream);
int nirgan_scene_tile_gather(const nirgan_scene_predict_desc* d, void* stream);
int nirgan_scene_finish(const nirgan_scene_predict_desc* d, void* stream);

/* ---------------------------------------------------------------------------------------
 * Valid-pixel masks of scene-pool windows: the third place nodata is handled.  A sampler accepts a window with up to max_invalid
 * invalid pixels and delivers them as ordinary values; nirgan_scene_valid gives, for the same window rows, which pixels of the
 * DELIVERED tile are clean, and nirgan_pix_loss_masked (above) keeps the others out of the generator's reconstruction losses.
 *
 * nirgan_scene_valid: ONE launch, no atomics, no host synchronisation.
 * table / table_host: int64 [S][NIRGAN_SCENE_TABLE_COLS] in the format of nirgan_scene_sample; columns 1, 2 and 4 (H_s, W_s, prefix
 * offset) are read, column 0 is carried by the table but not used (no pixel is read), column 3 (cum_windows) is IGNORED: the table
 * of any tile size will do.  prefix / prefix_elems: the scenes' invalid-prefix tables (nirgan_scene_invalid_prefix), or NULL.
 * window / window_host, n_windows, first, n, tile: as in nirgan_scene_gather_desc.  A row is { s, y0, x0, word }, parsed as there:
 *     view = word & 7;   f = ((word >> 16) & 7) + 1;   L = f * T;   y0, x0 in SOURCE pixels
 * With P the prefix table of scene s, [(H_s+1)][(W_s+1)]:
 *     c(p, q)  = P[y0+(p+1)f][x0+(q+1)f] - P[y0+pf][x0+(q+1)f] - P[y0+(p+1)f][x0+qf] + P[y0+pf][x0+qf]      (int32, exact)
 *     D[p][q]  = c(p, q) == 0 ? 1.0f : 0.0f                     the f x f source block of delivered pixel (p, q) holds no invalid pixel
 *     valid[i][0][j1][j2] = D[j1'][j2']
 * with (j1', j2') by the view rule of nirgan_tile_views_expand on the T x T tile: the mask has the orientation of the pixels that
 * either sampler, or nirgan_scene_gather, delivered for the same row.  A scene without a table (table[s][4] < 0), or prefix == NULL,
 * gives all ones.  A float pool's table counts NaN pixels, so the same rule serves it.  valid is float [n][1][T][T]; every element
 * is written by one thread, the output needs no initialisation, nothing outside it is written.
 *
 * window_host may be NULL: the rows were just written by a draw on the same stream and no host copy exists.  The kernel then bounds
 * every row itself: a row with s outside 0 .. S-1, y0 < 0, x0 < 0, y0 + L > H_s or x0 + L > W_s gives an ALL-ZERO tile and nothing of
 * the prefix tables is read for it; the other rows are unaffected.  (The kernel makes this check for every call.)  With window_host
 * set, such a row -- and a stray bit in its word, and (f*T)^2 at 2^31 or more -- is refused on the host as nirgan_scene_gather refuses
 * it, before any launch, the message naming the row.
 * Argument errors return NIRGAN_ERR_ARG before any launch: a null pointer (d, table, table_host, window, valid); S <= 0; tile, n or
 * n*tile*tile outside 1 .. 2^31-1; first < 0 or first + n > n_windows; negative prefix_elems; a table row with an extent outside
 * 1 .. 2^31-1; with prefix set, a prefix table outside prefix_elems.
 *
 * nirgan_valid_count: count[0] (int32, device, OVERWRITTEN) = the number of i < n with valid[i] != 0.f (-0.f is not counted; a
 * denormal, any other value and NaN are).  Integer sums: exact and independent of scheduling.  A 4-byte clear and one launch on the
 * stream.  n outside 1 .. 2^31-1 or a null pointer return NIRGAN_ERR_ARG before either.
 * ------------------------------------------------------------------------------------- */
typedef struct {
    int S;
    const int64_t* table;                 /* device [S][NIRGAN_SCENE_TABLE_COLS]; columns 1, 2 and 4 are read */
    const int64_t* table_host;            /* the same table in HOST memory: every check reads it */
    const int32_t* prefix; int64_t prefix_elems;   /* device, or NULL: all ones */
    int tile;                             /* side T of the DELIVERED tile */
    const int32_t* window;                /* device [n_windows][4] */
    const int32_t* window_host;           /* the same words in HOST memory, or NULL: the kernel bounds the rows */
    int64_t n_windows;
    int64_t first; int n;                 /* rows [first, first + n) */
    float* valid;                         /* [n][1][T][T], OVERWRITTEN */
} nirgan_scene_valid_desc;
int nirgan_scene_valid(const nirgan_scene_valid_desc* d, void* stream);
int nirgan_valid_count(const float* valid, int64_t n, int32_t* count, void* stream);

/* ---------------------------------------------------------------------------------------
 * Matching the histogram of a uint16 plane to a reference band (skimage.exposure.match_histograms on integer codes): a count pass,
 * a 65 536-entry table and a lookup pass, all integer-exact.  One descriptor serves the three entries; every entry checks ITS fields
 * before any launch and reads nothing else.  No host synchronisation, nothing is read back.
 *
 * A plane is n contiguous uint16 codes, 1 <= n <= 2^31-1, 2-byte aligned ONLY (a plane of a [C][H][W] view starts where it starts).
 * A table is 8-byte aligned: hist / src_hist / ref_hist int64 [NIRGAN_SCENE_CODES], lut uint16 [NIRGAN_SCENE_CODES], totals int64 [2].
 * With has_nodata set, `nodata` (0 .. 65535) is the code of an invalid pixel.
 *
 * nirgan_scene_hist       hist[v] += the number of elements of `plane` equal to v; with has_nodata, elements equal to nodata are not
 *   counted.  The entry ADDS (64-bit integer adds, exact in any order): the caller clears the table, several planes pool into one.
 *   One launch.
 * nirgan_scene_match_lut  the transfer table from src_hist to ref_hist.  With
 *     ns = sum src_hist,  nr = sum ref_hist,  cs[v] = sum_{u <= v} src_hist[u],
 *     t_0 < .. < t_{m-1} the codes with ref_hist > 0,  q_j = (double)(sum_{u <= t_j} ref_hist[u]) / (double)nr,  x_v = (double)cs[v] / (double)ns
 *   y_v is numpy's interp(x_v, q, t) in float64, every operation rounded on its own (no fused multiply-add):
 *     x_v <= q_0 -> t_0;   x_v >= q_{m-1} -> t_{m-1};   else with j the last index where q_j <= x_v:
 *     x_v == q_j -> t_j,   otherwise ((t_{j+1} - t_j) / (q_{j+1} - q_j)) * (x_v - q_j) + t_j.
 *   The ROUNDED quantiles are compared with each other, as numpy compares them.  lut[v] = rint(y_v), ties to even, for ALL 65 536 v;
 *   with has_nodata a result equal to nodata moves to nodata + 1 (65534 for 65535), the rule of nirgan_scene_finish: a valid pixel is
 *   never read as nodata.  ns == 0 or nr == 0 gives the identity table lut[v] = v; the device decides this.  totals, if not NULL,
 *   receives { ns, nr }.  Totals above 2^53 are outside the contract (the conversions to double would round).  One launch.
 * nirgan_scene_lut_apply  out[i] = (has_nodata && plane[i] == nodata) ? nodata : lut[plane[i]].  out == plane is allowed (in place), any
 *   other overlap of the two is refused.  One owner per element, 64-bit addressing, no atomics.  One launch.
 *
 * Argument errors return NIRGAN_ERR_ARG before any launch, the message names the entry: a null d or a null pointer the entry uses
 * (totals may be NULL); n outside 1 .. 2^31-1; has_nodata with nodata outside 0 .. 65535; a plane or `out` at an odd address; a table
 * that is not 8-byte aligned; `out` overlapping `plane` without being equal to it.
 * ------------------------------------------------------------------------------------- */
#define NIRGAN_SCENE_CODES 65536
typedef struct {
    const void* plane;                    /* device uint16 [n]: hist counts it, lut_apply reads it */
    int64_t n;
    int has_nodata, nodata;
    int64_t* hist;                        /* nirgan_scene_hist: [NIRGAN_SCENE_CODES], ADDED to */
    const int64_t* src_hist;              /* nirgan_scene_match_lut */
    const int64_t* ref_hist;
    int64_t* totals;                      /* [2] = { ns, nr }, or NULL */
    uint16_t* lut;                        /* [NIRGAN_SCENE_CODES]: written by match_lut, read by lut_apply */
    void* out;                            /* nirgan_scene_lut_apply: uint16 [n] */
} nirgan_scene_match_desc;
int nirgan_scene_hist(const nirgan_scene_match_desc* d, void* stream);
int nirgan_scene_match_lut(const nirgan_scene_match_desc* d, void* stream);
int nirgan_scene_lut_apply(const nirgan_scene_match_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NIRGAN_HIP_H */
