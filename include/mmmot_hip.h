/*
 * mmmot_hip.h - C ABI of libmmmot_hip.so, the MI355X (gfx950) device library
 * behind the mmMOT per-frame-pair network forward.
 *
 * The reference (ZwwWayne/mmMOT) is pure Python: its "FFI" for this path is
 * the set of ATen operators that TrackingNet.forward dispatches
 * (modules/tracking_net.py:165-193; operator inventory SURVEY.md section 2b,
 * K1-K18).  Each entry point below replaces a *fused group* of those
 * operator calls; the reference call sites are cited per function.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to contiguous fp32 / int32 data unless
 *    named h_* ; no torch types cross this boundary;
 *  - activations are ROW-major "position-major": one row per position
 *    (pixel / point / detection / detection-pair), channels contiguous.  This
 *    is the transpose of the reference's N,C,L layout and is an internal
 *    choice: MFMA A-fragments and 16-byte coalesced loads both want the
 *    reduction (channel) axis contiguous;
 *  - "row tiles": rows are processed in tiles of <=128 rows that never span
 *    two normalisation groups (a group = one frame-pair, or one
 *    (frame-pair, modality-row)); tile_row0/tile_nrows/tile_group describe
 *    the T tiles, grp_* arrays describe the G groups;
 *  - all launches are asynchronous on `stream` (a hipStream_t passed as
 *    void*); the functions never synchronise and never allocate;
 *  - return value: 0 on success, MMMOT_EINVAL (-1) for a contract violation
 *    (bad alignment / unsupported size), otherwise the positive hipError_t
 *    of the failed launch.
 */
#ifndef MMMOT_HIP_H
#define MMMOT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMMOT_OK 0
#define MMMOT_EINVAL (-1)

/* activation codes */
#define MMMOT_ACT_NONE 0
#define MMMOT_ACT_RELU 1
#define MMMOT_ACT_SIGMOID 2

/* A-operand modes of mmmot_gemm_rows */
#define MMMOT_A_PLAIN 0     /* A = X[r][k]                                  */
#define MMMOT_A_NORM_RELU 1 /* A = max(0, X[r][k]*sc[g][k] + sh[g][k])      */
#define MMMOT_A_PAIR 2      /* A = op(FA[a_off+i][k], FB[b_off+j][k])       */

/* pairwise operators (reference modules/gcn.py:6-41) */
#define MMMOT_PAIR_MULTIPLY 0  /* batch_multiply  gcn.py:6-14  */
#define MMMOT_PAIR_MINUS_ABS 1 /* batch_minus_abs gcn.py:17-28 */
#define MMMOT_PAIR_MINUS 2     /* batch_minus     gcn.py:31-41 */

/* softmax modes (reference modules/tracking_net.py:106-126) */
/* elementwise loss terms of mmmot_score_loss (reference cost.py:97-131) */
#define MMMOT_LOSS_BCE 0        /* F.binary_cross_entropy_with_logits */
#define MMMOT_LOSS_L2 1         /* F.mse_loss(score.mul(mask), gt) */
#define MMMOT_LOSS_SMOOTH_L1 2  /* F.smooth_l1_loss(score.mul(mask), gt) */
#define MMMOT_SM_SINGLE 1
#define MMMOT_SM_DUAL 2
#define MMMOT_SM_DUAL_ADD 3
#define MMMOT_SM_DUAL_MAX 4

/* fusion modes (reference modules/fusion_net.py) */
#define MMMOT_FUSION_A 0
#define MMMOT_FUSION_B 1
#define MMMOT_FUSION_C 2

/* library / device info -------------------------------------------------- */
/* ABI history: 1 = first round-1 cut; 2 = gemm colsum / gemm_ares / gram / points / crops entry points,
 * gn_finalize tile_nrows, segment_mean seg_div; 3 = hq8 arithmetic (mmmot_conv3x3_bn_relu_hq8, mmmot_conv1_fused_hq8,
 * mmmot_hq8_pack/unpack, mmmot_segment_mean hl16 = 2), patch-kernel test / timing knobs;
 * 4 = per-output-channel weight scales (oscale is a [Cout] vector in the hl16 / hq8 trunk entry points),
 * mmmot_trunk_range_read, the tile / LDS-DMA trunk kernels and their knobs removed, timing experiments only in
 * -DMMMOT_DEBUG builds; 5 = training backward of the pairwise block (mmmot_gn_bwd_*, mmmot_gemm_tn,
 * mmmot_pair_bwd, mmmot_pair_expand_bwd, mmmot_rowdot_bwd, mmmot_softmax_pairs_bwd, mmmot_fusion_c_bwd, mmmot_add_rows),
 * mmmot_pointnet_layer1 takes K = 3 | 4; mmmot_pn_mlp64 added (additive, still 5);
 * 6 = mmmot_trunk_range_bind (per-caller range-guard counter blocks); 7 - 9: see the entry points marked so below;
 * 10 = mmmot_gram_rows at K = 128 writes the 32 x 32 blocks on and above the block diagonal of Gout only (the finalize
 * entry point mirrors), mmmot_set_gemm_rows_variant: 2 rejected, 3 / 4 = the two forms of the wide kernel;
 * mmmot_segment_argmax, mmmot_pair_expand_max_bwd added (backward of end_mode 'max'; additive, still 10);
 * mmmot_mot3d added (3D MOT evaluation; additive, still 10). */
int mmmot_abi_version(void);
/* returns 0 and fills cu_count / gcn arch string (<=32 bytes) of device 0..; */
int mmmot_device_info(int device, int* cu_count, char* arch, int arch_len);

/* ---------------------------------------------------------------------------
 * VGG16-BN trunk layer: 3x3 conv (pad 1) + folded eval-BatchNorm + ReLU, with
 * the following 2x2/s2 max-pool optionally fused into the epilogue.
 * Replaces conv2d + batch_norm + relu_ (+ max_pool2d) of
 * reference modules/vgg.py:67-80 as regrouped by
 * modules/appear_net.py:130-157,166-172.
 *   first=1: `in` is the reference's NCHW crop tensor [L][3][H][W]
 *            (modules/tracking_net.py:132) and wp is [Cout][32]
 *            (k = (ky*3+kx)*3 + c, zero padded 27->32);
 *   first=0: `in` is NHWC [L][H][W][Cin], wp is [9][Cout][Cin].
 *   out: NHWC [L][H][W][Cout], or [L][H>>1][W>>1][Cout] when pool=1 (odd maps are floored like
 *        nn.MaxPool2d(2, 2), modules/vgg.py:72: the last row / column has no window).
 * Implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32).  Any H, W >= 1;
 * Cin % 32 == 0 (first=0); Cout % 64 == 0.
 * ------------------------------------------------------------------------- */
int mmmot_conv3x3_bn_relu(const float* in, const float* wp, const float* bias,
                          float* out, int L, int H, int W, int Cin, int Cout,
                          int first, int pool, void* stream);

/* ---------------------------------------------------------------------------
 * fp16-matrix-core variant of the trunk layer with fp32-class accuracy ("f16x3").
 * "hl16" split-half format (same bytes as fp32): a row of C channels is C/8
 * units of 32 bytes, unit u = [fp16 hi of channels 8u..8u+7 | fp16 lo of the
 * same channels], hi = fp16(x), lo = fp16(x - hi).  Every product is evaluated
 * as a_hi*w_hi + a_hi*w_lo + a_lo*w_hi on v_mfma_f32_32x32x16_f16 with fp32
 * accumulation (3 MFMAs per algorithmic product: ceiling 2.5 PF / 3).
 *   in  : hl16 NHWC [L][H][W][Cin]       wp: hl16 [9][Cout][Cin], output channel n host-scaled by 2^wshift[n]
 *   out : hl16 NHWC (pooled when pool=1)  oscale[Cout] = 2^-wshift[n], applied before the bias
 * Cin % 32 == 0, Cout % 64 == 0, any H, W >= 1 (pool=1 floors odd maps: out is [L][H>>1][W>>1][Cout]).  Same reference lines as above
 * (conv2d + batch_norm + relu_ (+ max_pool2d), modules/vgg.py:67-80).
 * Kernel: LDS-resident haloed activation patch + streamed weight ring, persistent workgroups of 256 pixels
 * (16x16 or 4 x 8x8 blocks) x 64/128 channels (conv3x3_hl16_patch.hip).
 * mmmot_conv3x3_first_hl16 is the Cin=3 layer (fp32 MFMA on the NCHW crops) that
 * emits hl16; mmmot_hl16_pack/unpack convert n fp32 values (n % 8 == 0). */
int mmmot_conv3x3_bn_relu_hl16_patch(const void* in, const void* wp, const float* bias, void* out,
                                     int L, int H, int W, int Cin, int Cout, int pool, const float* oscale,
                                     void* stream);
/* conv1_1 (3->64) + conv1_2 (64->64) + 2x2 max-pool of the VGG trunk in ONE kernel (reference modules/vgg.py:67-80,
 * layers 0-6 of vgg16_bn.features): the patch kernel computes conv1_1 for the haloed 18x18 patch of every tile in
 * its prologue instead of reading it, so the [L][H][W][64] tensor (537 MB per cfg3 pair) is never written.
 *   crops NCHW fp32 [L][3][H][W];  w1 hl16 [64][32] (k = (ky*3+kx)*3 + colour, zero-padded), bias1 [64], oscale1 (scalar);
 *   w2 hl16 [9][64][64], bias2 [64], oscale2 [64];  out hl16 NHWC [L][H/2][W/2][64].  H, W even.
 *   bias1 travels through the matrix cores in the k = 27 slot of w1's records (split hi + lo like a weight):
 *   |bias1[n]| / oscale1 must stay below 65504 (host: pack.conv1_weight_shift picks the shift for weights AND bias). */
int mmmot_conv1_fused_hl16(const float* crops, const void* w1, const float* bias1, float oscale1,
                           const void* w2, const float* bias2, const float* oscale2, void* out, int L, int H, int W,
                           void* stream);
/* ABI 6: mmmot_conv1_fused_hl16 / _hq8 fed by the 8-bit crops of the resize instead of the fp32 model input (SURVEY 8f
 * rank 3 "fuse into the first conv's loader"): crops_u8 [L][H][W][3] RGB (mmmot_crop_resize_norm's out_u8), ToTensor and
 * Normalize - x / 255, (x - mean) / std with IEEE divisions, reference utils/build_util.py:111-112,137-142 - applied while
 * the raw window of a tile is fetched; bit-identical to feeding the fp32 tensor.  q8 != 0: the hq8 contract (w2, out). */
int mmmot_conv1_fused_u8(const unsigned char* crops_u8, float mean0, float mean1, float mean2, float std0, float std1,
                         float std2, const void* w1, const float* bias1, float oscale1, const void* w2,
                         const float* bias2, const float* oscale2, void* out, int L, int H, int W, int q8, void* stream);
/* "hq8" arithmetic (trunk mode 'f16q8', same reference lines): the two correction terms of the hi/lo split run on
 * the fp8 matrix cores (one block-scaled K=64 MFMA), 2 instead of 3 fp16-MFMA equivalents per product.
 *   activation record per 32 channels (128 bytes, like hl16): [32 x fp16 hi | 32 x e4m3(a / 4) | 32 x e4m3((a - hi) * 512)]
 *   weight record per 32 input channels: [32 x fp16 hi(w') | 32 x e4m3((w' - hi) * 32) | 32 x e4m3(hi / 64)],
 *   w' = w * 2^wshift[n] with a shift PER OUTPUT CHANNEL n (max|w'| of every channel in (2^13, 2^14]: the e4m3 copies
 *   of a low-gain channel of a trained, BatchNorm-folded layer keep their precision).
 * e4m3 = OCP FP8 E4M3 (max 448).  Relative error of a product ~2^-15 instead of 2^-21 (hl16); end-to-end score
 * error stays below the 1e-3 budget (tools/study_fp8_correction.py, tests/test_hq8_gpu.py, tests/test_robust_gpu.py).
 * Cin % 32 == 0, Cout % 64 == 0, any H, W >= 1 (pool=1 floors odd maps).  mmmot_hq8_pack/unpack convert n fp32 values (n % 32 == 0). */
int mmmot_conv3x3_bn_relu_hq8(const void* in, const void* wp, const float* bias, void* out,
                              int L, int H, int W, int Cin, int Cout, int pool, const float* oscale, void* stream);
/* mmmot_conv1_fused_hl16 with conv1_2 in hq8 arithmetic: w1 stays hl16, w2 is hq8 [9][64][64], out is hq8 */
int mmmot_conv1_fused_hq8(const float* crops, const void* w1, const float* bias1, float oscale1,
                          const void* w2, const float* bias2, const float* oscale2, void* out, int L, int H, int W,
                          void* stream);
int mmmot_hq8_pack(const float* x, void* y, long n, void* stream);
int mmmot_hq8_unpack(const void* x, float* y, long n, void* stream);
/* Range guard of the reduced-range activation formats.  The trunk epilogues count, on the device,
 *   out4[0]: activation elements written with |a| > 1792 in hq8 mode (their e4m3 copies saturate: the products of
 *            that element fall back to fp16-class accuracy);
 *   out4[1]: elements clamped at +-65000 by the fp16 `hi` half (hl16 and hq8: the value itself is wrong);
 *   out4[2]: workgroup-lanes of the fused first launch whose conv1_1 outputs crossed the mode's limit;  out4[3]: 0.
 * Synchronous read of the current device's counters into a HOST array (the caller synchronises the launch stream
 * first); reset != 0 clears them.  mmmot_amd.Engine reads them on the first forward and periodically, and moves the
 * trunk to f16x3 / f32 when they are hit. */
int mmmot_trunk_range_read(unsigned int* out4, int reset);
/* ABI 6.  Counter block of the CALLER (device memory, 4 x uint32, same layout as above) that the trunk launches issued
 * by this host thread report to from now on; NULL returns to the library's per-device block.  The block travels as a
 * kernel argument: a launch - or a launch captured into a hipGraph - keeps the block it was issued with, so every
 * engine (and every captured forward) has its own window, zeroed and read by its owner with ordinary stream-ordered
 * copies (mmmot_amd.Engine: one asynchronous 16-byte read-back per forward, inspected one step later). */
int mmmot_trunk_range_bind(unsigned int* counters4);
/* tests: cap the persistent grid of the patch kernels (multiple of 8, 0 = one workgroup per CU) so that small
 * problems run several chained tiles per workgroup like production sizes do.  Results do not depend on it. */
int mmmot_set_patch_grid_limit(int n);
/* ABI 7.  tests: smallest block edge the trunk dispatcher may choose - 0 / 4 = automatic (maps of at most 4 x 4 pixels,
 * conv5_x at 64-pixel crops, reference modules/vgg.py:67-80, run 16 whole maps per 256-row tile without halo),
 * 8 = such maps run as one haloed 8 x 8 block at 25 % fill like before ABI 7.  Results do not depend on it, bit for bit. */
int mmmot_set_patch_min_block(int bs);
/* tests (additive, ABI unchanged): output channels per tile of the patch kernels - 0 = automatic (csrc/patch_choice.h: 64-
 * channel tiles where twice as many tiles fill the CUs better, and wherever Cout % 128 != 0), 64, or 128 = 128-channel
 * tiles wherever Cout % 128 == 0.  The fused first launches always run 64-channel tiles.  Any other value: MMMOT_EINVAL.
 * Results do not depend on it, bit for bit (tests/test_trunk_kernels_gpu.py). */
int mmmot_set_patch_tile_width(int bn);
/* What the next mmmot_conv3x3_bn_relu_hl16_patch / mmmot_conv3x3_raw_hl16 / mmmot_conv3x3_bn_relu_hq8 launch of this
 * shape would use under the three knobs above: bn = channels per tile (64 | 128), bs = block edge (16 | 8 | 4), items =
 * tiles (pixel tiles x channel tiles), grid = persistent workgroups.  Host pointers, any of them may be NULL.  No launch.
 * L, H, W >= 1, Cout % 64 == 0, else MMMOT_EINVAL.  The choice is one pure host function (csrc/patch_choice.h,
 * pinned without a GPU by tests/test_patch_choice_cpu.py). */
int mmmot_patch_choice(int L, int H, int W, int Cout, int* bn, int* bs, int* items, int* grid);
#ifdef MMMOT_DEBUG
/* -DMMMOT_DEBUG builds only (tools/, never the product library; csrc/patch_debug.h): phase timers of the patch kernel
 * (0 = the product kernels, 9 = the timed instantiations; results are correct either way) and their read-out. */
int mmmot_set_patch_variant(int v);
int mmmot_debug_read_patch_timers(unsigned long long* out8, int reset);
#endif
int mmmot_conv3x3_first_hl16(const float* in, const float* wp, const float* bias, void* out,
                             int L, int H, int W, int Cout, void* stream);
int mmmot_hl16_pack(const float* x, void* y, long n, void* stream);
int mmmot_hl16_unpack(const void* x, float* y, long n, void* stream);
/* ABI 7, training step: y = hl16(x * 2^(target - ex)) with max |x| = amax[0] = f * 2^ex, f in [0.5, 1) - a DEVICE scalar
 * (mmmot_absmax), NULL = unscaled; and the vector out[0..C) = 2^-(shift_a + shift_b) that undoes two such scales in the
 * consumer's epilogue.  No host round trip: gradients (1e-4 .. 1e-7) and freshly stepped weights are scaled where they are. */
int mmmot_hl16_pack_pow2(const float* x, void* y, long n, const float* amax, int target, void* stream);
int mmmot_pow2_oscale(float* out, int C, const float* amax_a, int target_a, const float* amax_b, int target_b, void* stream);
/* ABI 7, training step: the plain 3x3 convolution out[p][n] = oscale[n] * sum_taps in[p + off] . wp[tap][n] + bias[n] as
 * fp32 rows [L*H*W][Cout] (no BatchNorm, no ReLU: the training-mode forward of /root/reference/modules/vgg.py:74-76 keeps
 * the pre-BatchNorm tensor, and the input gradient is the same convolution of dZ with the flipped, transposed weights) on
 * the fp16 matrix cores (f16x3): in = hl16 rows [L*H*W][Cin], wp = hl16 [9][Cout][Cin].  Cin % 32 == 0, Cout % 64 == 0. */
int mmmot_conv3x3_raw_hl16(const void* in, const void* wp, const float* bias, float* out, int L, int H, int W, int Cin,
                           int Cout, const float* oscale, void* stream);

/* ---------------------------------------------------------------------------
 * Row GEMM with fused operand generation and statistics epilogue:
 *   v[r][n] = sum_k A(r,k) * W[n][k] + bias[n] + dbias[rowidx[r]][n]
 *   part[t][0][n] = S  = sum_{r in tile t} v[r][n]
 *   part[t][1][n] = M2 = sum_{r in tile t} (v[r][n] - S/nrows_t)^2   (tile-centred)
 *   Y[r][n] = act(v[r][n])
 * Replaces every conv1d(k=1) / conv2d(1x1) / linear of the path
 * (reference modules/point_net.py:28,40,125,134-138; fusion_net.py:14-29,
 * 53-60,80-83; gcn.py:59-66; new_end.py:48-58; tracking_net.py:92-100;
 * appear_net.py:19-25) together with the producer side of the following
 * GroupNorm (per-tile sums; mmmot_gn_finalize turns them into scale/shift)
 * and the consumer side of the preceding one (A_NORM_RELU prologue).
 * A_PAIR generates the N x M pairwise tensor of modules/gcn.py:6-41 on the
 * fly in LDS - it is never materialised in HBM.
 * K % 32 == 0, N % 64 == 0, all leading dimensions % 4 == 0, pointers 16-byte
 * aligned.  Y, part, bias, dbias may be NULL.
 * ------------------------------------------------------------------------- */
typedef struct mmmot_gemm_args {
  const float* X; int ldx;              /* PLAIN / NORM_RELU source rows      */
  const float* W;                       /* [N][K]                             */
  const float* bias;                    /* [N] or NULL                        */
  const float* dbias; const int* rowidx; int lddb; /* gathered bias or NULL   */
  float* Y; int ldy;                    /* output rows or NULL                */
  float* part;                          /* [T][2][N] or NULL                  */
  const float* sc; const float* sh; int ldsc;      /* [G][ldsc] (NORM_RELU)   */
  const float* FA; const float* FB; int ldf;       /* PAIR feature rows       */
  const int* tile_row0; const int* tile_nrows; const int* tile_group; /* [T]  */
  const int* grp_row0; const int* grp_M; const int* grp_aoff; const int* grp_boff; /* [G] PAIR */
  int T; int N; int K;
  int amode; int pairop; int act;
  /* w_hl16 = 1: W is in the hl16 split-half format ([N][K/8] units of [hi8|lo8] halves, values
   * pre-scaled by 1/oscale) and the contraction runs on the fp16 matrix cores with the 3-term
   * hi/lo split (fp32-class accuracy, see mmmot_conv3x3_bn_relu_hl16); requires K % 64 == 0.
   * The A operand stays fp32 in memory and is split while staged.  oscale multiplies the
   * accumulator before bias. */
  int w_hl16; float oscale;
  /* Fused consumer of the NEXT GroupNorm (v2): when colsum != NULL the epilogue also evaluates
   * colsum[t][n] = sum over the tile's rows of relu(v[r][n] * osc[g][n] + osh[g][n]) (g = tile_group[t]),
   * i.e. the per-tile part of "normalise + ReLU + per-detection mean" (reference
   * modules/point_net.py:28-39,138-148) without the [rows][N] tensor ever reaching HBM: run the GEMM once
   * with Y = NULL, part != NULL (statistics), finalize, and once with Y = NULL, colsum != NULL; tiles
   * must not straddle the segments to be averaged; mmmot_segment_mean over the tile rows (seg_div =
   * rows per segment) finishes the mean. */
  const float* osc; const float* osh; int ldosc;   /* [G][ldosc] or NULL                */
  float* colsum;                        /* [T][N] or NULL                     */
  /* ABI 7 (appended).  PAIR: nonzero = the caller guarantees BOTH grp_M[g] % 32 == 0 for every group AND
   * (tile_row0[t] - grp_row0[tile_group[t]]) % 32 == 0 for every tile (tiles cut every 128 rows from the start of their
   * group satisfy the second condition), i.e. the 32 rows of every 32-row block of a tile share their a_i row; the wide
   * kernel (csrc/gemm_wide.hip) then stages that row in LDS once per wave instead of requesting it per lane (it serves
   * PAIR launches only with this guarantee, takes a_i from the block's first row, and returns WRONG Y - silently - for a
   * caller that sets the flag on ragged or unaligned pair tiles).  0 is always safe: the tile kernel serves the launch. */
  int pair_uniform32;
} mmmot_gemm_args;
int mmmot_gemm_rows(const mmmot_gemm_args* a, void* stream);
/* ABI 7.  tests: which kernel serves mmmot_gemm_rows - 0 = automatic (the wide kernel of csrc/gemm_wide.hip for the
 * K >= 256 layers of the pairwise block, reference modules/gcn.py:59-66 / new_end.py:48-52, when w_hl16 = 1, amode is
 * PAIR or NORM_RELU, N % 256 == 0, no dbias / colsum / activation and the launch fills the chip), 1 = the tile kernel
 * only (the kernel before ABI 7), 3 / 4 = the wide kernel whenever the layer is eligible (N % 256 == 0, K = 256 or 512,
 * any size) with one 128-row tile per four-wave workgroup (two workgroups per CU) / two tiles per eight-wave workgroup;
 * 2 (the round-5 form of the wide kernel, removed in round 6) is rejected.  Y and part do not depend on it, bit for bit. */
int mmmot_set_gemm_rows_variant(int v);
/* tests (additive, ABI unchanged): cap the persistent grid of the wide kernel - 0 = automatic, n > 0: at most n
 * workgroups, rounded down to whole groups of 8 * (N / 256) and never below one such group (the launcher's floor, the grid
 * of an 8-CU part), so that a small problem walks the chains of items a production batch walks; negative: MMMOT_EINVAL.
 * Y and part do not depend on it, bit for bit (tests/test_wide_kernels_gpu.py). */
int mmmot_set_gemm_wide_grid_limit(int n);
/* What the next mmmot_gemm_rows launch of these arguments would use under the variant and the grid limit above: wide =
 * 1 the wide kernel | 0 the tile kernel, nh = 128-row tiles per workgroup of the wide kernel (1 | 2; 0 on the tile kernel),
 * items = items of the launch (wide: groups of nh row tiles x 256-column tiles, padded to whole groups of 8 * (N / 256);
 * tile kernel: T x column tiles), grid = workgroups.  Host pointers, any of them may be NULL.  No launch.  The argument
 * checks of mmmot_gemm_rows, MMMOT_EINVAL where it would return that.  The choice is one pure host function
 * (csrc/wide_choice.h, pinned without a GPU by tests/test_wide_choice_cpu.py). */
int mmmot_gemm_rows_choice(const mmmot_gemm_args* a, int* wide, int* nh, int* items, int* grid);

/* A-resident row GEMM for layers whose output is only ever reduced (PointNet conv5 128->1024 and
 * PointNet_v1.conv1 64->512, reference modules/point_net.py:28-39,138-148): the workgroup keeps its 128
 * activation rows (normalised, ReLU'd, hi/lo split once) in LDS and walks all N/128 channel tiles;
 *   v[r][n] = oscale * sum_k relu(X[r][k]*sc[g][k]+sh[g][k]) * W[n][k] + bias[n] + dbias[tile_dbrow[t]][n]
 * is never stored.  Outputs, per 64-row HALF tile h of tile t (row index 2t+h; a half may be empty):
 *   part   [2T][2][N]: sum and half-tile-centred M2 of v   -> mmmot_gn_finalize with tile_nrows = rows per half
 *   colsum [2T][N]   : sum of relu(v*osc[g][n]+osh[g][n])  -> mmmot_segment_mean with seg_div
 * W is hl16 ([N][K/8] units, pre-scaled by 1/oscale); K is 64 or 128; N % 256 == 0 (K = 64 with N <= 512,
 * served by the weight-resident kernel: N % 128 == 0); tiles must not straddle
 * the rows that share a dbias row (detection-aligned tiles).  At least one of part / colsum. */
typedef struct mmmot_gemm_ares_args {
  const float* X; int ldx;
  const float* sc; const float* sh; int ldsc;   /* [G][ldsc] prologue scale / shift         */
  const void* W;                                 /* hl16 weights                             */
  const float* bias;                             /* [N] or NULL                              */
  const float* dbias; const int* tile_dbrow; int lddb;  /* per-tile extra bias row or NULL   */
  const int* tile_row0; const int* tile_nrows; const int* tile_group; /* [T]                 */
  float* part;                                   /* [2T][2][N] or NULL                       */
  const float* osc; const float* osh; int ldosc; /* [G][ldosc], needed with colsum           */
  float* colsum;                                 /* [2T][N] or NULL                          */
  int T; int N; int K;
  float oscale;
} mmmot_gemm_ares_args;
int mmmot_gemm_ares(const mmmot_gemm_ares_args* a, void* stream);
/* ABI 7.  tests: which kernel serves the K = 128 consumer pass (colsum only) of mmmot_gemm_ares - 0 = automatic (the
 * weights-in-registers kernel of csrc/gemm_wreg.hip when N % 512 == 0 and the launch fills the chip), 1 = the streaming
 * kernel only (the kernel before ABI 7), 2 = the register kernel whenever the layer is eligible.  Results do not depend on
 * it, bit for bit.
 * K = 64, N <= 512 (PointNet_v1.conv1, csrc/gemm_wres.hip), since round 6: 0 = the independent-wave kernel for a column-sum
 * pass that gives every wave at least four 64-row half tiles, the two-barrier weight-resident kernel otherwise; 1 = the
 * streaming kernel (N % 256 == 0); 2 = the independent-wave kernel for every column-sum pass; 3 = the two-barrier kernel
 * only (K = 128: as 0).  Bit for bit the same column sums. */
int mmmot_set_gemm_ares_variant(int v);

/* ---------------------------------------------------------------------------
 * GroupNorm statistics of a 1x1-conv output from the second moments of its INPUT (v2):
 * for v = W a + b with a = relu(X*sc + sh) over the rows of a group, per output channel
 *   mean = w.m + b,  var = w^T Cov(a) w  (m = E[a], Cov = E[a a^T] - m m^T)
 * so PointNet conv5 128->1024 + GroupNorm(1024,1024) (reference modules/point_net.py:138) needs ONE pass of
 * the 128->1024 GEMM (the normalise + ReLU + per-detection-sum pass of mmmot_gemm_ares) instead of two.
 * mmmot_gram_rows: per super-tile t (tile_row0/nrows/group, any row count, fp32 accumulation restarts every 128
 *   rows; the 128-row sums are added up in float64 (K = 128) / compensated fp32 pairs (K = 64)) Gout[t][K][K] = sum a a^T
 *   and Sout[t][K] = sum a, float64.  K = 64 or 128.  K = 128 writes the 32 x 32 blocks on and above the block
 *   diagonal only (the matrix is symmetric; mmmot_gn_finalize_gram mirrors) - the other blocks of Gout are not touched.
 * mmmot_gn_finalize_gram: sums the super-tiles of every group (grp_tile0 / grp_ntiles), forms Cov in float64
 *   and writes sc[g][n] = gamma[n]*rstd, sh[g][n] = beta[n] - mean*sc for the N output channels of
 *   W [N][K] (fp32, unscaled) / bias [N] (may be NULL).  work: G*(K*K+K) doubles. */
int mmmot_gram_rows(const float* X, int ldx, int K, const float* sc, const float* sh, int ldsc,
                    const int* tile_row0, const int* tile_nrows, const int* tile_group, int T,
                    double* Gout, double* Sout, void* stream);
/* ABI 10.  tests / A-B: which kernel serves mmmot_gram_rows at K = 128 - 0 = automatic (by the number of super-tiles),
 * 1 = the four-wave form (two workgroups per CU), 2 = the pipelined eight-wave form (one workgroup per CU, both LDS plane
 * pairs, two sub-tiles of rows in flight in registers).  Gout / Sout do not depend on it, bit for bit (same blocks, same
 * summation order per block and per column sum). */
int mmmot_set_gram128_variant(int v);
int mmmot_gn_finalize_gram(const double* Gp, const double* Sp, const int* grp_tile0, const int* grp_ntiles,
                           const int* grp_count, int G, int K, const float* W, const float* bias, int N,
                           const float* gamma, const float* beta, float eps, double* work, float* sc,
                           float* sh, void* stream);
/* ABI 9.  The same route for a layer with a gathered per-detection bias, v[p] = W a[p] + dbias[det(p)]
 * (PointNet_v1.conv1 after the 1088 -> 512 split, reference modules/point_net.py:26-28): the super-tiles handed to
 * mmmot_gram_rows (K = 64) are cut along detections - super-tile t lies inside detection tile_det[t] (a row of dbias
 * [.][lddb]) and holds tile_nrows[t] rows - so that its column sums Sp[t] give the cross term:
 *   mean = w.m + dbar,  var = w^T Cov w + 2 (sum_t d_t (w.Sp[t]) / P - (w.m) dbar) + (sum_t c_t d_t^2 / P - dbar^2),
 * dbar = sum_t c_t d_t / P, float64 throughout.  Replaces the statistics pass of mmmot_gemm_ares over every point.
 * W [N][64] fp32 (unscaled); work: G*(K*K+K) doubles; sc / sh [G][N]. */
int mmmot_gn_finalize_gram_dbias(const double* Gp, const double* Sp, const int* grp_tile0, const int* grp_ntiles,
                                 const int* grp_count, int G, const int* tile_nrows, const int* tile_det, int K,
                                 const float* W, const float* dbias, int lddb, int N, const float* gamma,
                                 const float* beta, float eps, double* work, float* sc, float* sh, void* stream);

/* GroupNorm statistics -> per-channel scale/shift (fp64 combine).
 * part is [T][2][ldp] = per-tile (sum, tile-centred M2) as written by
 * mmmot_gemm_rows / mmmot_pointnet_layer1 (the C channels start at part[0];
 * ldp >= C lets one GEMM's statistics feed several norms over channel
 * sub-ranges); tiles are merged with Chan et al.'s parallel-variance update in
 * fp64, so the result is robust when |mean| >> std.  A group's tiles must be
 * consecutive 128-row chunks of its rows, the last one partial;
 * group g owns tiles [grp_tile0[g], +grp_ntiles[g]) and grp_count[g] rows;
 * the C channels are split into NG normalisation groups (nn.GroupNorm(NG, C),
 * eps, biased variance).  sc[g][c] = gamma[c]*rstd, sh[g][c] = beta[c]-mean*sc.
 * tile_nrows (v2, may be NULL): rows of every tile when the tiles are NOT plain 128-row chunks
 * (detection-aligned tiles of the fused PointNet path).
 * Replaces the statistics half of every F.group_norm on the path. */
int mmmot_gn_finalize(const float* part, const int* grp_tile0, const int* grp_ntiles,
                      const int* grp_count, const int* tile_nrows, int G, int ldp, int C, int NG,
                      const float* gamma, const float* beta, float eps,
                      float* sc, float* sh, void* stream);

/* Strided/ragged segment mean with optional normalise+ReLU prologue:
 *   out[s][c] = mean_{t<count[s]} f(X[start[s] + t*stride[s]][c])
 * Replaces the per-detection Python pooling loops of
 * reference modules/point_net.py:32-39,139-148, adaptive_avg_pool2d of
 * modules/appear_net.py:15,30 and the mean(dim=-2/-1) of
 * modules/new_end.py:70-71.  C % 4 == 0. seg_group / sc / sh may be NULL.
 * seg_div (v2, may be NULL): divide the segment sum by seg_div[s] instead of count[s] (rows of X
 * that are already per-tile partial sums, see mmmot_gemm_args.colsum).
 * relu is a flag word (v4): bit 0 = ReLU after the affine, bit 1 = MAXIMUM over the segment instead of the
 * mean (end_mode 'max' of NewEndIndicator_v2, modules/new_end.py:72-74); seg_div does not enter a maximum.
 * Every segment holds at least one row: count[s] >= 1 is the caller's to guarantee and is not checked (the counts
 * live on the device).  The batch plan guarantees it - every frame has a detection, every detection a point, every
 * pooling chunk a row (mmmot_amd/plan.py refuses anything else) - and the result for count[s] == 0 is unspecified
 * (the mean would be 0 / 0, the maximum the accumulators' start value). */
int mmmot_segment_mean(const float* X, int ldx, int C,
                       const int* seg_start, const int* seg_count, const int* seg_stride,
                       const int* seg_group, const int* seg_div, int nseg,
                       const float* sc, const float* sh, int ldsc, int relu,
                       float* out, int ldo,
                       int hl16 /* 1: X rows are in the hl16 split-half format, 2: hq8 records (C % 32 == 0) */,
                       void* stream);

/* out[omap ? omap[r] : r] = post(act(sum_k f(X[r][k])*w[k] + b)),
 * post(v) = v - (v < thr) when use_thr (reference tracking_net.py:161-162).
 * Final 1-channel layers: gcn.py:66, new_end.py:58, tracking_net.py:99. */
int mmmot_rowdot(const float* X, int ldx, int K, const float* w, float b,
                 const float* sc, const float* sh, int ldsc,
                 const int* tile_row0, const int* tile_nrows, const int* tile_group, int T,
                 int act, int use_thr, float thr,
                 float* out, const int* omap, void* stream);

/* Per-row LayerNorm (= GroupNorm(1,C) on L x C x 1 x 1, appear_net.py:19-25):
 * Y[r][c] = act(gamma[c]*(X[r][c]-mean_r)*rstd_r + beta[c]).  C % 64 == 0, C <= 1024 */
int mmmot_row_layernorm(const float* X, int ldx, int C, const float* gamma, const float* beta,
                        float eps, int relu, float* Y, int ldy, int R, void* stream);

/* One SkipPool head (reference modules/appear_net.py:19-32) after the global average pool, in one launch (ABI 6):
 *   out[r][0:128] = relu(LN_128(w4 . relu(LN_C4(w1 . LN_C(P[r]) + c1)) + c4))        LN = GroupNorm(1, .) of a row
 * P [R][C] pooled stage features (row stride ldp), w1 [C4][C], w4 [128][C4] fp32, C % 64 == 0 <= 512, C4 in {64, 128};
 * out rows have stride ldo (the stage's 128-column slice of the [L][1024] feature matrix). */
int mmmot_skippool_head(const float* P, int ldp, int C, int C4, const float* g0, const float* b0, const float* w1,
                        const float* c1, const float* g2, const float* b2, const float* w4, const float* c4,
                        const float* g5, const float* b5, float eps, float* out, int ldo, int R, void* stream);
/* PointNet first shared-MLP layer with the K x K STN transform folded into the
 * weights (point_net.py:119-125): Y[p][0..63] = W[64][K] x[p] + b, plus
 * per-tile statistics like mmmot_gemm_rows.  K = 3 (xyz; every shipped config sets without_reflectivity) or 4
 * (xyz + reflectivity, tracking_net.py:41); X is [P][K] as delivered in det_info['points']. */
int mmmot_pointnet_layer1(const float* X, int K, const float* W, const float* bias,
                          float* Y, float* part,
                          const int* tile_row0, const int* tile_nrows, int T, void* stream);

/* PointNet shared-MLP layer with 64 input channels (feat.conv2 / conv3 / conv4, point_net.py:134-137):
 *   v[r][n] = sum_k relu(X[r][k]*sc[g][k] + sh[g][k]) * W[n][k] * oscale + bias[n],   k < 64, N = 64 | 128
 * Y[r][n] = v (raw, the next layer normalises it) and part[t] = per-tile (sum, tile-centred M2) of v - exactly what
 * mmmot_gemm_rows computes for amode = MMMOT_A_NORM_RELU, w_hl16 = 1, K = 64 - from persistent workgroups that keep
 * W16 ([N][8] hl16 units, host-scaled by 1/oscale) in LDS and prefetch the next tile's rows.  tile_group may be NULL. */
int mmmot_pn_mlp64(const float* X, int ldx, const float* sc, const float* sh, int ldsc, const void* W16,
                   float oscale, const float* bias, float* Y, int ldy, float* part, const int* tile_row0,
                   const int* tile_nrows, const int* tile_group, int T, int N, void* stream);

/* Y[r][c] = act(X[r][c]*sc[g][c] + sh[g][c]); g from the tile table. C % 4 == 0 */
int mmmot_affine_act(const float* X, int ldx, int C, const float* sc, const float* sh, int ldsc,
                     const int* tile_row0, const int* tile_nrows, const int* tile_group, int T,
                     int act, float* Y, int ldy, void* stream);

/* Fusion module A/B/C combine (fusion_net.py:31-42,62-70,85-92).
 * cat: [Lt][2C] = [image | lidar] features; F: [3][Lt][C] = image, lidar, fused.
 *  A: fused = Y0*sc0+sh0
 *  B: fused = (Y0*sc0+sh0) + (Y1*sc1+sh1)
 *  C: Y0=[gate_p|input_p](image), Y1=[gate_i|input_i](lidar), ld 2C:
 *     fused = (s(g0)*(i0*sc0+sh0) + s(g1)*(i1*sc1+sh1)) / (s(g0)+s(g1)) */
int mmmot_fusion_combine(int mode, const float* cat, const float* Y0, int ld0,
                         const float* Y1, int ld1,
                         const float* sc0, const float* sh0, const float* sc1, const float* sh1, int ldsc,
                         const int* tile_row0, const int* tile_nrows, const int* tile_group, int T,
                         float* F, int Lt, int C, void* stream);

/* Softmax modes over each group's N x M logit block (tracking_net.py:106-126).
 * logits/out rows are ordered (group, i, j); one workgroup per group. */
int mmmot_softmax_pairs(const float* logits, float* out,
                        const int* grp_row0, const int* grp_N, const int* grp_M, int G,
                        int max_nm /* max over groups of N+M (LDS sizing) */,
                        int mode, void* stream);

/* ---------------------------------------------------------------------------
 * Point-cloud gather (the step that produces det_info['points'] /
 * det_info['points_split'] for the path above).  Replaces the numba loop
 * _points_in_convex_polygon_3d_jit (reference point_cloud/geometry.py:96-114) and the per-box
 * boolean-index loop of read_and_prep_points (point_cloud/preprocess.py:70-96).
 *   pts    [P][F] fp32, F = 3 or 4, xyz first
 *   planes [NB][6][4] fp64 rows (nx, ny, nz, d) of convex polygons whose normals point inwards (3D boxes,
 *          image / 2D-box frustums); a point is inside iff ((x*nx + y*ny) + z*nz) + d < 0 for all six,
 *          evaluated in fp64 left to right without FMA contraction - the reference's arithmetic, so the
 *          decision is bit-identical.  NB <= 256 per call.
 * mmmot_points_count : cnt (ints, NB*ceil(P/256) + NB) and split [NB+1] = first output row of every polygon;
 *                      with pad_empty an empty polygon owns ONE all-zero row (preprocess.py:80-81).
 * mmmot_points_scatter: out [split[NB]][Fo] = per polygon its inside points in input order; Fo == F, or
 *                      Fo == 3 with F == 4 (the reflectivity column dropped, preprocess.py:97-100).
 * The caller reads split[NB] (one D2H of the split it hands to the host plan anyway) to size out. */
int mmmot_points_count(const float* pts, int P, int F, const double* planes, int NB, int pad_empty,
                       int* cnt, int* split, void* stream);
int mmmot_points_scatter(const float* pts, int P, int F, const double* planes, int NB, const int* cnt,
                         const int* split, float* out, int Fo, void* stream);
/* Batched form: NS sweeps (points of sweep s = rows [sweep_row0[s], sweep_row0[s+1]) of pts) and NPOLY polygons
 * (polygons of sweep s = [poly0[s], poly0[s+1]), at most 256 per sweep) in one launch; filt[s] >= 0 names a polygon
 * of `planes` every emitted point of sweep s must ALSO be inside (the image frustum of remove_outside_points fused
 * into the per-box test: same rows, same order as filtering first, no intermediate array).  Host-built tables:
 * blk_sweep [NBLK] / blk_first [NS] (256-point blocks per sweep), cnt_off [NPOLY] (first counter of each polygon;
 * polygon totals are stored at cnt[cnt_total + j]; behind them, 8-byte aligned, the count pass leaves four 64-bit
 * membership masks per counter for the scatter pass, so cnt holds ((cnt_total + NPOLY + 1) & ~1) + 8 * cnt_total
 * ints - since ABI 8).  split [NPOLY+1] as above. */
int mmmot_points_count_batched(const float* pts, int F, int NS, int NPOLY, int NBLK, int cnt_total,
                               const double* planes, const int* blk_sweep, const int* blk_first,
                               const int* sweep_row0, const int* poly0, const int* filt, const int* cnt_off,
                               int pad_empty, int* cnt, int* split, void* stream);
int mmmot_points_scatter_batched(const float* pts, int F, int NS, int NPOLY, int NBLK, int cnt_total,
                                 const double* planes, const int* blk_sweep, const int* blk_first,
                                 const int* sweep_row0, const int* poly0, const int* filt, const int* cnt_off,
                                 const int* cnt, const int* split, float* out, int Fo, void* stream);

/* ---------------------------------------------------------------------------
 * Ego-motion alignment of extracted points: align_points (reference utils/data_util.py:512-520, called per pair at
 * dataset/test_seq_dataset.py:209 for the pair's second frame) with lidar_to_imu / imu_to_lidar
 * (point_cloud/box_np_ops.py:599-611).  One thread per row, several segments (frames) per launch.
 *   pts      [Q][F] fp32, F = 3 or 4, xyz first; rows of segment s = [seg_row0[s], seg_row0[s+1])
 *   seg_row0 [NS+1] ints, seg_row0[0] = 0, non-decreasing (an empty segment is allowed), seg_row0[NS] = Q
 *   xf       [NS][MMMOT_ALIGN_REC] fp64, one transform record per segment:
 *              [0, 16)   A = inv(imu2velo.T), row-major 4x4
 *              [16, 64)  up to MMMOT_ALIGN_MAX_CHAIN steps of 12: R row-major 3x3, then T; step 0 is applied first, so
 *                        the caller stores the reference's lists R, T from LAST to FIRST (align_points' loop order);
 *                        only the first `chain` steps are read
 *              [64, 80)  B = imu2velo.T, row-major 4x4
 *   out      row i goes to out + (out_row0 + i) * ldo, F floats (ldo >= F): a slice of a larger buffer is written in
 *            place, rows outside [out_row0, out_row0 + Q) and columns >= F are not touched
 * Arithmetic per row, fp64, every product and sum rounded on its own (no FMA contraction), sums in k order:
 *   p = (x, y, z, 1);  q[j] = ((p0*A[0][j] + p1*A[1][j]) + p2*A[2][j]) + A[3][j], j < 3;
 *   per step q[j] <- ((q0*R[j][0] + q1*R[j][1]) + q2*R[j][2]) + T[j];  then the row x B like the row x A;
 *   ONE rounding to fp32 at the store.  With F = 4 the fourth column is copied bit for bit.  Every row is transformed,
 *   the all-zero row of an empty box included (the reference aligns it too).
 * Returns MMMOT_EINVAL for F outside {3, 4}, a negative Q / NS / out_row0, chain outside [0, 4], and with Q > 0 for a
 * null pointer, NS < 1 or ldo < F.  Q = 0 is a no-op that returns 0. */
#define MMMOT_ALIGN_MAX_CHAIN 4
#define MMMOT_ALIGN_REC 80
int mmmot_align_points(const float* pts, int F, int Q, int NS, const int* seg_row0, const double* xf, int chain,
                       float* out, long out_row0, int ldo, void* stream);

/* ---------------------------------------------------------------------------
 * Gap filling of tracked sequences (csrc/fill_tracks.hip), additive in ABI 10: one interpolated box
 * for every LISTED frame that a track skipped between two of its observations, for S sequences in five launches
 * whatever the number of frames, sequences, tracks and holes.
 *   det         [L][12] fp32 per detection: 2D box x1 y1 x2 y2, h w l, x y z (camera frame), rotation_y, score
 *   ids         [L] track ID per detection, -1 = rejected
 *   frame_start [F+1] detections of listed frame p = [frame_start[p], frame_start[p+1]); 0 first, L last, non-decreasing
 *   frame_no    [F] frame numbers, strictly increasing inside a sequence
 *   seq_start   [S+1] listed frames of sequence s = [seq_start[s], seq_start[s+1]); 0 first, F last, non-decreasing
 *   xf          [F][max_fill+1][MMMOT_FILL_REC] fp64, or NULL for a standing camera.  Record (p, k-1), for the listed
 *               frames p and p+k of one sequence: [0, 16) C[p<-p+k], a row-vector 4x4 (row-major) that takes camera
 *               coordinates of frame p+k to those of frame p; [16, 32) its inverse; [32] the yaw step dyaw[p<-p+k].
 *               Records that reach past the end of a sequence are not read.
 *   wtab        [MMMOT_FILL_MAX+2][MMMOT_FILL_MAX+2] fp64, wtab[n][k] = k / n (host-made, so that a host restatement
 *               reads the same bits)
 *   work        [MMMOT_FILL_WORK(L)] ints of scratch
 *   fill_start  [F+1] out: the new rows of listed frame p = [fill_start[p], fill_start[p+1])
 *   out         [capacity][12] fp32, out_id [capacity], out_src [capacity][2] (indices of the two source detections)
 *   info        [S][4] out: status, rows, links filled, links too long (the last three 0 unless status is 0 or ECAPACITY)
 * A link joins detection i (listed frame pa) and the next detection j (listed frame pb) of the same ID >= 0 in the same
 * sequence; with n = frame_no[pb] - frame_no[pa] it is filled iff 2 <= n <= max_fill + 1, by one row per listed frame p
 * strictly between, ordered per frame by ascending ID.  With w = wtab[n][frame_no[p] - frame_no[pa]], all in fp64, every
 * product and sum rounded on its own, one rounding to fp32 at the store:
 *   2D box, h w l, score: (1 - w) a + w b;   location: b' = b C[pa<-pb] (b as (x, y, z, 1), columns 0..2, summed in k
 *   order), the blend of a and b', then times inv C[pa<-p] (both skipped when xf is NULL);   yaw: d = (ry_b +
 *   dyaw[pa<-pb]) - ry_a wrapped into [-pi, pi) by at most four steps of 2 pi, then ry_a + w d - dyaw[pa<-p], wrapped.
 * Status, per sequence, never a fault: EDUP an ID twice in one frame, ECONTRACT frame numbers that do not increase (or,
 * for every sequence of the call, a frame_start / seq_start that breaks the shape above) - such a sequence gets no rows;
 * ECAPACITY its rows reach past `capacity` - the rows below it are written, nothing past it, the counts are reported.
 * Returns MMMOT_EINVAL before any launch for S < 1, a negative L / F / capacity, max_fill outside [1, MMMOT_FILL_MAX]
 * and, with L > 0 and F > 0, a null pointer (xf may be null; out / out_id / out_src may be with capacity = 0).  L = 0 or
 * F = 0 is a no-op that returns 0.  No allocation, no synchronisation. */
#define MMMOT_FILL_MAX 30
#define MMMOT_FILL_REC 33
#define MMMOT_FILL_WORK(L) (3 * (long)(L) + 1)
#define MMMOT_FILL_EDUP 1
#define MMMOT_FILL_ECAPACITY 2
#define MMMOT_FILL_ECONTRACT 4
int mmmot_fill_tracks(const float* det, const int* ids, const int* frame_start, const int* frame_no,
                      const int* seq_start, const double* xf, const double* wtab, int L, int F, int S, int max_fill,
                      int capacity, int* work, int* fill_start, float* out, int* out_id, int* out_src, int* info,
                      void* stream);

/* ---------------------------------------------------------------------------
 * Smoothing of tracked sequences (csrc/smooth_tracks.hip; DESIGN section 12b, which states the order of every
 * operation), additive in ABI 10: a Kalman filter forwards and a Rauch-Tung-Striebel pass backwards along every track,
 * for S sequences in five launches whatever the number of rows, frames, sequences and tracks.
 *   det, ids, frame_start, frame_no, seq_start: the tables of mmmot_fill_tracks
 *   observed    [L] or NULL (every row observed): a row with observed == 0 carries no measurement
 *   xf0         [F][MMMOT_FILL_REC] fp64, or NULL for a standing camera: the record of listed frame p is C[a<-p] | its
 *               inverse | dyaw[a<-p] in the layout of mmmot_fill_tracks, a the first listed frame of p's sequence
 *   q_, r_, v0_ process noise (white acceleration; h w l: a random walk), measurement variance and initial velocity
 *               variance of the location (x y z), the yaw and the dimensions (h w l), per frame number
 *   yaw_flip    1: an unwrapped yaw step beyond pi/2 is taken as the detector's front / back confusion (pi is added)
 *   work        [MMMOT_SMOOTH_WORK(L)] ints of scratch, 8-byte aligned
 *   out         [L][12] fp32: the rows of det with h w l, x y z and rotation_y smoothed; the 2D box and the score copied
 *   out_vel     [L][4] fp32 or NULL: vx, vy, vz (the row's own frame's axes) and the yaw rate per frame number
 *   info        [S][4] out: status, chains smoothed, rows changed, rows copied
 * A track is the rows of one sequence with the same ID >= 0; its chain starts at its first observed row and holds every
 * later row (unobserved rows are predictions).  Rows with ID < 0, rows in front of a chain, chains of one row and every
 * channel group whose r is 0 are copied bit for bit, with velocity 0.  Status, per sequence, never a fault:
 * MMMOT_FILL_EDUP / MMMOT_FILL_ECONTRACT as for mmmot_fill_tracks - the sequence's rows are copied, info = status, 0, 0,
 * its rows; a frame_start / seq_start that breaks its shape gives every sequence ECONTRACT, all rows copied, counters 0.
 * Returns MMMOT_EINVAL before any launch for S < 1, a negative L / F, a negative, NaN or infinite parameter, v0 <= 0 for
 * a group with r > 0, yaw_flip outside {0, 1} and, with L > 0 and F > 0, a null pointer (observed, xf0 and out_vel may
 * be null), a work that is not 8-byte aligned or MMMOT_SMOOTH_WORK(L) >= 2^31.  L = 0 or F = 0 is a no-op that returns
 * 0.  No allocation, no synchronisation.  The launches go to `hip_stream`, as for mmmot_gate_links. */
#define MMMOT_SMOOTH_WORK(L) (75 * (long)(L) + 2)
int mmmot_smooth_tracks(const float* det, const int* ids, const int* frame_start, const int* frame_no,
                        const int* seq_start, const int* observed, const double* xf0, int L, int F, int S, double q_loc,
                        double r_loc, double v0_loc, double q_yaw, double r_yaw, double v0_yaw, double q_dim,
                        double r_dim, int yaw_flip, int* work, float* out, float* out_vel, int* info, void* hip_stream);

/* ---------------------------------------------------------------------------
 * Tracklet stitching (csrc/stitch_tracks.hip; DESIGN section 12c, which states the order of every operation), additive
 * in ABI 10: every track of a sequence is one node; the tail of a track is joined to the head of a later one when a
 * constant-velocity prediction reaches it, one to one by the exact solver of mmmot_associate_pairs, and the joined
 * tracks take the ID of the first.  Seven launches and the solver's, whatever the rows, frames, sequences and tracks.
 *   det, ids, frame_start, frame_no, seq_start: the tables of mmmot_fill_tracks
 *   vel         [L][4] fp32 or NULL: vx, vy, vz per frame number in the row's own frame's axes (out_vel of
 *               mmmot_smooth_tracks); word 3 is not read
 *   xf0         [F][MMMOT_FILL_REC] fp64 or NULL (a standing camera): the records of mmmot_smooth_tracks; only words
 *               0..15, C[a<-p], are read
 *   k_start     [S+1]: prefix table of the tracks per sequence, counted on the host; k_start[S] = n_tracks
 *   pairs       [S][4] = (K_s, K_s, 2 k_start[s], sum of K^2 of the sequences before s): the pair table of
 *               mmmot_associate_pairs over the link blocks; n_link = the sum over all sequences
 *   r2, inv_r2  [2][max_dt+1] fp64, host-made: row 0 (drift dt + slack)^2, row 1 (max_speed dt + slack)^2, and the
 *               reciprocals; entry 0 is never read
 *   max_k       the largest K_s; the solver is launched for min(max_k, MMMOT_STITCH_MAXK)
 *   work        [MMMOT_STITCH_WORK(L, F, S, n_tracks, n_link)] ints of scratch, 8-byte aligned
 *   out_ids     [L]: the ID of the root of the row's chain of tracks; rows with ID < 0 are copied
 *   next        [L]: for a matched tail row the flat index of the head row it was joined to, else -1
 *   links       [n_link] fp32: per sequence the [K_s][K_s] scores, tails on rows, heads on columns, at its link offset
 *   objective   [S] fp64 from the solver: the sum of the kept scores; NaN for K_s = 0 or a status
 *   info        [S][4] out: status, K_s, stitches, rows whose ID changed
 * A track is the rows of one sequence with the same ID >= 0 in listed-frame order, its head the first and its tail the
 * last; tracks are numbered by the ascending flat row index of their heads.  With M = words 0..15 of the row's frame's
 * record, P_j = ((x M[0][j] + y M[1][j]) + z M[2][j]) + M[3][j] and V_j = (vx M[0][j] + vy M[1][j]) + vz M[2][j] (the
 * fp32 values as fp64 when xf0 is NULL).  A track has a velocity iff vel is given and it has >= min_rows rows.
 * Candidate (i, j): dt = frame_no[head_j] - frame_no[tail_i], d = (double)dt; absent unless min_dt <= dt <= max_dt.
 * Errors e0 e0 + e2 e2 (mode 0), + e1 e1 last (mode 1), of ef: Ph - (Pt + d Vt); eb: Pt - (Ph - d Vh); es: Ph - Pt.
 * Both have a velocity: passes iff ef <= r2[0][dt] and eb <= r2[0][dt], d2 = eb > ef ? eb : ef; only the tail: d2 = ef
 * against row 0; only the head: d2 = eb against row 0; neither: d2 = es against row 1; with max_size_ratio > 0 also the
 * size test of mmmot_gate_links on the tail's and the head's h w l.  Every comparison fails on a NaN operand.  Score
 * (float)((1.0 - d2 inv_r2[m][dt]) - gap_penalty (d - 1.0)), every operator rounded on its own; an absent link is the
 * quiet NaN 0x7fc00000.  The solver keeps the maximum-weight matching of the links with a score > 0.
 * Status, per sequence, never a fault: MMMOT_FILL_EDUP / MMMOT_FILL_ECONTRACT as for mmmot_fill_tracks; ECONTRACT also
 * when the device counts another number of heads than k_start holds, or more than max_k; MMMOT_STITCH_ETOOMANY for more
 * than MMMOT_STITCH_MAXK tracks.  With a status out_ids = ids, next = -1, the link block is all NaN, the objective NaN,
 * info = status, 0, 0, 0.  A frame_start / seq_start that breaks its shape gives every sequence ECONTRACT and nothing
 * is read through them; so does a k_start / pairs that is not the table above (then all of links is NaN).
 * Returns MMMOT_EINVAL before any launch for S < 1, a negative L / F / n_tracks / n_link / max_k, min_dt < 1, max_dt <
 * min_dt or > MMMOT_STITCH_MAX_DT, a mode outside {0, 1}, min_rows < 1, a negative or NaN max_size_ratio or
 * gap_penalty and, with L > 0 and F > 0, a null pointer (vel and xf0 may be null), a work that is not 8-byte aligned
 * or MMMOT_STITCH_WORK(..) >= 2^31.  L = 0 or F = 0 is a no-op that returns 0.  No allocation, no synchronisation.
 * The launches go to `hip_stream`, as for mmmot_gate_links. */
#define MMMOT_STITCH_MAXK 512
#define MMMOT_STITCH_MAX_DT 256
#define MMMOT_STITCH_ETOOMANY 8
#define MMMOT_STITCH_WORK(L, F, S, T, NL) (4 * (long)(L) + (long)(F) + 5 * (long)(S) + 39 * (long)(T) + (long)(NL) + 2)
int mmmot_stitch_tracks(const float* det, const int* ids, const int* frame_start, const int* frame_no,
                        const int* seq_start, const float* vel, const double* xf0, const int* k_start,
                        const int* pairs, const double* r2, const double* inv_r2, int L, int F, int S, int n_tracks,
                        long n_link, int max_k, int min_dt, int max_dt, int min_rows, int mode, double max_size_ratio,
                        double gap_penalty, int* work, int* out_ids, int* next, float* links, double* objective,
                        int* info, void* hip_stream);

/* ---------------------------------------------------------------------------
 * Motion gate of links (csrc/gate_links.hip; DESIGN section 11, "Sequences: motion gate"), additive in ABI 10: a link
 * whose two 3D boxes lie further apart than an object travels in the elapsed frames is written as a quiet NaN, which
 * mmmot_associate, the chain entries and the sequence entries read as an absent edge.  ONE launch whatever NB, F and
 * the frame sizes; one workgroup per block.
 *   det         [L][12] fp32, the rows of mmmot_fill_tracks (read: h w l at 4..6, x y z at 7..9)
 *   frame_start [F+1], frame_no [F]: as for mmmot_fill_tracks; the frames of many sequences may follow each other
 *   blocks      [NB][4] = (frame a, frame b, link offset, 0): the n_a x n_b links from the detections of frame a to
 *               those of frame b, row-major at link + offset.  A pair is one block, a window its consecutive pairs, a
 *               sequence with skip links the gap-by-gap layout of mmmot_associate_sequences_gap
 *   xf          [F][rec_gaps][MMMOT_FILL_REC] fp64 or NULL (a standing camera); only words 0..15 of record (a, b-a-1)
 *               are read: C[a<-b], the row-vector 4x4 of mmmot_fill_tracks
 *   r2, inv_r2  [max_dt+1] fp64, host-made: r2[dt] = (max_speed * dt + slack)^2 and its reciprocal
 *   link        [n_link] fp32 or NULL (count-only: only kept is written);  out_link [n_link], NULL iff link is NULL; it
 *               may be link itself
 *   kept        [NB] out: the links of the block that passed (with link: and whose score is no NaN); -1 = broken block
 * For detection j of frame a and k of frame b, dt = frame_no[b] - frame_no[a], all in fp64, every product and sum
 * rounded on its own: p = (x_k, y_k, z_k, 1) C, columns 0..2 summed in order as in mmmot_align_points (skipped when xf
 * is NULL); d = loc_j - p; d2 = dx dx + dz dz (mode 0, the camera's ground plane), + dy dy last (mode 1).  The link
 * passes iff dt <= max_dt, d2 <= r2[dt] and - with max_size_ratio > 0 - for each of h, w, l max(a, b) <= max_size_ratio
 * * min(a, b) (fp64; max / min by a > b); every comparison fails on a NaN operand.  A passing score is copied bit for
 * bit when weight == 0, else it becomes (float)((double)s - weight * (d2 * inv_r2[dt])); a NaN score is copied as it
 * is and not counted; a gated link is written as the quiet NaN 0x7fc00000.
 * A block is broken - kept = -1, nothing else of it read or written - when a >= b, a frame index lies outside [0, F),
 * frame_no[b] <= frame_no[a], with records b - a > rec_gaps, the offset is negative or the link range reaches past
 * n_link, or frame_start leaves [0, L] or decreases at a or b.  Returns MMMOT_EINVAL before any launch for a negative
 * NB / L / F / n_link, max_dt outside [1, MMMOT_GATE_MAX_DT], a mode outside {0, 1}, a max_size_ratio or weight that
 * is negative or NaN, link NULL and out_link not (or the reverse), xf with rec_gaps < 1 and, with NB > 0, a null table
 * (det may be null with L = 0).  NB = 0 is a no-op that returns 0.  No allocation, no synchronisation.  The launch
 * goes to `hip_stream`, a hipStream_t the caller passes itself (the Python binding appends the current stream only to
 * the 82 entries whose last parameter is named `stream`, a set tests/test_abi_parse_cpu.py pins). */
#define MMMOT_GATE_MAX_DT 64
int mmmot_gate_links(const float* det, const int* frame_start, const int* frame_no, const int* blocks,
                     const double* xf, const double* r2, const double* inv_r2, const float* link, float* out_link,
                     int* kept, int L, int F, int NB, int rec_gaps, long n_link, int mode, int max_dt,
                     double max_size_ratio, double weight, void* hip_stream);

/* ---------------------------------------------------------------------------
 * Per-detection image preparation: crop with zero padding -> antialiased bilinear
 * resize to S x S -> to_tensor -> normalize = the model input ``dets`` [N][3][S][S].  Replaces, per
 * detection, PIL img.crop(box).resize((S, S), Image.BILINEAR) + torchvision ToTensor/Normalize
 * (reference dataset/test_seq_dataset.py:212-218, utils/build_util.py:111-112,137-142) with Pillow's
 * arithmetic (Resample.c: double-precision triangle coefficients, 22-bit fixed point, two passes with an
 * 8-bit intermediate): the uint8 image and the float32 tensor are bit-identical to that pipeline.
 *   img   [H][W][3] uint8 (RGB frame, device)      boxes [N][4] int (x1, y1, x2, y2), may leave the frame
 *   kmax  >= 2*ceil(max(1, max box extent / S)) + 1 (coefficients per output index)
 *   mean_std [6] floats (mean rgb, std rgb)          work  N*2*S*(2+kmax) ints (scratch)
 *   out   [N][3][S][S] fp32                           out_u8 [N][S][S][3] uint8 or NULL (the resized image)
 * S <= 256. */
/* out (fp32 model input) or out_u8 may be NULL (not both).  mmmot_u8_normalize: ToTensor + Normalize of 8-bit crops
 * [N][S][S][3] -> fp32 [N][3][S][S] for the paths that cannot take bytes (exact-fp32 trunk, unfused first layer). */
int mmmot_u8_normalize(const unsigned char* u8, int N, int S, const float* mean_std, float* out, void* stream);
int mmmot_crop_resize_norm(const unsigned char* img, int H, int W, const int* boxes, int N, int S, int kmax,
                           const float* mean_std, int* work, float* out, unsigned char* out_u8, void* stream);

/* The crops of NI images in ONE launch pair (additive in ABI 10): mmmot_crop_resize_norm with the image behind a table.
 *   images [NI][4] int64, device: per image (device address of its uint8 pixels, H, W, row pitch in bytes >= 3 W);
 *   img_of [N] int32, device: crop n is cut from image img_of[n];
 *   boxes / S / mean_std / out / out_u8 as above, crop after crop in the order of `boxes`;
 *   kmax and work (N*2*S*(2+kmax) ints) sized for the LARGEST box of the launch.
 * The arithmetic is that of the single form (one coefficient routine, one pixel routine): out and out_u8 are bit-identical
 * to NI calls of it, concatenated.  The table lives on the device, so its contents are the caller's to validate; a crop
 * whose img_of lies outside [0, NI) is skipped by the kernel (its output is not written).  N = 0 is a no-op that returns
 * 0.  MMMOT_EINVAL before any launch: a null pointer (both outputs NULL), NI < 1, N < 0, S outside [1, 256], kmax < 3. */
int mmmot_crop_resize_norm_multi(const long long* images, int NI, const int* img_of, const int* boxes, int N, int S,
                                 int kmax, const float* mean_std, int* work, float* out, unsigned char* out_u8,
                                 void* stream);

/* Training augmentation of those 8-bit crops (reference utils/build_util.py:110-144 train_transform behind
 * dataset/patchwise_dataset.py:161-171): per crop torchvision's resized_crop(img, top, left, h, w, (S, S), BILINEAR) -
 * for a PIL image img.crop((left, top, left + w, top + h)).resize((S, S), BILINEAR) - then hflip when flip is set
 * (out[.., x] = res[.., S - 1 - x]), then to_tensor + normalize.  Pillow's arithmetic as above; the region lies inside
 * the crop, so there is no padding and at most 3 taps per output index.  One launch for all L crops, no scratch.
 *   crops_u8 [L][S][S][3] uint8 (out_u8 of mmmot_crop_resize_norm)
 *   params   [L][5] int, device: top, left, h, w, flip (0 | 1) with 0 <= top, 1 <= h, top + h <= S, the same for
 *            left / w.  The caller validates the table; the kernel clamps a region to the crop all the same.
 *   mean_std [6] floats (needed with out)
 *   out      [L][3][S][S] fp32 model input, or NULL      out_u8 [L][S][S][3] the augmented 8-bit crop, or NULL (not both)
 * MMMOT_EINVAL before any launch: crops_u8 or params NULL, both outputs NULL, L < 1, S < 1 or S > 256. */
int mmmot_crop_augment(const unsigned char* crops_u8, const int* params, int L, int S, const float* mean_std,
                       float* out, unsigned char* out_u8, void* stream);

/* ---------------------------------------------------------------------------
 * Training backward of the pairwise block (first slice; ABI 5): gradients of
 * affinity_module.forward + NewEndIndicator_v2.forward + the softmax modes of TrackingNet.associate
 * (reference modules/gcn.py:68-82, new_end.py:62-82, tracking_net.py:106-126; the step that needs them is
 * tracking_model.py:50-66: forward -> loss -> backward).  Per layer  y = A W^T + b, yhat = (y - mean) rstd,
 * z = yhat gamma + beta, a = relu(z):
 *   dz = dA [z > 0];  dgamma = sum_r dz yhat;  dbeta = sum_r dz;  dy = rstd (gamma dz - m1 - yhat m2);
 *   dA_in = dy W (mmmot_gemm_rows with W^T);  dW = dy^T A_in, db = sum_r dy (mmmot_gemm_tn).
 * yhat is recomputed from the stored pre-norm y with sc1 = rstd, sh1 = -mean rstd, i.e. the output of
 * mmmot_gn_finalize called with gamma = 1, beta = 0.  All fp32 (exact fp32 MFMA in mmmot_gemm_tn).
 * ------------------------------------------------------------------------- */
/* pass 1: P[t][0][c] = sum over the rows of tile t of dz, P[t][1][c] = sum of dz*yhat  (P is [T][2][C]) */
int mmmot_gn_bwd_partial(const float* dA, int ldda, const float* Y, int ldy, int C, const float* sc1,
                         const float* sh1, int ldsc, const float* gamma, const float* beta, int relu,
                         const int* tile_row0, const int* tile_nrows, const int* tile_group, int T, float* P,
                         void* stream);
/* pass 2: S [G][2][C] = sums of P over the tiles of each group (mmmot_segment_mean with divisor 1) ->
 * M [G][2][C]: m1 = sum_{c in norm group} gamma_c S[g][0][c] / cnt, m2 likewise from S[g][1], broadcast to the
 * channels of the norm group; cnt = grp_count[g] * C / NG. */
int mmmot_gn_bwd_finalize(const float* S, const int* grp_count, int G, int C, int NG, const float* gamma, float* M,
                          void* stream);
/* pass 3: dY[r][c] = sc1[g][c] * (gamma_c dz - M[g][0][c] - yhat M[g][1][c]) */
int mmmot_gn_bwd_apply(const float* dA, int ldda, const float* Y, int ldy, int C, const float* sc1, const float* sh1,
                       int ldsc, const float* gamma, const float* beta, int relu, const float* M,
                       const int* tile_row0, const int* tile_nrows, const int* tile_group, int T, float* dY, int lddy,
                       void* stream);
/* dW[n][k] = sum_r dY[r][n] * A(r,k), db[n] = sum_r dY[r][n]; A(r,k) is regenerated like the forward's A operand
 * (MMMOT_A_PLAIN / MMMOT_A_NORM_RELU / MMMOT_A_PAIR).  N % 64 == 0, K % 64 == 0.  Deterministic (row split with
 * per-share partial outputs, no atomics). */
typedef struct mmmot_gemm_tn_args {
  const float* dY; int lddy;            /* [rows][N] gradient of the layer's pre-norm output */
  const float* X; int ldx;              /* PLAIN / NORM_RELU source rows                      */
  const float* sc; const float* sh; int ldsc;
  const float* FA; const float* FB; int ldf;   /* PAIR operands                               */
  const int* tile_row0; const int* tile_nrows; const int* tile_group;
  const int* grp_row0; const int* grp_M; const int* grp_aoff; const int* grp_boff;
  int T; int N; int K; int amode; int pairop;
  int nsplit;                           /* >= 1: the tiles are split into nsplit contiguous shares, share s writes
                                           its partial sums to dW + s*N*K and db + s*N (the caller adds them up)   */
  float* dW;                            /* [nsplit][N][K]                                     */
  float* db;                            /* [nsplit][N] or NULL                                */
} mmmot_gemm_tn_args;
int mmmot_gemm_tn(const mmmot_gemm_tn_args* a, void* stream);
/* mmmot_gemm_tn on the fp16 matrix cores (3-term hi/lo split, fp32 accumulation; csrc/gemm_tn_f16.hip): same arguments
 * and results contract (tiles of at most 128 rows).  dyamax: device pointer to max |dY| (mmmot_absmax below) - dY is
 * scaled by the power of two that puts its maximum at 2^10 before the fp16 split (gradients of 1e-6 would otherwise sit
 * in fp16's subnormals) and the result scaled back exactly; NULL = no scaling. */
int mmmot_gemm_tn_f16(const mmmot_gemm_tn_args* a, const float* dyamax, void* stream);
/* *out (one device float) = max |X[r][c]| over a [R][C] tensor with row stride ld; C % 4 == 0.  Asynchronous. */
int mmmot_absmax(const float* X, int ld, long R, int C, float* out, void* stream);
/* backward of the pairwise operand generation (gcn.py:6-41): side 0 accumulates d op / d a over j into
 * dF[aoff[g] + i], side 1 d op / d b over i into dF[boff[g] + j]; one workgroup per entry of (blk_group, blk_idx)
 * = every (group, i) resp. (group, j); dF is accumulated into (+=), rows of one launch are distinct. */
int mmmot_pair_bwd(const float* dX, int lddx, const float* F, int ldf, float* dF, int lddf, int C,
                   const int* grp_row0, const int* grp_N, const int* grp_M, const int* grp_aoff,
                   const int* grp_boff, const int* blk_group, const int* blk_idx, int nblk, int pairop, int side,
                   void* stream);
/* backward of the strided means that make the new / end vectors (new_end.py:70-71):
 * dA[(g,i,j)][c] = dV[vrow0[g] + j][c] / N + dV[vrow0[g] + M + i][c] / M */
int mmmot_pair_expand_bwd(const float* dV, int lddv, float* dA, int ldda, int C, const int* tile_row0,
                          const int* tile_nrows, const int* tile_group, int T, const int* grp_row0,
                          const int* grp_N, const int* grp_M, const int* grp_vrow0, void* stream);
/* end_mode 'max' (new_end.py:72-74; additive, still ABI 10): the backward of the strided MAXIMA that make the new / end
 * vectors, in two launches.  The forward (mmmot_segment_mean, flag bit 1) records nothing; the indices are recomputed.
 * mmmot_segment_argmax: idx_out[s][c] (int32, row stride ldo) = the FIRST t in [0, count[s]) that attains
 *   max_t a(t),  a(t) = f(X[start[s] + t*stride[s]][c]),  f = the affine (sc / sh, may both be NULL) and ReLU (relu = 1)
 * of mmmot_segment_mean in the same fmaf / fmaxf form: a(idx) is bit-equal to what the forward wrote.  First maximum is
 * torch's rule for max(dim), which the reference differentiates through.  fp32 rows only; segment tables and the
 * count[s] >= 1 contract as for mmmot_segment_mean.  MMMOT_EINVAL before any launch: X / seg_start / seg_count / idx_out
 * NULL, nseg <= 0, C <= 0 or C % 4, a leading dimension that is no multiple of 4 or below C, a pointer off 16 bytes,
 * only one of sc / sh, relu outside 0 / 1. */
int mmmot_segment_argmax(const float* X, int ldx, int C, const int* seg_start, const int* seg_count,
                         const int* seg_stride, const int* seg_group, int nseg, const float* sc, const float* sh,
                         int ldsc, int relu, int* idx_out, int ldo, void* stream);
/* mmmot_pair_expand_max_bwd: the counterpart of mmmot_pair_expand_bwd (same tile and group tables; idx = the table of
 * mmmot_segment_argmax over plan.v_segs, rows as dV):
 *   dA[(g,i,j)][c] = (idx[vrow0[g] + j][c] == i ? dV[vrow0[g] + j][c] : 0)
 *                  + (idx[vrow0[g] + M + i][c] == j ? dV[vrow0[g] + M + i][c] : 0)
 * Every element of dA is written exactly once (no zero-fill, no atomics): deterministic.  C % 4 == 0. */
int mmmot_pair_expand_max_bwd(const float* dV, int lddv, const int* idx, int ldi, float* dA, int ldda, int C,
                              const int* tile_row0, const int* tile_nrows, const int* tile_group, int T,
                              const int* grp_row0, const int* grp_N, const int* grp_M, const int* grp_vrow0,
                              void* stream);
/* backward of mmmot_rowdot (a = relu(X*sc + sh), act NONE or SIGMOID): gpre[r] = gout[gidx ? gidx[r] : r] * act';
 * dA[r][k] = gpre[r] w[k]; PW[t][k] = sum_{r in tile t} gpre[r] a(r,k) (k < K), PW[t][K] = sum_r gpre[r]. */
int mmmot_rowdot_bwd(const float* X, int ldx, int K, const float* w, float b, const float* sc, const float* sh,
                     int ldsc, const int* tile_row0, const int* tile_nrows, const int* tile_group, int T, int act,
                     const float* gout, const int* gidx, float* dA, int ldda, float* PW, int ldpw, void* stream);
/* backward of mmmot_softmax_pairs: dlogits from dout, the row / column softmaxes are recomputed from the logits */
int mmmot_softmax_pairs_bwd(const float* logits, const float* dout, float* dlogits, const int* grp_row0,
                            const int* grp_N, const int* grp_M, int G, int max_nm, int mode, void* stream);

/* backward of the fusion module C combine (fusion_net.py:31-42; Y_j = [gate_j | input_j] rows as in the forward):
 * DY_j[:, 0:C] = dL/d gate pre-activation, DN_j = dL/d normalised input (goes through mmmot_gn_bwd_* with relu = 0
 * into DY_j[:, C:2C]).  Modes A / B need no kernel (dn = dfused). */
int mmmot_fusion_c_bwd(const float* dFu, const float* Y0, int ld0, const float* Y1, int ld1, const float* sc0,
                       const float* sh0, const float* sc1, const float* sh1, int ldsc, const int* tile_row0,
                       const int* tile_nrows, const int* tile_group, int T, float* DY0, float* DY1, int lddy,
                       float* DN0, float* DN1, int C, void* stream);
/* Y[r][c] = A[r][c] + B[r][c] (two gradient paths into one feature); C % 4 == 0 */
int mmmot_add_rows(const float* A, int lda, const float* B, int ldb, float* Y, int ldy, long R, int C, void* stream);

/* ---------------------------------------------------------------------------
 * Training step, second slice (ABI 6, additive): LiDAR-encoder backward helpers and the loss (csrc/train.hip).
 *
 * mmmot_rows_gather_scale: backward of the per-detection average pools of PointNet (reference
 * modules/point_net.py:32-39 and 139-148: `avg_pool(x[:, :, start:end])`, for conv5 followed by `.repeat` back to the
 * points): X[r][c] = S[rowidx[r]][c] * scale[rowidx[r]]  (scale = 1 / points of the detection; NULL = 1).  C % 4 == 0. */
int mmmot_rows_gather_scale(const float* S, int lds, const int* rowidx, const float* scale, float* X, int ldx, long R,
                            int C, void* stream);
/* ---- third slice: the VGG16-BN trunk in TRAINING mode (reference modules/vgg.py:67-80 under .train(): BatchNorm2d on
 * the statistics of the batch) and its backward; fp32 NHWC, exact fp32 matrix cores (conv3x3.hip, csrc/train_vgg.hip) ----
 * mmmot_conv3x3_raw: out = conv3x3(in, wp) + bias (no BatchNorm fold, no ReLU); layouts of mmmot_conv3x3_bn_relu.  Also
 * the input gradient of a layer: in = dZ, wp = the layer's weights with taps flipped and Cin / Cout swapped, bias = 0. */
int mmmot_conv3x3_raw(const float* in, const float* wp, const float* bias, float* out, int L, int H, int W, int Cin,
                      int Cout, int first, void* stream);
/* per-tile statistics of an existing tensor: part[t][0][c] = sum_r Y[r][c], part[t][1][c] = sum_r (Y[r][c] - tile mean)^2
 * (the `part` contract of mmmot_gemm_rows; input of mmmot_gn_finalize).  C % 4 == 0. */
int mmmot_rows_stats(const float* Y, int ldy, int C, const int* tile_row0, const int* tile_nrows, int T, float* part,
                     void* stream);
/* A = relu(Z * sc + sh) per channel (sc / sh [C]: the batch statistics folded by mmmot_gn_finalize), followed by the
 * 2x2 / stride-2 max-pool with floor semantics when pool != 0.  Z NHWC [L][H][W][C] -> A [L][H >> pool][W >> pool][C]. */
int mmmot_bn_relu_pool(const float* Z, int C, const float* sc, const float* sh, int L, int H, int W, int pool, float* A,
                       void* stream);
/* backward of that max-pool: dA [L][H][W][C] = dP of the window at the window's first maximum of relu(Z * sc + sh)
 * (PyTorch's tie rule), zero elsewhere (odd maps: the last row / column belongs to no window). */
int mmmot_maxpool_bwd(const float* Z, int C, const float* sc, const float* sh, const float* dP, int L, int H, int W,
                      float* dA, void* stream);
/* weight gradient of a 3x3 convolution: dW[s][tap][co][ci] = sum over share s of the pixels of dZ[p][co] * A[p + off(tap)][ci]
 * (zero padding); nsplit shares, the caller adds them.  Cin % 64 == 0, Cout % 64 == 0. */
int mmmot_conv3x3_wgrad(const float* dZ, const float* A, int L, int H, int W, int Cin, int Cout, int nsplit, float* dW,
                        void* stream);
/* ABI 7.  The same weight gradient on the fp16 matrix cores (3-term hi/lo split, the pixel axis as the K of the MFMA like
 * mmmot_gemm_tn_f16): dZ is scaled by the power of two that puts dzamax[0] = max |dZ| (device scalar, mmmot_absmax; NULL =
 * no scaling) at 2^10 and the result scaled back exactly.  Same output layout; fp32-class (products exact to 2^-22).
 * Since round 6 a workgroup owns a (channel-tile pair, tap ROW, share): nsplit such that (Cout/T)(Cin/T) * 3 * nsplit fills
 * the CUs once (T = 128 where the channel count allows, else 64) is the fast choice (mmmot_amd/train_vgg.py:_wgrad_shares);
 * a share sums 64-pixel chunks in fp32 on the matrix cores' accumulators. */
int mmmot_conv3x3_wgrad_f16(const float* dZ, const float* A, int L, int H, int W, int Cin, int Cout, int nsplit, float* dW,
                            const float* dzamax, void* stream);
/* first layer (NCHW crops X [L][3][H][W], Cout = 64): PW[b][co][28] partial sums over block b's pixels of
 * (dW1[co][k = tap * 3 + colour], k < 27 | db1[co]); the caller adds the nblocks partials. */
int mmmot_conv3x3_first_wgrad(const float* dZ, const float* X, int L, int H, int W, float* PW, int nblocks, void* stream);
/* weight / bias gradient of PointNetfeatGN.conv1 with the first transform folded in (forward: mmmot_pointnet_layer1;
 * reference modules/point_net.py:119-125): per-tile partials PW[t][c * (K + 1) + k] = sum_r dY[r][c] X[r][k] (k < K),
 * [..][K] = sum_r dY[r][c]; dY [P][64], X [P][K], K = 3 | 4.  The caller adds the T partial rows. */
int mmmot_pointnet_layer1_bwd(const float* dY, const float* X, int K, const int* tile_row0, const int* tile_nrows, int T,
                              float* PW, void* stream);
/* One term of TrackingLoss (reference cost.py:134-185: DetLoss :97-131 on det / new / end scores, LinkLoss :66-94 on a
 * link block) with its gradient: x [R][C] scores (R modality rows), y [C] target shared by the rows, mask
 * m(c) = mr(mrow[c / M]) * mc(mcol[c % M]) (NULL vectors: 1) with mask_mode 1: v == 1 (LinkLoss' `gt_det == 1`),
 * 2: v != ignore (DetLoss' ignore_index), 0: no mask.  g[r][c] = scale * dl/dx, PL[b] = scale * sum of l over block b's
 * elements (b < nblocks), added to the value PL[b] holds when accumulate != 0 (one block: the terms of a loss add up in
 * PL[0], launch after launch on one stream); scale = ratio / (R * C) reproduces the reference's reduction='mean'. */
int mmmot_score_loss(const float* x, int ldx, const float* y, const float* mrow, const float* mcol, int M, int mask_mode,
                     float ignore, int kind, float scale, int R, int C, float* g, int ldg, float* PL, int nblocks,
                     int accumulate, void* stream);
/* ABI 9.  The 'ghm' type of DetLoss (reference cost.py:105-110,126-128 -> modules/ghm_loss.py:15-61, GHMC_Loss):
 * gradient-harmonised BCE-with-logits of x [R][C] against y [C] (shared by the R rows), entries with y == ignore masked.
 * |sigmoid(x) - y| of the valid elements is histogrammed over `bins` (<= 64) equal bins of [0, 1]; acc_sum [bins]
 * (float64, device) is the module's running state, updated in place: acc <- momentum * acc + (1 - momentum) * count for
 * every non-empty bin (momentum == 0: acc = count, acc_sum untouched); weight = float(tot / acc) / (non-empty bins),
 * tot = max(valid elements, 1).  g[r][c] = scale * w * (sigmoid(x) - y) / tot (weights are constants of the graph),
 * PL[0] (+)= scale * sum(w * bce) / tot (accumulate != 0: added, like mmmot_score_loss).  One workgroup; R * C <= 2^24.
 * momentum travels as fp32 and is widened to float64 on the device: bit-faithful to the
 * reference's Python-float arithmetic for values fp32 represents exactly (the reference's hard-wired 0.75); any other value
 * (0.9, say) differs from it by ~1e-8 relative per step. */
int mmmot_ghm_loss(const float* x, int ldx, const float* y, float ignore, float scale, int R, int C, int bins,
                   float momentum, double* acc_sum, float* g, int ldg, float* PL, int accumulate, void* stream);

/* Frame-pair association (reference solvers.py:9-138, ortools_solve with det_split = [N, M]; csrc/assign.hip), exact,
 * additive in ABI 10.  The binary program of the two frames is a maximum-weight bipartite matching: with, in fp64,
 * a_i = det_i + new_i, ua_i = max(0, a_i + end_i) (i < N), b_j = det_{N+j} + end_{N+j}, vb_j = max(0, b_j + new_{N+j})
 * (j < M) and g_ij = link_ij + a_i - ua_i + b_j - vb_j, its optimum is sum ua + sum vb + max over matchings of
 * sum max(g_ij, 0).  One workgroup per pair runs a shortest-augmenting-path assignment with fp64 duals, ties to the
 * smallest index: results are deterministic and do not depend on the pair's place in the batch.
 *   det / new_score / end_score: fp32, pair p's L = N + M scores at [pairs[4p + 2], + L);
 *   link: fp32, pair p's row-major N x M block at pairs[4p + 3];  pairs: int32 [B][4] = (N, M, score offset, link offset);
 *   max_nm >= max over pairs of N and M, 1 <= max_nm <= 512 (LDS sizing; a pair outside [1, max_nm] is not solved and
 *   gets a NaN objective);
 *   out: fp32, pair p's block at out_off[p] = [det L | new L | end L | link N*M], the 0 / 1 values of ortools_solve's
 *   assign_det / assign_new / assign_end / assign_link[0]: a matched (i, j) has det = 1 on both, new_i = end_j = 1,
 *   end_i = new_j = 0, link_ij = 1 (only pairs with g_ij > 0 are matched); an unmatched frame-0 (frame-1) detection has
 *   det = new = end = [ua_i > 0] ([vb_j > 0]);  objective: fp64 [B], the optimum of the program.
 * Scores must be finite (a NaN gain counts as no gain).  Returns MMMOT_EINVAL on a null pointer, B < 1 or max_nm outside
 * [1, 512] before any launch. */
int mmmot_associate_pairs(const float* det, const float* new_score, const float* end_score, const float* link,
                          const int* pairs, int B, int max_nm, float* out, const int* out_off, double* objective,
                          void* stream);
/* tests / A-B: which kernel serves mmmot_associate_pairs - 0 = automatic (max_nm <= 128: one wave with the link block
 * staged in LDS; above: four waves reading it from global memory), 1 / 2 = one / four waves
 * reading global memory, 3 / 4 = one / four waves with the LDS stage (max_nm <= 128, else MMMOT_EINVAL).  Results do not
 * depend on it, bit for bit. */
int mmmot_set_assign_variant(int variant);

/* Association of chains of T >= 2 frames (reference solvers.py:9-138, ortools_solve with any len(det_split);
 * csrc/assign_chain.hip), exact, additive in ABI 10.  The program - binaries det_i / new_i / end_i per detection and
 * link_t[j][k] per adjacent frame pair, maximise the scored sum under end + sum_k link_t[j][k] = det (t < T - 1),
 * new + sum_j link_{t-1}[j][k] = det (t > 0), new = det in frame 0 and end = det in frame T - 1 - is a min-cost flow on
 * the layered network source -> in(v) (-new_v), in(v) -> out(v) (capacity 1, -det_v), out(t, j) -> in(t + 1, k)
 * (-link_t[j][k]), out(v) -> sink (-end_v): a unit of flow is a trajectory.  One workgroup per chain augments along
 * successive shortest paths (Dijkstra on fp64 reduced costs, ties to the smallest node index, in(v) = v, out(v) = L + v,
 * sink = 2L) until the cheapest path gains nothing: results are deterministic and do not depend on the chain's place in
 * the batch.
 *   det / new_score / end_score: fp32, chain c's L = sum n_t scores at [score offset, + L), frame after frame;
 *   link: fp32, chain c's row-major blocks link_0 (n_0 x n_1) .. link_{T-2}, one after the other from its link offset;
 *   chains: int32 [B][MMMOT_CHAIN_ROW] = (T, score offset, link offset, n_0 .. n_7), 2 <= T <= 8, entries past n_{T-1}
 *   ignored; 0 <= n_t <= max_n <= 512 (an empty frame carries no trajectory across it), 1 <= L <= max_L <= 1024 (LDS
 *   sizing; a chain outside these limits is not solved and gets a NaN objective, nothing else of it is written);
 *   out: fp32, chain c's block at out_off[c] = [det L | new L | end L | link_0 | .. | link_{T-2}], the 0 / 1 values of
 *   ortools_solve's assign_det / assign_new / assign_end / assign_link, every element written;
 *   objective: fp64 [B], the optimum of the program.
 * A NaN score means "variable absent" (its edge does not exist); infinite scores are clamped to +-1e30.  Returns
 * MMMOT_EINVAL on a null pointer, B < 1, max_n outside [1, 512], max_L outside [max_n, min(1024, 8 max_n)] before any
 * launch. */
#define MMMOT_CHAIN_MAXT 8
#define MMMOT_CHAIN_ROW (3 + MMMOT_CHAIN_MAXT)
int mmmot_associate_chains(const float* det, const float* new_score, const float* end_score, const float* link,
                           const int* chains, int B, int max_n, int max_L, float* out, const int* out_off,
                           double* objective, void* stream);
/* tests / A-B: which kernel serves mmmot_associate_chains - 0 = automatic (2 max_L + 1 <= 256 nodes: one wave; above:
 * four waves), 1 / 2 = one / four waves.  Results do not depend on it, bit for bit. */
int mmmot_set_chain_variant(int variant);

/* Association of WHOLE sequences (ortools_solve at len(det_split) = the sequence's length; csrc/assign_sequence.hip),
 * exact, additive in ABI 10.  The program and its network are those of mmmot_associate_chains; one workgroup per
 * sequence augments along successive shortest paths, each found by a label-correcting search that alternates a forward
 * sweep over the frames with a backward sweep along the trajectories until a pass lowers no label (true costs, no
 * potentials; ties to the smallest node index, the source first).  Results are deterministic and do not depend on the
 * sequence's place in the batch, on the batch, or on the kernel variant.
 *   det / new_score / end_score: fp32 [n_scores], sequence s's L = sum n_t scores at [score offset, + L);
 *   link: fp32 [n_link], its row-major blocks link_0 (n_0 x n_1) .. link_{T-2} one after the other from its link offset;
 *   seqs: int32 [B][MMMOT_SEQ_ROW] = (T, score offset, link offset, offset of n_0 in nts, output offset, workspace
 *   offset in 8-byte units);  nts: int32 [n_nts], the n_t of every sequence;
 *   limits: 2 <= T <= 4096, 0 <= n_t <= max_n <= 512 (an empty frame carries no trajectory across it), 1 <= L <= max_L
 *   <= 65536, the link scores of a sequence < 2^31 - 1;
 *   out: fp32 [n_out], sequence s's block [det L | new L | end L | link_0 | .. | link_{T-2}] at its output offset, the
 *   0 / 1 values of ortools_solve, every element written;
 *   ids: int32 [n_scores], at the score offset, every element of the sequence written: -1 where det = 0, else the trajectory's number - trajectories are numbered
 *   0, 1, .. in the order of (first frame, detection index);
 *   objective: fp64 [B];  info: int32 [B][4] = (status, trajectories, augmentations, passes);
 *   max_T: the largest T of the launch (the frame starts and link offsets of a sequence are kept in LDS);
 *   ws: workspace of ws_units 8-byte units, 8-byte aligned: per sequence (53 L + 7) / 8 units of search state (labels,
 *   parents, used / pred / succ, a copy of the scores) from its workspace offset - read and written only when the state does not fit LDS.
 * Every loop is bounded by the sizes: augmentations <= L, passes per augmentation <= 2L + 2, path walk <= 2L + 2.  A
 * bound that is hit gives a NaN objective and status MMMOT_SEQ_EAUG / EPASS / EWALK (the block is still written in
 * full, its content is then unspecified); a sequence outside the limits or the buffers gets a NaN objective and
 * MMMOT_SEQ_ECONTRACT, and nothing else of it is read or written.  A NaN score means "variable absent"; infinite scores
 * are clamped to +-1e30.  Returns MMMOT_EINVAL on a null pointer, B < 1, max_T outside [2, 4096], max_n outside [1, 512], max_L
 * outside [1, 65536], a negative size or a misaligned workspace before any launch. */
#define MMMOT_SEQ_ROW 6
#define MMMOT_SEQ_MAXT 4096
#define MMMOT_SEQ_MAXL 65536
#define MMMOT_SEQ_OK 0
#define MMMOT_SEQ_ECONTRACT 1
#define MMMOT_SEQ_EAUG 2
#define MMMOT_SEQ_EPASS 3
#define MMMOT_SEQ_EWALK 4
int mmmot_associate_sequences(const float* det, const float* new_score, const float* end_score, const float* link,
                              const int* seqs, const int* nts, int B, int n_nts, int max_T, int max_n, int max_L,
                              int n_scores, long long n_link, float* out, long long n_out, int* ids, double* objective,
                              int* info, double* ws, long long ws_units, void* stream);
/* tests / A-B: which kernel serves mmmot_associate_sequences - 0 = automatic (state in LDS when max_L <= 2304, one wave
 * when max_n <= 16, else four), 1 / 2 = one / four waves with the state in the workspace, 3 / 4 = one / four waves with
 * the state in LDS (max_L <= 2304, else MMMOT_EINVAL).  Results do not depend on it, bit for bit. */
int mmmot_set_sequence_variant(int variant);

/* Association of whole sequences with SKIP LINKS (csrc/assign_sequence.hip too), exact, additive in ABI 10: the program
 * of mmmot_associate_sequences with link blocks link^g_t (n_t x n_{t+g}) for every gap g = 1 .. max_gap, t = 0 ..
 * T-1-g, so that a trajectory may miss up to max_gap - 1 frames (and may cross an empty frame).  For every detection v
 * of frame t: det_v = new_v + sum_g sum_j link^g_{t-g}[j][v] = end_v + sum_g sum_k link^g_t[v][k], all variables 0 / 1,
 * maximise sum score * variable.  The network gains the arcs out(t, j) -> in(t + g, k); the search is that of
 * mmmot_associate_sequences - a forward sweep relaxes in(k) of frame t over the source and over out(j) of the frames
 * t-1 .. t-max_gap, a backward sweep follows pred, which may lie up to max_gap frames back - with its tie rule (the
 * smallest node index, the source first: the earlier frame wins), its bounds and its status words.  With max_gap = 1 the
 * results are those of mmmot_associate_sequences, bit for bit.  Results are deterministic and do not depend on the
 * sequence's place in the batch, on the batch, or on the kernel variant.
 *   det / new_score / end_score / seqs / nts / ids / objective / info: as mmmot_associate_sequences;
 *   link: fp32 [n_link], from the sequence's link offset its row-major blocks gap by gap: link^1_0 .. link^1_{T-2}, then
 *   link^2_0 .. link^2_{T-3}, .. link^G_0 .. link^G_{T-1-G}; a block with n_t = 0 or n_{t+g} = 0 has no elements;
 *   out: fp32 [n_out], sequence s's block [det L | new L | end L | the link blocks in the order of `link`] at its output
 *   offset, 0 / 1 values, every element written;
 *   limits: those of mmmot_associate_sequences, 1 <= max_gap <= MMMOT_SEQ_MAXGAP, max_gap < T for every sequence, the
 *   link scores of a sequence (all gaps) < 2^31 - 1;
 *   ws: workspace of ws_units 8-byte units, 8-byte aligned: per sequence, from its workspace offset, (max_gap T + 1) / 2
 *   units for the max_gap x T table of block offsets, then (53 L + 7) / 8 units of search state.  The table is read and
 *   written there only when it does not fit LDS beside the frame starts and the state (the dynamic LDS request never
 *   exceeds that of mmmot_associate_sequences), the state only when L > 2304 or the variant says so.
 * A bound that is hit gives a NaN objective and MMMOT_SEQ_EAUG / EPASS / EWALK; a sequence outside the limits or the
 * buffers - max_gap >= T included - gets a NaN objective and MMMOT_SEQ_ECONTRACT, and nothing else of it is read or
 * written.  A NaN score means "variable absent"; infinite scores are clamped to +-1e30.  Returns MMMOT_EINVAL on a null
 * pointer, B < 1, max_T outside [2, 4096], max_n outside [1, 512], max_L outside [1, 65536], max_gap outside [1, 8] or
 * >= max_T, a negative size or a misaligned workspace before any launch. */
#define MMMOT_SEQ_MAXGAP 8
int mmmot_associate_sequences_gap(const float* det, const float* new_score, const float* end_score, const float* link,
                                  const int* seqs, const int* nts, int B, int n_nts, int max_T, int max_n, int max_L,
                                  int max_gap, int n_scores, long long n_link, float* out, long long n_out, int* ids,
                                  double* objective, int* info, double* ws, long long ws_units, void* stream);
/* tests / A-B: which kernel serves mmmot_associate_sequences_gap - the variants of mmmot_set_sequence_variant.  Results
 * do not depend on it, bit for bit. */
int mmmot_set_sequence_gap_variant(int variant);

/* Track IDs from pair assignments (reference tracking_model.py:218-292 assign_det_id, then :109-216 align_id, restated
 * by detection index; csrc/track_ids.hip), additive in ABI 10.  One workgroup walks the B CONSECUTIVE pairs of ONE
 * sequence in order; queued behind mmmot_associate_pairs it reads that call's `out` / `pairs` / `out_off` as they are.
 *   blocks: fp32, pair p's [det L | new L | end L | link N*M] at out_off[p] (0 / 1 values);  pairs: int32 [B][4], only
 *   N and M are read, 0 <= N, M <= max_nm <= 512 (max_nm <= 128: one wave, above: four; same results);
 *   frame_idx: int32 [B][2], the frame indices (>= 0) of each pair's two frames - a stored frame is "the pair's first
 *   frame" when the indices are equal;
 *   state: int32 [MMMOT_TRACK_STATE_INTS], the sequence's state, read and rewritten in full: [0] last_id, [1] index of
 *   the stored frame or -1, [2] error flags (sticky), [3] detections of the stored frame, then its per-detection IDs
 *   (-1: not kept / beyond the frame).  A new sequence starts from {0, -1, 0, 0, -1 ...};
 *   ids_out: int32, pair after pair [ids of frame 0: N | ids of frame 1: M | frame_start | last_id after the pair]: an
 *   ID of -1 marks a detection with assign_det != 1; frame_start = 1 when the stored frame was the pair's first frame
 *   (only the second frame is emitted, as align_id returns it), else 0.
 * A kept second-frame detection with new != 1 must have exactly one link, from a kept row (what a solver output always
 * gives): otherwise it gets -1 and MMMOT_TRACK_EINFEASIBLE is set in state[2].  MMMOT_TRACK_ECONTRACT: a pair outside
 * [0, max_nm] (the walk stops there) or a stored frame whose detection count differs from the pair's first frame.
 * Returns MMMOT_EINVAL on a null pointer, B < 1 or max_nm outside [0, 512] before any launch. */
#define MMMOT_TRACK_STATE_HEAD 4
#define MMMOT_TRACK_STATE_INTS (MMMOT_TRACK_STATE_HEAD + 512)
#define MMMOT_TRACK_EINFEASIBLE 1
#define MMMOT_TRACK_ECONTRACT 2
int mmmot_track_ids(const float* blocks, const int* pairs, const int* out_off, const int* frame_idx, int B, int max_nm,
                    int* state, int* ids_out, void* stream);

/* Track IDs from the assignments of WINDOWS of 2 .. 8 frames (assign_det_id + align_id on len(det_split) frames;
 * csrc/track_ids.hip: the kernel body of mmmot_track_ids on the chain table), additive in ABI 10.  One workgroup walks
 * the B CONSECUTIVE windows of ONE sequence in order;
 * queued behind mmmot_associate_chains it reads that call's `out` / `chains` / `out_off` as they are.
 *   blocks: fp32, window c's [det L | new L | end L | link_0 | .. | link_{T-2}] at out_off[c] (0 / 1 values);
 *   chains: int32 [B][11] (T, score offset, link offset, n_0 .. n_7), only T and n_0 .. n_{T-1} are read, 2 <= T <= 8,
 *   0 <= n_t <= max_n <= 512 (max_n <= 128: one wave, above: four; same results);
 *   frame_idx: int32 [B][8], the frame indices (>= 0) of each window's T frames;
 *   state: the block of mmmot_track_ids, read and rewritten in full - pair and window launches may alternate on it;
 *   ids_out: int32, window after window [ids of all L detections, frame after frame | frame_start | last_id after the
 *   window | stored]: frame_start = 1 when the stored frame was the window's frame 0 (frames 1 .. T-1 are emitted);
 *   stored = 1 when the window's last frame became the stored frame: always unless frame_start = 1 and frame 1 keeps no
 *   detection - then the state keeps its frame (only last_id moves) and the window's frames are NOT part of the tracks,
 *   the reference's behaviour.  For T = 2 the first L + 2 words and the state are those of mmmot_track_ids.
 * A kept detection of a frame t >= 1 with new != 1 must have exactly one link from frame t-1, from a row with an ID:
 * otherwise it gets -1 and MMMOT_TRACK_EINFEASIBLE is set.  MMMOT_TRACK_ECONTRACT: a window outside 2 <= T <= 8,
 * 0 <= n_t <= max_n (the walk stops there) or a stored frame whose detection count differs from the window's frame 0.
 * Returns MMMOT_EINVAL on a null pointer, B < 1 or max_n outside [0, 512] before any launch. */
int mmmot_track_chain_ids(const float* blocks, const int* chains, const int* out_off, const int* frame_idx, int B,
                          int max_n, int* state, int* ids_out, void* stream);

/* The ID step of S sequences in ONE launch (csrc/track_ids.hip: one workgroup per sequence runs the walk of the single
 * forms), additive in ABI 10.  The arguments are those of mmmot_track_ids / mmmot_track_chain_ids, except:
 *   states: int32 [S][MMMOT_TRACK_STATE_INTS], row s the state of sequence s;
 *   seq_start: int32 [S + 1], device: entries [seq_start[s], seq_start[s+1]) of the launch are the CONSECUTIVE pairs
 *   (windows) of sequence s, in order.
 * Contract:
 *   - a sequence with an empty range is neither read nor written;
 *   - error flags are per sequence (word [2] of its row) and sticky, as in the single forms;
 *   - a range that is decreasing or leaves [0, B] sets MMMOT_TRACK_ECONTRACT in that sequence's row: nothing of it is
 *     walked and its ids_out words are not written.  The same holds for a sequence with an entry outside the launch's
 *     limits in FRONT of its range (its place in ids_out cannot be told);
 *   - ids_out has the layout of the single forms, entry after entry in launch order; the words of a sequence depend on
 *     its own entries and state only, never on what the other sequences of the launch hold or do.
 * The wave count follows max_nm / max_n as in the single forms.  Returns MMMOT_EINVAL before any launch for a null
 * pointer, S < 1, B < 1 or max_nm / max_n outside [0, 512]. */
int mmmot_track_ids_multi(const float* blocks, const int* pairs, const int* out_off, const int* frame_idx,
                          const int* seq_start, int S, int B, int max_nm, int* states, int* ids_out, void* stream);
int mmmot_track_chain_ids_multi(const float* blocks, const int* chains, const int* out_off, const int* frame_idx,
                                const int* seq_start, int S, int B, int max_n, int* states, int* ids_out, void* stream);

/* CLEAR-MOT evaluation of tracked sequences (reference kitti_devkit/evaluate_tracking.py:393-792
 * compute3rdPartyMetrics; csrc/clear_mot.hip), additive in ABI 10.  Four launches: one workgroup per frame (Hungarian
 * association of ground truth and tracker boxes on c = 1 - IoU gated at min_overlap, the ignore logic and the per-frame
 * counters), one lane per ground-truth trajectory (ID switches, fragments, MT / PT / ML), one workgroup per sequence and
 * one lane for the totals.  All frames of all S sequences of the call go in one launch.
 *   boxes: fp64 [nG + nT + nD][4] (x1, y1, x2, y2): the ground-truth objects, then the tracker objects, then the
 *   DontCare areas, each frame's contiguous;
 *   frames: int32 [NF][6] = first object and count of the frame in the three sections (g_off, G, t_off, T, d_off, D),
 *   0 <= G, T <= 128, 0 <= D <= 64; a frame outside these limits or the sections gets -1 counters and NaN sums;
 *   g_attr: int32 [nG][3] = truncation, occlusion, class code (1 = the neighbouring class: van / person_sitting);
 *   t_attr: int32 [nT][2] = track ID, class code;
 *   traj_off: int32 [NTr + 1], traj_obj: int32 [nG]: trajectory k's objects in frame order are
 *   traj_obj[traj_off[k] .. traj_off[k + 1]) (indices into the ground-truth section);
 *   seq_off: int32 [S + 1][2] = first frame and first trajectory of each sequence (row S: NF, NTr).
 * Outputs, every element written: frame_d fp64 [NF][2] = sum of 1 - c over the matches, MODP_t; frame_i int32 [NF][6] =
 * tp (ignored ones included), itp, fn, ifn, fp, ignored trackers; gt_out int32 [nG][2] = matched tracker ID or -1,
 * ignored flag; traj_i int32 [NTr][4] = ignored, ID switches, fragments, 0 MT / 1 PT / 2 ML / -1 ignored;
 * seq_d fp64 [S + 1][2] = sum of 1 - c, sum of MODP_t; seq_i int32 [S + 1][12] = tp, itp, fn, ifn, fp, ignored trackers,
 * ID switches, fragments, MT, PT, ML, ignored trajectories; row S holds the totals.  The sums of a sequence do not depend
 * on what else the call holds.  Returns MMMOT_EINVAL on a missing or misaligned pointer, a negative count or S < 1. */
int mmmot_clear_mot(const double* boxes, int nG, int nT, int nD, const int* frames, int NF, const int* g_attr,
                    const int* t_attr, const int* traj_off, const int* traj_obj, int NTr, const int* seq_off, int S,
                    double min_overlap, double min_height, double max_truncation, double max_occlusion,
                    double* frame_d, int* frame_i, int* gt_out, int* traj_i, double* seq_d, int* seq_i, void* stream);

/* HOTA and IDF1 evaluation of tracked sequences (csrc/hota.hip, DESIGN.md section 13 "HOTA / IDF1"; the rules are
 * restated in tests/hota_ref.py), additive in ABI 10.  A fixed number of launches whatever NF and S: one clear of the
 * work tables, the preparation of every frame (one wave per frame), pass 1 (one workgroup per sequence walks its frames
 * in order), pass 2 (one wave per frame), the per-sequence sums, the IDF1 matching (one wave per sequence), the totals.
 *   boxes, frames: as in mmmot_clear_mot (ground truth = every non-DontCare row); frame_seq: int32 [NF] = the frame's
 *   sequence;
 *   g_attr: int32 [nG][4] = truncation, occlusion, class code (0 main, 1 neighbouring), dense ID in [0, G_s) (not read
 *   for the neighbouring class);  t_id: int32 [nT] = dense ID in [0, T_s).  IDs are unique within a frame;
 *   seq_tab: int32 [S + 1][6] = first frame, G_s, T_s, first cell, first gt ID slot, first tracker ID slot (row S: NF, 0,
 *   0, cells, sumG, sumT), G_s, T_s <= 2048, G_s T_s <= 2^18;  cells = sum G_s T_s, sumG = sum G_s, sumT = sum T_s;
 *   max_boxes / max_dontcare: the caller's largest frame (per side / DontCare areas), at most 128 / 64;
 *   prepare: 1 = the KITTI preparation (min_height, max_truncation, max_occlusion), 0 = keep every main-class ground
 *   truth row and every tracker row;
 *   work: 8-byte aligned, work_bytes >= 8 cells + 4 (20 cells + sumG + sumT + nG + nT); cleared by the call.
 * Outputs, every element written: frame_d fp64 [NF][21] = value of the preparation assignment, value of the pass-2
 * assignment, LocSum of the 19 alpha;  frame_i int32 [NF][21] = TP of the 19 alpha, kept ground truth, kept tracker
 * boxes;  seq_d fp64 [S + 1][76] = LocSum[19], sum mc A [19], sum mc mc / max(1, gt_count) [19], sum mc mc / max(1,
 * tr_count) [19] - in row S the last three are the TP-weighted sums  sum_s (x_s / max(1, TP_s)) TP_s;  seq_i int32
 * [S + 1][24] = TP[19], kept ground truth, kept tracker boxes, IDTP, status (0, or -1 when a frame or the sequence lay
 * outside the limits: such a frame gets -1 / NaN rows and nothing of it is read), pad; row S holds the totals.  No
 * floating-point atomics: two calls on the same input return the same bits, and a sequence's values do not depend on
 * what else the call holds.  Returns MMMOT_EINVAL before any launch on a missing or misaligned pointer, a negative
 * count, S < 1, max_boxes > 128, max_dontcare > 64, cells > 2^18 S, sumG or sumT > 2048 S, prepare outside {0, 1} or a
 * work block that is too small. */
int mmmot_hota(const double* boxes, int nG, int nT, int nD, const int* frames, int NF, const int* frame_seq,
               const int* g_attr, const int* t_id, const int* seq_tab, int S, int cells, int sumG, int sumT,
               int max_boxes, int max_dontcare, double min_height, double max_truncation, double max_occlusion,
               int prepare, void* work, long long work_bytes, double* frame_d, int* frame_i, double* seq_d, int* seq_i,
               void* stream);

/* 3D MOT evaluation of tracked sequences: CLEAR-MOT on a rotated-box overlap, and the AMOTA sweep over `levels` score
 * thresholds (csrc/mot3d.hip, DESIGN.md section 13 "3D / AMOTA"; the rules are restated in tests/mot3d_ref.py), additive
 * in ABI 10.  The frame evaluation is the one of mmmot_clear_mot (csrc/cm_search.h) with c = 1 - overlap read from a
 * per-frame table; level l < levels keeps the tracker objects whose track score is >= thr[l], level `levels` keeps all
 * (pass A).  Two phases, because the caller sorts between them:
 *   phase 0: the overlap table, then pass A (frame, trajectory, sequence, total launches) into level `levels` of every
 *   output, and msig fp64 [nG] = the track score of the partner of every ground-truth object that is a true positive and
 *   not ignored, -inf elsewhere (the caller pre-fills it with -inf);
 *   phase 1: msig holds the same values SORTED DESCENDING; one launch writes thr fp64 [levels] (+inf where the level is
 *   unreachable) and reach int32 [levels], then the four launches run with a level dimension into levels 0 .. levels - 1.
 * The launch count depends on neither NF nor S nor levels.
 *   boxes, frames, g_attr, t_attr, traj_off, traj_obj, seq_off and the limits: as in mmmot_clear_mot;
 *   box3d: fp64 [nG + nT][12] = the four footprint corners (x, z), y - h, y, w l, h w l, formed by the caller (not read
 *   in mode 2);  sigma: fp64 [nT] = track score of every tracker object;
 *   cell_off: int32 [NF] = first cell of the frame's [G][T] table, cells = their total < 2^31;  table: fp64 [cells] (work);
 *   mode: 0 = IoU3D, 1 = IoUbev, 2 = the 2D IoU of mmmot_clear_mot;  gate: a cell is valid where c <= gate.
 * Outputs as in mmmot_clear_mot with a leading level axis [levels + 1]: frame_d [..][NF][2], frame_i [..][NF][6], gt_out
 * [..][nG][2], traj_i [..][NTr][4], seq_d [..][S + 1][2], seq_i [..][S + 1][12]; phase 0 writes level `levels` only.  A
 * frame outside the limits, the sections or the table is marked and nothing of it is read.  No floating-point atomics: two
 * calls return the same bits.  Returns MMMOT_EINVAL before any launch on a missing or misaligned pointer, a negative
 * count, S < 1, cells >= 2^31, mode outside 0..2, levels outside 0..1024, phase outside {0, 1} or phase 1 at levels 0. */
int mmmot_mot3d(const double* boxes, const double* box3d, const double* sigma, int nG, int nT, int nD,
                const int* frames, const int* cell_off, int NF, const int* g_attr, const int* t_attr,
                const int* traj_off, const int* traj_obj, int NTr, const int* seq_off, int S, int mode, int levels,
                int phase, double gate, double min_height, double max_truncation, double max_occlusion, double* table,
                long long cells, double* msig, double* frame_d, int* frame_i, int* gt_out, int* traj_i, double* seq_d,
                int* seq_i, double* thr, int* reach, void* stream);

/* Training targets of chains (reference tracking_model.py:294-351, TrackingModule.generate_gt, restated literally;
 * csrc/labels.hip), additive in ABI 10.  One workgroup per chain, ids and classes staged in LDS, every output element
 * written once by a plain store: results are deterministic and do not depend on the chain's place in the batch.
 *   ids / cls: int32, chain c's L = sum n_t values at [score offset, + L), frame after frame;
 *   chains: the int32 [B][MMMOT_CHAIN_ROW] table of mmmot_associate_chains (T, score offset, link offset, n_0 .. n_7; the
 *   link offset is not read), 2 <= T <= 8, 0 <= n_t <= max_n <= 512, 1 <= L <= max_L <= 1024;
 *   out: fp32, chain c's block at out_off[c] = [gt_det L | gt_new L | gt_end L | link_0 | .. | link_{T-2}] (link_t
 *   row-major n_t x n_{t+1}), 0 / 1 values, every element written, zeros included: the caller does not clear it.
 * For detection j of frame t with pos = (cls == 1): gt_det = pos; succ = the smallest k of frame t + 1 with an equal id -
 * by id alone, whatever that detection's class, and -1 equals -1; link_t[j][k] = pos && k == succ; gt_end = pos && (t ==
 * T - 1 || no succ); gt_new = pos && (t == 0 || no equal id in frame t - 1).  An empty neighbour frame matches nothing.
 * A chain outside the limits gets a NaN in the first element of its block (gt_det[0]) and nothing else of it is written.
 * Returns MMMOT_EINVAL on a null pointer, B < 1, max_n outside [1, 512], max_L outside [max_n, min(1024, 8 max_n)] before
 * any launch. */
int mmmot_generate_gt(const int* ids, const int* cls, const int* chains, int B, int max_n, int max_L, float* out,
                      const int* out_off, void* stream);

/* Ground-truth identity and class of every detection (reference dataset/common.py:82-111, generate_det_id_matrix with
 * calculate_distance, restated literally; csrc/labels.hip), NF frames in one launch, one workgroup per frame, additive
 * in ABI 10.
 *   det_xywh / gt_xywh: fp64 [.][4] boxes as x, y, w, h (finite), 8-byte aligned;  gt_id / gt_name: int32 per gt box;
 *   frames: int32 [NF][4] = (det offset, n_det, gt offset, n_gt) in boxes, 0 <= n_det, n_gt <= max_n <= 512;
 *   det_id / det_cls: int32 per detection, written for every detection of every frame.
 * Per (gt i, det d), in fp64 with one IEEE operation per step (no FMA contraction): isect = the product over both axes
 * of max(min(br) - max(tl), 0) with br = tl + size, union = a_gt + a_det - isect, dist = 1 - isect / union; union == 0
 * or dist > max_iou count as 10; the value is rounded to fp32.  Gt i points at arg-min over d of these fp32 values, ties
 * to the smallest d - a gt that overlaps nothing (a row of 10s) points at det 0.  Det d takes the LARGEST i that points
 * at it (the reference overwrites in the order of i): det_id = gt_id[i], det_cls = 1 if gt_name[i] == car_code, -1 if
 * == dontcare_code, else 0; a det nobody points at gets id -1, cls 0 (so n_gt = 0 gives that to every det).  n_det = 0
 * writes nothing; neither does a frame outside the limits or with a negative offset.
 * Returns MMMOT_EINVAL on a null or misaligned pointer, NF < 1 or max_n outside [1, 512] before any launch. */
int mmmot_match_dets(const double* det_xywh, const double* gt_xywh, const int* gt_id, const int* gt_name,
                     const int* frames, int NF, int car_code, int dontcare_code, double max_iou, int max_n, int* det_id,
                     int* det_cls, void* stream);

/* Adam step of every tensor of an optimizer in ONE launch (torch.optim.Adam's single-tensor arithmetic with the fastai
 * OptimWrapper's decoupled decay folded in; csrc/adam_step.hip), additive in ABI 10.
 * Multi-tensor apply: `table` holds one row per tensor, `chunks` one int32 (tensor index, chunk index) row per
 * MMMOT_ADAM_CHUNK elements of a tensor; one workgroup of 256 threads serves one chunk.  With t the tensor's own step
 * count after increment, its row carries (computed in double on the host, rounded to fp32 once)
 *   step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t), decay = 1 - wd*lr (decoupled decay) or 1,
 *   l2 = wd (decay added to the gradient) or 0,
 * and every element goes through, in fp32 with one IEEE operation per step (no FMA contraction):
 *   p = p * decay (skipped when decay == 1);  g' = g + l2 * p (skipped when l2 == 0);  m = m + (1 - beta1) * (g' - m);
 *   v = v * beta2 + (1 - beta2) * g' * g';  p = p - step_size * (m / (sqrt(v) / bc2_sqrt + eps)).
 * A row without MMMOT_ADAM_HAS_GRAD is decayed (p = p * decay) and nothing else of it is read or written.  NaN and Inf
 * propagate.  16-byte loads and stores where the row's four bases are 16-byte aligned (p alone for a row without a
 * gradient), one element per access otherwise.  Every element is read and written by exactly one lane: the result does
 * not depend on the chunk geometry or on the order of either table.  A chunk row that names no tensor of the table or
 * starts behind its tensor's end touches nothing.  The tensors must not overlap.
 * Returns MMMOT_EINVAL before any launch on a null or misaligned table, n_tensors < 1, n_chunks < 1, a beta outside
 * [0, 1), or an eps that is negative, infinite or above FLT_MAX (NaN included for all three). */
#define MMMOT_ADAM_CHUNK 4096
#define MMMOT_ADAM_HAS_GRAD 1
typedef struct mmmot_adam_row {
  float* p;        /* parameter, updated in place */
  const float* g;  /* gradient (not read without MMMOT_ADAM_HAS_GRAD) */
  float* m;        /* exp_avg, updated in place */
  float* v;        /* exp_avg_sq, updated in place */
  long long numel;
  float step_size, bc2_sqrt, decay, l2;
  int flags, reserved;
} mmmot_adam_row; /* 64 bytes */
int mmmot_adam_step(const mmmot_adam_row* table, int n_tensors, const int* chunks, int n_chunks, double beta1,
                    double beta2, double eps, void* stream);
/* MMMOT_ADAM_CHUNK of the library that is loaded. */
int mmmot_adam_chunk_elems(void);
/* The chunk table of mmmot_adam_step for tensors of h_numel[0 .. n_tensors) elements, built on the HOST (h_*: host
 * pointers; it depends on the sizes only - build and upload it once): *h_count = the number of rows, and, when h_chunks
 * is given, cap >= *h_count rows of two int32 are written, tensor after tensor.  h_chunks == NULL (cap 0) asks for the
 * count alone.  Returns MMMOT_EINVAL on a null h_numel / h_count, n_tensors < 1, a numel < 1, cap < the count, or more
 * than 2^31 - 1 rows. */
int mmmot_adam_chunks(const long long* h_numel, int n_tensors, int* h_chunks, long long cap, long long* h_count);

/* ---------------------------------------------------------------------------
 * Dropout of the LiDAR encoder in training mode (reference modules/point_net.py:28-39: nn.Dropout(p) over points x
 * channels between relu(bn1(conv1)) and the per-detection average pool; csrc/dropout.hip),
 * additive in ABI 10.  The mask is generated in registers and never stored:
 *   w = philox4x32_10(counter = (r, c >> 2, 0, 0), key = (seed & 0xffffffff, seed >> 32))    (csrc/philox.h)
 *   keep(r, c) = w[c & 3] >= threshold     (unsigned; threshold = min(round(p * 2^32), 0xFFFFFFFF), 0 keeps everything)
 * for row r (< 2^32) and channel c of a [R][C] tensor - a function of (seed, r, c) alone, whatever the grid.
 *
 * mmmot_segment_mean_dropout: out[s][c] = (1 / seg_count[s]) * sum_t keep(r, c) * scale * relu(X[r][c] * sc[g][c] + sh[g][c])
 * with r = seg_start[s] + t, g = seg_group[s] (NULL: 0); contiguous fp32 rows.  Decomposition and summation order of
 * mmmot_segment_mean: with threshold = 0, scale = 1 it is bit-identical to mmmot_segment_mean(relu = 1).
 * mmmot_rows_gather_scale_dropout: X[r][c] = keep(r, c) * dscale * (S[rowidx[r]][c] * scale[rowidx[r]]) (scale NULL: 1),
 * the inner product as mmmot_rows_gather_scale forms it.
 * mmmot_dropout_mask: out[r][c] = keep(r, c) as a byte, out a contiguous [R][C] array.
 * All three: C % 4 == 0, leading dimensions multiples of 4 and >= C, 16-byte aligned pointers, R < 2^32; MMMOT_EINVAL
 * otherwise.  Nothing is allocated, nothing synchronises. */
int mmmot_segment_mean_dropout(const float* X, int ldx, int C, const int* seg_start, const int* seg_count,
                               const int* seg_group, int nseg, const float* sc, const float* sh, int ldsc,
                               unsigned long long seed, unsigned threshold, float scale, float* out, int ldo,
                               void* stream);
int mmmot_rows_gather_scale_dropout(const float* S, int lds, const int* rowidx, const float* scale, float* X, int ldx,
                                    long R, int C, unsigned long long seed, unsigned threshold, float dscale,
                                    void* stream);
int mmmot_dropout_mask(unsigned long long seed, unsigned threshold, long R, int C, unsigned char* out, void* stream);

/* MFMA fragment-layout self test: C[32][32] = A[32][K] * B[32][K]^T through
 * the same fragment mapping the GEMM kernels use (K % 8 == 0). */
int mmmot_selftest_mfma(const float* A, const float* B, float* C, int K, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMMOT_HIP_H */
