/*
 * libeunet_hip -- C-ABI of the MI355X-native Enhanced-UNet training hot path.
 *
 * Conventions
 *   - Every entry point returns 0 on success or a negative EUNET_ERR_* code;
 *     eunet_last_error() returns the message (thread-local).
 *   - The library never allocates, frees or synchronises: all buffers and
 *     workspaces are owned by the caller (the torch caching allocator in the
 *     Python host); every launch is enqueued on the `stream` argument only
 *     (a hipStream_t passed as void*), so RCCL/DDP stream ordering stays valid.
 *   - Activations are NHWC views (eunet_act); dtype EUNET_F32 or EUNET_BF16.
 *     BatchNorm statistics, losses, weights-for-the-optimizer and all
 *     reductions are fp32 (partials combined in fp64).
 *   - Stateless and re-entrant.
 *
 * The reference exposes this path only as Python (no FFI): each entry point
 * below names the reference call site it replaces (file:line in
 * whh1747012859/Enhanced-UNet).  INTEGRATION.md shows the ctypes binding.
 */
#ifndef EUNET_H
#define EUNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EUNET_OK 0
#define EUNET_ERR_INVALID (-1)
#define EUNET_ERR_HIP (-2)

enum { EUNET_F32 = 0, EUNET_BF16 = 1 };

/* NHWC view: element (n,y,x,c) lives at ptr + ((n*h + y)*w + x)*ctot + coff + c
 *
 * The activation-view contract, checked by every entry point that takes views before it launches
 * anything (a violation returns EUNET_ERR_INVALID and touches no memory):
 *   - a valid view has a non-null ptr, n, h, w, c > 0, 0 <= coff, coff + c <= ctot and dtype EUNET_F32 or
 *     EUNET_BF16 (any other code is refused, also where a function takes a bare dtype argument);
 *   - the views of one call agree in dtype and n, and in h and w up to the factor 2 the op defines (pool,
 *     upsample, upconv), optional (nullable) views included; where channels correspond, in c too.  The
 *     exceptions are stated at the function (eunet_conv3x3_dgrad's fp32 gx, the small-K fp32 path of
 *     eunet_upsample_bwd);
 *   - the ops that move whole 16-byte channel units need c, ctot and coff to be multiples of the unit, 8
 *     (bf16) or 4 (fp32) elements: eunet_conv3x3_*, eunet_conv_small_wgrad (dy), eunet_bnrelu*, the
 *     eunet_bn_bwd_*, eunet_pool_bwd_*, eunet_upsample_bwd* (vector path) and eunet_conv1x1_bwd* families and
 *     the eunet_*upconv2x2_* passes (which also need 16-byte aligned pointers).  eunet_nchw_to_nhwc,
 *     eunet_conv_small_fwd and the fusion entry points take any channel layout their comment allows. */
typedef struct {
  void* ptr;
  int n, h, w;  /* batch, rows, cols */
  int c;        /* channels in this view */
  int ctot;     /* channel stride of the underlying buffer (>= coff + c) */
  int coff;     /* first channel of the view inside the buffer */
  int dtype;    /* EUNET_F32 | EUNET_BF16 */
} eunet_act;

const char* eunet_version(void);
const char* eunet_last_error(void);

/* ---- layout conversion ----------------------------------------------------
 * images.to(device) + NCHW->NHWC (train_eval.py:242); x [N,C,H,W] fp32 */
int eunet_nchw_to_nhwc(const float* x, const eunet_act* out, void* stream);

/* ---- stream ordering (the backward's weight-gradient side stream; no reference counterpart: the
 * reference's backward is one stream, train_eval.py:230-243) -------------------------------------
 * `to` waits for everything enqueued on `from` so far (device-scope event release, no timing).  Both
 * streams must be on one device (any current device of the calling thread). */
int eunet_stream_wait(void* from, void* to);

/* ---- update guard (train_eval.py:325 -> FocalLoss:39: an out-of-range target raises inside the
 * loss of that batch, before its backward and optimizer.step(), so neither that batch nor any later
 * one updates the model) ----------------------------------------------------------------------------
 * guard: a device fp64 word on `device` (null: no guard).  While *guard != 0 at kernel time,
 * eunet_bn_finalize leaves the running statistics and num_batches_tracked untouched and
 * eunet_clip_adamw leaves parameters, gradients, moments and step counters untouched.  The Trainer
 * points it at the loss's out-of-range target counter, so a deferred (sync-free) epoch keeps the
 * reference's state at the raise and raises at its next host synchronisation.  The pointer is read
 * at launch (a captured graph keeps the one it was captured with). */
int eunet_set_update_guard(int device, const double* guard);

/* ---- Conv2d 3x3, padding 1 (models.py:219,222 / autograd) -----------------
 * Weights are re-packed every step from the fp32 torch parameter
 * [Cout][Cin][3][3] into the MFMA-ready layout.  transpose_flip=1 packs the
 * dgrad operand W'[ci][co][8-t] so dgrad runs through the forward kernel. */
int eunet_conv3x3_packed_bytes(int cout, int cin, int dtype, size_t* bytes);
int eunet_conv3x3_pack(const float* w, int cout, int cin, int transpose_flip, void* wp, int dtype,
                       void* stream);
/* up to EUNET_PACK_MAX packs in one launch (a step's forward and dgrad operands: the weights do
 * not change between the forward and the backward); each wp sized by eunet_conv3x3_packed_bytes */
#define EUNET_PACK_MAX 32
typedef struct {
  const float* w;  /* torch [cout][cin][3][3] fp32 */
  int cout, cin, flip;
  void* wp;
} eunet_pack_desc;
int eunet_conv3x3_pack_many(const eunet_pack_desc* descs, int n, int dtype, void* stream);
/* number of pixel tiles = rows of the BatchNorm statistics partial buffer */
int eunet_conv3x3_tiles(const eunet_act* y, int* tiles);
/* y = conv(t(x)) + bias, t = relu(x*in_scale+in_shift) per input channel when
 * in_scale != NULL (the preceding BN+ReLU fused into the operand load, zero
 * padding applied after the transform).  in_nstride = 0: one [cin] scale/shift
 * pair; > 0: per-sample pairs at in_scale + n*in_nstride (a BN+ReLU followed by a
 * Dropout2d keep-mask/(1-p), models.py:287,291, folded into the affine).  stats (nullable): [tiles][2][cout]
 * per-tile (sum, M2) plus [tiles] counts appended after 2*cout*tiles floats. */
int eunet_conv3x3_fwd(const eunet_act* x, const float* in_scale, const float* in_shift,
                      int in_nstride, const void* wp, const float* bias, const eunet_act* y, float* stats,
                      void* stream);
/* dgrad (wp_t packed with transpose_flip) fused with the reduction half of the
 * BatchNorm backward of the layer whose output gradient it produces (autograd of
 * models.py:220-221, BN+ReLU after the conv): y = that layer's pre-BN output,
 * part [tiles][2][gx.c] = per-tile (sum g', sum g' xhat), g' = gx [y scale + shift > 0],
 * xhat = (y - mean) invstd, gx as stored (rounded); scale / shift = the BN's forward
 * affine (eunet_bn_finalize), so the ReLU mask is bit-identical to the forward's and to
 * every other BN-backward kernel's.  Replaces conv3x3_fwd(dgrad) + bn_bwd_reduce;
 * colsum(part, tiles, 2C) -> (dbeta, dgamma).
 * gscale (nullable) [N][gx.c]: gx is scaled per sample and channel before the store
 * and the reduction (the backward of a Dropout2d between the BN+ReLU and this conv). */
int eunet_conv3x3_dgrad_bnbwd(const eunet_act* dy, const void* wp_t, const eunet_act* gx,
                              const eunet_act* y, const float* mean, const float* invstd,
                              const float* scale, const float* shift, const float* gscale,
                              float* part, void* stream);
/* plain dgrad (autograd of models.py:219,222 w.r.t. the conv input): gx = conv(dy, W') with
 * wp_t packed transpose_flip; gscale (nullable) [N][gx.c] scales gx per sample and channel.  gx has dy's
 * dtype, or (the one mixed-dtype call) fp32 for a bf16 dy: the output is then stored unrounded, and gx's
 * c, ctot and coff are still multiples of dy's unit of 8 */
int eunet_conv3x3_dgrad(const eunet_act* dy, const void* wp_t, const eunet_act* gx, const float* gscale,
                        void* stream);
/* wgrad (split over pixel tiles): dw_part [nsplit][cout][9][cin] and
 * db_part [nsplit][cout] (db only when db_part != NULL) */
int eunet_conv3x3_wgrad_splits(const eunet_act* dy, int cin, int dtype, int* nsplit);
int eunet_conv3x3_wgrad(const eunet_act* x, const float* in_scale, const float* in_shift,
                        int in_nstride, const eunet_act* dy, float* dw_part, float* db_part, int nsplit,
                        void* stream);
/* reduce split partials -> torch layout dw [cout][cin][taps], db [cout] (fp64 combine) */
int eunet_wgrad_reduce(const float* dw_part, const float* db_part, int nsplit, int cout, int cin,
                       int taps, float* dw, float* db, void* stream);

/* ---- direct 3x3 conv for Cin <= 8: enc1.0 (models.py:203, Cin = in_channels) and the
 *      dual-branch fusion_head.0 (models.py:285, Cin = 2K); no bias when bias == NULL */
int eunet_conv_small_fwd(const eunet_act* x, const float* w, const float* bias,
                         const eunet_act* y, float* stats, void* stream);
int eunet_conv_small_wgrad_splits(const eunet_act* dy, int* nsplit);
/* dy is read in whole 16-byte units (the view contract at eunet_act); x (Cin <= 8) may have any layout */
int eunet_conv_small_wgrad(const eunet_act* x, const eunet_act* dy, float* dw_part,
                           float* db_part, int nsplit, void* stream);

/* ---- BatchNorm2d train-mode statistics (models.py:220,223; eps 1e-5, momentum 0.1)
 * combine per-tile (sum, M2, count) partials (Chan, fp64); update running
 * stats with the UNBIASED variance; emit mean, invstd and the fused affine
 * scale = gamma*invstd, shift = beta - mean*scale; num_batches_tracked (nullable,
 * int64) is incremented on the device. */
int eunet_bn_finalize(const float* stats, int tiles, int c, const float* gamma, const float* beta,
                      float eps, float momentum, float* run_mean, float* run_var, float* mean,
                      float* invstd, float* scale, float* shift, int64_t* num_batches_tracked,
                      void* stream);
/* eval-mode affine from running stats */
int eunet_bn_eval_affine(int c, const float* gamma, const float* beta, const float* run_mean,
                         const float* run_var, float eps, float* scale, float* shift, void* stream);

/* BN-apply + ReLU, out = relu(y * scale + shift) (models.py:219-222: the BatchNorm2d + ReLU between
 * the two convs of a DoubleConv), materialised once for the second conv's forward and weight
 * gradient (which then read it without applying the transform per staged halo pixel) */
int eunet_bnrelu(const eunet_act* y, const float* scale, const float* shift, const eunet_act* out, void* stream);

/* ---- fused BN-apply + ReLU consumers ----------------------------------------
 * pool: MaxPool2d(2) (models.py:214, 229-231); act (nullable) receives the
 * full-resolution activation (the skip tensor, written into its concat slot,
 * models.py:233-235). */
int eunet_bnrelu_pool(const eunet_act* y, const float* scale, const float* shift,
                      const eunet_act* act, const eunet_act* pooled, void* stream);
/* Upsample x2 bilinear, align_corners=False (models.py:215, 233-236) */
int eunet_bnrelu_upsample(const eunet_act* y, const float* scale, const float* shift,
                          const eunet_act* out, void* stream);
/* ---- learned decoder upsample: ConvTranspose2d(C, C, kernel_size=2, stride=2) ------------------------
 * No reference line to cite: the reference has no transposed convolution.  The source is the project's
 * own statement of purpose, BASELINE.json north_star ("bilinear/transposed-conv upsample"); the model
 * keyword upsample="transpose" puts this layer where eunet_bnrelu_upsample stands (the three trunk
 * upsamples; the last, K-channel one inside the head / ktail kernels stays bilinear).
 *   d  = relu(fmaf(y, scale, shift))                  (rounded to the compute dtype)
 *   up[n, 2i+a, 2j+b, co] = bias[co] + sum_ci d[n,i,j,ci] * W[ci,co,a,b]       a, b in {0, 1}
 * y: the producing block's pre-BN conv output, scale / shift its BN affine; W the torch parameter
 * [C][C][2][2] fp32.  C must be a multiple of 32 and the 2x view has y's n, 2h, 2w and c (anything
 * else: EUNET_ERR_INVALID); views honour ctot / coff.  MFMA kernels for both dtypes.
 * pack: W -> wp (eunet_upconv2x2_packed_bytes bytes, the compute dtype): the forward's [4C][C] image
 * followed by the data gradient's [C][4C] one; once per step. */
int eunet_upconv2x2_packed_bytes(int c, int dtype, size_t* bytes);
int eunet_upconv2x2_pack(const float* w, int c, void* wp, int dtype, void* stream);
int eunet_bnrelu_upconv2x2_fwd(const eunet_act* y, const float* scale, const float* shift, const void* wp,
                               const float* bias, const eunet_act* out, void* stream);
/* gd[n,i,j,ci] = sum_{a,b,co} g[n,2i+a,2j+b,co] * W[ci,co,a,b]: the gradient w.r.t. d (the post-ReLU
 * activation; the block's BN backward applies the ReLU mask from y: eunet_bn_bwd_reduce / _apply) */
int eunet_upconv2x2_dgrad(const eunet_act* g, const void* wp, const eunet_act* gd, void* stream);
/* dW[ci,co,a,b] = sum_{n,i,j} d * g and db[co] = sum g, split over pixel tiles (y: the low-res view):
 * dw_part [nsplit][C][4][C] = [ci][2a+b][co] (eunet_wgrad_reduce(cout = cin = C, taps = 4) gives torch's
 * [ci][co][2][2]) and db_part (nullable) [nsplit][4][C] (eunet_colsum over its nsplit * 4 rows gives
 * db); fixed summation order, no atomics: two runs are bit-identical */
int eunet_upconv2x2_wgrad_splits(const eunet_act* y, int dtype, int* nsplit);
int eunet_upconv2x2_wgrad(const eunet_act* y, const float* scale, const float* shift, const eunet_act* g,
                          float* dw_part, float* db_part, int nsplit, void* stream);
/* dec1 1x1 conv (models.py:212,236), commuted before the upsample:
 * z[p][k] = b[k] + sum_c w[k][c] * relu(bn(y))[p][c]; z fp32 NHWC [N,H,W,K] */
int eunet_bnrelu_conv1x1(const eunet_act* y, const float* scale, const float* shift,
                         const float* w, const float* b, int k, float* z, void* stream);

/* ---- baseline network unet (models.py:175-243, SMP-absent BasicUNet) -------------------------------
 * The K-channel (K = 1..3) fp32 tails behind the 1x1 head.  z_lo [N,h,w,K] NHWC fp32, out NCHW fp32.
 *   EUNET_KTAIL_UP2:    out [N,K,2h,2w] = up2(z_lo), bilinear x2, align_corners=False: the final
 *                       upsample of UNet.forward (models.py:236, dec1 commuted before it)
 *   EUNET_KTAIL_SMOOTH: out [N,K,h,w] = mean2x2(up2(z_lo)): the training loop's 2H -> H bilinear
 *                       resize of the unet output (train_eval.py:306-310), computed as the separable
 *                       (1/8, 3/4, 1/8) filter with replicate edges */
enum { EUNET_KTAIL_UP2 = 0, EUNET_KTAIL_SMOOTH = 1 };
int eunet_ktail_fwd(int mode, const float* z_lo, int n, int h, int w, int k, float* out, void* stream);
/* their adjoints (autograd of the above): g NCHW ([N,K,2h,2w] for UP2, [N,K,h,w] for SMOOTH) ->
 * gz_lo [N,h,w,K] NHWC */
int eunet_ktail_bwd(int mode, const float* g, int n, int h, int w, int k, float* gz_lo, void* stream);

/* ---- enhance head at 2H + residual + 2x2 mean (models.py:308-313,336-337;
 *      train_eval.py:306-310 resize == 2x2 mean) ------------------------------
 * z: [N,H,W,K] fp32. out2h (nullable) [N,K,2H,2W] fp32 NCHW, logits
 * (nullable) [N,K,H,W] fp32 NCHW.  Head BN stats saved in mean/invstd (64).
 * dtype: EUNET_F32 = fp32 FMA path; EUNET_BF16 = bf16 MFMA GEMMs with fp32
 * accumulation (the reference's autocast precision for these convs). */
int eunet_head_workspace_bytes(int n, int h, int w, int k, int dtype, size_t* bytes);
int eunet_head_fwd(const float* z, int n, int h, int w, int k, const float* w1, const float* b1,
                   const float* gamma, const float* beta, const float* w2, const float* b2,
                   int training, float eps, float momentum, float* run_mean, float* run_var,
                   float* mean, float* invstd, float* out2h, float* logits, int dtype,
                   void* ws, void* stream);
/* backward from g_logits (or g_out2h when g_logits == NULL).  Writes gz and the
 * head parameter gradients gw1 [64][K][3][3], gb1, ggamma, gbeta, gw2 [K][64], gb2.
 * dtype as for head_fwd (EUNET_BF16: g_h never leaves the chip; the W1 gradient
 * is fused into the g_h pass). */
int eunet_head_bwd(const float* z, int n, int h, int w, int k, const float* w1, const float* b1,
                   const float* gamma, const float* beta, const float* w2, const float* mean,
                   const float* invstd, const float* g_logits, const float* g_out2h, float* gz,
                   float* gw1, float* gb1, float* ggamma, float* gbeta, float* gw2, float* gb2,
                   int dtype, void* ws, void* stream);

/* ---- per-pixel losses: the shape rule --------------------------------------
 * Every forward and backward entry point of the per-pixel losses below (eunet_loss_*, eunet_bce_dice_*,
 * eunet_boundary_loss_*, eunet_lovasz_errors / _fwd / _bwd, the _w variants included) takes logits [N,K,H,W] fp32 NCHW with
 *   N in 1..64, K in 1..3, H > 0, W > 0 and H*W < 2^31 - 1024,
 * and returns EUNET_ERR_INVALID for anything else, before any launch (csrc/pixelloss.h, pl_shape_ok).  N <= 64
 * is the finalize block's per-sample storage; the last bound keeps a plane index plus one tile of 1024 pixels in
 * an int.  A backward call takes the shape of the forward call whose sums it reads. */

/* ---- combined loss (train_eval.py:28-60, 134-197, 262-337) ----------------
 * logits [N,K,H,W] fp32 NCHW, target [N,H,W] int64 (the shape rule above).  params (nullable = the
 * Trainer's enhanced_unet configuration, eunet_loss_reference_params):
 *   loss = w_focal * focal + (1/N) sum_n [w_dice dice_n + w_tversky tversky_n]
 *   focal = sum over all pixels of alpha_t (1 - pt)^gamma ce / F_den, ce = -w_t log p_t
 *           (F.cross_entropy weight = ce_weight, ignore_index pixels give ce = 0),
 *           F_den = N*H*W (FocalLoss.mean(), train_eval.py:60) or, focal_norm = 1, the sum
 *           of w_t (nn.CrossEntropyLoss(weight) mean reduction, train_eval.py:80)
 *   dice_n / tversky_n: Trainer.dice_loss / tversky_loss (:134-181), class mean over
 *           class_div classes (3 in _compute_combined_loss for any K, :192-193).
 * sums (caller-owned, saved for backward): eunet_loss_sums_len floats = [N][3+3K] partial
 * sums, then F_den, then the number of targets outside [0, K) that are not ignore_index
 * (an error in the reference: F.cross_entropy raises; the host reports it at its next sync).
 * loss: 1 fp32 on device.  parts (nullable): [N][3] focal/dice/tversky per sample. */
#define EUNET_NO_IGNORE (-2147483647 - 1) /* INT32_MIN */
typedef struct {
  float ce_weight[3];      /* FocalLoss class_weights (F.cross_entropy weight); 1 = none */
  float alpha[3];          /* FocalLoss alpha per class; 1 = none */
  float gamma;             /* FocalLoss gamma */
  int ignore_index;        /* FocalLoss ignore_index; EUNET_NO_IGNORE = none */
  float dice_weight[3];    /* Trainer.dice_loss class weights [1, 15, 8] */
  float tversky_weight[3]; /* Trainer.tversky_loss class weights [1, 12, 6] */
  float tversky_alpha;     /* 0.7 */
  float w_focal, w_dice, w_tversky;  /* term weights (2.5, 2.5, 1.0 for enhanced_unet) */
  float class_div;         /* num_classes of dice_loss / tversky_loss */
  int focal_norm;          /* 0 pixel mean, 1 ce-weight mean (CrossEntropyLoss) */
} eunet_loss_params;
int eunet_loss_reference_params(eunet_loss_params* params);
int eunet_loss_sums_len(int n, int k, int* len);
int eunet_loss_workspace_bytes(int n, int k, int h, int w, size_t* bytes);
int eunet_loss_fwd(const float* logits, const int64_t* target, int n, int k, int h, int w,
                   const eunet_loss_params* params, float* sums, float* loss, float* parts, void* ws,
                   void* stream);
/* glogits = d loss / d logits * (*gloss) (gloss: device scalar) */
int eunet_loss_bwd(const float* logits, const int64_t* target, int n, int k, int h, int w,
                   const eunet_loss_params* params, const float* sums, const float* gloss, float* glogits,
                   void* stream);

/* ---- sigmoid BCE + soft Dice loss (bce_dice.hip) ---------------------------
 * No reference line to cite: the reference has no BCE.  The source is the
 * project's own statement of purpose, BASELINE.json north_star ("BCE/Dice"); this comment is the
 * definition.  logits x [N,K,H,W] fp32 NCHW, target [N,H,W] int64; K = 1..3, N <= 64 (as
 * eunet_loss_fwd; anything else: EUNET_ERR_INVALID).  One logit per class, a sigmoid each.
 *   target_mode ONEHOT (K >= 2):      t_c = [target == c],  valid iff 0 <= target < K
 *   target_mode FOREGROUND (K = 1):   t_0 = [target >= 1],  valid iff target >= 0  (a 0/1/2
 *                                     background/live/dead mask trains "cell")
 *   target_mode AUTO: FOREGROUND for K = 1, ONEHOT otherwise.  FOREGROUND with K != 1, ONEHOT
 *   with K = 1 and smooth <= 0 are EUNET_ERR_INVALID.
 * A pixel equal to ignore_index contributes to nothing: not to the BCE sum, not to its
 * denominator, not to I, S or T (eunet_loss_fwd differs: there an ignored pixel's probability still
 * counts in S).  A pixel that is neither valid nor ignored contributes nothing either and is
 * counted; the count is the last element of sums, where eunet_loss_fwd puts it.
 *   sp(z) = max(z, 0) + log1p(exp(-|z|)), sig = sigmoid, V_n = valid pixels of sample n, V = sum V_n
 *   bce(x,t)_c = cw_c (pw_c t sp(-x) + (1 - t) sp(x))
 *                (F.binary_cross_entropy_with_logits(weight = cw, pos_weight = pw))
 *   BCE    = sum_{n, c, valid px} bce / (K max(1, V))
 *   bce_n  = sum_{c, valid px of n} bce / (K max(1, V_n))
 *   per (n, c) over valid pixels: I = sum sig(x) t, S = sum sig(x), T = sum t
 *   dice_n = (1/K) sum_c dw_c (1 - (2 I + smooth) / (S + T + smooth))
 *   loss   = w_bce BCE + w_dice (1/N) sum_n dice_n
 * A batch without a valid pixel gives loss 0 and gradient 0.
 * sums (caller-owned, saved for backward): eunet_bce_dice_sums_len floats = [N][3+3K] rows of
 * (bce sum, I[K], S[K], T[K], V_n, out-of-range count), then V, then the out-of-range count of
 * the batch.  loss: 1 fp32 on device.  parts (nullable): [N][2] = (bce_n, dice_n).
 * ws: eunet_bce_dice_workspace_bytes.  The sums are taken in a fixed order: two runs are
 * bit-identical. */
enum { EUNET_BCE_TARGET_AUTO = 0, EUNET_BCE_TARGET_ONEHOT = 1, EUNET_BCE_TARGET_FOREGROUND = 2 };
typedef struct {
  float pos_weight[3];   /* pw: weight of the positive term per class; 1 = none */
  float class_weight[3]; /* cw: weight of a class's BCE; 1 = none */
  float dice_weight[3];  /* dw: weight of a class's Dice term; 1 = none */
  float w_bce, w_dice;   /* term weights */
  float smooth;          /* Dice smoothing, > 0 (1e-6: Trainer.dice_loss's, train_eval.py:134-157) */
  int ignore_index;      /* EUNET_NO_IGNORE = none */
  int target_mode;       /* EUNET_BCE_TARGET_* */
} eunet_bce_dice_params;
/* pw = cw = dw = 1, w_bce = w_dice = 1, smooth 1e-6, no ignore index, target_mode AUTO (what a
 * null params pointer means) */
int eunet_bce_dice_default_params(eunet_bce_dice_params* params);
int eunet_bce_dice_sums_len(int n, int k, int* len);
int eunet_bce_dice_workspace_bytes(int n, int k, int h, int w, size_t* bytes);
int eunet_bce_dice_fwd(const float* logits, const int64_t* target, int n, int k, int h, int w,
                       const eunet_bce_dice_params* params, float* sums, float* loss, float* parts, void* ws,
                       void* stream);
/* glogits = (*gloss) d loss / d logits (gloss: device scalar g), analytic per pixel from sums, with
 * U = S + T + smooth:
 *   g [ w_bce cw_c (-pw_c t sig(-x) + (1 - t) sig(x)) / (K max(1, V))
 *       + w_dice dw_c / (N K) (-2 t / U + (2 I + smooth) / U^2) sig(x) sig(-x) ]
 * and 0 on ignored and out-of-range pixels. */
int eunet_bce_dice_bwd(const float* logits, const int64_t* target, int n, int k, int h, int w,
                       const eunet_bce_dice_params* params, const float* sums, const float* gloss, float* glogits,
                       void* stream);

/* ---- U-Net border weight map, instance separation, pixel-weighted losses (weightmap.hip) ----
 * No reference line to cite: the reference fills its polygons into one 0/1/2 mask and weights a pixel by
 * its class only.  The map is the per-pixel weight of Ronneberger et al., "U-Net" (2015), eq. 2; this
 * comment is the definition.
 *
 * labels [N,H,W] int64: 0 is background, any other value an instance id.  Ids need not be contiguous and
 * may exceed 16 bits; the same id in two separate places is one instance.  The kernel tells ids apart by
 * their low 32 bits (every id in [1, 2^32) is safe; an id whose low 32 bits are 0 would read as
 * background).  semantic (nullable) [N,H,W] int64.
 *
 * Distances.  For a pixel x of sample n and an id i, over the pixels q of that sample with labels(q) = i,
 * |qx - xx| <= R and |qy - xy| <= R (a square window, inclusive, cut at the image edge, never wrapped):
 *   d_i(x) = min ||x - q||  (Euclidean);  d1 <= d2 = the two smallest d_i(x) over DISTINCT ids.
 *   border(x) = w0 exp(-(d1 + d2)^2 / (2 sigma^2))  where labels(x) = 0 and two distinct ids lie in the window
 *   border(x) = 0                                   elsewhere: cell pixels, background with < 2 ids in reach
 *   base(x)   = class_weight[semantic(x)] when semantic is given and its value is 0, 1 or 2, else 1
 *   out(x)    = base(x) + border(x)
 * radius R: EUNET_WMAP_RADIUS_AUTO = ceil(5.5 sigma).  sigma > 0, w0 >= 0 and 1 <= R <= 48 are required,
 * anything else is EUNET_ERR_INVALID.  class_weight: 3 host floats (nullable = 1, 1, 1).
 * The window is part of the definition, not an approximation: where the untruncated map (R = infinity)
 * differs from this one, a distance beyond R is involved, so d1 + d2 > R and both border terms are below
 * w0 exp(-R^2 / (2 sigma^2)) -- at the default R that is 2.7e-7 w0.
 * No host synchronisation, no allocation; enqueued on stream only. */
#define EUNET_WMAP_RADIUS_AUTO (-1)
int eunet_border_weight_map(const int64_t* labels, const int64_t* semantic, int n, int h, int w,
                            const float* class_weight, float w0, float sigma, int radius, float* out,
                            void* stream);
/* The usual companion of the map, exact integer work (ids compared in all 64 bits):
 *   labels'(x) = 0 and semantic'(x) = 0 where some pixel of the 3x3 neighbourhood of x, inside the image,
 *   has a label that is neither 0 nor labels(x); every other pixel is unchanged.
 * Both outputs are computed from the inputs (not in place: the outputs must not alias the inputs), so both
 * sides of a contact lose one pixel.  semantic and semantic_out are both given or both null. */
int eunet_separate_instances(const int64_t* labels, const int64_t* semantic, int n, int h, int w,
                             int64_t* labels_out, int64_t* semantic_out, void* stream);
/* eunet_loss_fwd / _bwd with a per-pixel weight m = pixel_weight [N,H,W] fp32 (non-null; it takes no
 * gradient): the per-pixel focal summand alpha_t (1 - pt)^gamma ce is multiplied by m(x), F_den stays
 * N*H*W, Dice and Tversky are untouched; ignored and out-of-range pixels contribute as in eunet_loss_fwd
 * (nothing to the focal term, whatever their weight).  focal_norm = 1 is EUNET_ERR_INVALID here: its
 * denominator would need a definition of its own.  The logit gradient gets the factor m(x) on its focal
 * part only.  sums / ws layouts are eunet_loss_fwd's; m = 1 everywhere gives eunet_loss_fwd's bits. */
int eunet_loss_fwd_w(const float* logits, const int64_t* target, const float* pixel_weight, int n, int k,
                     int h, int w, const eunet_loss_params* params, float* sums, float* loss, float* parts,
                     void* ws, void* stream);
int eunet_loss_bwd_w(const float* logits, const int64_t* target, const float* pixel_weight, int n, int k,
                     int h, int w, const eunet_loss_params* params, const float* sums, const float* gloss,
                     float* glogits, void* stream);
/* eunet_bce_dice_fwd / _bwd with a per-pixel weight m (as above): bce(x,t)_c is multiplied by m(x), in BCE
 * and in bce_n; the denominators K max(1, V) and the Dice terms are untouched, so m = 1 is the unweighted
 * loss, bit for bit.  The logit gradient gets the factor m(x) on its BCE part only. */
int eunet_bce_dice_fwd_w(const float* logits, const int64_t* target, const float* pixel_weight, int n, int k,
                         int h, int w, const eunet_bce_dice_params* params, float* sums, float* loss,
                         float* parts, void* ws, void* stream);
int eunet_bce_dice_bwd_w(const float* logits, const int64_t* target, const float* pixel_weight, int n, int k,
                         int h, int w, const eunet_bce_dice_params* params, const float* sums,
                         const float* gloss, float* glogits, void* stream);

/* ---- elastic deformation and affine warp of image and labels (warp.hip) -------------------------
 * No reference line to cite: the reference's augmentations are photometric or a mirror.  The deformation is
 * the one of Ronneberger et al., "U-Net" (2015), §3.1: random displacement vectors on a coarse grid, a
 * per-pixel displacement by bicubic interpolation, image and labels moved together; this comment is the
 * definition.  No host synchronisation, no allocation; enqueued on stream only.
 *
 * eunet_warp_grid writes the dense sampling map grid [h][w][2] fp32, (sx, sy) in absolute source pixels:
 *   sx = m00 x + m01 y + m02 + Dx(y, x)      sy = m10 x + m11 y + m12 + Dy(y, x)
 * m: six host doubles (nullable = identity), the 2x3 inverse map, destination to source, as cv2.warpAffine
 * with WARP_INVERSE_MAP; used in fp32.  D is the bicubic interpolation of the control displacements ctrl
 * [2][gh][gw] (device fp32; plane 0 dx, plane 1 dy, in pixels), defined to be exactly
 * F.interpolate(ctrl[None], size=(h, w), mode="bicubic", align_corners=True): the cubic-convolution kernel
 * with A = -0.75 at u = x (gw - 1) / (w - 1) (0 when w == 1), taps floor(u) - 1 .. floor(u) + 2 with indices
 * clamped to [0, gw - 1]; the same along y.  2 <= gh, gw <= 16; 1 <= h, w <= 2^20. */
int eunet_warp_grid(const float* ctrl, int gh, int gw, const double* m, int h, int w, float* grid, void* stream);
/* Both gathers read a map grid [ho][wo][2] (8-byte aligned) whose size is independent of the source's
 * (hi, wi), and are pure functions of its fp32 values: with sx clamped to +-2^20,
 *   qx = rint(32 sx)  (round-half-even; the product is exact in fp32), qy likewise;
 * a non-finite sx or sy gives `fill` under both border rules.  Every tap index goes through the border rule
 * on its own:
 *   EUNET_WARP_CONSTANT:   an index outside [0, n) contributes `fill`
 *   EUNET_WARP_REFLECT101: r = i mod 2(n - 1) taken non-negative, r = 2(n - 1) - r if r >= n; r = 0 if n == 1
 *                          (any number of reflections)
 * eunet_warp_u8: bilinear, HWC uint8, 1 <= c <= 4, integer after the one rounding above:
 *   ix = qx >> 5 (floor), fx = qx & 31, iy and fy likewise; taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1)
 *   with weights (32-fx)(32-fy), fx(32-fy), (32-fx)fy, fx fy;  out = (sum w p + 512) >> 10.
 * eunet_warp_labels: nearest, ix = (qx + 16) >> 5 and iy likewise, over `planes` planes [planes][hi][wi] ->
 *   [planes][ho][wo] of elem_bytes = 8 (int64) or 1 (uint8; fill in 0..255) that share the one map; output
 *   pixel (y, x) reads grid[flip_v ? ho-1-y : y][flip_h ? wo-1-x : x], so the flagged result is the unflagged
 *   one mirrored (as eunet_rasterize_instances takes the training flips).  planes == 0 is a no-op.
 * Not in place.  Sides up to 2^20; a source (plane) below 2^31 bytes (pixels). */
#define EUNET_WARP_CONSTANT 0
#define EUNET_WARP_REFLECT101 1
int eunet_warp_u8(const uint8_t* src, int hi, int wi, int c, const float* grid, int ho, int wo, int border,
                  int fill, uint8_t* dst, void* stream);
int eunet_warp_labels(const void* src, int elem_bytes, int planes, int hi, int wi, const float* grid, int ho,
                      int wo, int border, long long fill, int flip_h, int flip_v, void* dst, void* stream);

/* ---- backward helpers ----------------------------------------------------
 * BN(+ReLU) backward (autograd of models.py:220-224): g is the gradient w.r.t.
 * the ReLU output, y the pre-BN conv output, mean / invstd the batch statistics and
 * scale / shift the forward affine (scale = gamma invstd, shift = beta - mean scale, as
 * eunet_bn_finalize emits them).  The ReLU mask g' = g [y scale + shift > 0] is the
 * forward's, bit for bit, in every BN-backward kernel (reduce, apply, and the fused
 * reductions below), so the apply subtracts sums over exactly the g' it applies.
 * reduce -> part [tiles][2][c] (sum g', sum g'*xhat); colsum -> (dbeta, dgamma);
 * apply -> gy = scale (g' - dbeta/n - xhat dgamma/n). */
int eunet_bn_bwd_tiles(const eunet_act* y, int* tiles);
int eunet_bn_bwd_reduce(const eunet_act* g, const eunet_act* y, const float* mean,
                        const float* invstd, const float* scale, const float* shift, float* part,
                        void* stream);
/* deterministic column sum of a [rows][cols] fp32 partial matrix (fp64 two-stage) */
int eunet_colsum_ws_bytes(int rows, int cols, size_t* bytes);
int eunet_colsum(const float* part, int rows, int cols, float* out, void* ws, void* stream);
/* the same with columns >= split written to out_hi[col - split] (e.g. dbeta | dgamma straight
 * into their two gradient slots) */
int eunet_colsum_split(const float* part, int rows, int cols, int split, float* out_lo,
                       float* out_hi, void* ws, void* stream);
int eunet_bn_bwd_apply(const eunet_act* g, const eunet_act* y, const float* mean,
                       const float* invstd, const float* scale, const float* shift,
                       const float* dbeta, const float* dgamma, const eunet_act* gy,
                       void* stream);
/* Bounds-checked debug build (make -C enhanced-unet_amd debug -> libeunet_hip_debug.so, compiled with
 * -DEUNET_DEBUG): device-side checks on staging offsets, tile / split / block indices
 * and output addresses record the first failing check per source unit without trapping.
 * eunet_debug_enabled: 1 in the debug build, 0 in the release library (where the checks compile away).
 * eunet_debug_status: synchronises the device; *count = failed checks since the last reset,
 * *unit_line = unit * 100000 + source line of the first (units: 1 capi, 2 conv3x3, 3 bn_pool_up,
 * 4 head, 5 instances, 6 baselines, 7 upconv, 8 bce_dice, 9 weightmap, 10 tiling, 11 warp,
 * 12 boundary, 13 watershed, 14 pairs, 15 sdf, 16 cellprops, 17 hull, 18 loss, 19 lovasz; 0 = none).
 * eunet_debug_selftest launches one deliberately failing check (capi unit). */
int eunet_debug_enabled(void);
int eunet_debug_status(unsigned* unit_line, unsigned* count, int reset);
int eunet_debug_selftest(void* stream);
/* MaxPool2d backward (first max in row-major order wins, recomputed from the
 * saved activation) + the skip-path gradient: gout = gskip + scatter(gpool) */
int eunet_pool_bwd_add(const eunet_act* act, const eunet_act* gpool, const eunet_act* gskip,
                       const eunet_act* gout, void* stream);
/* Upsample x2 backward (adjoint of the bilinear taps).  Dense fp32 views (ctot == c, coff == 0) of c <= 4
 * channels take a scalar path without the 16-byte unit requirement (the K-channel logits of the head) */
int eunet_upsample_bwd(const eunet_act* ghi, const eunet_act* glo, void* stream);
/* The two producers above with the reduction half of eunet_bn_bwd_reduce fused in: gout / glo is
 * the gradient w.r.t. relu(bn(y)) of the DoubleConv output y (models.py:222-223), and
 * part[rows][2][C] receives (sum g', sum g' xhat) per block, rows from the *_rows query (0: the
 * channel count does not allow the fused form -- use the separate reduce).  The fused max-pool
 * adjoint does not read act (only its shape): it recomputes the activation from y as
 * eunet_bnrelu_pool stored it, round(relu(y scale + shift)), so act must be that tensor. */
int eunet_pool_bwd_add_bnr_rows(const eunet_act* gout, int* rows);
int eunet_pool_bwd_add_bnr(const eunet_act* act, const eunet_act* gpool, const eunet_act* gskip,
                           const eunet_act* gout, const eunet_act* y, const float* mean, const float* invstd,
                           const float* scale, const float* shift, float* part, void* stream);
/* gout may be NULL in eunet_pool_bwd_add_bnr: the gradient is then only reduced, and the block's apply
 * recomputes it -- eunet_bn_bwd_apply_pool = eunet_bn_bwd_apply on gout = gskip + scatter(gpool), formed and
 * rounded per 2x2 window as eunet_pool_bwd_add_bnr forms it (the same gy bit for bit, without gout's write and
 * read; even H and W).  Reference: the autograd of models.py:214, 228-230 (MaxPool2d(2) after each encoder block,
 * its input also the skip input of the decoder concat, :232-234) and models.py:222-223 (the block's second
 * BatchNorm). */
int eunet_bn_bwd_apply_pool(const eunet_act* gpool, const eunet_act* gskip, const eunet_act* y, const float* mean,
                            const float* invstd, const float* scale, const float* shift, const float* dbeta,
                            const float* dgamma, const eunet_act* gy, void* stream);
int eunet_upsample_bwd_bnr_rows(const eunet_act* glo, int* rows);
int eunet_upsample_bwd_bnr(const eunet_act* ghi, const eunet_act* glo, const eunet_act* y, const float* mean,
                           const float* invstd, const float* scale, const float* shift, float* part, void* stream);
/* dec1 1x1 backward: gact = W^T gz (w.r.t. relu(bn(y))), part [tiles][K*C + K]
 * = per-tile (gW, gb) partials */
int eunet_conv1x1_bwd_tiles(const eunet_act* y, int* tiles);
int eunet_conv1x1_bwd(const eunet_act* y, const float* scale, const float* shift,
                      const float* w, int k, const float* gz, const eunet_act* gact, float* part,
                      void* stream);
/* the same, also writing the BN-backward partial sums of y's BatchNorm over the gradient it
 * produces (what eunet_bn_bwd_reduce would compute from gact): bn_part [tiles][2][C] = per-tile
 * (sum g', sum g' xhat), g' = gact where relu(bn(y)) > 0 (scale/shift are that BN's affine form).
 * gact may be NULL: the gradient is then only reduced, not stored, and eunet_bn_bwd_apply_1x1
 * recomputes it for the apply. */
int eunet_conv1x1_bwd_bnr(const eunet_act* y, const float* scale, const float* shift,
                          const float* w, int k, const float* gz, const eunet_act* gact, float* part,
                          const float* mean, const float* invstd, float* bn_part, void* stream);
/* eunet_bn_bwd_apply for the gradient eunet_conv1x1_bwd_bnr produced without storing it: g = W^T gz
 * (w [K][C], gz [N*H*W][K] fp32) recomputed per pixel with conv1x1_bwd's arithmetic and rounding to
 * y's dtype, then gy = scale (g' - dbeta/n - xhat dgamma/n) as eunet_bn_bwd_apply -- the same gy bit for
 * bit, without the C-channel gradient's write and read.  Reference: the autograd of models.py:212, 236
 * (dec1 = Conv2d 1x1 on relu(bn(dec2's conv .3 output)), models.py:220-223). */
int eunet_bn_bwd_apply_1x1(const eunet_act* y, const float* w, int k, const float* gz, const float* mean,
                           const float* invstd, const float* scale, const float* shift, const float* dbeta,
                           const float* dgamma, const eunet_act* gy, void* stream);

/* ---- optimizer tail of the Trainer step (optim.hip; train_eval.py:341-343, AdamW from :120)
 * clip_grad_norm_(max_norm) + AdamW (decoupled weight decay) over every parameter tensor in three
 * launches.  One eunet_opt_tensor per parameter: its fp32 data, gradient (scaled in place by the
 * clip coefficient, as clip_grad_norm_ leaves it), AdamW exp_avg / exp_avg_sq and the fp32 device
 * step counter torch's fused AdamW keeps (incremented here).  eunet_opt_table writes the nt x 7
 * int64 host table (copy it to the device) and the launch's block count; partial holds nblocks
 * doubles; coef (1 float) receives the clip coefficient, total_norm (nullable) the gradient norm. */
typedef struct {
  float* param; float* grad; float* exp_avg; float* exp_avg_sq; float* step; long long numel;
} eunet_opt_tensor;
int eunet_opt_table(const eunet_opt_tensor* tensors, int nt, int64_t* table, int* nblocks);
/* grads: host array of the nt gradient pointers (nt <= EUNET_OPT_KARG_MAX; they travel as a kernel
 * argument, so a table built once serves steps whose gradients move), or null for larger nt (the
 * table's grad column is used) */
#define EUNET_OPT_KARG_MAX 256
int eunet_clip_adamw(const int64_t* table, int nt, int nblocks, float* const* grads, float max_norm,
                     double lr, double beta1, double beta2, double eps, double weight_decay,
                     double* partial, float* coef, float* total_norm, void* stream);

/* ---- evaluation path (evalpath.hip) ---------------------------------------
 * Semantic metric counts (metrics.py:29-58, calculate_semantic_metrics): pred, gt
 * int64 [n][hw]; counts int64 [n][3 classes][3] = (#pred==c, #gt==c, #both==c),
 * zeroed by the call.  IoU / Dice follow from the counts on the host. */
int eunet_semantic_counts(const int64_t* pred, const int64_t* gt, int n, long long hw,
                          int64_t* counts, void* stream);
/* calculate_iou / calculate_dice (metrics.py:12-26) of two int64 masks of n elements:
 * out int64[4] = (#(a!=0 & b!=0), #(a!=0 | b!=0), sum a, sum b), zeroed by the call */
int eunet_binary_overlap(const int64_t* a, const int64_t* b, long long n, int64_t* out,
                         void* stream);
/* Bilinear resample, align_corners=False, PyTorch upsample_bilinear2d index math
 * (F.interpolate in train_eval.py:413, 441-449): x [planes][hin][win] ->
 * y [planes][hout][wout]; scale_* = 1/scale_factor or hin/hout; flip_* mirror the
 * destination index (torch.flip, train_eval.py:427-437). */
int eunet_resize_bilinear(const float* x, int planes, int hin, int win, float* y, int hout,
                          int wout, float scale_h, float scale_w, int flip_h, int flip_w,
                          void* stream);
/* softmax over K (2 or 3) of logits [K][hp][wp], cropped to [h][w] and optionally
 * flipped (F.softmax + crop, train_eval.py:414-417) -> probs [K][h][w] */
int eunet_softmax_crop(const float* logits, int k, int hp, int wp, int h, int w, int flip_h,
                       int flip_w, float* probs, void* stream);
/* TTA mean (train_eval.py:453): mode 0 acc = p, 1 acc += p, 2 acc = (acc + p) / count */
int eunet_accumulate(float* acc, const float* p, long long n, int mode, float count,
                     void* stream);
/* _convert_probs_to_mask (train_eval.py:455-568): probs [K][h][w] (K = 3; K = 2 with a
 * zero dead-cell probability) -> mask int64 [h][w]; counts: 2 int64 of workspace. */
int eunet_probs_to_mask(const float* probs, int k, int h, int w, int64_t* mask,
                        int64_t* counts, void* stream);
/* The prediction path of a model trained with eunet_bce_dice_fwd (no reference line: BASELINE.json
 * north_star "BCE/Dice").  eunet_sigmoid_crop is eunet_softmax_crop's sibling: sigmoid of each of the
 * K (1..3) logits [K][hp][wp], cropped to [h][w] and optionally flipped -> probs [K][h][w].
 * eunet_probs_threshold: probs [K][h][w] -> mask int64 [h][w]; K = 1: [p >= threshold]; K >= 2:
 * the argmax over K, the first maximum on ties (threshold unused). */
int eunet_sigmoid_crop(const float* logits, int k, int hp, int wp, int h, int w, int flip_h,
                       int flip_w, float* probs, void* stream);
int eunet_probs_threshold(const float* probs, int k, int h, int w, float threshold, int64_t* mask,
                          void* stream);

/* ---- pixel-level score histograms (curves.hip) --------------------------------
 * The one device pass behind the ROC, PR and calibration statistics of visualization.py:1096-1199, 1819-1900
 * (plot_roc_curves, plot_pr_curves, plot_calibration_curve), which the reference feeds by copying every
 * image's softmax to the host (train_eval.py:1291-1306).  probs fp32 [n][k][hw] (k = 1..3), mask int64
 * [n][hw]; edges: bins + 1 device floats (bins = 1..3072), strictly increasing with edges[0] = 0 and
 * edges[bins] = 1 (the caller's duty: only pointers and ranges are checked here).
 *   hist int64 [k][bins][3] = per class c and bin b (#negatives, #positives, confidence sum); invalid int64 [1].
 * Both are ADDED to, never zeroed: a validation set accumulates into one pair (integer adds, order-free).
 * Bin: bin(p) = the i with edges[i] <= p < edges[i+1], compared in fp32, and the last bin is closed: every
 *   finite p >= edges[bins-1] goes to bin bins-1 (p == 1, and a test-time-augmentation mean that rounds a hair
 *   above 1).  This is a deliberate difference from the reference's `p >= e[i] & p < e[i+1]`
 *   (visualization.py:1854), which silently drops every saturated p == 1.0; it is the convention of sklearn's
 *   calibration_curve.  -0.0 goes to bin 0.  A p that is NaN, +-inf or < 0 adds 1 to invalid[0] and counts
 *   nowhere else.
 * Truth: a pixel with mask == ignore_index counts nowhere, for any class, and its p is not examined (the
 *   reference filters 255 in its ROC and PR functions but not in its calibration function; here the rule is the
 *   same for all three).  Otherwise the pixel is a positive of class c when mask == c; for k == 1 when
 *   mask >= 1 (the one-logit target of eunet_bce_dice_fwd).  A label outside [0, k) is a negative of every
 *   class, as in the reference.
 * Conf: hist[c][b][2] += llrint(min(p, 1) * 2^24): the scaling is exact in fp32 and the rounding is to nearest
 *   even, so the sum is an integer and a pure function of the input; a bin's mean confidence is
 *   conf / 2^24 / (neg + pos), within 2^-25 of the true mean. */
int eunet_score_hist(const float* probs, const int64_t* mask, int n, int k, long long hw,
                     const float* edges, int bins, int ignore_index, int64_t* hist, int64_t* invalid,
                     void* stream);

/* ---- exact distance transform and boundary statistics (boundary.hip) -----------
 * What the contour metrics of segmentation rest on (Hausdorff distance and its 95th percentile, average symmetric
 * surface distance, surface Dice at a tolerance, boundary F1, Boundary IoU), and the two rows of
 * visualization.py:1687-1751 (plot_boundary_accuracy), which the reference forms on the host with scipy.ndimage.
 * Maps are int64 [n][h][w]; values are compared in all 64 bits (1 and 1 + 2^32 are different values).
 *   Region  R_v(M) = {x : M(x) = v}.
 *   Edge    E_v(M) = the pixels of R_v(M) that have a 4-neighbour which lies outside the image or is not in R_v(M):
 *           m & ~scipy.ndimage.binary_erosion(m) with scipy's defaults (cross element, border_value=0), the
 *           convention of MONAI's get_mask_edges.
 *   Squared distance  D_S(x) = min over q in S, in the same sample, of (x_y - q_y)^2 + (x_x - q_x)^2: an int32,
 *           exact.  When a sample has no site it is EUNET_EDT_NONE = INT32_MAX everywhere in that sample.
 * eunet_edt_sq: out int32 [n][nv][h][w], out[i][j] = D_S of sample i for the site set S of values[j] (a HOST
 *   array of nv = 1..8 values): R_v for EUNET_EDT_EQ, the complement of R_v for EUNET_EDT_NE, E_v for
 *   EUNET_EDT_EDGE.  1 <= h, w <= 8192 (2 * 8191^2 fits an int32), 1 <= n <= 65535.  Two kernels, no
 *   workspace (the row pass runs in place), no host synchronisation. */
#define EUNET_EDT_EQ 0
#define EUNET_EDT_NE 1
#define EUNET_EDT_EDGE 2
#define EUNET_EDT_NONE 2147483647
#define EUNET_EDT_MAX_VALUES 8
#define EUNET_EDT_MAX_SIDE 8192
int eunet_edt_sq(const int64_t* labels, int n, int h, int w, const int64_t* values, int nv, int mode,
                 int32_t* out, void* stream);
/* eunet_boundary_stats: the one pass behind every contour metric, for pred and gt int64 [n][h][w] and the classes
 * c = 0 .. k-1 (k = 1..3).
 * Ignore rule: a pixel with gt == ignore_index counts as ignore_index in pred as well, before anything else (in
 *   the kernels' predicate; no copy is written).  The ignored area is therefore one region in both maps, its
 *   edges coincide at distance 0 and favour neither side.  refrows alone is computed WITHOUT the rule.
 * All outputs are int64 and are ADDED to, never zeroed (a validation set accumulates into one set of buffers);
 * the one exception is the maximum, which is combined by max.
 *   surf [k][2][cap2 + 5], cap2 = cap^2, cap = 1..EUNET_BOUNDARY_MAX_CAP.  Direction 0 visits every x in
 *     E_c(pred) with d2 = D_{E_c(gt)}(x); direction 1 every x in E_c(gt) with d2 = D_{E_c(pred)}(x).
 *       [d2] for d2 <= cap2: the number of edge pixels at exactly that squared distance;
 *       [cap2+1]: the count with cap2 < d2 < NONE;  [cap2+2]: the count with d2 = NONE (the other map has no
 *       edge of this class in that image);  [cap2+3]: the largest finite d2 (0 when there is none);
 *       [cap2+4]: the sum over finite d2 of floor(2^16 sqrt(d2)), the integer square root of d2 * 2^32: a pure
 *       integer function, so the sum is order-free.
 *   band [k][nr][3], for a HOST array of nr = 0..8 integer radii r >= 0:  B_r(M) = {x in R_c(M) :
 *     D_{E_c(M)}(x) <= r^2}, the part of the region within r pixels of its own contour; the entries are
 *     (|B_r(pred)|, |B_r(gt)|, |B_r(pred) & B_r(gt)|): the Boundary IoU of Cheng et al. (2021) with a Euclidean
 *     band; r = 0 is the contour itself.  band may be null when nr = 0.
 *   refrows [n][k][2][3], per image (the reference averages per-image ratios), on the maps as they are.
 *     Row 0, the reference's boundary binary_dilation(m) & ~binary_erosion(m): the pixels whose radius-1 L1
 *     diamond holds both a pixel of the class and a position that is not of the class or lies outside the image.
 *     Row 1, the reference's interior binary_erosion(m, iterations=2): the pixels whose whole radius-2 L1 diamond
 *     is inside the image and of the class.  Each row holds (|pred set|, |gt set|, |both|).
 * ws: int32 [2][n][k][h][w] of workspace (eunet_boundary_workspace_bytes): the EDGE transforms of both maps.
 * Limits as eunet_edt_sq's; no host synchronisation, no allocation. */
#define EUNET_BOUNDARY_MAX_CAP 64
#define EUNET_BOUNDARY_MAX_RADII 8
int eunet_boundary_workspace_bytes(int n, int k, int h, int w, size_t* bytes);
int eunet_boundary_stats(const int64_t* pred, const int64_t* gt, int n, int h, int w, int k, int ignore_index,
                         int cap, const int* radii, int nr, int32_t* ws, int64_t* surf, int64_t* band,
                         int64_t* refrows, void* stream);

/* ---- distance-transform watershed (watershed.hip) ------------------------------
 * Splits touching cells along the ridges of a squared-distance map (train_eval.py:654-850: the docstring of
 * semantic_to_instances promises a watershed; the reference runs a ladder of fixed erosions).  The definition is
 * integer and order-free.  Input: planes D int32 [p][h][w] of squared distances, what eunet_edt_sq gives in mode
 * EUNET_EDT_NE: foreground is D > 0, a plane without background holds EUNET_EDT_NONE.
 *   Ascent  key(q) = (D[q], -q), q the linear index in the plane, compared lexicographically.  up(q) = the
 *           foreground pixel of largest key among q and its 8 neighbours inside the image.  Keys strictly increase
 *           along up, so every foreground pixel reaches one root (a local key maximum); a basin is the set of
 *           pixels of one root, its peak is D[root].  Plateaus resolve by the index alone.
 *   Saddle  of two basins a != b: the maximum, over the pairs of 8-adjacent pixels x in a, y in b, of
 *           min(D[x], D[y]).
 *   Merge   on the host (eunet.ops.merge_basins): the saddle edges sorted by (-saddle, min(a, b), max(a, b)) in
 *           root indices; a union-find whose representative is the member root of largest key; for an edge whose
 *           ends lie in different sets, lo = the set with the smaller representative key joins the other when
 *           sqrt(D[lo]) - sqrt(saddle) < depth (fp64, depth in pixels).  depth 0 merges nothing, depth inf leaves
 *           the 8-connected components.
 *   Ids     sets numbered 1..m per plane in raster order of each set's first pixel (eunet_label_components'
 *           convention), background 0.
 * Limits: 1 <= h, w <= 8192, 1 <= p <= 65535, p h w < 2^31.  ws: eunet_watershed_workspace_bytes; it carries the
 * roots from eunet_watershed_basins to eunet_watershed_peaks.
 * eunet_watershed_basins: basin int32 [p][h][w] = the basins numbered 1..counts[plane] in raster order of each
 *   basin's first pixel, background 0; counts int32 [p].  Adjacent foreground pixels are never both roots, so
 *   counts[plane] <= ceil(h / 2) ceil(w / 2).  No host synchronisation: pointer jumping runs its ceil(log2(h w)) + 1
 *   rounds as launches that return at once after the first round that changed nothing.
 * eunet_watershed_peaks: with offs int32 [p] (device) = the exclusive prefix sum of counts and nb_total their sum,
 *   root[offs[plane] + b - 1] = the root pixel of basin b of that plane (index in the plane), peak[...] = its D.
 * eunet_watershed_saddles: fills an open-addressing hash table of `capacity` slots (a power of two >= 2):
 *   keys int64 [capacity] = (a << 32) | b with a < b the slots of eunet_watershed_peaks, -1 where empty; vals int32
 *   [capacity] = the pair's saddle.  The call clears the table first.  An insert that finds
 *   min(capacity, 64) successive slots taken adds one to *overflow (device int32) and stores nothing: when
 *   *overflow != 0 the table is incomplete and the call is repeated with a larger one.
 * eunet_watershed_relabel: ids[i] = table[offs[plane] + basin[i] - 1] on the foreground (table: device int32
 *   [nb_total] of ids 1..amax), 0 elsewhere; ids may be basin itself.  areas int32 [p][amax] is zeroed and counts
 *   the pixels of every id. */
#define EUNET_WATERSHED_FLAG_WORDS 32
int eunet_watershed_workspace_bytes(int p, int h, int w, size_t* bytes);
int eunet_watershed_basins(const int32_t* dist, int p, int h, int w, int32_t* basin, int32_t* counts, int32_t* ws,
                           void* stream);
int eunet_watershed_peaks(const int32_t* dist, const int32_t* basin, const int32_t* ws, int p, int h, int w,
                          const int32_t* offs, int nb_total, int32_t* root, int32_t* peak, void* stream);
int eunet_watershed_saddles(const int32_t* dist, const int32_t* basin, int p, int h, int w, const int32_t* offs,
                            int64_t* keys, int32_t* vals, long long capacity, int32_t* overflow, void* stream);
int eunet_watershed_relabel(const int32_t* basin, int p, int h, int w, const int32_t* offs, const int32_t* table,
                            int nb_total, int32_t* ids, int32_t* areas, int amax, void* stream);

/* ---- label-map instance metrics (pairs.hip) --------------------------------------
 * No reference line: the reference scores instances through dense mask stacks (metrics.py:61-194).  Two integer id
 * maps hold the same information, and every instance-level score of the pair (Panoptic Quality, the Aggregated
 * Jaccard Index, object Dice, SEG, the F1 sweep over IoU; eunet/metrics.py, instance_stats_from_pairs) is a function
 * of their sparse contingency table.
 * eunet_label_pairs: a and b are p planes of h x w ids, each int32 or int64 independently (a_bytes / b_bytes 4 or
 *   8).  For every pixel with a >= 0 and b >= 0 and not (a == 0 && b == 0) the count of the key (plane, a, b) grows
 *   by one: background against background is counted nowhere, and a negative id on either side marks an ignored
 *   pixel, counted nowhere.  An id above EUNET_PAIRS_MAX_ID on a pixel that is not ignored is counted in *invalid
 *   (device int64) and nowhere else.  The table is an open-addressing hash table of `capacity` slots (a power of two
 *   in 2..2^30): keys int64 [capacity] = plane << 48 | a << 24 | b, -1 where empty; counts int32 [capacity].  The
 *   call clears the table, *overflow and *invalid first.  An insert that finds min(capacity, 64) successive slots
 *   taken adds one to *overflow (device int32) and stores nothing: when *overflow != 0 the table is incomplete and
 *   the call is repeated with a larger one.  Integer and order-free.  Limits: 1 <= h, w <= 8192, 1 <= p <= 65535,
 *   p h w < 2^31.
 * eunet_labels_from_stack: masks uint8 [n][h][w] (non-zero = set), ids int32 [n] on the device -> out int32 [h][w],
 *   out[i] = ids[j] for the largest j with masks[j][i] != 0 and ids[j] > 0, 0 where there is none (later planes
 *   overwrite earlier ones: eunet_rasterize_polygons' rule); where ignore (uint8 [h][w], may be null) is non-zero,
 *   out[i] = -1.  *overlap (device int64, zeroed by the call) = the pixels claimed by more than one selected plane,
 *   ignored pixels included.  n may be 0 (masks and ids are then not read).  n <= 65535, h w < 2^31. */
#define EUNET_PAIRS_MAX_ID 16777215 /* 2^24 - 1 */
int eunet_label_pairs(const void* a, int a_bytes, const void* b, int b_bytes, int p, int h, int w, int64_t* keys,
                      int32_t* counts, long long capacity, int32_t* overflow, int64_t* invalid, void* stream);
int eunet_labels_from_stack(const uint8_t* masks, int n, int h, int w, const int32_t* ids, const uint8_t* ignore,
                            int32_t* out, int64_t* overlap, void* stream);

/* ---- per-cell measurements (cellprops.hip) ------------------------------------------
 * No reference line: the reference measures nothing per cell beyond the counts.  This comment is the definition.
 * eunet_cell_stats: ids are p planes of h x w ids, int32 or int64 (elem_bytes 4 or 8); id 0 is background and the
 *   ids 1..n are measured (0 <= n <= EUNET_PAIRS_MAX_ID).  A pixel whose id is negative or above n is counted in
 *   skipped[plane] (device int64 [p], zeroed by the call), is measured nowhere and is "not this label" for its
 *   neighbours.  With x the column and y the row index of a pixel:
 *   geom int64 [p][n + 1][EUNET_CELL_GEOM_COLS], written entirely by the call (it need not be cleared); row 0 of a
 *   plane stays zero; row i holds for the pixels of id i
 *     0          area
 *     1, 2       sum x, sum y
 *     3, 4, 5    sum x^2, sum y^2, sum x y
 *     6 .. 9     x0, y0, x1, y1 of the bounding box, inclusive; a label with no pixel has w, h, -1, -1
 *     10 .. 13   the bit-quad counts q1, q2, q3, qd (Gray 1971): over all (h + 1) (w + 1) windows of 2 x 2 pixels
 *                of the plane padded by one pixel of "outside", by how many of the window's four pixels carry the
 *                label: exactly one -> q1, two that share an edge -> q2, the two on a diagonal -> qd, three -> q3
 *                (four: not counted, the area covers them).  A window of up to four labels counts for each.
 *   From these, on the host (eunet/metrics.py, cell_measurements): the crack perimeter q1 + q2 + q3 + 2 qd (unit
 *   pixel edges between the label and anything else, the image border included), the Euler number (q1 - q3 - 2 qd)
 *   / 4 for 8-connectivity and (q1 - q3 + 2 qd) / 4 for 4-connectivity, and Gray's perimeter estimate
 *   q2 + (q1 + q3 + 2 qd) / sqrt 2.
 *   image: null, or uint8 [h][w][c] (HWC, c = 1..3; c = 0 without an image) shared by all planes, of any byte
 *   alignment (a lane reads its four pixels as dwords where they are 4-byte aligned and byte by byte otherwise);
 *   inten int64 [p][n + 1][c][4], written entirely by the call: per channel sum v, sum v^2, min v, max v over the
 *   label's pixels; a label with no pixel has min 255 and max 0; row 0 stays zero.  inten is not touched without
 *   an image.
 *   Every value is an integer below 2^63 (sum x^2 <= 8191^2 2^26) formed with 64-bit integer atomics, the bounding
 *   box and the intensity range with signed atomic min / max on the values themselves: the tables do not depend on
 *   the order of evaluation.  One pass over the ids and the image (a run of one id within 256 pixels of a row adds
 *   its sums once, in closed form) and one pass over the windows (only windows that are not of one value add).
 *   Limits: 1 <= h, w <= EUNET_EDT_MAX_SIDE, 1 <= p <= 65535.  No host synchronisation, no allocation. */
#define EUNET_CELL_GEOM_COLS 14
int eunet_cell_stats(const void* ids, int elem_bytes, int p, int h, int w, int n, const uint8_t* image, int c,
                     int64_t* geom, int64_t* inten, int64_t* skipped, void* stream);

/* ---- per-cell convex hulls (hull.hip) -------------------------------------------------
 * No reference line: the reference measures nothing per cell.  This comment is the definition.
 * eunet_cell_hulls: ids, elem_bytes, p, h, w, n as for eunet_cell_stats; ids 0, negative ids and ids above n are not
 *   measured.  The point set of label i is the four corner lattice points (x, y), (x + 1, y), (x, y + 1),
 *   (x + 1, y + 1) of every pixel (column x, row y) carrying id i: the hull is that of the pixel SQUARES, so its area
 *   is >= the label's area and the solidity area / convex area lies in (0, 1], 1 for a rectangle.
 *   The hull is strictly convex: no vertex lies on the segment between its neighbours.  The vertices are listed from
 *   the corner with the smallest y, then the smallest x, along the top edge first: top edge left to right, right chain
 *   downwards, bottom edge right to left, left chain upwards.  With y pointing down this makes the shoelace sum
 *   sum_k (x_k y_{k+1} - x_{k+1} y_k) positive; the unit pixel gives (0,0), (1,0), (1,1), (0,1) and the sum 2.  A label
 *   with a pixel has at least 4 vertices and at most 2 (rows + 1), rows = y1 - y0 + 1 of its bounding box.
 *   The caller gives the row layout, which it has from eunet_cell_stats' bounding boxes (eunet/ops.py, cell_hulls):
 *   with L = p (n + 1) and r = plane (n + 1) + id the flat index of a label, row_off int64 [L + 1] (device) is the
 *   exclusive cumulative sum of the labels' row counts (0 for id 0 and for a label with no pixel), R = row_off[L] <=
 *   EUNET_CELL_HULL_MAX_ROWS, and row_y0 int32 [L] (device) the image row of a label's first row.
 *   Every entry of the four outputs is written by the call; a label with no pixel has all zeros.
 *   ext int32 [R][2]: row row_off[r] + (y - row_y0[r]) holds the smallest and the largest x of label r in image row y;
 *     a row of the label's box where it has no pixel holds (w, -1).
 *   verts int32 [2 (R + L)][2]: the hull vertices (x, y) of label r start at slot 2 (row_off[r] + r), of which the
 *     label owns 2 (rows + 1); slots past the label's vertex count are zero.
 *   hull int64 [p][n + 1][EUNET_CELL_HULL_COLS]:
 *     0        the number of hull vertices
 *     1        twice the hull's area (the shoelace sum)
 *     2        sum over the edges of floor(2^16 sqrt((double)(dx^2 + dy^2))): the hull's perimeter in 2^-16 pixels, the
 *              fp64 square root taken from the exact integer
 *     3        the largest squared distance between two hull vertices (the maximum Feret diameter squared)
 *     4 .. 7   xa, ya, xb, yb of the vertex pair (i < j) attaining it; among equals the lexicographically smallest
 *              (i, j) in vertex order
 *     8        c: per hull edge e = (v_k -> v_{k+1}), c_e = the maximum over all vertices v of cross(v_{k+1} - v_k,
 *              v - v_k), an integer >= 0; column 8 is the c_e of the edge with the smallest c_e^2 / |e|^2 (compared
 *              exactly, in 128-bit products: c_e^2 |e'|^2 reaches 2^81), the smallest k among equals
 *     9, 10    dx, dy of that edge; the minimum Feret diameter is c / sqrt(dx^2 + dy^2), measured across the edge
 *   outside int64 [p]: the measured pixels whose row falls outside [row_y0[r], row_y0[r] + rows) of their label, or
 *     whose label's slice does not lie inside 0..R in order.  They are stored nowhere: when outside is not all zero the
 *     layout is not this map's and the tables mean nothing.  No store leaves the tables whatever the layout holds.
 *   One pass over the ids (a run of one id within 256 pixels of a row issues one 32-bit atomic min and one atomic max)
 *   and one wave per label: Andrew's monotone chain over the row extents, which are sorted by y already, then the
 *   vertex pairs and edge x vertex pairs shared by the 64 lanes.  Every value is an integer and does not depend on the
 *   order of evaluation.  Limits as eunet_cell_stats; pointers 8-byte aligned (row_y0 4).  No host synchronisation, no
 *   allocation. */
#define EUNET_CELL_HULL_COLS 11
#define EUNET_CELL_HULL_MAX_ROWS 268435456 /* 2^28 */
int eunet_cell_hulls(const void* ids, int elem_bytes, int p, int h, int w, int n, const int64_t* row_off,
                     const int32_t* row_y0, int32_t* ext, int32_t* verts, int64_t* hull, int64_t* outside,
                     void* stream);

/* ---- nearest-cell transform, label expansion and cell contacts (neighbors.hip) ------------------
 * No reference line: the reference counts cells and relates none to another.  This comment is the definition.
 * ids are p planes of h x w ids, int32 or int64 (elem_bytes 4 or 8), as for eunet_cell_stats.  With x the column and
 * y the row of a pixel, its linear index in its plane is y w + x.
 * eunet_nearest_site: the feature transform.  The sites of a plane are its pixels with id >= 1; ids <= 0 are not
 *   sites.  dist int32 [p][h][w] = the exact squared Euclidean distance of every pixel to the nearest site of its own
 *   plane, site int32 [p][h][w] = the linear index of that site.  Tie rule: among the sites at the minimum distance the
 *   one of smallest linear index wins, so (dist, site) is the lexicographic minimum of (d^2, index) over all sites of
 *   the plane.  A site is its own nearest site (0, own index).  A plane without a site holds EUNET_EDT_NONE and -1.
 *   Two kernels: a column pass (one thread per column, the row of the nearest site of the own column, the smaller row
 *   among two equally near, -1 without one) and a row pass (one block per row, scanning outward from r = 0 and
 *   stopping at the first r with r^2 > best, strictly: a candidate at r^2 == best in the pixel's own row ties the
 *   best and may have the smaller index).  The column pass leaves its rows in site, the row pass works in place.
 * eunet_expand_label_map: skimage.segmentation.expand_labels with the tie rule above (the name eunet_expand_labels
 *   is the instance unit's label map -> mask stack).  out has the element size and shape of ids and must not overlap
 *   them.  out(x) = ids(x) where ids(x) != 0: negative ids ("ignore") are kept and never overwritten, and they are no
 *   sites.  Elsewhere out(x) = ids(site(x)) when dist(x) <= limit2 and 0 otherwise; a plane without a site stays 0
 *   where it was 0.  limit2 = floor(distance^2), formed by the caller in 64 bits; limit2 < 0 means no limit, the
 *   discrete Voronoi partition of the plane.  ws int32 [p][h][w] is the column pass's output; the row pass gathers
 *   the id while it still holds the winner and scans no further than r^2 <= limit2.
 * eunet_label_contacts: the sparse adjacency table of one id map.  Connectivity 4: every pixel is paired with its
 *   right and its lower neighbour; connectivity 8: also with its lower-left and lower-right neighbour, so every
 *   unordered pair of adjacent pixels is seen once.  A pair carrying two different ids >= 1 adds 1 to the count of the
 *   key (plane, min id, max id); 0 and negative ids take no part.  At connectivity 4 a count is the number of unit
 *   pixel sides the two labels share.  An id above EUNET_PAIRS_MAX_ID on any pixel is counted in *invalid (device
 *   int64) and takes no part.  keys, counts, capacity, overflow: the open-addressing table of eunet_label_pairs with
 *   the key plane << 48 | min << 24 | max, cleared by the call together with *invalid; when *overflow != 0 the table
 *   is incomplete and the call is repeated with a larger one.  One pass; a run of equal keys along a row within 256
 *   pixels inserts once, with its length.
 * Every value is an integer and does not depend on the order of evaluation: two runs give identical bits.  Limits
 * are eunet_edt_sq's: 1 <= h, w <= EUNET_EDT_MAX_SIDE, 1 <= p <= 65535.  ids and out aligned to elem_bytes, the int32
 * arrays to 4 and the int64 ones to 8 bytes.  No host synchronisation, no allocation. */
int eunet_nearest_site(const void* ids, int elem_bytes, int p, int h, int w, int32_t* dist, int32_t* site,
                       void* stream);
int eunet_expand_label_map(const void* ids, int elem_bytes, int p, int h, int w, long long limit2, int32_t* ws,
                           void* out, void* stream);
int eunet_label_contacts(const void* ids, int elem_bytes, int p, int h, int w, int connectivity, int64_t* keys,
                         int32_t* counts, long long capacity, int32_t* overflow, int64_t* invalid, void* stream);

/* ---- signed distance maps and the boundary loss (sdf.hip) ---------------------------
 * No reference line to cite: every loss of the reference is a region loss.  The boundary loss of Kervadec et al.,
 * "Boundary loss for highly unbalanced segmentation" (MIDL 2019), integrates the class probability against the
 * signed distance map of the ground truth; this comment is the definition of both.
 *
 * eunet_signed_distance: target int64 [N][H][W] -> out fp32 [N][K][H][W], K = 1..3.  Per sample n and class c the
 * region is R = {x : target(x) = c}; for K = 1 the single class is "foreground", R = {x : target(x) >= 1}
 * (EUNET_BCE_TARGET_FOREGROUND's rule; the call writes [target >= 1 and not ignored] to an int64 scratch plane of
 * the workspace and transforms that).  With the exact int32 values of eunet_edt_sq,
 *   Dout(x) = the squared distance to the nearest pixel of R         (EUNET_EDT_EQ)
 *   Din(x)  = the squared distance to the nearest pixel not in R     (EUNET_EDT_NE)
 *   phi_c(x) = +sqrt(Dout(x))        for x outside R
 *   phi_c(x) = -(sqrt(Din(x)) - 1)   for x in R
 * which is Kervadec's dist(neg) neg - (dist(pos) - 1) pos: a pixel of R that touches the complement has phi = 0,
 * the first pixel outside has phi = +1.
 *   Empty:  if R or its complement is empty in sample n, phi_c = 0 on the whole sample (there is no contour to pull
 *           towards; EUNET_EDT_NONE never reaches a square root).
 *   Ignore: a pixel equal to ignore_index (EUNET_NO_IGNORE = none) belongs to no class: it is outside every R and
 *           is a site of every complement, and its own phi_c is 0 for every c, so it adds nothing to the loss.
 *           The consequence: an ignored region acts as "not the class" and attracts the contour of an adjacent
 *           region at distance 1 (a region pixel next to it has phi = 0, as next to any other class).  For K >= 2
 *           ignore_index must not be one of 0 .. K-1 (EUNET_ERR_INVALID).  Any other value outside 0 .. K-1 is
 *           simply of no class.
 *   out = scale * clamp(phi, -clip, +clip); clip = 0 means no clamp, otherwise clip must be finite and > 0; scale
 *           must be finite.  The square root, the clamp and the scaling are in fp64 from the exact integer, and the
 *           result is rounded to fp32 once.
 * ws (eunet_signed_distance_workspace_bytes): int32 [2][N][K][H][W], the EQ and the NE transform, followed for
 * K = 1 by the int64 [N][H][W] foreground plane; 8-byte aligned.  One elementwise kernel after the two transforms
 * reads both planes and the target and writes out, 16 bytes per lane when H W % 4 == 0 and the pointers are
 * 16-byte aligned.  Limits are eunet_edt_sq's (h, w <= 8192, n <= 65535); no host synchronisation, no allocation. */
int eunet_signed_distance_workspace_bytes(int n, int k, int h, int w, size_t* bytes);
int eunet_signed_distance(const int64_t* target, int n, int k, int h, int w, int ignore_index, float clip,
                          float scale, int32_t* ws, float* out, void* stream);
/* eunet_boundary_loss_fwd: logits z and dist fp32 [N][K][H][W], K = 1..3, N <= 64.  dist is any map (the loss is
 * linear in the probabilities): eunet_signed_distance's, clipped, normalised or otherwise prepared.
 *   p = softmax over c of z (EUNET_BOUNDARY_SOFTMAX, K = 2, 3; K = 1 is EUNET_ERR_INVALID) or p_c = sigmoid(z_c)
 *   (EUNET_BOUNDARY_SIGMOID, K = 1..3); w = class_weight, K host floats (null: all 1; Kervadec's idc = [1] is
 *   (0, 1, 0)); Kw = max(1, #{c < K : w_c != 0}).
 *   loss     = sum_{n,c,x} w_c p_c(x) dist_c(x) / (N H W Kw)
 *   parts[n] = the same sum over sample n / (H W Kw)              (nullable; loss = the mean of parts)
 * ws: eunet_boundary_loss_workspace_bytes (one float per sample and tile of 1024 pixels).  The partials are summed
 * in fp64 in a fixed order: two runs are bit-identical.
 * eunet_boundary_loss_bwd: glogits = (*gloss) d loss / d z (gloss: device scalar g), one pass, nothing saved:
 *   softmax:  g p_j (w_j dist_j - sum_c w_c p_c dist_c) / (N H W Kw)
 *   sigmoid:  g w_c dist_c p_c (1 - p_c) / (N H W Kw)
 * The softmax is max-subtracted and the sigmoid pair comes from one exp, so logits of +-100 neither overflow nor
 * cancel. */
enum { EUNET_BOUNDARY_SOFTMAX = 0, EUNET_BOUNDARY_SIGMOID = 1 };
int eunet_boundary_loss_workspace_bytes(int n, int h, int w, size_t* bytes);
int eunet_boundary_loss_fwd(const float* logits, const float* dist, int n, int k, int h, int w, int activation,
                            const float* class_weight, float* loss, float* parts, void* ws, void* stream);
int eunet_boundary_loss_bwd(const float* logits, const float* dist, int n, int k, int h, int w, int activation,
                            const float* class_weight, const float* gloss, float* glogits, void* stream);

/* ---- Lovasz losses (lovasz.hip) -----------------------------------------------
 * No reference line to cite: every loss of the reference is a sum over pixels, and its metrics are IoU.  The
 * Lovasz-Softmax and Lovasz hinge losses of Berman, Triki and Blaschko, "The Lovasz-Softmax loss: a tractable
 * surrogate for the optimization of the intersection-over-union measure in neural networks" (CVPR 2018), are the
 * convex extension of the Jaccard set loss; this comment is their definition here.
 *
 * Elements and segments.  logits fp32 [N][K][H][W] (the shape rule of the per-pixel losses, and N H W < 2^31),
 * target int64 [N][H][W].  per_image = 0: S = K segments (one per class) of L = N H W elements, an element's index
 * in its segment being n H W + y W + x.  per_image = 1: S = N K segments, segment n K + c, of L = H W elements with
 * the index y W + x.
 * Errors and flags of element (n, c, x):
 *   EUNET_LOVASZ_SOFTMAX (K = 2, 3): p = softmax over c (max-subtracted), fg = [target == c], e = |fg - p_c|
 *   EUNET_LOVASZ_HINGE   (K = 1..3, one binary problem per logit z_c): fg = [target == c], for K = 1
 *       fg = [target >= 1] (EUNET_BCE_TARGET_FOREGROUND's rule); e = 1 - z_c (2 fg - 1).  The loss uses max(e, 0),
 *       the order e itself (Berman's lovasz_hinge_flat).
 *   flag = 0 background, 1 foreground, 2 ignored: target == ignore_index (EUNET_NO_IGNORE = none), or a target
 *       outside 0 .. K-1 (for the hinge with K = 1: below 0), which is also counted (`bad`, reported the way
 *       eunet_bce_dice_fwd's last sum is).  A flag-2 element takes part in nothing; eunet_lovasz_errors writes 0
 *       for its error.
 * Order.  In a segment the valid elements are ordered by error descending, equal errors by index ascending (the
 * sort is stable), the ignored ones follow in index order.  -0 counts as +0; a NaN sorts ahead of +inf (as
 * torch.sort(descending=True) places it; the loss is then NaN, and nothing is read or stored out of range).
 * Gradient of the extension, from integers.  G = the segment's foreground count, V = its valid count, F_r = the
 * foreground count among the first r sorted elements (r = 1..V), I_r = G - F_r, U_r = G + r - F_r:
 *   g_r = 1 / U_r                        the element of rank r is foreground
 *   g_r = I_r / ((U_r - 1) U_r)          it is background
 *   g_1 = 1, g_r = 0 otherwise           G = 0
 * (J_r - J_{r-1} of the paper in closed form), evaluated as double(I) / (double(U - 1) * double(U)) or
 * 1.0 / double(U) and rounded once to fp32: correctly rounded operations on integers, the same bits anywhere.
 * Loss.  l_s = sum_r eb_(r) g_r, eb = e (softmax) or max(e, 0) (hinge), in fp64 in a fixed order (per-block
 * partials, one finalize block): two runs are bit-identical.  A segment is selected by classes_mode:
 * EUNET_LOVASZ_PRESENT G > 0, EUNET_LOVASZ_ALL V > 0, EUNET_LOVASZ_LISTED V > 0 and bit c of class_mask set.
 * per_image = 0: loss = the mean of l_s over the selected segments; per_image = 1: the mean over the N samples of
 * the mean over each sample's selected segments.  An empty mean is 0.  The selection is made on the device.
 *
 * eunet_lovasz_errors: errors fp32 and flags uint8, both [N][K][H][W].
 * eunet_lovasz_sort: errors fp32 and flags uint8 [S][L] (S <= 65535, L < 2^31; a flag >= 2 is ignored) -> order
 *   int32 [S][L] (the permutation: order[s][r] = the index of the element of rank r+1, ignored ones last), grad
 *   fp32 [S][L] (g at the element's own index, 0 where ignored), counts int64 [S][2] = (G, V).
 * eunet_lovasz_fwd: weights fp32 [N][K][H][W] = g at every element's own position (0 where ignored), factor fp32
 *   [S] = the segment's share of the mean (1 / #selected, per_image: 1 / (N #selected of the sample); 0 for a
 *   segment that is not selected), loss 1 fp32, parts (nullable) fp32 [S] = l_s, NaN where not selected, counts
 *   (nullable) int64 [S][2], bad (nullable) 1 fp32 = the out-of-range targets.  The scaling of weights is left to
 *   the backward: it multiplies by factor[segment] as it reads.
 * eunet_lovasz_bwd: glogits = (*gloss) d loss / d z with w_c = weights factor[segment], one pass (16 bytes per lane
 *   when H W % 4 == 0 and the pointers are 16-byte aligned):
 *   softmax: sum_c w_c s_c p_c ([c == j] - p_j), s_c = sign(p_c - fg_c), sign(0) = 0 (torch.abs's derivative)
 *   hinge:   -w_c (2 fg_c - 1) [e_c > 0]
 * ws: eunet_lovasz_workspace_bytes(S, L) for S segments of L elements, a function of the shape alone: keys and
 * payloads, both double-buffered (16 bytes per element), the sort's block x digit table, the scan's block counts, the
 * per-block count rows and
 * the fp64 partials; 256-byte aligned.  All K classes are sorted at once.  Every call issues launches on the given
 * stream only: no host read-back, no allocation. */
enum { EUNET_LOVASZ_SOFTMAX = 0, EUNET_LOVASZ_HINGE = 1 };
enum { EUNET_LOVASZ_PRESENT = 0, EUNET_LOVASZ_ALL = 1, EUNET_LOVASZ_LISTED = 2 };
int eunet_lovasz_workspace_bytes(int s, int l, size_t* bytes);
int eunet_lovasz_errors(const float* logits, const int64_t* target, int n, int k, int h, int w, int activation,
                        int ignore_index, float* errors, uint8_t* flags, void* stream);
int eunet_lovasz_sort(const float* errors, const uint8_t* flags, int s, int l, int32_t* order, float* grad,
                      int64_t* counts, void* ws, void* stream);
int eunet_lovasz_fwd(const float* logits, const int64_t* target, int n, int k, int h, int w, int activation,
                     int per_image, int classes_mode, int class_mask, int ignore_index, float* weights,
                     float* factor, float* loss, float* parts, int64_t* counts, float* bad, void* ws, void* stream);
int eunet_lovasz_bwd(const float* logits, const int64_t* target, int n, int k, int h, int w, int activation,
                     int per_image, const float* weights, const float* factor, const float* gloss, float* glogits,
                     void* stream);

/* ---- overlap-tile inference (tiling.hip) -------------------------------------
 * Prediction on an image larger than one forward pass (no reference line: the reference's only answer to a
 * large field of view is the resize down to max_size, dataset.py; overlap-tile prediction is the strategy
 * of the U-Net paper, Ronneberger et al. 2015, section 2).  The image [C][h][w] is extended to hp x wp = h, w rounded up to
 * multiples of 32 by the reflect pad to the bottom / right of train_eval.py:397-417 (position r >= n reads
 * 2 (n - 1) - r; hp - h < h and wp - w < w, as F.pad demands) and cut into ny x nx tiles of th x tw pixels
 * (multiples of 32, th <= hp, tw <= wp).  Along an axis of padded length L, tile extent e and stride S (a
 * positive multiple of 32): n = 1 if L <= e else ceil((L - e) / S) + 1 tiles with origins
 * o(i) = min(i S, L - e); tile number = iy * nx + ix.  The geometry is passed by value and the counts are
 * derived from it; every offset is 64-bit.
 * eunet_tile_gather: tiles [count][C][th][tw] (16-byte aligned) = tile numbers first .. first + count - 1
 * of the extended image, read through the reflect index (no padded copy is made); C = 1..4.
 * eunet_tile_blend: tile logits [ny nx][K][th][tw] (K = 1..3, 16-byte aligned) -> probs [K][h][w],
 *   probs[k][y'][x'] = sum_n w_n act(logits_n)[k] / sum_n w_n  over the tiles n that cover (y, x), summed in
 * increasing tile number in fp32 (one thread per pixel: deterministic, no atomics), cropped to h x w, with
 * y' = flip_h ? h - 1 - y : y and x' likewise (eunet_softmax_crop's flips).  act: EUNET_TILE_ACT_NONE, _SOFTMAX
 * (over K, eunet_softmax_crop's arithmetic) or _SIGMOID (eunet_sigmoid_crop's).  w_n = wy(ty) wx(tx) at the
 * tile-local position; per axis, for a tile at origin o:
 *   EUNET_TILE_CROP      1 if (o > 0 ? margin : 0) <= t < e - (o + e < L ? margin : 0) else 0; margin a
 *                        multiple of 16 with S + 2 margin <= e wherever an axis has more than one tile
 *   EUNET_TILE_CONSTANT  1 (S <= e)
 *   EUNET_TILE_GAUSSIAN  wy[t] / wx[t]: device tables of th / tw floats (wx 16-byte aligned); null otherwise
 * In crop mode at most two cores overlap per axis, so sum w is 1, 2 or 4 and the mean of bit-equal tile
 * values is exact: with margin >= the network's receptive radius (eunet.tiling.RECEPTIVE_MARGIN) the result
 * is the whole-image forward's, bit for bit. */
#define EUNET_TILE_CROP 0
#define EUNET_TILE_CONSTANT 1
#define EUNET_TILE_GAUSSIAN 2
#define EUNET_TILE_ACT_NONE 0
#define EUNET_TILE_ACT_SOFTMAX 1
#define EUNET_TILE_ACT_SIGMOID 2
int eunet_tile_gather(const float* image, int c, int h, int w, int hp, int wp, int th, int tw, int sy,
                      int sx, int first, int count, float* tiles, void* stream);
int eunet_tile_blend(const float* logits, int k, int h, int w, int hp, int wp, int th, int tw, int sy,
                     int sx, int mode, int margin, const float* wy, const float* wx, int activation,
                     int flip_h, int flip_w, float* probs, void* stream);

/* ---- instance-level evaluation (instances.hip) ------------------------------
 * Pairwise mask overlap (metrics.py:61-194, calculate_instance_metrics: the calculate_iou
 * of metrics.py:12-18 per (prediction, ground-truth) pair).  eunet_pack_masks: masks
 * uint8 [n][h][w] (non-zero = set) -> packed uint64 [n][ceil(hw/64)], bit b of word j =
 * pixel 64 j + b, the tail word zero-filled; areas int64 [n] = set pixels per mask.
 * h * w < 2^31. */
int eunet_pack_masks(const uint8_t* masks, int n, int h, int w, uint64_t* packed, int64_t* areas,
                     void* stream);
/* eunet_pack_masks in the same single pass plus the bounding box of the set pixels
 * (cv2.boundingRect(mask), train_eval.py:959, 978): packed and areas as above, bbox int32
 * [n][4] = (xmin, ymin, xmax, ymax), inclusive; an empty mask gives (w, h, -1, -1).
 * cv2's (x, y, w, h) = (xmin, ymin, xmax - xmin + 1, ymax - ymin + 1) is formed by the caller. */
int eunet_pack_masks_bbox(const uint8_t* masks, int n, int h, int w, uint64_t* packed,
                          int64_t* areas, int32_t* bbox, void* stream);
/* COCOeval.evaluateImg's greedy matching (pycocotools, behind calculate_coco_metrics,
 * metrics.py:283-294, collected at train_eval.py:951-992) of one image: every class, both
 * IoU types and all thresholds in one launch.  Device inputs: inter int64 [d][g] (pixel
 * overlaps), area_d [d] / area_g [g] int64 pixel areas, box_d [d][4] / box_g [g][4] int32
 * (x, y, w, h), 16-byte aligned, cls_d [d] / cls_g [g] int32 in {0, 1}; thrs: t doubles on
 * the HOST.  Detections come in visiting order (per class: stable sort by descending score,
 * cut at maxDets).  match int32 [2][t][d], type 0 bbox / 1 segm: the index (0..g-1) of the
 * ground truth the detection takes, or -1: the untaken ground truth of the detection's class
 * with the largest IoU >= min(thr, 1 - 1e-10), the larger index on equal IoU.  IoU in fp64:
 * segm inter / (area_d + area_g - inter) (0 when inter == 0), bbox the integer intersection
 * rectangle over the integer union (0 when the rectangles do not meet).  Limits: d <= 4096,
 * g <= 8192, t <= 16.  Reads the classes back to check them: synchronises the stream. */
int eunet_coco_match(const int64_t* inter, const int64_t* area_d, const int64_t* area_g,
                     const int32_t* box_d, const int32_t* box_g, const int32_t* cls_d,
                     const int32_t* cls_g, int d, int g, const double* thrs, int t, int32_t* match,
                     void* stream);
/* inter int64 [p][g] = sum over words of popcount(a[p][.] & b[g][.]) (np.logical_and(m1,
 * m2).sum(), metrics.py:14), zeroed by the call.  IoU = inter / (area_p + area_g - inter)
 * is formed on the host.  Masks may overlap one another. */
int eunet_pairwise_overlap(const uint64_t* a, int p, const uint64_t* b, int g, long long words,
                           int64_t* inter, void* stream);
/* cv2.erode / cv2.dilate / cv2.morphologyEx(MORPH_OPEN) (train_eval.py:674, 702, 712, 719,
 * 725, 749, 756, 768, 775) of a uint8 [h][w] image by the element cv2.getStructuringElement(
 * cv2.MORPH_ELLIPSE, (k, k)) returns (train_eval.py:673, 699, 767): elem 0 -> k = 2,
 * 1 -> k = 3, 2 -> k = 5.  OpenCV conventions: un-reflected element, anchor (k/2, k/2),
 * pixels outside the image neither erode nor dilate.  iterations > 1 ping-pong through tmp
 * ([h][w], may be null for one iteration); src, dst, tmp distinct. */
int eunet_morph_u8(const uint8_t* src, uint8_t* dst, uint8_t* tmp, int h, int w, int elem,
                   int dilate, int iterations, void* stream);
/* skimage.measure.label(img, connectivity=2, return_num=True) (train_eval.py:678, 705, 720,
 * 750, 769) of a uint8 [h][w] image (non-zero = set): labels int32 [h][w], numbered 1..n in
 * raster order of each component's first pixel; *n_out (device int32) = n; areas int32
 * [areas_cap >= ceil(h/2) * ceil(w/2)] = pixels per label, zeroed by the call.
 * ws: eunet_label_workspace_bytes of device workspace. */
int eunet_label_workspace_bytes(int h, int w, size_t* bytes);
int eunet_label_components(const uint8_t* img, int h, int w, int32_t* labels, int32_t* n_out,
                           int32_t* areas, int areas_cap, int32_t* ws, void* stream);
/* The same with the connectivity as an argument: 8 is eunet_label_components; 4 unites a pixel with its W and N
 * neighbours only (scipy.ndimage.label's default structure, visualization.py:1753-1817), same numbering, and
 * areas_cap >= ceil(h w / 2) (the checkerboard). */
int eunet_label_components_conn(const uint8_t* img, int h, int w, int32_t* labels, int32_t* n_out,
                                int32_t* areas, int areas_cap, int32_t* ws, int connectivity, void* stream);
/* cv2.findContours(mask, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)[0][0] + cv2.arcLength(., True)
 * (train_eval.py:819-821) for every label k = 1..n of an int32 label map at once (Suzuki-Abe
 * outer-border following, 8-connectivity): stats int32 [n][8] = (axis-aligned chain steps,
 * diagonal chain steps, area, start pixel, bounding box x0, y0, x1, y1); the perimeter is
 * n_axis + n_diag * sqrt(2) on the host.  A label with several components is followed on the
 * one whose raster-first pixel comes last (OpenCV lists contours in reverse order of
 * discovery).  ws: int32 [h * w] of device workspace. */
int eunet_outer_perimeter(const int32_t* labels, int h, int w, int n, int32_t* stats, int32_t* ws,
                          void* stream);
/* Per-pixel helpers of semantic_to_instances (train_eval.py:654-850), n elements each:
 * mask_eq: dst = (src == value) as 0/1 for an int32 / int64 source (elem_bytes 4 / 8; :666,
 * :689, :710), count (device int64) = ones; mask_and: cv2.bitwise_and of two 0/1 images + its
 * sum (:713-716); write_label: markers[mask != 0] = label (:694, :729 ...); relabel_table:
 * markers[i] = table[labels[i] - 1] where that entry is > 0 (every region under 200 px in
 * one pass, :692-695); expand_labels: out uint8 [m][n], out[table[labels[i] - 1]][i] = 1
 * where the entry is >= 0 (instance_mask = final_markers == label_id, :805), zeroed first. */
int eunet_mask_eq(const void* src, int elem_bytes, long long n, long long value, uint8_t* dst,
                  int64_t* count, void* stream);
int eunet_mask_and(const uint8_t* a, const uint8_t* b, long long n, uint8_t* dst, int64_t* count,
                   void* stream);
int eunet_write_label(const uint8_t* mask, long long n, int label, int32_t* markers, void* stream);
int eunet_relabel_table(const int32_t* labels, long long n, const int32_t* table, int n_labels,
                        int32_t* markers, void* stream);
int eunet_expand_labels(const int32_t* labels, long long n, const int32_t* table, int n_labels,
                        int m, uint8_t* out, void* stream);

/* ---- dual-branch fusion (fusion.hip) -----------------------------------------
 * SMP-path EnhancedUNet (models.py:253-302, 316-333): ff = cat(unetpp, deeplab) with the
 * branch outputs za, zb NHWC fp32 [n,h,w,K]; all gate tensors fp32 NHWC.  Per-tile
 * partials: BN statistics in the eunet_bn_finalize layout ([tiles][2][C] + counts),
 * gradient partials [tiles][cols] reduced with eunet_colsum.  K <= 3.
 * tiles: pixel tiles of the per-pixel kernels; gate_tiles: 16x32 tiles of gate_bwd3. */
int eunet_fusion_tiles(int n, int h, int w, int* tiles, int* gate_tiles);
/* attention_gate.0 (3x3, 2K->K, no bias; models.py:280): a [P][K] + BN1 stats; also
 * copies za, zb to the NCHW aux outputs (_aux_outputs, models.py:329-332) */
int eunet_gate_fwd(const float* za, const float* zb, int n, int h, int w, int k, const float* w1,
                   float* a, float* st1, float* aux_a, float* aux_b, void* stream);
/* GELU(BN1) + attention_gate.3 (1x1 K->2K, models.py:282-283): b [P][2K] + BN2 stats */
int eunet_gate_mid_fwd(const float* za, const float* zb, int n, int h, int w, int k, const float* a,
                       const float* sc1, const float* sh1, const float* w2, float* b, float* st2,
                       void* stream);
/* Sigmoid(BN2) * ff (models.py:284, 322-323) -> f2 [n,h,w,8] view c = 2K, compute dtype */
int eunet_gate_out_fwd(const float* za, const float* zb, int n, int h, int w, int k, const float* b,
                       const float* sc2, const float* sh2, const eunet_act* f2, void* stream);
/* fusion_head.11 on relu(bn3(y3)) + fusion_residual on f2 (models.py:294, 296, 325-328)
 * -> out NCHW fp32 [n,K,h,w] */
int eunet_fusion_out_fwd(const float* za, const float* zb, int k, const eunet_act* y3,
                         const float* sc3, const float* sh3, const float* w11, const float* b11,
                         const float* b, const float* sc2, const float* sh2, const float* wr,
                         const float* br, float* out, void* stream);
/* backward of the residual + output layout: gz [P][K] (NHWC, for eunet_conv1x1_bwd),
 * gf2res [P][2K] = Wr^T gout, part [tiles][K*2K + K] = (dWr, dbr) partials */
int eunet_fusion_out_bwd(const float* za, const float* zb, int n, int h, int w, int k,
                         const float* gout, const float* b, const float* sc2, const float* sh2,
                         const float* wr, float* gz, float* gf2res, float* part, void* stream);
/* gate backward: (1) sigmoid/product: gffd [P][2K], gbhat [P][2K], BN2 partials [tiles][2][2K];
 * (2) BN2 apply, 1x1, GELU': gabn [P][K], partials [tiles][2K*K + 2K] = (dWg2, BN1 sums);
 * (3) BN1 apply + transposed 3x3 + aux-output gradients (nullable, NCHW) -> branch gradients
 *     gz_a, gz_b [P][K]; partials [gate_tiles][K*2K*9] of dWg1 */
int eunet_gate_bwd1(const float* za, const float* zb, int k, const eunet_act* gf2conv,
                    const float* gf2res, const float* b, const float* mean2, const float* istd2,
                    const float* gam2, const float* bet2, float* gffd, float* gbhat, float* part,
                    void* stream);
int eunet_gate_bwd2(int n, int h, int w, int k, const float* gbhat, const float* b,
                    const float* mean2, const float* istd2, const float* gam2, const float* dbet2,
                    const float* dgam2, const float* a, const float* mean1, const float* istd1,
                    const float* gam1, const float* bet1, const float* w2, float* gabn, float* part,
                    void* stream);
int eunet_gate_bwd3(const float* za, const float* zb, int n, int h, int w, int k,
                    const float* gabn, const float* a, const float* mean1, const float* istd1,
                    const float* gam1, const float* dbet1, const float* dgam1, const float* w1,
                    const float* gffd, const float* gaux_a, const float* gaux_b, float* gz_a,
                    float* gz_b, float* part, void* stream);
/* Dropout2d(p) after a BN+ReLU (models.py:287, 291) folded into per-sample affines:
 * keep [n][c] in {0,1} -> nscale/nshift [n][c] = scale/shift * keep/(1-p) (for the
 * in_nstride operand transform of eunet_conv3x3_fwd / _wgrad) and gscale (nullable)
 * [n][c] = keep/(1-p) (for eunet_conv3x3_dgrad_bnbwd) */
int eunet_dropout_affine(const float* scale, const float* shift, const float* keep, int n, int c,
                         float p, float* nscale, float* nshift, float* gscale, void* stream);
/* consistency term of the auxiliary supervision (train_eval.py:207-232): loss =
 * sum_b c_b (1/n) sum_i MSE(softmax(branch_b[i]), softmax(fused[i])), c_b = 0.4 w_b;
 * part: [n][tiles][2] workspace (eunet_consistency_tiles).  bwd ACCUMULATES into the
 * three NCHW gradients, scaled by the device scalar gloss. */
int eunet_consistency_tiles(int h, int w, int* tiles);
int eunet_consistency_fwd(const float* fused, const float* br0, const float* br1, int n, int k,
                          int h, int w, float c0, float c1, float* part, float* loss,
                          void* stream);
int eunet_consistency_bwd(const float* fused, const float* br0, const float* br1, int n, int k,
                          int h, int w, float c0, float c1, const float* gloss, float* gfused,
                          float* g0, float* g1, void* stream);

/* ---- device-side data path (datapath.hip; dataset.py:133-321) ----------------
 * rasterize: LabelMe polygons (int32 (x, y) vertices as dataset.py:185-188 truncates them;
 * polygon i = pts[poly_off[i] .. poly_off[i+1]), label 1 live / 2 dead) -> int64 semantic
 * mask [h][w], later polygons overwrite earlier ones (dataset.py:197-201).  Fill rule:
 * even-odd at the pixel centre, plus every lattice pixel on an edge. */
int eunet_rasterize_polygons(const int* pts, const int* poly_off, const int* labels, int npoly,
                             int h, int w, int64_t* mask, void* stream);
/* per-instance uint8 masks [npoly][h][w] (dataset.py:184-193, 'instance_masks'), same fill rule,
 * mirrored horizontally (flip_h) / vertically (flip_v) as the training flips mirror every
 * instance mask (dataset.py:209-222) */
int eunet_rasterize_instances(const int* pts, const int* poly_off, int npoly, int h, int w, int flip_h,
                              int flip_v, uint8_t* masks, void* stream);
/* cv2.flip (dataset.py:208-222): mode 1 horizontal, 0 vertical; HWC uint8 / int64 mask */
int eunet_flip_u8(const uint8_t* src, uint8_t* dst, int h, int w, int c, int mode, void* stream);
int eunet_flip_mask(const int64_t* src, int64_t* dst, int h, int w, int mode, void* stream);
/* numpy pixel augmentations in the reference's order, each rounded to uint8 as numpy does:
 * flags bit0 brightness (:243), bit1 contrast (:251), bit2 + noise[n] fp32 (:266-268),
 * bit3 gamma LUT[256] (:273-276) */
int eunet_augment_u8(uint8_t* img, long long n, int flags, double alpha, double beta,
                     const float* noise, const uint8_t* lut, void* stream);
/* dataset.py:225-257 without the host round trip for the live ratio: counts = the [3][3]
 * eunet_semantic_counts of the (flipped) semantic mask (device); flags bit 0 brightness, bit 1
 * contrast; u_alpha / u_beta = the random.random() draws that random.uniform(a, b) = a + (b-a) u
 * would have made in the reference's ratio-dependent branches (one draw in every branch). */
int eunet_augment_ratio_u8(uint8_t* img, long long n, const long long* counts, int flags, double u_alpha,
                           double u_beta, void* stream);
/* transforms.ToTensor (dataset.py:302-305): HWC uint8 -> CHW float32 / 255 */
int eunet_to_tensor(const uint8_t* img, int h, int w, int c, float* out, void* stream);
/* bilinear uint8 resize with cv2 INTER_LINEAR's half-pixel mapping (dataset.py:145-157);
 * cv2's fixed-point weights are not reproduced (parity unpinned: cv2 is absent) */
int eunet_resize_u8(const uint8_t* src, int hi, int wi, int c, uint8_t* dst, int ho, int wo,
                    void* stream);

/* ---- cv2 image operations of the data / evaluation paths (imgproc.hip) -------------------------
 * Replace the cv2 calls of dataset.py:58-131 (cell-specific preprocessing), dataset.py:255-294
 * (HSV / CLAHE / sharpen augmentations) and train_eval.py:365-395 (Evaluator preprocessing).
 * All images HWC uint8 RGB, npix = h * w.  cv2 is absent from this image: the formulas follow
 * OpenCV's documented algorithms (parity unpinned). */
/* COLOR_RGB2LAB / COLOR_LAB2RGB for 8U (dataset.py:63, 71, 268, 272; train_eval.py:380-385): cv2's
 * bit-exact fixed-point conversion (RGB2Lab_b / Lab2RGBinteger of OpenCV >= 3.4 color_lab.cpp).  The
 * tables are built on the host once and copied to each device on its first call (synchronous). */
int eunet_rgb2lab_u8(const uint8_t* rgb, uint8_t* lab, long long npix, void* stream);
int eunet_lab2rgb_u8(const uint8_t* lab, uint8_t* rgb, long long npix, void* stream);
/* The host-side Lab tables (no device needed; a checker's view of what the kernels use): gamma[256],
 * cbrt[3072], yf[512], invgamma[4096] as uint16 then c_fwd[9], c_inv[9] as int32 -- 15 744 + 72 bytes. */
int eunet_lab_tables(void* out, size_t bytes);
/* cv2.COLOR_RGB2GRAY: (4899 R + 9617 G + 1868 B + 8192) >> 14 */
int eunet_rgb2gray_u8(const uint8_t* rgb, uint8_t* gray, long long npix, void* stream);
/* in place RGB -> HSV (8U, H in [0, 180)) -> adjust -> RGB.  mode bit0: S *= sat_mul
 * (dataset.py:257-261); bit1: H = (H + hue_add) mod 180, V *= val_mul (:288-292); fp32 with
 * clip and astype(uint8) truncation as the reference's float32 arrays */
int eunet_hsv_adjust_u8(uint8_t* rgb, long long npix, float sat_mul, float hue_add, float val_mul,
                        int mode, void* stream);
/* cv2.createCLAHE(clip_limit, (tiles_x, tiles_y)).apply.  mode 0: src/dst gray [h][w];
 * mode 1: src is a Lab image, its L channel is equalised and dst receives the RGB image
 * (LAB2RGB fused, dataset.py:65-71 / train_eval.py:375-381).  luts: tiles_x*tiles_y*256 bytes */
int eunet_clahe_u8(const uint8_t* src, int mode, int h, int w, double clip_limit, int tiles_x,
                   int tiles_y, uint8_t* luts, uint8_t* dst, void* stream);
/* cv2.filter2D(src, -1, k9) with a 3x3 kernel (row-major), BORDER_REFLECT_101; src != dst */
int eunet_filter3x3_u8(const uint8_t* src, uint8_t* dst, int h, int w, int c, const float* k9,
                       void* stream);
/* GaussianBlur(3x3, 1.0) + addWeighted(src, 1.3, blur, -0.3, 0) (dataset.py:126-128); src != dst */
int eunet_unsharp_u8(const uint8_t* src, uint8_t* dst, int h, int w, int c, void* stream);
/* Sobel magnitude / |Laplacian| (CV_64F) of a gray image, each max-normalised to uint8 and
 * blended 0.7 / 0.3 (dataset.py:78-91).  ws: eunet_edge_features_workspace_bytes */
int eunet_edge_features_workspace_bytes(int h, int w, size_t* bytes);
int eunet_edge_features_u8(const uint8_t* gray, int h, int w, void* ws, uint8_t* edges, void* stream);
/* in place img *= 1.1 where live_mask > 0 (dataset.py:103-107) */
int eunet_live_boost_u8(uint8_t* img, const int64_t* live_mask, long long npix, void* stream);
/* dataset.py:109-124: where dead_mask > 0 the CLAHE'd gray dead_gray replaces clahe_img (dead_gray
 * null = no dead pixels), then edge blend 0.9 / 0.1 and 0.85 / 0.15 mix with orig */
int eunet_cell_mix_u8(const uint8_t* orig, const uint8_t* clahe_img, const uint8_t* edges,
                      const int64_t* dead_mask, const uint8_t* dead_gray, long long npix,
                      uint8_t* out, void* stream);
/* Evaluator input (train_eval.py:367-377): CHW float -> HWC uint8, x * 255 when max(x) <= 1
 * (max reduced on the device), astype(uint8) truncation.  ws: eunet_chw_to_u8_workspace_bytes */
int eunet_chw_to_u8_workspace_bytes(int c, int h, int w, size_t* bytes);
int eunet_chw_to_u8(const float* x, int c, int h, int w, void* ws, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EUNET_H */
