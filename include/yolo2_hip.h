/* yolo2_hip.h -- C ABI of the MI355X (gfx950) YOLOv2 hot path.
 *
 * The reference (ruiminshen/yolo-tf) has no FFI layer: its hot path is Python calling
 * TensorFlow-1.0 ops and NumPy.  This header is the boundary a maintainer would bind instead of
 * those ops (ctypes stub in INTEGRATION.md).  Each entry names the reference call site it
 * replaces (file:line into the reference tree).
 *
 * Conventions
 *   - plain pointers are DEVICE pointers unless marked host; the caller owns every buffer
 *     (outputs and workspaces included); the only allocation behind the ABI is the 32 KiB flag pool named below.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream) and may be issued from several host threads at once.  Library-owned state, all of it: a thread-local
 *     error string; a thread-local record of the last conv / wgrad plan (diagnostics below); one 32 KiB per-device pool
 *     of stream-K hand-off flags, created on first use and handed out under a mutex (yolo2_conv2d_ws & co.; freed by
 *     yolo2_shutdown()); tuning knobs read once from the environment (YOLO2_* A/B switches); and the
 *     process-wide test switch yolo2_debug_set_wgrad_variant.
 *   - return value: 0 = OK, otherwise a YOLO2_E_* code; yolo2_last_error() describes it.
 *   - activations are NHWC with an explicit pixel stride `ld*` (elements between consecutive
 *     pixels, >= channel count, multiple of 8); lanes in [C, ld) are padding the kernels never
 *     write and always read as zero (the caller zero-fills buffers once at allocation).
 *   - dtype selects the storage/compute type of activations and prepared filters:
 *     YOLO2_F32 (parity mode, f32 MFMA, exact fmaf chains) or YOLO2_BF16 (bf16 MFMA, f32
 *     accumulate).  Parameters, statistics, gradients of parameters and optimizer state are
 *     always f32.
 */
#ifndef YOLO2_HIP_H
#define YOLO2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { YOLO2_F32 = 0, YOLO2_BF16 = 1 };
enum {
    YOLO2_OK = 0,
    YOLO2_E_ARG = 1,      /* bad shape / alignment / enum */
    YOLO2_E_LAUNCH = 2,   /* HIP launch or runtime error */
    YOLO2_E_UNSUPPORTED = 3
};

int yolo2_abi_version(void);
const char *yolo2_last_error(void);
/* CRC32C (Castagnoli) of a HOST buffer, continuing from `crc` (0 to start): TFRecord / TensorBoard event / TF checkpoint files
 * (the reference reads and writes them through TensorFlow: utils/data/cache.py:95-100, train.py:141-145, detect.py:104-106) */
uint32_t yolo2_crc32c(const void *data, size_t n, uint32_t crc);
/* releases the library-owned stream-K flag pools (after synchronising their devices); any later call re-creates them */
int yolo2_shutdown(void);
/* Synchronises `stream` and reports errors only the device can detect: a stream-K convolution whose tile owner gave up waiting for a
 * partner workgroup's partial tile (the wait is bounded at 2 s; conv_shared.h y2_sk_wait_and_clear).  YOLO2_E_LAUNCH then means that
 * convolution outputs produced since the previous check are invalid; the flag pool is reset and the process may continue.  The counterpart
 * of the reference surfacing failures as exceptions instead of hanging (utils/postprocess.py:22-35 asserts, detect.py:70 check_numerics). */
int yolo2_check_async_errors(void *stream);
/* The asynchronous form: enqueues on `stream` a copy of the current device's YOLO2_ASYNC_ERROR_WORDS give-up counters into caller-owned PINNED
 * host memory and returns at once.  When the copy has completed (event / stream query) any non-zero word means yolo2_check_async_errors will
 * report YOLO2_E_LAUNCH: a host polls this every step (no synchronisation, one 32-byte copy) and only pays for the synchronising call when
 * something went wrong.  Same per-device semantics as yolo2_check_async_errors. */
#define YOLO2_ASYNC_ERROR_WORDS 8
int yolo2_async_error_snapshot(unsigned *host_words, void *stream);

/* ---- workspace sizes, in bytes, of every entry that takes caller-owned scratch (`ws`): pure host queries ----------------
 * yolo2_conv2d_workspace_bytes: the largest scratch any variant of yolo2_conv2d_ws / _bn / _bias_leaky can use for the
 * shape (stream-K: one f32 256x128 tile slot per CU = 33.5 MB on MI355X; K-sliced grids: the f32 [B*H*W][Nf] partial image);
 * a smaller buffer only disables variants.  The others are exact minimum sizes. */
size_t yolo2_conv2d_workspace_bytes(int B, int H, int W, int Cp, int Nf, int ksize, int dtype);
size_t yolo2_bn_workspace_bytes(int C);              /* yolo2_bn_stats*, yolo2_bn_leaky(_pool)_bwd_reduce */
size_t yolo2_bias_grad_workspace_bytes(int ld);
size_t yolo2_image_prep_workspace_bytes(int B);
size_t yolo2_loss_workspace_bytes(int B, int cells, int A);
size_t yolo2_nms_workspace_bytes(int B, int N, int C);
size_t yolo2_clip_workspace_bytes(int nseg);
size_t yolo2_augment_workspace_bytes(int B);

/* ---- convolution: slim.layers.conv2d, model/yolo2/inference.py:37-48,73-118 ------------------
 * Implicit-GEMM NHWC convolution, stride 1, SAME zero padding, ksize 1 or 3:
 *   O[b,h,w,n] = bias[n] + sum_{r,s,c<Cp} P[b,h+r-pad,w+s-pad,c] * F[n][(r*ksize+s)*Cp + c]
 * P: [B,H,W,ldp] (dtype), F: [Nf][ksize*ksize*Cp] (dtype, K-contiguous, from yolo2_filter_prep),
 * O: [B,H,W,ldo] (dtype), bias: f32[Nf] or NULL.  Forward uses the OHWI filter; the data
 * gradient is the same call with P = dY and the flipped/transposed filter. */
int yolo2_conv2d(const void *P, const void *F, const float *bias, void *O,
                 int B, int H, int W, int Cp, int ldp, int Nf, int ldo, int ksize,
                 int dtype, void *stream);

/* Same convolution with a caller-owned f32 workspace: when the M x N tile grid cannot fill the chip
 * (13x13 / 26x26 stages at small batch) the K loop is sliced across workgroups, partial tiles are
 * accumulated in `ws` (>= B*H*W*Nf floats for slicing to be considered; smaller = no slicing) and a
 * finishing kernel writes O.  Grids below one tile per CU with a long reduction instead run "stream-K": one
 * workgroup per CU, equal contiguous shares of the flat (tile, K step) space, partial tiles parked in `ws`
 * (needs >= CUs*256*128 floats = 33.6 MB on MI355X for the 256x128 tile, half for 128x128) and fixed up inside the same
 * launch through library-owned hand-off flags.
 * `ws` may hold anything on entry.  Results agree with yolo2_conv2d to f32 rounding of the partial sums. */
int yolo2_conv2d_ws(const void *P, const void *F, const float *bias, void *O, float *ws,
                    size_t ws_bytes, int B, int H, int W, int Cp, int ldp, int Nf, int ldo,
                    int ksize, int dtype, void *stream);

/* Filter gradient of the same convolution (tf.gradients of conv2d, train.py:127-129):
 *   dW[r,s,c,n] += sum_{b,h,w} X[b,h+r-pad,w+s-pad,c] * dY[b,h,w,n]       (HWIO, f32)
 * dW must be zeroed by the caller when yolo2_conv2d_wgrad_accumulates() says so: pixel-range splits accumulate with
 * f32 atomics. */
/* 1 if yolo2_conv2d_wgrad ADDS into dW for this shape (several pixel ranges per tile: the caller must zero dW first),
 * 0 if it overwrites every element (single range: dW may hold anything).  Pure host query, no launch. */
int yolo2_conv2d_wgrad_accumulates(int B, int H, int W, int Cin, int ldx, int Cout, int ldy, int ksize, int dtype);
int yolo2_conv2d_wgrad(const void *X, const void *dY, float *dW,
                       int B, int H, int W, int Cin, int ldx, int Cout, int ldy, int ksize,
                       int dtype, void *stream);

/* Workspace form of the same filter gradient (tf.gradients of conv2d, train.py:127-129; call sites model/yolo2/inference.py:37-48,73-118): the
 * deterministic training mode.  Where yolo2_conv2d_wgrad splits the pixel reduction over several workgroups and lets them meet in f32 atomics, here
 * every partial result goes with plain stores into a slot of its own in `ws` (slot r = pixel range r of the per-tap and the row-of-taps kernels, workgroup r
 * of conv1's kernel and of the image layer's; slot layout = the layout of dW, HWIO) and a second launch on the same stream, wgrad_reduce_kernel, overwrites
 * dW with the sum of the slots in an order that depends on the number of slots alone.
 * Bytes of workspace for a shape: slots x slot_floats x 4 with slot_floats = k*k*Cin*Cout rounded up to a multiple of 4 (16-byte slots);
 * 0 = the plan is a single range (yolo2_conv2d_wgrad stores already), and for arguments yolo2_conv2d_wgrad_ws would refuse.  Pure host query, no launch.
 * workspace_bytes > 0 exactly when yolo2_conv2d_wgrad_accumulates() == 1 (both read one plan function); the one exception is the scalar-gather test
 * hook, yolo2_debug_set_wgrad_variant(1), under which accumulates answers 1 for every shape to be safe. */
size_t yolo2_conv2d_wgrad_workspace_bytes(int B, int H, int W, int Cin, int ldx, int Cout, int ldy, int ksize, int dtype);
/* Same result contract as yolo2_conv2d_wgrad, except: dW is OVERWRITTEN for every shape (it may hold anything on entry, and so may ws), the value is a
 * pure function of (X, dY, shape, compute-unit count of the device) -- bitwise equal from call to call, buffer to buffer, process to process --, and
 * no float atomic is issued.  ws: 16-byte aligned; may be NULL when the query returns 0.  ws_bytes below the query's answer: YOLO2_E_ARG, nothing
 * launched.  The tiles, ranges and block placement are those of yolo2_conv2d_wgrad (one plan function serves both and the plan queries). */
int yolo2_conv2d_wgrad_ws(const void *X, const void *dY, float *dW, float *ws, size_t ws_bytes, int B, int H, int W,
                          int Cin, int ldx, int Cout, int ldy, int ksize, int dtype, void *stream);
/* Deterministic mode of the CALLING THREAD (default 0), for the entry points whose launch rule or reduction would otherwise sum floats in arrival
 * order: with it on, yolo2_conv2d_ws / _bias_leaky never take the K-sliced form (f32 atomics into the partial image; stream-K or the unsplit grid run
 * instead).  Results stay within the same bounds; they become a pure function of the inputs.  A deterministic engine switches it on for the
 * duration of its own sweeps and off again, so it can share a process (and a thread) with default engines and direct callers. */
int yolo2_set_deterministic(int on);
int yolo2_get_deterministic(void);

/* HWIO f32 master weights [k,k,Cin,Cout] -> the two K-contiguous operand layouts:
 *   Ffwd [Cout][k*k*ldcin]  : Ffwd[n][koff(r*k+s, c, ldcin)]  = W[r,s,c,n]
 *   Fdgr [Cin ][k*k*ldcout] : Fdgr[c][koff(r*k+s, n, ldcout)] = W[k-1-r,k-1-s,c,n]
 * (zero in the padding lanes).  Either output may be NULL.  K order inside a row, for ld channels and t = k*k taps:
 *   koff(tap, c, ld) = (c / kc) * t * kc + tap * kc + c % kc,   kc = 64 if (t > 1 and ld % 64 == 0) else ld
 * i.e. 64-channel chunk outermost, then tap, then channel: the 9 shifted reads of a pixel-tile x 64-channel slab are
 * consecutive K steps, so they hit in L2 (tap-major order measured 15x the algorithmic fabric traffic in the 13x13
 * stages).  The layout is an implementation detail shared by yolo2_filter_prep* and yolo2_conv2d*. */
int yolo2_filter_prep(const float *W, void *Ffwd, void *Fdgr, int ksize, int Cin, int ldcin,
                      int Cout, int ldcout, int dtype, void *stream);

/* The same for every layer of a network in one launch.  `descs_device` is a DEVICE array of n descriptors
 * sorted by first_block; layer i owns blocks [first_block_i, first_block_{i+1}) and needs
 * yolo2_filter_prep_blocks(ksize, ldcin, ldcout) = ksize^2 * ceil(ldcin / YOLO2_FILTER_PREP_TILE) * ceil(ldcout / YOLO2_FILTER_PREP_TILE_N) of them
 * (one block = one (c, n) tile of one tap); total_blocks = end of the last layer.  ldcin, ldcout must be multiples of 8 and Ffwd/Fdgr 16-byte aligned. */
#define YOLO2_FILTER_PREP_TILE 64       /* input channels per tile */
#define YOLO2_FILTER_PREP_TILE_N 128   /* filters per tile (round 6: 128 -- the master arrays then move in 512-byte runs) */
int yolo2_filter_prep_blocks(int ksize, int ldcin, int ldcout);
typedef struct yolo2_filter_desc {
    const float *W;      /* HWIO f32 master weights */
    void *Ffwd;          /* [Cout][k*k*ldcin]  or NULL */
    void *Fdgr;          /* [Cin ][k*k*ldcout] or NULL */
    int ksize, cin, ldcin, cout, ldcout, first_block;
} yolo2_filter_desc;
int yolo2_filter_prep_batch(const yolo2_filter_desc *descs_device, int n, int total_blocks, int dtype,
                            void *stream);

/* tf.train.AdamOptimizer's ApplyAdam (train.py:73-79,127) over every convolution filter of the descriptor table AND the operand layouts
 * of the updated filters, in one pass: equal, bit for bit, to yolo2_adam on the same elements followed by yolo2_filter_prep_batch.
 * descs[i].W must point into `params`; grads / m / v are arenas with the same element layout.  small_ranges_device: n_small pairs
 * (element offset, count) of the parameters that are not filters (gamma, beta, biases), updated by the same launch.  alpha is the
 * bias-corrected step size (lr * sqrt(1 - beta2^t) / (1 - beta1^t)), gscale multiplies the gradient (1 / world size).  A table may hold ONE
 * layer (first_block 0: a layer updated as soon as its gradient is final, while backward continues on another stream) or none (n = 0,
 * total_blocks = 0: only the small ranges). */
int yolo2_adam_filter_prep(const yolo2_filter_desc *descs_device, int n, int total_blocks, const long *small_ranges_device, int n_small,
                           float *params, const float *grads, float *m, float *v, float alpha, float beta1, float beta2, float eps,
                           float gscale, int dtype, void *stream);

/* Inference form of a batch-normalised layer with the moving statistics folded into the operands
 * (W' = W * gamma/sqrt(var+eps) per output channel, bias' = beta - mean*gamma/sqrt(var+eps)):
 *   O = leaky_relu(conv(P, F') + bias', alpha)      -- conv + batch_norm(is_training=False) + leaky_relu of
 * model/yolo2/inference.py:62-66,73-112 in one launch; as yolo2_conv2d_ws otherwise. */
int yolo2_conv2d_bias_leaky(const void *P, const void *F, const float *bias, void *O, float *ws, size_t ws_bytes, int B,
                            int H, int W, int Cp, int ldp, int Nf, int ldo, int ksize, float alpha, int dtype, void *stream);

/* Data-gradient convolution whose output dX is the gradient of a batch-normalised producer layer's activation
 * (a = leaky_relu(batch_norm(y)), model/yolo2/inference.py:62-66): as yolo2_conv2d_ws(dY, F, NULL, dX, ...) FOLLOWED BY
 * yolo2_bn_leaky_bwd_reduce(dX, ldo, Yprev, mean, var, gamma, beta, dgamma, dbeta, ...) -- the gradients of slim.batch_norm's
 * gamma/beta that tf.gradients derives (train.py:123-129) -- with the reduction done by the convolution's epilogue while the
 * tile is still on chip (partial rows in bn_part, f32 [2][YOLO2_BN_PART_ROWS][Nf], zero on entry and on return), so dX and
 * Yprev are not re-read by a separate pass.  Shapes the epilogue cannot take (Nf % (16/elem size) != 0, K-sliced grids) run
 * the two-step form internally with red_ws (>= yolo2_bn_workspace_bytes(Nf)): the results are the same up to summation order.
 * Yprev: [B*H*W][Nf] (pixel stride Nf).  pending: NULL -> dgamma/dbeta are final on return (stream order).  Non-NULL -> the
 * caller finishes: *pending = 1 means the sums are still in bn_part and yolo2_bn_part_to_grads must follow (a caller timing
 * the convolution launch alone brackets just this call); 0 means dgamma/dbeta were already written by the two-step form. */
int yolo2_conv2d_dgrad_bn(const void *dY, const void *F, void *dX, float *ws, size_t ws_bytes, int B, int H, int W, int Cp, int ldp,
                          int Nf, int ldo, int ksize, const void *Yprev, const float *mean, const float *var, const float *gamma,
                          const float *beta, float *dgamma, float *dbeta, float *bn_part, double *red_ws, float eps, float alpha,
                          int *pending, int dtype, void *stream);
/* 1 when yolo2_conv2d_dgrad_bn would take the sums from its epilogue for a data gradient with Nf output channels on B x H x W pixels, 0 when the launch
 * rule prefers a plain data gradient there (3x3, <= 64 channels, >= 100k pixels: the reduction then costs less as its own pass): a host that asks first
 * calls yolo2_conv2d_ws + yolo2_bn_leaky_bwd_reduce_part + yolo2_bn_leaky_bwd_apply_fin for such a layer (engine.Engine._bind does) */
int yolo2_conv2d_dgrad_bn_fuses(int B, int H, int W, int Nf, int ksize, int dtype);
/* column sums of the partial rows left by yolo2_conv2d_dgrad_bn: plane 0 -> dgamma, plane 1 -> dbeta; rows zeroed again */
int yolo2_bn_part_to_grads(float *bn_part, int C, float *dgamma, float *dbeta, void *stream);

/* Forward convolution of a batch-normalised layer (no bias): as yolo2_conv2d_ws, and the per-channel shifted sums
 *   sum_m (y[m,n] - shift[n]),  sum_m (y[m,n] - shift[n])^2        (y = the stored, rounded output)
 * are accumulated into bn_part, f32 [2][YOLO2_BN_PART_ROWS][Nf], by the convolution's own epilogue (f32 atomics on
 * row (tile % ROWS)); yolo2_bn_finalize turns them into the batch moments.  This replaces the separate statistics
 * pass over y of slim.batch_norm's tf.nn.moments (model/yolo2/inference.py:62-66).  bn_part must be all zero on entry
 * (yolo2_bn_finalize leaves it zero); shift is any per-channel estimate of the mean (the engine passes
 * moving_mean): it only conditions the single-pass variance.  Requires ldo == Nf. */
#define YOLO2_BN_PART_ROWS 256
int yolo2_conv2d_bn(const void *P, const void *F, void *O, float *ws, size_t ws_bytes, int B, int H, int W, int Cp, int ldp,
                    int Nf, int ldo, int ksize, const float *shift, float *bn_part, int dtype, void *stream);
/* mean[c] = shift[c] + S1/M, var[c] = S2/M - (S1/M)^2 (biased, f64), optional moving-average update as
 * yolo2_bn_stats_ema (moving_* may both be NULL); zeroes bn_part. */
int yolo2_bn_finalize(float *bn_part, const float *shift, long M, int C, float *mean, float *var, float *moving_mean,
                      float *moving_var, double decay, void *stream);

/* ---- Consumers that finalise the partial rows themselves (one launch instead of finalize + apply): slim.batch_norm's
 * tf.nn.moments + assign_moving_average + normalisation (model/yolo2/inference.py:62-66) and the dgamma / dbeta + dY of its gradient
 * (train.py:123-129), fed by the partial rows a producer left behind: yolo2_conv2d_bn / yolo2_conv2d_dgrad_bn (bn_part layout
 * [2][YOLO2_BN_PART_ROWS][C]) or a *_reduce_part call ([2][rows][C] in its ws).  `rows` = how many partial rows the producer used:
 * yolo2_last_bn_part_rows() right after the producing call on the same host thread (a producer wraps its tiles around few rows when
 * it has many, so that this prologue stays short), or *rows of the reduce_part call.  yolo2_bn_fin_supported(rows, C, dtype) says
 * whether the shape qualifies (C / (16 / elem size) a power of two; rows x channel-slice small enough that a per-workgroup
 * prologue beats a separate finalisation launch); otherwise use yolo2_bn_finalize / yolo2_bn_part_to_grads / the plain pairs.
 * The rows are only READ here.  zero / zero_floats (multiple of 4, 16-byte aligned; may be NULL / 0): a float range this launch
 * clears on the side -- the engine keeps two partial buffers and has each consumer clear the one its predecessor finished with, so
 * every producer finds zero rows without a memset launch.  Results equal the two-launch forms up to f64 summation order.
 * `shift` (the per-channel values the producer subtracted) is read by EVERY workgroup of the launch while the first workgroup of each
 * channel slice stores mean / var and updates moving_mean / moving_var in place: it must not alias any of them (YOLO2_E_ARG if it
 * does).  A caller that shifts by the moving mean hands in a copy taken before the step (engine.Engine.state_snap). */
/* yolo2_bn_leaky_pool_fin: ymax (optional, [B*(H/2)*(W/2)][C], dense) receives the raw convolution output AT the arg-max of each
 * window.  Only arg-max positions carry gradient, so the layer's backward reduction is then yolo2_bn_leaky_bwd_reduce_part over
 * (dP, ymax) at the POOLED resolution: a quarter of the rows, and neither Y nor idx are read.  A_full (optional, dense [B*H*W][C])
 * also receives the un-pooled activation, for a layer whose activation has a second reader (idx may then be NULL). */
int yolo2_last_bn_part_rows(void);
int yolo2_bn_fin_supported(int rows, int C, int dtype);
int yolo2_bn_leaky_fin(const void *Y, const float *bn_part, int rows, const float *shift, float *mean, float *var, float *moving_mean,
                       float *moving_var, double decay, const float *gamma, const float *beta, void *A, long M, int C, int lda,
                       float eps, float alpha, float *zero, long zero_floats, int dtype, void *stream);
int yolo2_bn_leaky_pool_fin(const void *Y, const float *bn_part, int rows, const float *shift, float *mean, float *var,
                            float *moving_mean, float *moving_var, double decay, const float *gamma, const float *beta, void *P,
                            unsigned char *idx, void *ymax, void *A_full, int B, int H, int W, int C, int ldp, float eps, float alpha,
                            float *zero, long zero_floats, int dtype, void *stream);
/* part: [2][rows][C] with plane_stride floats between the two planes (YOLO2_BN_PART_ROWS * C for bn_part, rows * C for a ws) */
int yolo2_bn_leaky_bwd_apply_fin(const void *dA, int ldda, const void *Y, const float *mean, const float *var, const float *gamma,
                                 const float *beta, const float *part, int rows, long plane_stride, float *dgamma, float *dbeta,
                                 void *dY, long M, int C, float eps, float alpha, float *zero, long zero_floats, int dtype, void *stream);
int yolo2_bn_leaky_pool_bwd_apply_fin(const void *dP, int lddp, const unsigned char *idx, const void *Y, const float *mean,
                                      const float *var, const float *gamma, const float *beta, const float *part, int rows,
                                      long plane_stride, float *dgamma, float *dbeta, void *dY, int B, int H, int W, int C, float eps,
                                      float alpha, float *zero, long zero_floats, int dtype, void *stream);
/* The image layer (3 channels in an 8-wide pixel, 32 filters, 3x3 + batch_norm + leaky_relu + 2x2 max_pool: reference model/yolo2/inference.py:62-66):
 * yolo2_bn_leaky_pool_bwd_apply_fin + yolo2_conv2d_wgrad in ONE launch.  The layer's output gradient (the largest tensor of the network) is formed
 * per 32-pixel row segment in LDS from the raw forward output Y [B,H,W,32], the pooled gradient dP [B,H/2,W/2,lddp] and the arg-max codes idx
 * [B,H/2,W/2,32] and consumed there by the filter-gradient MFMAs; dgamma / dbeta come from the partial rows like in the *_fin call.  dW [3][3][Cin][32]
 * f32 is ACCUMULATED into (zero it first); X [B,H,W,8]. */
int yolo2_first_layer_wgrad_bn(const void *X, const void *Y, const void *dP, int lddp, const unsigned char *idx, const float *mean, const float *var,
                               const float *gamma, const float *beta, const float *part, int rows, long plane_stride, float *dgamma, float *dbeta,
                               float *dW, int B, int H, int W, int Cin, float eps, float alpha, float *zero, long zero_floats, int dtype, void *stream);
/* pass 1 of the BN + leaky backward alone: partial rows [2][*rows][C] (f32) left in ws for a *_bwd_apply_fin call */
int yolo2_bn_leaky_bwd_reduce_part(const void *dA, int ldda, const void *Y, const float *mean, const float *var, const float *gamma,
                                   const float *beta, double *ws, int *rows, int rows_limit, long M, int C, float eps, float alpha,
                                   int dtype, void *stream);
int yolo2_bn_leaky_pool_bwd_reduce_part(const void *dP, int lddp, const unsigned char *idx, const void *Y, const float *mean,
                                        const float *var, const float *gamma, const float *beta, double *ws, int *rows,
                                        int rows_limit, int B, int H, int W, int C, float eps, float alpha, int dtype, void *stream);

/* ---- The image layer fused with its consumers: conv0 (3 -> 32 filters, 3x3; model/yolo2/inference.py:72-74 `net = conv2d(net, 32)` followed
 * by `max_pool2d`) is 0.9 % of the arithmetic but its raw output is the largest tensor of the network (5.5 M pixels x 32 channels per
 * image).  These entries never store it: each one re-computes the output patch it needs from the image (P: [B,H,W,8], 3 real channels;
 * F: the forward filter operand of yolo2_filter_prep, [32][72]) and applies its elementwise work to the accumulators.  Results equal
 *   yolo2_conv2d_bn + yolo2_bn_finalize                      (yolo2_first_layer_stats + yolo2_bn_finalize)
 *   yolo2_bn_leaky_pool on the stored output                 (yolo2_first_layer_bn_leaky_pool)
 *   yolo2_bn_leaky_pool_bwd_reduce / _bwd_apply               (yolo2_first_layer_pool_bwd_reduce + yolo2_bn_part_to_grads / ..._bwd_apply)
 * bit for bit up to f32 summation order: the recomputed output is rounded to dtype exactly where the unfused path stores it.
 * H and W even; bn_part: f32 [2][YOLO2_BN_PART_ROWS][32], zero on entry. */
int yolo2_first_layer_stats(const void *P, const void *F, int B, int H, int W, const float *shift, float *bn_part, int dtype, void *stream);
int yolo2_first_layer_bn_leaky_pool(const void *P, const void *F, const float *mean, const float *var, const float *gamma,
                                    const float *beta, void *Pout, unsigned char *idx, int B, int H, int W, int ldp, float eps,
                                    float alpha, int dtype, void *stream);
int yolo2_first_layer_pool_bwd_reduce(const void *P, const void *F, const void *dP, int lddp, const unsigned char *idx,
                                      const float *mean, const float *var, const float *gamma, const float *beta, float *bn_part,
                                      int B, int H, int W, float eps, float alpha, int dtype, void *stream);
int yolo2_first_layer_pool_bwd_apply(const void *P, const void *F, const void *dP, int lddp, const unsigned char *idx,
                                     const float *mean, const float *var, const float *gamma, const float *beta,
                                     const float *dgamma, const float *dbeta, void *dY, int B, int H, int W, float eps, float alpha,
                                     int dtype, void *stream);

/* ---- batch norm + leaky ReLU: closure model/yolo2/inference.py:62-66 + model/yolo/function.py:21-24
 * Y is the raw convolution output [M = B*H*W][C] (pixel stride C). */
/* batch mean and biased variance over M rows (tf.nn.moments); ws: >= 1025*C doubles of scratch
 * (per-block partial sums; any content) */
int yolo2_bn_stats(const void *Y, float *mean, float *var, double *ws, long M, int C,
                   int dtype, void *stream);
/* yolo2_bn_stats + yolo2_bn_ema in one pass (the moving-average update rides in the finalisation kernel) */
int yolo2_bn_stats_ema(const void *Y, float *mean, float *var, float *moving_mean, float *moving_var,
                       double decay, double *ws, long M, int C, int dtype, void *stream);
/* moving -= f32(1-decay)*(moving-batch)   (assign_moving_average, decay 0.999; 1-decay is formed in
 * double and then rounded, as TF's Python side does) */
int yolo2_bn_ema(float *moving_mean, float *moving_var, const float *mean, const float *var,
                 int C, double decay, void *stream);
/* A[m,c] = leaky(gamma*(Y-mean)/sqrt(var+eps)+beta); A has pixel stride lda (concat target) */
int yolo2_bn_leaky(const void *Y, const float *mean, const float *var, const float *gamma,
                   const float *beta, void *A, long M, int C, int lda, float eps, float alpha,
                   int dtype, void *stream);
/* backward, pass 1: dgamma[c] = sum g*xhat, dbeta[c] = sum g with g = dA * leaky'(z);
 * ws: >= 1024*C doubles of scratch */
int yolo2_bn_leaky_bwd_reduce(const void *dA, int ldda, const void *Y, const float *mean,
                              const float *var, const float *gamma, const float *beta,
                              float *dgamma, float *dbeta, double *ws, long M, int C,
                              float eps, float alpha, int dtype, void *stream);
/* backward, pass 2: dY = gamma*inv*(g - dbeta/M - xhat*dgamma/M) */
int yolo2_bn_leaky_bwd_apply(const void *dA, int ldda, const void *Y, const float *mean,
                             const float *var, const float *gamma, const float *beta,
                             const float *dgamma, const float *dbeta, void *dY, long M, int C,
                             float eps, float alpha, int dtype, void *stream);

/* ---- BN + leaky + 2x2/2 max pool fused (layers whose only consumer is the pool: model/yolo2/inference.py:70-95,
 * `net = slim.layers.max_pool2d(net)` right after a conv): the full-resolution activation and its gradient never reach
 * HBM.  P[b,oh,ow,c] = max over the window of leaky(bn(Y)) rounded to dtype; idx (may be NULL for inference) receives
 * one byte per pooled element: the window position 0..3 (row-major) of the FIRST maximum, which is where
 * tf.nn.max_pool's gradient goes.  The backward pair equals yolo2_maxpool_bwd followed by yolo2_bn_leaky_bwd_*. */
int yolo2_bn_leaky_pool(const void *Y, const float *mean, const float *var, const float *gamma, const float *beta, void *P,
                        unsigned char *idx, int B, int H, int W, int C, int ldp, float eps, float alpha, int dtype, void *stream);
int yolo2_bn_leaky_pool_bwd_reduce(const void *dP, int lddp, const unsigned char *idx, const void *Y, const float *mean,
                                   const float *var, const float *gamma, const float *beta, float *dgamma, float *dbeta,
                                   double *ws, int B, int H, int W, int C, float eps, float alpha, int dtype, void *stream);
int yolo2_bn_leaky_pool_bwd_apply(const void *dP, int lddp, const unsigned char *idx, const void *Y, const float *mean,
                                  const float *var, const float *gamma, const float *beta, const float *dgamma,
                                  const float *dbeta, void *dY, int B, int H, int W, int C, float eps, float alpha,
                                  int dtype, void *stream);

/* ---- max pool 2x2, SAME: slim.layers.max_pool2d, model/yolo2/inference.py:38,42,74,83,96 ------
 * stride 2 (H,W even) or stride 1 (pads bottom/right; tiny model).  Backward routes to the
 * first maximum in row-major window order. */
int yolo2_maxpool_fwd(const void *A, void *P, int B, int H, int W, int C, int stride,
                      int dtype, void *stream);
int yolo2_maxpool_bwd(const void *A, const void *dP, void *dA, int B, int H, int W, int C,
                      int stride, int dtype, void *stream);
/* dA += the routed gradient, rounded to the element type like yolo2_maxpool_bwd into a temporary + yolo2_add_inplace (stride 2 only):
 * the second writer of a tensor's gradient (Darknet-19's passthrough fan-out at the 26x26 stage) */
int yolo2_maxpool_bwd_acc(const void *A, const void *dP, void *dA, int B, int H, int W, int C, int dtype, void *stream);

/* ---- reorg / concat: model/yolo2/function.py:22-29, model/yolo2/inference.py:114-116 ----------
 * out[b,y,x,(sy*2+sx)*C+c] = in[b,2y+sy,2x+sx,c]; `out` has pixel stride ldo so it can be the
 * leading channels of the concat buffer.  yolo2_reorg_bwd is the inverse move. */
int yolo2_reorg(const void *in, void *out, int B, int H, int W, int C, int ldo, int dtype,
                void *stream);
int yolo2_reorg_bwd(const void *dout, int ldd, void *din, int B, int H, int W, int C, int dtype,
                    void *stream);
/* dst[m, 0:C] = src[m, 0:C] with independent pixel strides (tf.concat second operand / slice) */
int yolo2_copy_channels(const void *src, int lds, void *dst, int ldd, long M, int C, int dtype,
                        void *stream);
/* dst += src elementwise over n elements (passthrough gradient join) */
int yolo2_add_inplace(void *dst, const void *src, long n, int dtype, void *stream);
/* dbias[c] = sum_m dY[m,c]  (final conv biases, model/yolo2/inference.py:118); ws >= 512*ld doubles */
int yolo2_bias_grad(const void *dY, int ld, float *dbias, double *ws, long M, int C, int dtype,
                    void *stream);

/* ---- input: tf.image.per_image_standardization train.py:103 / utils/preprocess.py:23-25 --------
 * img: f32 [B,H,W,3] (0..255); out: dtype [B,H,W,8] (channels 3..7 zero).
 * mode 0: (x-mean)/max(std,1/sqrt(N)) per image; mode 1: x/255 (detect.py:37-38);
 * mode 2: plain cast.  ws: yolo2_image_prep_workspace_bytes(B) (mode 0: 64 partial (sum, sum of squares) pairs per image; any content). */
int yolo2_image_prep(const float *img, void *out, double *ws, int B, int HW, int mode, int dtype,
                     void *stream);

/* ---- head decode: Model.__init__, model/yolo2/__init__.py:28-59 (detection block :50-56) ------
 * logits [B,cells,ld] (channel order per anchor: iou,x,y,w,h,cls...), anchors f32[A][2] (w,h).
 * Outputs f32: conf [B,cells,A,C], xy_min/xy_max [B,cells,A,2]; nan_flag (int, device) is set
 * non-zero if any output is NaN/Inf (tf.check_numerics, detect.py:70). */
int yolo2_head_decode(const void *logits, int ld, const float *anchors, float *conf,
                      float *xy_min, float *xy_max, int *nan_flag, int B, int cell_h, int cell_w,
                      int A, int C, int dtype, void *stream);

/* The other Model attributes the reference's callers read (demo_detect.py:62: prob, iou, xy_min, wh; model/yolo2/__init__.py:36-56),
 * f32: iou [B,cells,A] = sigmoid(ch 0), prob [B,cells,A,C] = softmax(classes), xy [B,cells,A,2] = cell_xy + sigmoid(ch 1:3),
 * wh [B,cells,A,2] = exp(ch 3:5) * anchors.  Any output may be NULL (at least one must not be). */
int yolo2_head_decode_attrs(const void *logits, int ld, const float *anchors, float *iou, float *prob,
                            float *xy, float *wh, int B, int cell_h, int cell_w, int A, int C,
                            int dtype, void *stream);

/* ---- loss forward+backward: Objectives, model/yolo2/__init__.py:62-94 + Builder :114-119 -----
 * labels (f32): mask[B,cells], prob[B,cells,C], coords[B,cells,4], off_min/off_max[B,cells,2],
 * areas[B,cells].  hparam = HOST pointer to the 4 weights {iou_best, iou_normal, coords, prob}.
 * objectives (f32[4], same order) receives the UNWEIGHTED sums / cnt, cnt = B*cells*A.
 * dlogits (dtype, [B,cells,ld], may be NULL) receives d(total weighted loss)/d logits, padding
 * lanes zeroed.  ws: >= 4*ceil(B*cells*L/256) floats, L = smallest power of two >= A. */
int yolo2_loss(const void *logits, int ld, const float *anchors, const float *mask,
               const float *prob, const float *coords, const float *off_min, const float *off_max,
               const float *areas, const float *hparam, float *objectives, void *dlogits,
               float *ws, int B, int cell_h, int cell_w, int A, int C, int dtype, void *stream);
/* yolo2_loss in two halves: the kernel that writes dlogits and per-workgroup partial sums into ws (all a training step needs), and the
 * reduction of those partials into the four objective values, run only when they are read (summaries). */
int yolo2_loss_partials(const void *logits, int ld, const float *anchors, const float *mask, const float *prob,
                        const float *coords, const float *off_min, const float *off_max, const float *areas,
                        const float *hparam, void *dlogits, float *ws, int B, int cell_h, int cell_w, int A, int C, int dtype,
                        void *stream);
int yolo2_loss_objectives(const float *ws, float *objectives, int B, int cell_h, int cell_w, int A, void *stream);
/* yolo2_loss / yolo2_loss_partials with the box regression loss chosen: box_loss 0 = mse (the two entries above, bit for bit), 1 = iou,
 * 2 = giou, 3 = diou, 4 = ciou; anything else is an argument error.  In modes 1..4 the `coords` objective is sum(mask_best * (1 - q)) / cnt
 * for the mode's score q of the predicted box against the cell's target (cell units relative to the cell) and
 * channels 1..4 of dlogits hold its exact derivative, weighted by hparam[2]; every other output is what mode 0 writes.  Same workspace;
 * yolo2_loss_objectives reduces the partials of every mode. */
int yolo2_loss_box(const void *logits, int ld, const float *anchors, const float *mask,
                   const float *prob, const float *coords, const float *off_min, const float *off_max,
                   const float *areas, const float *hparam, float *objectives, void *dlogits,
                   float *ws, int B, int cell_h, int cell_w, int A, int C, int dtype, void *stream, int box_loss);
int yolo2_loss_box_partials(const void *logits, int ld, const float *anchors, const float *mask, const float *prob,
                            const float *coords, const float *off_min, const float *off_max, const float *areas,
                            const float *hparam, void *dlogits, float *ws, int B, int cell_h, int cell_w, int A, int C, int dtype,
                            void *stream, int box_loss);
/* Every option of the YOLOv2 loss in one struct; later options join it.  With {sizeof, 0, 0, 0, 0, 0, any} the two
 * entries below are yolo2_loss / yolo2_loss_partials, with only box_loss set yolo2_loss_box / yolo2_loss_box_partials, bit for bit.
 *   ignore_thresh t: a lane that is not responsible and whose predicted box has an IoU above t (strictly) with a ground truth box of its
 *     image -- the object cells of the label tensors, one box per cell: cell_xy + off_min .. cell_xy + off_max, area `areas` -- takes no part
 *     in iou_normal and gets no objectness gradient.  cnt is not renormalised.
 *   rescore: the objectness target of a responsible lane is its own matching IoU (a constant in the derivative) instead of 1.
 *   class_loss: 0 the squared error on the softmax; 1 the cross-entropy -sum_k tt_k log p_k; 2 focal, -sum_k tt_k (1 - p_k)^gamma log p_k, on
 *     tt_k = (1 - eps) t_k + eps * sum(t) / C of the (possibly multi-hot) label row t; in the `prob` objective and the class channels of dlogits.
 * A NULL opt, a size other than sizeof(yolo2_loss_options), an out-of-range or non-finite field, and label_smoothing != 0 with class_loss 0
 * are argument errors: nothing is launched, nothing is written.  Same workspace; yolo2_loss_objectives reduces the partials of every mode. */
typedef struct yolo2_loss_options {
    int   size;             /* sizeof(yolo2_loss_options): a larger, later struct is refused by an older library and vice versa */
    int   box_loss;         /* as yolo2_loss_box */
    int   class_loss;       /* 0 mse, 1 ce, 2 focal */
    int   rescore;          /* 0 | 1 */
    float ignore_thresh;    /* 0 = off, else 0 < t < 1 */
    float label_smoothing;  /* 0 <= eps < 1; must be 0 with class_loss mse */
    float focal_gamma;      /* 0 or >= 1; read with class_loss focal only */
} yolo2_loss_options;
int yolo2_loss_ex(const void *logits, int ld, const float *anchors, const float *mask,
                  const float *prob, const float *coords, const float *off_min, const float *off_max,
                  const float *areas, const float *hparam, float *objectives, void *dlogits,
                  float *ws, int B, int cell_h, int cell_w, int A, int C, int dtype, void *stream, const yolo2_loss_options *opt);
int yolo2_loss_ex_partials(const void *logits, int ld, const float *anchors, const float *mask, const float *prob,
                           const float *coords, const float *off_min, const float *off_max, const float *areas,
                           const float *hparam, void *dlogits, float *ws, int B, int cell_h, int cell_w, int A, int C, int dtype,
                           void *stream, const yolo2_loss_options *opt);

/* ---- objectness-scaled distillation (Mehta & Ozturk, ECCV-W 2018; csrc/distill.hip) -------------------
 * Two YOLOv2 heads of the same geometry: `student` [B,cells,ld_s] (dtype_s) and `teacher` [B,cells,ld_t] (dtype_t), each YOLO2_F32 or
 * YOLO2_BF16 and the two may differ; the real channels of a row are A x (iou, x, y, w, h, C classes).  With n = B*cells*A, s / t a
 * lane of the student / teacher, sg the sigmoid and m = sg(t0) (scale_by_objectness 1) or 1 (0), the three UNWEIGHTED objectives are
 *   objectness = 1/n sum (sg(s0) - sg(t0))^2
 *   coords     = 1/n sum m [(sg(s1) - sg(t1))^2 + (sg(s2) - sg(t2))^2 + (s3 - t3)^2 + (s4 - t4)^2]
 *   prob       = 1/n sum m sum_k (p_k - q_k)^2                       class_term 0 (mse), p = softmax(s[5:] / T), q = softmax(t[5:] / T)
 *              = 1/n sum m T^2 sum_k q_k (log q_k - log p_k)         class_term 1 (kl)
 * and total = weight * (w_objectness * objectness + w_coords * coords + w_prob * prob).  The teacher is a constant.
 * yolo2_distill_partials ADDS d total / d student into dlogits (dtype_s, [B,cells,ld_s], read and written: dl = store(f32(dl) + g) over
 * the A*(5+C) real channels of a row; padding channels are not touched; NULL: objectives only) and stores three partial sums per
 * workgroup into ws (yolo2_distill_workspace_bytes) with plain stores; yolo2_distill_objectives reduces them in index order into
 * objectives f32[3] {objectness, coords, prob}.  No atomics: bitwise reproducible.  A NULL student, teacher, ws or opt, an unknown dtype, a
 * size other than sizeof(yolo2_distill_options), a temperature that is not positive and finite, a negative or non-finite weight and an
 * unknown class_term are argument errors: nothing is launched, nothing is written. */
typedef struct yolo2_distill_options {
    int   size;                 /* sizeof(yolo2_distill_options) */
    int   class_term;           /* 0 mse, 1 kl */
    int   scale_by_objectness;  /* 0 | 1 */
    float weight;               /* the global weight, >= 0 */
    float w_objectness;         /* >= 0 */
    float w_coords;             /* >= 0 */
    float w_prob;               /* >= 0 */
    float temperature;          /* T > 0 */
} yolo2_distill_options;
size_t yolo2_distill_workspace_bytes(int B, int cells, int A);
int yolo2_distill_partials(const void *student, int ld_s, int dtype_s, const void *teacher, int ld_t, int dtype_t, void *dlogits,
                           float *ws, int B, int cell_h, int cell_w, int A, int C, void *stream, const yolo2_distill_options *opt);
int yolo2_distill_objectives(const float *ws, float *objectives, int B, int cell_h, int cell_w, int A, void *stream);

/* ---- YOLO (v1) family, SURVEY 8f-4: model/yolo/__init__.py:37-100, model/yolo/inference.py:24-66 --------------------------
 * Network output row per image [cells*C class scores | cells*boxes*(iou, x, y, sqrt_w, sqrt_h)], all linear; `ld` = row stride.
 * yolo1_loss: Objectives + d(total weighted loss)/d(net) (label tensors and hparam order as yolo2_loss; prob is masked by the
 * cell mask, cnt = B*cells*boxes); ws as yolo2_loss with A = boxes_per_cell.  yolo1_head_decode: the detection block (conf = iou *
 * prob, corners in cell units). */
int yolo1_loss(const void *net, int ld, const float *mask, const float *prob, const float *coords, const float *off_min,
               const float *off_max, const float *areas, const float *hparam, float *objectives, void *dnet, float *ws,
               int B, int cell_h, int cell_w, int boxes_per_cell, int C, int dtype, void *stream);
int yolo1_head_decode(const void *net, int ld, float *conf, float *xy_min, float *xy_max, int *nan_flag, int B, int cell_h,
                      int cell_w, int boxes_per_cell, int C, int dtype, void *stream);
/* leaky_relu backward of an un-normalised layer, from its OUTPUT a: dZ = a >= 0 ? dA : alpha*dA (model/yolo/function.py:21-24;
 * n elements, a multiple of 8 (bf16) / 4 (f32)) */
int yolo2_leaky_bwd(const void *A, const void *dA, void *dZ, long n, float alpha, int dtype, void *stream);
/* slim.layers.dropout in training (model/yolo/inference.py:57,60): Y = X * keep / keep_prob, keep ~ Bernoulli(keep_prob) from a
 * counter-based hash of (seed, index); the byte mask is written for the backward pass.  seed == 0: `mask` is an input. */
int yolo2_dropout(const void *X, void *Y, unsigned char *mask, long n, float keep_prob, unsigned long long seed, int dtype,
                  void *stream);
int yolo2_dropout_bwd(const void *dY, const unsigned char *mask, void *dX, long n, float keep_prob, int dtype, void *stream);
/* slim.l2_regularizer(scale) on a weight tensor (model/yolo/inference.py:55): g += scale*w, *loss += scale*sum(w^2)/2 (device double) */
int yolo2_l2_regularizer(const float *w, float *g, long n, float scale, double *loss, void *stream);

/* ---- NMS: utils/postprocess.py:39-51 (iou :21-36), batched over images -----------------------
 * conf [B,N,C] f32 is updated in place exactly as the reference mutates it; order_out [B,N]
 * (int, may be NULL) receives per image the box indices in the order of the reference's
 * returned list (stable descending sort by the last class, ties carried from earlier classes).
 * ws: >= B*C*N ints. */
int yolo2_nms(float *conf, const float *xy_min, const float *xy_max, int *order_out, int *ws,
              int B, int N, int C, float threshold, float threshold_iou, void *stream);

/* ---- Soft-NMS (Bodla et al., ICCV 2017; new work, the reference has none), batched over images and classes ---------------
 * Per (image, class): the candidates are the boxes with conf > threshold (NaN is none).  The best remaining candidate by (score
 * descending, box index ascending) is picked -- its score is final -- and every other remaining candidate's score is multiplied by
 *   YOLO2_NMS_HARD      IoU >= threshold_iou ? 0 : 1
 *   YOLO2_NMS_LINEAR    IoU >= threshold_iou ? 1 - IoU : 1
 *   YOLO2_NMS_GAUSSIAN  soft_exp(-(IoU * IoU) / sigma)      (csrc/soft_exp.h; threshold_iou is unused)
 * then the best is selected again, until none is left above `threshold`.  Picked boxes keep their final score, every other candidate is
 * written as +0.0f, non-candidates are not touched.  IoU as in yolo2_nms (`>=`, not the paper's `>`); f32, bit for bit reproducible.
 * conf [B,N,C] is updated in place; xy_min / xy_max [B,N,2] finite with xy_min <= xy_max.  order_out [B,N] (int, may be NULL) receives per
 * image the box indices by (max over classes of the FINAL scores descending, box index ascending), written by a second launch.
 * 1 <= N <= 4096, threshold >= 0, threshold_iou finite, sigma finite and >= 1/64 (Gaussian only); anything else is YOLO2_E_ARG before any
 * HIP call.  No workspace.  Per class only: there is no class-agnostic mode and no limit on the number of detections. */
#define YOLO2_NMS_HARD 0
#define YOLO2_NMS_LINEAR 1
#define YOLO2_NMS_GAUSSIAN 2
int yolo2_soft_nms(float *conf, const float *xy_min, const float *xy_max, int *order_out, int B, int N, int C, int method,
                   float threshold, float threshold_iou, float sigma, void *stream);

/* ---- test-time augmentation (new work, the reference has none): views of one image -> one frame -> Weighted Boxes Fusion ---------------
 * A view is (width, height, flip); the base view is the first and its grid (cell_w0, cell_h0) is the frame of the result.
 *
 * yolo2_tta_gather: one view's conf [B,N,C], xy_min / xy_max [B,N,2] (cells of the view's grid (cw, ch)) -> rows offset .. offset+N-1 of
 * the pooled out_conf [B,M,C], out_xy_min / out_xy_max [B,M,2]; no other row is touched.  sx = f32(cell_w0) / f32(cw) and sy =
 * f32(cell_h0) / f32(ch) are the caller's (computed once, in f32).  x' = x * sx, or with flip xmin' = cell_w0 - xmax * sx and xmax' =
 * cell_w0 - xmin * sx; y' = y * sy; conf is copied.  One elementwise launch.  B, N, C >= 1, 1 <= M <= 32768, 0 <= offset <= M - N, sx, sy,
 * cell_w0 finite, flip 0 or 1; anything else is YOLO2_E_ARG before any HIP call.
 *
 * yolo2_wbf (Solovyev, Wang, Gabruseva, Image and Vision Computing 2021; per class, unit view weights, conf_type = avg).  Per (image,
 * class): the candidates are the pooled boxes with conf > threshold (NaN is none), taken by (score descending, pooled index ascending).
 * A candidate's IoU is computed with every cluster's CURRENT FUSED box (yolo2_nms's operation order, the cluster in the picked box's
 * place); the best cluster is the one of largest IoU, lowest index among equals.  If there is one and its IoU >= fuse_iou (`>=` as in
 * yolo2_nms, not the paper's `>`) the candidate joins: Sx0 += s * x0 ... (one multiply, one add), S += s, T += 1, fused box = sums / S.
 * Otherwise it opens a cluster whose fused box is the candidate's box itself (sums s * x, S = s, T = 1).  A cluster's score is
 * ((S / T) * min(T, V)) / V.  Per image the clusters are written class ascending, in creation order inside a class, to out_conf [B,R,C]
 * (the score in the class's column, +0.0f in the others), out_xy_min / out_xy_max [B,R,2]; rows[b] = the number of rows written, and every
 * row from there up to R is +0.0f.  f32, bit for bit reproducible (tests/tta_ref.py).  `flags` (one int, zeroed by the caller, only ever
 * OR-ed) receives YOLO2_WBF_FLAG_CANDIDATES: more than YOLO2_WBF_MAX_CANDIDATES candidates in some (image, class); _CLUSTERS: more than
 * max_per_class clusters in some (image, class) -- such an (image, class) emits nothing; _ROWS: more than R clusters in an image, which
 * emits its first R.  A caller treats a non-zero word as an error.  Two launches: fuse (one workgroup per (image, class)) and emit (one
 * per image).  ws: yolo2_wbf_workspace_bytes(B, C, max_per_class) bytes, 16-byte aligned, any content.
 * B >= 1, 1 <= M <= 32768, C >= 1, threshold >= 0, fuse_iou finite, V >= 1, 1 <= max_per_class <= 1024, R >= 1; anything else is
 * YOLO2_E_ARG before any HIP call.  Boxes finite with xy_min <= xy_max.  Unit view weights and per class only. */
#define YOLO2_WBF_MAX_CANDIDATES 4096
#define YOLO2_WBF_FLAG_CANDIDATES 1
#define YOLO2_WBF_FLAG_CLUSTERS 2
#define YOLO2_WBF_FLAG_ROWS 4
size_t yolo2_wbf_workspace_bytes(int B, int C, int max_per_class);
int yolo2_tta_gather(const float *conf, const float *xy_min, const float *xy_max, float *out_conf, float *out_xy_min, float *out_xy_max,
                     int B, int N, int C, int M, int offset, float sx, float sy, float cell_w0, int flip, void *stream);
int yolo2_wbf(const float *conf, const float *xy_min, const float *xy_max, float *out_conf, float *out_xy_min, float *out_xy_max, int *rows,
              int *flags, void *ws, int B, int M, int C, int V, int max_per_class, int R, float threshold, float fuse_iou, void *stream);

/* ---- optimizers: train.py:70-80 (TF-1.0 Apply* kernels), flat f32 buffers of n elements ------ */
int yolo2_adam(float *w, const float *g, float *m, float *v, long n, float alpha, float beta1,
               float beta2, float eps, float gscale, void *stream);   /* alpha = lr*sqrt(1-b2^t)/(1-b1^t) */
int yolo2_momentum(float *w, const float *g, float *acc, long n, float lr, float momentum,
                   float gscale, void *stream);
int yolo2_sgd(float *w, const float *g, long n, float lr, float gscale, void *stream);
int yolo2_rmsprop(float *w, const float *g, float *ms, float *mom, long n, float lr, float decay,
                  float momentum, float eps, float gscale, void *stream);
int yolo2_adagrad(float *w, const float *g, float *acc, long n, float lr, float gscale,
                  void *stream);
int yolo2_adadelta(float *w, const float *g, float *acc, float *acc_update, long n, float lr,
                   float rho, float eps, float gscale, void *stream);
/* tf.train.FtrlOptimizer (train.py:78, config.ini [optimizer_ftrl]): TF-1.0 ApplyFtrl;
 * accum starts at initial_accumulator_value, linear at 0; lr_power <= 0 (-0.5 takes the sqrt form) */
int yolo2_ftrl(float *w, const float *g, float *accum, float *linear, long n, float lr, float lr_power,
               float l1, float l2, float gscale, void *stream);
/* tf.train.ExponentialMovingAverage's assign_moving_average over a flat f32 arena: ema -= (ema - w) * one_minus_decay, per element
 * d = ema - w; d = d * one_minus_decay; ema = ema - d, each rounded once in f32 (no FMA), NaN / inf propagating.  One launch; any n >= 1 and any
 * 4-byte aligned pointers (16-byte accesses where both are 16-byte aligned at the same element); 0 <= one_minus_decay <= 1. */
int yolo2_ema_update(float *ema, const float *w, long n, float one_minus_decay, void *stream);
/* Gradient accumulation, the mean over the micro-batches and weight decay in one launch over the flat f32 arenas (csrc/grad_combine.hip).
 *   YOLO2_GRAD_STORE  acc[i] = g[i]                       (the first micro-batch: acc never needs zeroing)
 *   YOLO2_GRAD_ADD    acc[i] = acc[i] + g[i]
 *   YOLO2_GRAD_FINAL  s = g[i]; if (acc) s = acc[i] + s; s = s * scale; for i inside a range and decay != 0: s = s + decay * w[i]; g[i] = s;
 *                     for i inside a range and shrink != 1: w[i] = w[i] * shrink      (decoupled decay: w *= 1 - lr * wd ahead of the update)
 * Every operation is rounded once in f32 (no FMA), NaN / inf propagating; tests/grad_combine_ref.py states the same in NumPy and the two agree bit for bit.
 * ranges_device: n_ranges >= 0 sorted, disjoint half-open element ranges {b0,e0,b1,e1,...} inside [0, n) in DEVICE memory, any begins and ends (the caller
 * checks the order: yolo_tf_amd.ops.grad_ranges); it and w are read only in FINAL with n_ranges > 0 and (decay != 0 or shrink != 1), and must not be NULL then.
 * n >= 0 (0: nothing is launched); acc must not be NULL in STORE / ADD; any 4-byte aligned pointers (16-byte accesses where the arenas that are read are aligned
 * alike).  A workgroup takes chunks of YOLO2_GRAD_COMBINE_CHUNK elements and finds a chunk's place in the table once. */
enum { YOLO2_GRAD_STORE = 0, YOLO2_GRAD_ADD = 1, YOLO2_GRAD_FINAL = 2 };
#define YOLO2_GRAD_COMBINE_CHUNK 4096
int yolo2_grad_combine(float *g, float *acc, float *w, long n, int mode, float scale, float decay, float shrink,
                       const long *ranges_device, int n_ranges, void *stream);
/* x *= scale (1/world averaging of the all-reduced gradient ahead of clip_by_norm) */
int yolo2_scale(float *x, long n, float scale, void *stream);
/* x[a:b] = 0 for nranges half-open element ranges given as a HOST array {a0,b0,a1,b1,...}: the accumulating filter
 * gradients (yolo2_conv2d_wgrad_accumulates) are cleared per step, nothing else */
int yolo2_zero_ranges(float *x, const long *ranges_host, int nranges, void *stream);
/* Inference-time batch-norm folding for yolo2_conv2d_bias_leaky (slim.batch_norm is_training=False,
 * model/yolo2/inference.py:62-66): Wf[r,n] = W[r,n]*s[n], bias[n] = beta[n] - moving_mean[n]*s[n],
 * s = gamma/sqrt(moving_var+eps); W, Wf: HWIO f32 viewed as [rows = k*k*Cin][C]. */
int yolo2_bn_fold(const float *W, const float *gamma, const float *beta, const float *moving_mean,
                  const float *moving_var, float *Wf, float *bias, long rows, int C, float eps, void *stream);
/* per-tensor tf.clip_by_norm (slim create_train_op clip_gradient_norm, train.py:127-129):
 * seg_off int64[nseg+1] element offsets into g; ws >= nseg doubles */
int yolo2_clip_by_norm(float *g, const long *seg_off, int nseg, float clip, double *ws,
                       void *stream);
/* the same clip (tf.clip_by_norm, train.py:127-129) with every tensor's sum of squares formed in a fixed order, for the deterministic training mode: 64
 * workgroups per tensor store one partial each (no atomic), the scale pass adds them in index order.  ws: yolo2_clip_fixed_workspace_bytes(nseg) bytes
 * (64 doubles per tensor), may hold anything on entry; a smaller ws_bytes: YOLO2_E_ARG, nothing launched. */
size_t yolo2_clip_fixed_workspace_bytes(int nseg);
int yolo2_clip_by_norm_fixed(float *g, const long *seg_off, int nseg, float clip, double *ws, size_t ws_bytes, void *stream);

/* ---- diagnostics -----------------------------------------------------------------------------
 * fills out[64*4] with the raw result of ds_read_b64_tr_b16 over a 0..N ramp (layout self-test) */
int yolo2_selftest_tr16(short *out, void *stream);
/* Which kernel variant the calling thread's most recent yolo2_conv2d* / yolo2_conv2d_wgrad call launched (the choice is
 * shape-driven, so parity tests assert that the variant they mean to check is the one that ran):
 *   conv plan  out8 = {tile pixels BM, tile filters BN, waves, 16-byte chunks per K row, LDS stages,
 *                      split (0 none, 1 K-sliced + finishing kernel, 2 stream-K), grid x, grid y};  all -1 = first-layer kernel
 *   wgrad plan out8 = {tile channels BC, tile filters BN, waves, taps paired, pixel ranges, XCD-local placement,
 *                      workgroups, direct store (no atomics)};                                      all -1 = first-layer kernel
 * The conv plan words are a copy of what the launch rule (csrc/conv_route.hip y2_conv_route) decided for the call; the persistent and tap-fused
 * families report their own constants there (stages 9 / 18; split bit 8: the BN-backward sums came from the epilogue; tap-fused grid y bits 8..:
 * the owner cost in use).  yolo2_debug_conv_route gives the same words without a launch. */
int yolo2_debug_last_conv_plan(int *out8);
/* host-side route of a yolo2_conv2d* call, computed by the function the launch uses.  Nothing is launched or allocated; with cus > 0 no device is
 * touched at all (cus <= 0 asks the runtime for the current device's CU count once per process, like a launch).
 *   mode: 0 plain, 1 bias and / or activation, 2 yolo2_conv2d_bn, 3 yolo2_conv2d_dgrad_bn;  align_bits: 1 = O, 2 = F, 4 = Yprev 16-byte aligned;
 *   ws_bytes: 0 = no workspace;  cus: compute units (= stream workgroups; <= 0: the process's current value);
 *   exclude: families / features that step aside -- 1 image layer, 2 conv_c32, 4 conv_c64, 8 conv_d1, 16 tap-fused, 32 its loader / consumer member,
 *   64 everything stream-K.  Not an explicit snapshot: the process-wide debug setters, the environment knobs and the calling thread's deterministic
 *   flag are read at the time of the call, as a launch reads them.
 *   out12 = {the eight conv plan words, partial rows (0: none written), statistics source (0 none, 1 the kernel's epilogue, 2 a column-sum pass over
 *            the output, 3 the two-step BN-backward reduction), pending (dgrad_bn), family (0 image layer, 1 c32, 2 c64, 3 d1, 4 pp, 5 s4, 6 igemm)} */
int yolo2_debug_conv_route(int B, int H, int W, int Cp, int ldp, int Nf, int ldo, int ksize, int dtype, int mode, int align_bits, size_t ws_bytes,
                           int cus, unsigned exclude, int *out12);
/* measurement hook: launches an empty kernel (bench.py calibrates the overhead of its HIP-event brackets with it) */
int yolo2_debug_noop(void *stream);
/* test hook (process-wide): 0 = per-tap 3x3 kernels only; 2 (and any other non-zero value) = the ping-pong tap-fused kernel (csrc/conv_pp.hip) wherever
 * its launch rule admits it; 3 = the loader / consumer member of the same family under the same rule (csrc/conv_s4.hip: four computing waves of
 * 128 x 64 + four loader waves; plan word `waves` = 4).  YOLO2_IGEMM_TAP sets the initial value. */
int yolo2_debug_set_igemm_tap(int mode);
/* experiments build of csrc/conv_s4.hip only (timing ablations, phase stamps); ignored by the product build */
int yolo2_debug_set_s4_abl(int abl);
/* test / A-B hook for the ping-pong kernel.  grid: 0 = by rule (default), 1 = stream-K over one workgroup per CU, 2 = one workgroup per
 * tile, >= 8 = that many workgroups, <= -2 = every tile cut into exactly -grid shares, -1 = keep; a stream-K grid never exceeds the
 * number of K steps.  sched: the kernel's LOAD-phase order (2 in the product build; others only in scripts/pp_experiments_build.sh's;
 * an order the library was not built with sends the layer to the per-tap kernels).  min_steps / min_share: the rule's gates (K steps
 * per tile, K steps per workgroup).  A negative argument keeps the current value. */
int yolo2_debug_set_pp(int grid, int sched, int min_steps, int min_share);
/* tests / A-B: cost units (in K steps) the stream-K partition of the ping-pong kernel charges to the workgroup that owns a tile -- it also waits for
 * and sums its partners' partial tiles and runs the epilogue, so it gets up to that many fewer K steps (csrc/conv_pp.hip "cost-balanced shares");
 * 0 = equal K-step shares.  The library clamps it below half a share.  YOLO2_PP_CV sets the initial value. */
int yolo2_debug_set_pp_cost(int cv);
/* tests: the stream-K owners' wait limit in microseconds (0 = the default, 2 s); unclamped != 0 lets a grid forced through yolo2_debug_set_pp
 * exceed the number of K steps -- a partition no owner can be served by, which must end in yolo2_check_async_errors() == YOLO2_E_LAUNCH */
int yolo2_debug_set_streamk_wait_us(int us, int unclamped);
int yolo2_debug_last_wgrad_plan(int *out8);
/* process-wide, tests / A-B only: 0 = product rule (bf16 3x3 layers: the row-of-taps kernel of csrc/conv_wgrad3.hip; everything else: the per-tap
 * transpose-read kernel of csrc/conv_wgrad.hip); 1 = scalar reference gather (layout-proof, slow); 2 = the per-tap kernel for every shape
 * (round 4's path); 10 + v = variant v (0..2) of the row-of-taps kernel for every shape it can take.  YOLO2_WGRAD_VARIANT sets the initial value. */
void yolo2_debug_set_wgrad_variant(int variant);
/* host-side plan of the row-of-taps filter-gradient kernel for a shape on a device with `cus` compute units (force_variant < 0: by rule):
 * out9 = {variant (-1: not taken), pixel ranges, padded pixels per range, workgroups, XCD mapping, plain stores, channel tile, filter tile, waves} */
int yolo2_debug_wgrad_row_plan(int B, int H, int W, int Cin, int Cout, int cus, int force_variant, int *out9);
/* host-side plan of yolo2_conv2d_wgrad_ws for a shape on a device with `cus` compute units (the function the workspace query and the launch use):
 * out4 = {kernel family (0 image layer, 1 conv1's kernel, 2 row-of-taps kernel, 3 per-tap kernel), slots (1: single range, no workspace),
 *         floats per slot, workgroups of the producer launch}.  After a yolo2_conv2d_wgrad_ws call yolo2_debug_last_wgrad_plan reports the plan words of
 * yolo2_conv2d_wgrad with `pixel ranges` = slots; the image layer reports {8, 32, 4, 9, slots, 0, slots, 0} instead of all -1. */
int yolo2_debug_wgrad_ws_plan(int B, int H, int W, int Cin, int ldx, int Cout, int ldy, int ksize, int dtype, int cus, int *out4);
/* the multiply-high division constants of that kernel's DMA address arithmetic: floor(q / d) == (uint64(q) * m >> 32) >> s for 0 <= q < 2^31 */
int yolo2_debug_magic_u32(unsigned d, unsigned *m, unsigned *s);

/* ---- on-device input pipeline: utils/data/__init__.py:50-109,162-175 + utils/preprocess.py:28-71 after JPEG
 * decode.  `src` holds the decoded uint8 RGB images back to back (any sizes); per image the caller supplies the
 * outcome of every random draw of the reference (tf.random_uniform / tf.cond):
 *   crop_*      tf.image.crop_to_bounding_box arguments (whole image when random_crop is not taken)
 *   flags       which branches were taken; brightness = delta added (tf.image.random_brightness, max_delta 63),
 *               saturation / contrast = factors in [0.5, 1.5], hue = delta in [-0.032, 0.032],
 *               noise_scale = U(5, 15) multiplying tf.truncated_normal (generated on the device from noise_seed)
 * out: f32 [B, H, W, 3] in 0..255 (tf.clip_by_value), ready for yolo2_image_prep.  ws: >= 3*B doubles when any image
 * takes the contrast branch (per-channel means of AdjustContrastv2). */
#define YOLO2_AUG_FLIP 1u
#define YOLO2_AUG_BRIGHTNESS 2u
#define YOLO2_AUG_SATURATION 4u
#define YOLO2_AUG_HUE 8u
#define YOLO2_AUG_CONTRAST 16u
#define YOLO2_AUG_NOISE 32u
#define YOLO2_AUG_GRAY 64u
typedef struct yolo2_augment_params {
    long long src_offset;            /* byte offset of the image's first pixel in src */
    int src_w, src_h;
    int crop_x, crop_y, crop_w, crop_h;
    unsigned flags;
    float brightness, saturation, hue, contrast, noise_scale;
    unsigned long long noise_seed;
} yolo2_augment_params;
int yolo2_augment_images(const unsigned char *src, const yolo2_augment_params *params_device, double *ws, float *out,
                         int B, int H, int W, int any_contrast, void *stream);

/* ---- mosaic and MixUp (new work, the reference has neither): an output image composed of several sources.
 * tiles [B][L][T] (device), L = 1 or 2 layers of T = 1 .. 4 tiles.  A tile resizes its crop of its source to a VIEW of view_w x view_h
 * pixels -- the tap rule of yolo2_augment_images with (W, H) = (view_w, view_h), its same-size copy shortcut included -- and places view
 * pixel (0, 0) at output pixel (origin_x, origin_y), which may be negative or beyond the frame.  The tile supplies the output pixels of
 * its half-open rectangle [x0, x1) x [y0, y1): at (x, y), with (u, v) = (x - origin_x, y - origin_y), the view's pixel (v, u) where
 * 0 <= u < view_w and 0 <= v < view_h (with `flip` the view is mirrored first: u -> view_w - 1 - u), and `fill` on all three channels
 * elsewhere.  A slot with x1 <= x0 or y1 <= y0 is unused.  The caller guarantees that the rectangles of a layer partition the frame
 * (a pixel no rectangle holds is not written; the part of a rectangle beyond the frame is ignored) and, as for yolo2_augment_images,
 * that every crop lies inside its source.
 * mix [B] (device) is the weight lam of layer 0: with L = 2 and mix[b] != 1 the pixel is a * lam + b * (1.0f - lam) of the two layers'
 * values in f32 without contraction; with mix[b] == 1 layer 1 is not evaluated (its tiles may hold anything).  mix may be NULL when
 * L = 1.  The chain of yolo2_augment_images then runs on the composite, driven by photo [B] (device; flags and scalars only, the
 * geometry fields and YOLO2_AUG_FLIP are ignored): brightness, saturation, hue, contrast about the COMPOSITE's per-channel mean (fill
 * included), noise indexed by the output pixel, grey, clip.  One full-frame tile (L = T = 1, view = frame, origin 0) gives the bits of
 * yolo2_augment_images.  out: f32 [B, H, W, 3]; ws: yolo2_augment_workspace_bytes(B) bytes when any image takes the contrast branch, any
 * content.  L, T out of range, a NULL mix with L = 2, a NULL ws with any_contrast, H * W >= 2^30: YOLO2_E_ARG before any HIP call.
 * 2 x 2 layouts are what the host builds; no rotation or shear, no per-tile colour. */
typedef struct yolo2_compose_tile {
    long long src_offset;            /* as yolo2_augment_params */
    int src_w, src_h;
    int crop_x, crop_y, crop_w, crop_h;
    int view_w, view_h;
    int origin_x, origin_y;
    int x0, y0, x1, y1;
    unsigned flip;
} yolo2_compose_tile;
int yolo2_compose_images(const unsigned char *src, const yolo2_compose_tile *tiles, const yolo2_augment_params *photo,
                         const float *mix, double *ws, float *out, int B, int L, int T, int H, int W, float fill,
                         int any_contrast, void *stream);

/* transform_labels (utils/data/__init__.py:112-145) for a batch: objects_coord [total,4] = (xmin,ymin,xmax,ymax) in
 * [0,1], objects_class [total], image b owns objects first_object[b] .. first_object[b+1]-1 (processed in order: the
 * last object of a cell wins, class bits accumulate).  Outputs are the loss's label tensors, each [B, cells, ...],
 * bit-exact with the reference.  error_flag (device int, caller zeroes it): bit 0 = object outside the grid or class
 * out of range (the reference raises IndexError), bit 1 = negative box extent (the reference asserts). */
int yolo2_transform_labels(const int *objects_class, const float *objects_coord, const int *first_object, float *mask,
                           float *prob, float *coords, float *offset_xy_min, float *offset_xy_max, float *areas, int B,
                           int classes, int cell_width, int cell_height, int *error_flag, void *stream);

/* ---- data-parallel support (new work: the reference has no multi-GPU path, README.md:99).  The collectives themselves run in
 * torch.distributed (RCCL); the library only provides what has to happen on the device around them. */
/* Stream-K convolution launches use n workgroups instead of one per CU (0 = default): a data-parallel process leaves the CUs an
 * RCCL ring occupies to it.  Process-wide; never affects results. */
int yolo2_set_stream_workgroups(int n);
int yolo2_get_stream_workgroups(void);
/* gradient wire format: round an f32 range to bf16 / widen it back (16-byte aligned pointers) */
int yolo2_cast_f32_bf16(const float *src, void *dst, long n, void *stream);
int yolo2_cast_bf16_f32(const void *src, float *dst, long n, void *stream);
/* test instrument: `workgroups` persistent workgroups, one whole CU each (160 KiB LDS), until *stop != 0 or max_us have passed;
 * *started counts the resident ones (what a collective's persistent kernels look like to the dispatcher) */
int yolo2_debug_occupy(int workgroups, int *stop, int *started, int max_us, void *stream);

/* ---- evaluation: PASCAL VOC average precision of the detections a batch leaves on the device (new work: the reference has no
 * evaluator).  COCO's protocol has its own section and entry points below ("evaluation, COCO protocol").
 *
 * Stage A, yolo2_eval_collect, once per detect batch; no host synchronisation, no copy to the host.
 *   conf [B,N,C] f32 after NMS (zeros where suppressed), xy_min / xy_max [B,N,2] f32 in cell units.  Ground truth: gt_class [G] int,
 *   gt_box [G,4] f32 (xmin, ymin, xmax, ymax) IN THE SAME CELL UNITS (no coordinate transform happens here), gt_difficult [G] bytes,
 *   gt_first [B+1] CSR offsets per image (at most YOLO2_EVAL_MAX_GT_PER_IMAGE boxes in one image).  All device pointers, non-null even
 *   when G == 0.  image_base = dataset index of the batch's first image; images b >= n_valid are padding: no records, no npos.
 *   Detections: YOLO2_EVAL_MODE_DETECT = one per box, class = FIRST arg-max of conf[i,:], score = that value, kept if score > threshold
 *   (what detect.py prints); YOLO2_EVAL_MODE_ALL = one per (box, class) with conf[i,c] > threshold (what Darknet's `valid` emits).  NaN
 *   scores make no detection.
 *   Matching (VOC devkit), independent per (image, class): detections are visited in (score descending, box index ascending) order; the
 *   candidate is the ground truth of the same image and class with the highest IoU, ties to the lowest index, already matched boxes
 *   included; IoU is f32 in the reference's operation order, (a1+a2)-inter with floor 1e-10 (utils/postprocess.py:21-36).
 *   iou > iou_threshold (strict) and candidate difficult: IGNORED; iou > iou_threshold and candidate not yet matched: TP, the candidate
 *   becomes matched; iou > iou_threshold and candidate matched: FP (duplicate); otherwise FP.
 *   Output: yolo2_eval_record entries appended to `records` (capacity max_records) in (image, box, class) order, at positions that come
 *   from counts and prefix sums only (two runs give bitwise equal buffers), and npos[C] += non-difficult ground truth per class.
 *   state: YOLO2_EVAL_STATE_WORDS 8-byte words the caller zeroes before the first collect: [0] records wanted so far, [1] error bits.
 *   Nothing is ever written at or past records[max_records]; word 0 keeps counting, and yolo2_eval_finalize reports both numbers.
 *   ws: yolo2_eval_collect_workspace_bytes(B).
 * Stage B, yolo2_eval_finalize, once per evaluation; reads the record count from `state` on the device (no synchronisation).
 *   Sorts the non-ignored records per class by (score descending, image index ascending, box index ascending) -- a radix sort on the
 *   device over box (< N), image (< n_images), score bits and class -- and integrates: inclusive counts of TP and FP along that order,
 *   recall = tp / npos, precision = tp / (tp + fp) in f64; ap07 = mean over t = k/10, k = 0..10 of the highest precision among points
 *   with recall >= t (0 if none); ap12 = area under the monotone precision envelope, summed where recall changes.  npos == 0: both NaN;
 *   npos > 0 and no detections: 0.
 *   results: yolo2_eval_result_bytes(C) bytes of 8-byte words: ap07 [C] f64, ap12 [C] f64, then int64 npos [C], tp [C], fp [C],
 *   ignored [C], records held, records wanted (> max_records: the buffer was too small and every other number is void), error bits
 *   (1: ground truth class outside [0,C); 2: gt_first not ascending within [0,G] or too many boxes in an image; 4: a record's image, box
 *   or class outside n_images, N, C).  Optional (may be NULL): sorted_records [max_records] (class-major, ignored records last),
 *   cum_tp / cum_fp [max_records] int = the inclusive counts per class along the sorted order.
 *   ws: yolo2_eval_workspace_bytes(max_records, C) = two record buffers + the digit table of the sort, each rounded up to 256 bytes. */
enum { YOLO2_EVAL_MODE_DETECT = 0, YOLO2_EVAL_MODE_ALL = 1 };
enum { YOLO2_EVAL_FP = 0, YOLO2_EVAL_TP = 1, YOLO2_EVAL_IGNORED = 2 };
#define YOLO2_EVAL_MAX_GT_PER_IMAGE 512
#define YOLO2_EVAL_MAX_CLASSES (1 << 20)
#define YOLO2_EVAL_STATE_WORDS 2
typedef struct {
    float score;
    int image;                 /* dataset index */
    int box;                   /* index into the N boxes of the image */
    unsigned class_flag;       /* class << 2 | YOLO2_EVAL_FP / _TP / _IGNORED */
} yolo2_eval_record;
size_t yolo2_eval_record_bytes(long max_records);                 /* 16 * max_records */
size_t yolo2_eval_collect_workspace_bytes(int B);                 /* 4 * B */
size_t yolo2_eval_workspace_bytes(long max_records, int C);
size_t yolo2_eval_result_bytes(int C);                            /* 8 * (6 C + 3) */
int yolo2_eval_collect(const float *conf, const float *xy_min, const float *xy_max, const int *gt_class, const float *gt_box,
                       const unsigned char *gt_difficult, const int *gt_first, int G, int B, int N, int C, int n_valid, int image_base,
                       int mode, float threshold, float iou_threshold, void *records, long max_records, unsigned long long *state,
                       int *npos, int *ws, void *stream);
int yolo2_eval_finalize(const void *records, long max_records, unsigned long long *state, const int *npos, int C, int n_images, int N,
                        void *ws, size_t ws_bytes, void *results, void *sorted_records, int *cum_tp, int *cum_fp, void *stream);

/* ---- evaluation, COCO protocol: pycocotools' COCOeval for iouType 'bbox', restated (new work).  AP / AR over IoU thresholds, area
 * ranges and detection limits.  Two deviations from pycocotools, both deliberate: IoU is f32 (the IoU of the section above; pycocotools
 * uses f64), so that a comparison at a threshold gives the same answer on the device and in the checker bit for bit; and `area` of a
 * ground truth box is whatever the caller passes (the pixel area of the box unless it knows the segmentation's).
 *
 * Detections are formed exactly as in the section above (modes, strict > threshold, NaN, -0 -> +0).  Inside one (image, class) they are
 * ordered by score descending, then box index ascending; the position in that order is the RANK.  Only ranks < max_dets (at most
 * YOLO2_EVAL_COCO_MAX_DETS) produce a record.
 * Ground truth: gt_class [G], gt_box [G,4] in cell units, gt_area [G] f32 in source-image pixels, gt_flags [G] bytes: bit 0 = ignore,
 * bit 1 = crowd (crowd implies ignore: either bit ignores).  Under area range [lo, hi] a box is IGNORED when a flag bit is set, or
 * area < lo, or area > hi.
 * Tables come from the HOST (read during the call, passed to the kernels by value): area_ranges [A][2] f32 (A <= 4), iou_thresholds
 * [T] f32 (T <= 10), recall_thresholds [R] f64 (R <= 101, ascending), slices [S][2] int = (area range index, detection limit <=
 * max_dets), S <= 8.  None may be NaN.
 * scale [B,2] f32 = source pixels per cell (x, y) of each image.  A detection's area is ((xmax-xmin)*scale_x) * ((ymax-ymin)*scale_y)
 * in f32, contraction off.
 * IoU against a non-crowd box: that f32 IoU.  Against a crowd box: inter / fmaxf((xmax-xmin)*(ymax-ymin) of the detection, 1e-10f), f32.
 * Matching, per (image, class, area range a, IoU threshold t), detections in rank order.  The class's boxes are scanned non-ignored
 * (under a) first, then ignored, each group in index order.  Per detection: best = min((double)t, 1 - 1e-10), m = none; for each box g
 * in scan order: skip g if it is matched at (a, t) and not crowd; STOP if m is set, m is not ignored and g is ignored; skip g if
 * (double)iou(d, g) < best; otherwise best = iou, m = g (>=: of equal overlaps the LAST in scan order wins; iou == t matches).  If m is
 * set the detection is MATCHED, it is IGNORED exactly when m is ignored, and m becomes matched (a crowd box can be taken again).  An
 * unmatched detection is ignored when its own area is < lo or > hi.  The outcome for the first k detections does not depend on later
 * ones, so matching runs once with max_dets and smaller detection limits are rank filters.
 * Record (40 bytes): score, image, box, class, rank, and two bit sets: bit a * T + t of `matched` / `ignored`.  Records are appended in
 * (image, class, rank) order at positions that come from counts and prefix sums only.  npig [A][C] int (caller zeroes it) += the boxes
 * of the class not ignored under range a.  state, capacity and overflow: as in the section above (nothing is written at or past
 * records[max_records], word 0 keeps counting, finalize reports both).  ws: yolo2_eval_coco_collect_workspace_bytes(B, N, C).
 * C <= YOLO2_EVAL_COCO_MAX_CLASSES.  Box coordinates must be finite: overlaps of NaN boxes follow fminf / fmaxf and are no part of
 * the rules.
 * Finalize: sorts by (class, score descending, image ascending, rank ascending) and, per class k, slice s = (a, limit), threshold t:
 * takes the records with rank < limit in that order, drops those ignored at (a, t); npig == 0: ap = recall = -1; otherwise cumulative
 * tp / fp, rc = tp / npig, pr = tp / ((fp + tp) + 2.220446049250313e-16) in f64; recall[s,t,k] = last rc (0 without records); pr is
 * made non-increasing from the back (reverse running maximum); q[r] = pr at the first index with rc >= recall_thresholds[r], 0 if
 * none; ap[s,t,k] = (q[0] + ... + q[R-1], added in index order) / R.
 * results: yolo2_eval_coco_result_bytes(S, T, A, C) bytes of 8-byte words: ap [S][T][C] f64, recall [S][T][C] f64, npig [A][C] int64,
 * records held, records wanted, error bits (as above; 4 also covers a rank >= max_dets).
 * ws of finalize: yolo2_eval_coco_workspace_bytes(max_records, C) = two buffers of 16-byte sort keys + the digit table. */
#define YOLO2_EVAL_COCO_MAX_AREAS 4
#define YOLO2_EVAL_COCO_MAX_IOUS 10
#define YOLO2_EVAL_COCO_MAX_RECALLS 101
#define YOLO2_EVAL_COCO_MAX_SLICES 8
#define YOLO2_EVAL_COCO_MAX_DETS 128
#define YOLO2_EVAL_COCO_MAX_CLASSES 1024
typedef struct {
    float score;
    int image;                 /* dataset index */
    int box;                   /* index into the N boxes of the image */
    int cls;
    int rank;                  /* position among the detections of its (image, class) */
    unsigned reserved;         /* 0 */
    unsigned long long matched;    /* bit a * T + t */
    unsigned long long ignored;    /* bit a * T + t */
} yolo2_eval_coco_record;
size_t yolo2_eval_coco_record_bytes(long max_records);            /* 40 * max_records */
size_t yolo2_eval_coco_collect_workspace_bytes(int B, int N, int C);
size_t yolo2_eval_coco_workspace_bytes(long max_records, int C);
size_t yolo2_eval_coco_result_bytes(int S, int T, int A, int C);  /* 8 * (2 S T C + A C + 3) */
int yolo2_eval_coco_collect(const float *conf, const float *xy_min, const float *xy_max, const int *gt_class, const float *gt_box,
                            const float *gt_area, const unsigned char *gt_flags, const int *gt_first, const float *scale, int G, int B,
                            int N, int C, int n_valid, int image_base, int mode, float threshold, const float *area_ranges, int A,
                            const float *iou_thresholds, int T, int max_dets, void *records, long max_records,
                            unsigned long long *state, int *npig, void *ws, size_t ws_bytes, void *stream);
int yolo2_eval_coco_finalize(const void *records, long max_records, unsigned long long *state, const int *npig, int C, int n_images, int N,
                             int A, int T, int max_dets, const int *slices, int S, const double *recall_thresholds, int R, void *ws,
                             size_t ws_bytes, void *results, void *stream);

/* ---- dimension clusters: the anchors of a dataset (new work).  The reference lists "Dimension cluster" as an unchecked roadmap item
 * (README.md:88) and has no code for it; every YOLOv2 model reads the result through `[yolo2] anchors` (model/yolo2/__init__.py:106).
 * The method is YOLO9000 (Redmon & Farhadi 2016), section 2 "Dimension Clusters": k-means over the ground truth boxes' (w, h) with
 * distance 1 - IoU.  Many JOBS = (k, centroids) run in one launch; one Lloyd iteration is yolo2_anchor_assign + yolo2_anchor_update.
 *
 * boxes [n][2] f32 = (w, h) in grid-cell units (the unit of config/yolo2/anchors/ *.tsv), 16-byte aligned, 1 <= n <=
 * YOLO2_ANCHOR_MAX_BOXES, every value finite with 2^-12 <= v < 2^12 (the caller checks the values: the fixed-point sums below rely on it).
 * centroids [jobs][kmax][2] f32, job_k [jobs] int with 1 <= job_k <= kmax <= YOLO2_ANCHOR_MAX_K; slots at and past job_k are never
 * read or written.  jobs <= YOLO2_ANCHOR_MAX_JOBS.
 * Assign: for box (w, h) and centroid (cw, ch), f32, no contraction, in this order: inter = min(w,cw) * min(h,ch); uni = (w*h + cw*ch)
 *   - inter; iou = inter / uni (correctly rounded).  The box belongs to the centroid of largest iou, of equal ones to the lowest index.
 *   Into ws, per job: per cluster count, sum of rint(w * 2^24), sum of rint(h * 2^24) (rint of the f64 product, half to even), then one
 *   sum of rint(best_iou * 2^30): 64-bit integers, so the sums are exact and the same whatever the order of the adds.
 *   done [jobs] (may be NULL): a job with done != 0 is skipped.  assignment (may be NULL): [jobs][n] bytes, the cluster of every box.
 * Update (done and iterations given): a non-empty cluster's centroid becomes (float)((double)sum / (double)count * 2^-24) for w and h;
 *   an empty one keeps its bits.  iterations[job] += 1; when no centroid of the job changed bitwise, done[job] = 1 (with exact sums:
 *   no box changed cluster).  A job with done != 0 on entry is left alone altogether.
 * Score (done and iterations both NULL): the centroids stay; counts and / or avg_iou are required.
 * Both passes: counts [jobs][kmax] int64 and avg_iou [jobs] f64 = sum / 2^30 / n (each may be NULL) describe the assignment just
 *   consumed, i.e. the centroids yolo2_anchor_assign ran with, and the job's workspace words are cleared.
 * ws: yolo2_anchor_workspace_bytes(jobs, kmax) = 8 * jobs * (3 * kmax + 1) bytes, zeroed by the caller ONCE, at allocation.
 * n of the update call is the n of the assign call it follows. */
#define YOLO2_ANCHOR_MAX_K 32
#define YOLO2_ANCHOR_MAX_JOBS 65535
#define YOLO2_ANCHOR_MAX_BOXES ((1 << 27) - 1)
size_t yolo2_anchor_workspace_bytes(int jobs, int kmax);           /* 0 for arguments out of range */
int yolo2_anchor_assign(const float *boxes, int n, const float *centroids, const int *job_k, int jobs, int kmax,
                        unsigned long long *ws, size_t ws_bytes, const int *done, unsigned char *assignment, void *stream);
int yolo2_anchor_update(float *centroids, const int *job_k, int jobs, int kmax, unsigned long long *ws, size_t ws_bytes, int n,
                        int *done, int *iterations, long long *counts, double *avg_iou, void *stream);

/* ---- histogram summaries (new work): what the reference's train.py:44-60 asks tf.summary.histogram for, of many device tensors in
 * one call.  Specification: tests/summary_ref.py (TensorFlow 1.x core/lib/histogram/histogram.cc restated; unpinned against TensorFlow).
 * 1550 buckets: limits {-p reversed, 0, p, DBL_MAX} with p = 1e-12 * 1.1^i by repeated f64 multiplication while < 1e20 (774 values);
 * a finite value x, widened exactly to f64, goes to bucket upper_bound(limits, x); NaN / +-inf are left out and counted.
 *
 * A job is one tensor: `rows` rows of `c` values with row stride `ld` elements (a flat range of n values: rows = 1, c = ld = n; rows = 0:
 * an empty job), `dtype` YOLO2_F32 or YOLO2_BF16, `base` aligned to its element only.  Lanes c <= j < ld of a row are padding: whatever
 * they hold never reaches the result (the bytes between base and the last row's last value must be readable).  `first_item` is the sum
 * of yolo2_histogram_items() over the jobs before it; `items` of the call is that sum over all of them.  The job table lives in DEVICE memory.
 * out [njobs][YOLO2_HIST_WORDS] 64-bit words per job: YOLO2_HIST_BUCKETS counts (u64), then min, max, sum, sum_squares (f64), then num,
 * nonfinite (u64); an empty job reports min = DBL_MAX, max = -DBL_MAX.  Counts, num, nonfinite, min and max are exact; the sums are f64
 * accumulations.  The whole record of a job is bitwise reproducible and depends on the job alone: no float atomic is issued.
 * One call enqueues three operations whatever njobs is and never synchronises; ws needs no initialisation. */
#define YOLO2_HIST_BUCKETS 1550
#define YOLO2_HIST_WORDS (YOLO2_HIST_BUCKETS + 6)
typedef struct yolo2_hist_job {
    const void *base;
    long long rows;
    int c, ld, dtype;
    int first_item;
} yolo2_hist_job;
size_t yolo2_histogram_workspace_bytes(int njobs);
size_t yolo2_histogram_result_bytes(int njobs);                    /* njobs * YOLO2_HIST_WORDS * 8 */
int yolo2_histogram_items(long long rows, int c, int ld, int dtype);   /* work items of one job (a count, not a status); 0 for an empty or malformed one */
int yolo2_histogram(const yolo2_hist_job *jobs, int njobs, int items, void *out, size_t out_bytes, void *ws, size_t ws_bytes, void *stream);

/* ---- image summaries (new work): what the reference's train.py:44-53 asks tf.summary.image for, of many device images in one call.
 * Specification: tests/image_summary_ref.py (TensorFlow 1.x core/kernels/summary_image_op.cc NormalizeFloatImage plus the reference's
 * channel sum, restated; unpinned against TensorFlow).
 *
 * A job is ONE image of one tensor: `rows` = H*W pixels of `c` values every `ld` elements, `dtype` YOLO2_F32 or YOLO2_BF16 (widened to f32),
 * `base` aligned to its element only (16-byte loads are used when base and ld allow them).  Lanes c <= j < ld of a pixel are padding or a
 * concat neighbour and are never read.  depth = c for c in {1, 3, 4}; any other c is summed to ONE channel: f64, sequential from +0.0 inside
 * each group of YOLO2_IMAGE_GROUP consecutive channels, the group partials added in ascending order to a total that starts at +0.0, one
 * rounding to f32.  A pixel is finite when all its depth values are; image_min / image_max are taken over the values of the finite pixels
 * (+inf / -inf when there are none); image_min < 0: scale = 127 / max(|min|, |max|) (0 if that is < 1e-6f), offset = 128; otherwise
 * scale = 255 / image_max (0 if image_max < 1e-6f), offset = 0; byte = uint8(trunc(x * scale + offset)) with the product and the sum each
 * rounded to f32; a non-finite pixel becomes (255, 0, 0, 255)[:depth].  rows = 0 is an empty job.
 * out: njobs records of YOLO2_IMAGE_RECORD_BYTES {f32 image_min, f32 image_max, u32 non-finite pixels, f32 scale}, then the images: job j
 * writes rows * depth bytes, packed [rows][depth], at byte `out_offset` from `out` (>= njobs * YOLO2_IMAGE_RECORD_BYTES; the ranges of two
 * jobs must not overlap).  `sum_offset`: for a summed job, the index of its first f32 in the sums area of the workspace (rows floats,
 * disjoint between jobs; ignored otherwise).  `first_item` is the sum of yolo2_image_summary_items() over the jobs before it; `items` of
 * the call is that sum over all of them.  The job table lives in DEVICE memory; a malformed job, or one whose ranges leave out / ws, is
 * treated as empty.  ws: yolo2_image_summary_workspace_bytes(njobs, sum of rows over the summed jobs), no initialisation needed.
 * Every byte of a job's result depends on the job alone: min / max go through integer atomics on order-preserving keys, no float atomic is
 * issued.  One call enqueues four operations whatever njobs is and never synchronises. */
#define YOLO2_IMAGE_GROUP 8
#define YOLO2_IMAGE_RECORD_BYTES 16
typedef struct yolo2_image_job {
    const void *base;
    long long rows;
    int c, ld, dtype;
    int first_item;
    long long out_offset;
    long long sum_offset;
} yolo2_image_job;
size_t yolo2_image_summary_workspace_bytes(int njobs, long long sum_pixels);
size_t yolo2_image_summary_result_bytes(int njobs, long long image_bytes);   /* njobs * YOLO2_IMAGE_RECORD_BYTES + image_bytes */
int yolo2_image_summary_items(long long rows, int c, int ld, int dtype);      /* work items of one job (a count, not a status); 0 for an empty or malformed one */
int yolo2_image_summary_depth(int c);                                          /* channels of the image made from c: c for 1, 3, 4, otherwise 1 (a count) */
int yolo2_image_summary(const yolo2_image_job *jobs, int njobs, int items, void *out, size_t out_bytes, void *ws, size_t ws_bytes, void *stream);

/* ---- int8 inference (post-training quantisation; DESIGN.md section 15, specification: tests/quant_ref.py) -----------------------------
 * Symmetric int8 in -127 .. 127: q = clip(rint(x * inv_s), -127, 127) in f32, NaN -> 0, inv_s = float32(1) / s computed by the host.
 *
 * yolo2_conv2d_i8: NHWC implicit GEMM on the int8 MFMA, 3x3 / 1x1, stride 1, SAME; arguments as yolo2_conv2d_bias_leaky with byte operands:
 *   acc[m, n] = sum over taps and channels of P * F, exact int32 (F: [Nf][ksize*ksize][Cp] int8, the kernel's own layout, made by the host)
 *   t = float(acc) * mult[n];  y = t + bias[n];  y = y > 0 ? y : y * alpha     -- f32, every operation rounded (no fma); alpha == 1: linear
 *   out_kind YOLO2_I8_OUT_I8:   O int8  = clip(rint(y * inv_s_out), -127, 127)
 *            YOLO2_I8_OUT_BF16: O bf16  = y rounded to nearest even (the logits yolo2_head_decode reads)
 *            YOLO2_I8_OUT_F32:  O f32   = y
 *            YOLO2_I8_OUT_ACC:  O int32 = acc, the raw accumulators (diagnostic mode of the tests; mult / bias may be NULL)
 * ldp / ldo: pixel strides in ELEMENTS of P / O, so a producer can write at a channel offset inside a concat buffer.  Nf is arbitrary (the
 * store tail is masked).  Cp and ldp must be multiples of 16 and P, F 16-byte aligned; anything else is YOLO2_E_ARG ("argument check
 * failed") before any launch.  No workspace, no library-owned state; ksize * ksize * Cp < 2^17 keeps every int32 sum exact. */
enum { YOLO2_I8_OUT_I8 = 0, YOLO2_I8_OUT_BF16 = 1, YOLO2_I8_OUT_F32 = 2, YOLO2_I8_OUT_ACC = 3 };
int yolo2_conv2d_i8(const void *P, const void *F, const float *mult, const float *bias, void *O, int B, int H, int W, int Cp, int ldp,
                    int Nf, int ldo, int ksize, float alpha, float inv_s_out, int out_kind, void *stream);
/* Running abs-max of a list of tensors in one launch (calibration).  jobs: DEVICE table; job j reads `rows` rows of `c` values (dtype
 * YOLO2_F32 / YOLO2_BF16) with row stride `ld` and folds into record `slot` of out: out[2*slot] = max(out[2*slot], bit pattern of the
 * largest finite |x|), out[2*slot + 1] += number of non-finite values (ignored by the maximum).  Several jobs may share a slot.  The caller
 * zeroes `out` once; successive calls (batches) keep accumulating.  Non-negative floats order like their bit patterns, so the maximum is an
 * integer atomic and the result is exact and order-independent. */
typedef struct yolo2_absmax_job {
    const void *base;
    long long rows;
    int c, ld, dtype;
    int slot;
} yolo2_absmax_job;
int yolo2_absmax(const yolo2_absmax_job *jobs, int njobs, unsigned *out, void *stream);
/* Histograms of |x| of a list of tensors in one launch: the second calibration pass, after yolo2_absmax has fixed the ranges (the
 * percentile, MSE and entropy thresholds of yolo_tf_amd/quant.py are chosen from them on the host).  Specification: tests/calib_ref.py.
 * jobs: DEVICE table; job j reads its tensor as a yolo2_absmax job does and adds into record `slot` of out, YOLO2_CALIB_WORDS u64 words:
 * YOLO2_CALIB_BINS equal bins over [0, limit], then the number of non-finite values, then the number of values above `limit`.  Several jobs
 * may share a slot (a scale class: same limit, same inv_width).  The rule, for every element:
 *   a = |float(x)|
 *   a is NaN or inf: word[BINS] += 1, nothing else
 *   t = a * inv_width                          one f32 multiply, one rounding; inv_width = float32(2048) / limit, computed by the HOST
 *   b = (t >= 2048.f) ? 2047 : (int)t          compare before converting (t may be +inf)
 *   word[b] += 1
 *   a > limit: word[BINS + 1] += 1             the value was clamped into the last bin
 * Everything behind the one multiply is integer, so a record is exact, independent of the order of the elements and identical run to run.
 * The caller zeroes `out` once; successive calls (batches) keep accumulating.  limit and inv_width must be finite and > 0; a job that is not
 * well formed (that, rows <= 0, c <= 0, ld < c, rows * ld > 2^40, slot < 0, an unknown dtype) counts nothing.  `base` needs the alignment
 * of its element only (16-byte loads are used where base, c and ld allow).  NULL jobs / out or njobs outside 1 .. 65535 is YOLO2_E_ARG
 * before any launch.  No workspace, no library-owned state, one launch. */
#define YOLO2_CALIB_BINS  2048
#define YOLO2_CALIB_WORDS (YOLO2_CALIB_BINS + 2)      /* u64 words per record */
typedef struct yolo2_calib_job {
    const void *base;
    long long rows;
    int c, ld, dtype;
    int slot;
    float limit, inv_width;
} yolo2_calib_job;
int yolo2_calib_histogram(const yolo2_calib_job *jobs, int njobs, unsigned long long *out, void *stream);
/* Q[r*ldq + j] = quantise(X[r*ldx + j]) for r < rows, j < c (X: f32 / bf16) */
int yolo2_quantize(const void *X, int ldx, void *Q, int ldq, long rows, int c, float inv_s, int dtype, void *stream);
/* 2x2 SAME max pool on int8 bytes, stride 2 (output ceil(H/2) x ceil(W/2)) or stride 1 (output H x W); the window is clipped at the
 * bottom / right edge.  lda / ldp: pixel strides of A / P. */
int yolo2_maxpool_i8(const void *A, int lda, void *P, int ldp, int B, int H, int W, int C, int stride, void *stream);
/* yolo2_reorg on int8 bytes: out[b,y,x,(sy*2+sx)*C+c] = in[b,2y+sy,2x+sx,c]; `in` dense, `out` with pixel stride ldo */
int yolo2_reorg_i8(const void *in, void *out, int B, int H, int W, int C, int ldo, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* YOLO2_HIP_H */
