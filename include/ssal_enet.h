/*
 * ssal_enet.h -- C ABI of libssal_hip.so: the MI355X (gfx950) pool-scoring hot path.
 *
 * The reference (alfrunesiq/SemanticSegmentationActiveLearning) has no FFI: the path sits behind a
 * Python object API (models.ENet, xops.*, and score tensors assembled inline in active_learning.py)
 * executed by the TensorFlow runtime.  Each entry point below states the reference interface it
 * replaces (file:line, relative to the reference root).  INTEGRATION.md shows the ctypes stub a
 * reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / HIP types (a stream is passed as void* = hipStream_t).
 *   - every function returns an int status (SSAL_OK == 0); nothing throws across the boundary.
 *     ssal_last_error() returns a thread-local message for the last non-zero status.
 *   - "dev" pointers are device (HBM) pointers owned by the caller and only borrowed for the call;
 *     "host" pointers are host memory.  The library owns only the weights inside a handle.
 *   - activations are fp32 NHWC, conv kernels HWIO, transposed-conv kernels HW-O-I (TF layouts);
 *     all launches are stream-ordered and asynchronous.
 *   - threading: forward / score / run_layer on a COMMITTED handle may be called from any number of host threads at
 *     the same time, provided every concurrent call has its own stream and its own workspace (the image-group schedule
 *     draws its fork / join events per call from a mutex-protected pool; its side streams are one process-wide pool per
 *     device).  set_tensor / commit / destroy must not overlap any other call on the same handle.  A handle lives on
 *     ONE device -- the device that was current at commit; a call made with another current device returns
 *     SSAL_ESTATE (create one handle per device).  A call that fails half way still joins its side-stream chains into
 *     the caller's stream before it returns.
 */
#ifndef SSAL_ENET_H
#define SSAL_ENET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSAL_OK        0
#define SSAL_EINVAL    1 /* bad argument (maps to ValueError) */
#define SSAL_EHIP      2 /* HIP runtime error */
#define SSAL_ENOTIMPL  3 /* maps to NotImplementedError (active_learning.py:259-260) */
#define SSAL_ESTATE    4 /* handle not committed / tensor missing */
#define SSAL_ENOMEM    5 /* workspace too small */

/* acquisition measures, active_learning.py:239-260 (conf/default_params.json "measure") */
#define SSAL_MEASURE_ENTROPY     0
#define SSAL_MEASURE_MARGIN      1
#define SSAL_MEASURE_CONFIDENCE  2

/* arithmetic modes of the *_arith entry points.
 *   SSAL_ARITH_F32     the default and the only mode of every other entry point: exact fp32 (fmaf chains in (kh, kw, ci)
 *                      order on v_mfma_f32_*), bit-identical to the parity oracle.
 *   SSAL_ARITH_BF16X3  OPT-IN: the 128-channel regular / dilated / asymmetric bottlenecks (Bottleneck2_1 .. 3_8), the
 *                      downsample block Bottleneck2_0 and the upsample block Bottleneck4_0 (18 of the 29 launches) evaluate their convolutions on v_mfma_f32_32x32x16_bf16 with every fp32 operand
 *                      split into three bf16 terms and the six leading cross products accumulated in fp32 (what is dropped
 *                      is O(2^-24) relative per product).  Same accuracy class as fp32, a different summation: logits differ
 *                      from the default mode by <= ~1e-5, per-pixel confidences by <= 1e-4 (north_star's tolerance), per-image
 *                      scores by <= 1e-6; the max-pool + argmax of both pooling blocks is evaluated in exact fp32 (inside
 *                      Bottleneck2_0's split-operand kernel too), so the pooling indices are bit-identical.  No reference counterpart (the reference computes in fp32 on TensorFlow).
 *                      ICNet (include/ssal_icnet.h, the *_arith entries): every convolution the exact path gives to the plain
 *                      implicit-GEMM kernel k_igemm<NT, 0> -- the 1x1 reduce / increase / projection convolutions, the 3x3
 *                      convolutions on 64, 128 and 256 channels, conv5_4_k1, conv2_sub1, conv3_sub1, conv3_sub1_proj and
 *                      conv3_1_sub2_proj: 54 of the 64 convolutions of a forward call -- runs on k_igemm_bf16x3<NT>, and
 *                      conv2_2 / conv2_3 of a score call on k_bottleneck_bf16x3; the first convolutions, k_conv3x3_c32, both
 *                      up-sampling forms, the dual (projection-shortcut) launches, the conv6_cls head, pooling and the score
 *                      kernel stay exact. */
#define SSAL_ARITH_F32     0
#define SSAL_ARITH_BF16X3  1

typedef struct ssal_enet ssal_enet;

const char *ssal_version(void);
const char *ssal_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Model handle: replaces the models.ENet object (models/__init__.py:1-3, models/enet/enet.py:6-407).
 * Tensor names are the reference attribute names "<Layer>.<attr>", e.g. "Initial.kernel",
 * "Bottleneck2_3.conv_kernel.0" (KernelCol, [5,1,f,f]) / ".1" (KernelRow, [1,5,f,f]),
 * "Bottleneck4_0.res_kernel", "Final.kernel"  (enet_modules.py:139-187,366-523,730-865,1070-1214,1349-1356).
 * ---------------------------------------------------------------------------------------------- */
int ssal_enet_create(int c_in, int classes, ssal_enet **out);
int ssal_enet_destroy(ssal_enet *net);
int ssal_enet_num_tensors(const ssal_enet *net);
int ssal_enet_tensor_info(const ssal_enet *net, int i, const char **name, int *ndim, int64_t dims[4]);
/* copy one parameter tensor from host memory into the handle (staged until commit) */
int ssal_enet_set_tensor(ssal_enet *net, const char *name, const float *host, int64_t numel);
/* fold the batch-norm statistics (extra_ops.py:181-184, eps=1e-3), re-layout kernels and upload */
int ssal_enet_commit(ssal_enet *net, void *stream);
/* bytes of device scratch needed by forward/score for a batch of n images of h x w */
int64_t ssal_enet_workspace_bytes(const ssal_enet *net, int n, int h, int w);

/* ENet.call(inputs, training=False) -> logits   (models/enet/enet.py:320-407)
 * x_dev: [n,h,w,c_in] fp32, logits_dev: [n,h,w,classes] fp32; h,w divisible by 8. */
int ssal_enet_forward_nhwc(ssal_enet *net, const float *x_dev, int n, int h, int w,
                           float *logits_dev, void *ws_dev, int64_t ws_bytes, void *stream);

/* ENet.call + softmax + acquisition measure + float64 per-image mean, fused
 * (active_learning.py:229-263: pseudo_logits, pseudo_label, pseudo_prob, pseudo_confidence,
 *  pseudo_mean_confidence, pseudo_mask).  The logits never reach HBM.
 * scores_dev: [n] float64 (required).  Optional outputs (NULL to skip):
 *   label_dev [n,h,w] uint8  = argmax_k logits                      (:234-236)
 *   mask_dev  [n,h,w] uint8  = conf < threshold ? 0 : 1             (:265-269)
 *   conf_dev  [n,h,w] fp32   = per-pixel confidence                 (:243-258) */
int ssal_enet_score_nhwc(ssal_enet *net, const float *x_dev, int n, int h, int w, int measure,
                         float threshold, double *scores_dev, uint8_t *label_dev, uint8_t *mask_dev,
                         float *conf_dev, void *ws_dev, int64_t ws_bytes, void *stream);

/* The same two entry points on the DECODED frame: x_dev [n,h,w,c_in] uint8.  The reference converts right after
 * decoding, `tf.image.convert_image_dtype(image, tf.float32)` = u8 * float32(1/255) (tensortools/input.py:289-290);
 * here the Initial block does that conversion on the fly: identical bits out, a quarter of the bytes over PCIe
 * and into the first kernel. */
int ssal_enet_forward_nhwc_u8(ssal_enet *net, const uint8_t *x_dev, int n, int h, int w,
                              float *logits_dev, void *ws_dev, int64_t ws_bytes, void *stream);
int ssal_enet_score_nhwc_u8(ssal_enet *net, const uint8_t *x_dev, int n, int h, int w, int measure,
                            float threshold, double *scores_dev, uint8_t *label_dev, uint8_t *mask_dev,
                            float *conf_dev, void *ws_dev, int64_t ws_bytes, void *stream);

/* forward / score with an explicit arithmetic mode (SSAL_ARITH_*); x_dev is float32 (x_is_u8 == 0) or the decoded uint8
 * frame (x_is_u8 != 0).  arithmetic == SSAL_ARITH_F32 is exactly ssal_enet_forward_nhwc / ssal_enet_score_nhwc (_u8).
 * Replaces the same reference code (models/enet/enet.py:320-407, active_learning.py:229-263). */
int ssal_enet_forward_nhwc_arith(ssal_enet *net, const void *x_dev, int x_is_u8, int n, int h, int w, int arithmetic,
                                 float *logits_dev, void *ws_dev, int64_t ws_bytes, void *stream);
int ssal_enet_score_nhwc_arith(ssal_enet *net, const void *x_dev, int x_is_u8, int n, int h, int w, int measure,
                               float threshold, int arithmetic, double *scores_dev, uint8_t *label_dev, uint8_t *mask_dev,
                               float *conf_dev, void *ws_dev, int64_t ws_bytes, void *stream);

/* Validation pass, fused: ENet.call(training=False) -> argmax -> masked confusion matrix, the val / test branch of the
 * reference loop (active_learning.py:277-282 val_net and val_pred = argmax(val_logits); tensortools.metrics.Metrics
 * :390-427 with its confusion update, tensortools/metrics.py:8-27,226-257).  The logits and the predicted labels never
 * reach HBM: the Final kernel reads labels_dev / mask_dev [n,h,w] uint8 (mask_dev NULL = weight 1) and ADDS
 * bincount(classes * label + argmax, weights = mask) into confusion_dev int64 [classes][classes] (row = label, column =
 * prediction; a key >= classes^2, e.g. label 255, is dropped), as the reference's assign_add does -- zero it first for a
 * per-batch matrix.  x_dev and arithmetic as in ssal_enet_score_nhwc_arith.  The workspace is
 * ssal_enet_eval_workspace_bytes (>= ssal_enet_workspace_bytes; the first part is laid out as a score call's). */
int64_t ssal_enet_eval_workspace_bytes(const ssal_enet *net, int n, int h, int w);
int ssal_enet_evaluate_nhwc_arith(ssal_enet *net, const void *x_dev, int x_is_u8, int n, int h, int w, int arithmetic,
                                  const uint8_t *labels_dev, const uint8_t *mask_dev, int64_t *confusion_dev,
                                  void *ws_dev, int64_t ws_bytes, void *stream);

/* Byte offsets into the workspace of the last forward/score call of the tensors behind
 * ENet.endpoint_outputs (models/enet/enet.py:311-318): offs[0] bottleneck5_1 [n,h/2,w/2,16],
 * offs[1] bottleneck4_2 [n,h/4,w/4,64], offs[2] bottleneck3_8 [n,h/8,w/8,128]. */
int ssal_enet_endpoint_offsets(const ssal_enet *net, int n, int h, int w, int64_t offs[3]);

/* The max-pooling indices ENet.call hands from Bottleneck1_0 / Bottleneck2_0 to Bottleneck5_0 / Bottleneck4_0
 * (models/enet/enet.py:331,338,359,364), of the LAST forward/score call that ran on this workspace, converted from
 * the internal 1-byte window codes to the reference's int64 per-image index (y*W + x)*C + c:
 * which = 1 -> argmax1 [n,h/4,w/4,16], which = 2 -> argmax2 [n,h/8,w/8,64]. */
int ssal_enet_export_argmax(const ssal_enet *net, const void *ws_dev, int64_t ws_bytes, int n, int h, int w,
                            int which, int64_t *argmax_out_dev, void *stream);

/* Run ONE layer of the handle (Layer.__call__ of enet_modules.py: Initial :190-224, Bottleneck
 * :526-599, BottleneckDownsample :868-938, BottleneckUpsample :1217-1292, Final :1359-1381).
 * x_dev [n,h,w,cin] -> y_dev (shape by layer kind).  argmax tensors use the reference's int64
 * per-image index (y*W + x)*C + c: argmax_out_dev is written by a Downsample
 * layer, argmax_in_dev is consumed by an Upsample layer; NULL otherwise. */
int ssal_enet_run_layer(ssal_enet *net, const char *layer, const float *x_dev, int n, int h, int w,
                        float *y_dev, int64_t *argmax_out_dev, const int64_t *argmax_in_dev,
                        void *ws_dev, int64_t ws_bytes, void *stream);
int64_t ssal_enet_layer_workspace_bytes(const ssal_enet *net, const char *layer, int n, int h, int w);
/* the same with an arithmetic mode (layers the mode has no kernel for run in exact fp32) */
int ssal_enet_run_layer_arith(ssal_enet *net, const char *layer, const float *x_dev, int n, int h, int w, int arithmetic,
                              float *y_dev, int64_t *argmax_out_dev, const int64_t *argmax_in_dev, void *ws_dev,
                              int64_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Stand-alone operators
 * ---------------------------------------------------------------------------------------------- */

/* softmax + measure + float64 mean on materialised logits (active_learning.py:239-263) */
int64_t ssal_score_workspace_bytes(int n, int h, int w);
int ssal_score_logits_nhwc(const float *logits_dev, int n, int h, int w, int classes, int measure,
                           float threshold, double *scores_dev, uint8_t *label_dev,
                           uint8_t *mask_dev, float *conf_dev, void *ws_dev, int64_t ws_bytes,
                           void *stream);

/* ------------------------------------------------------------------------------------------------
 * Region scores (region-level acquisition; no reference counterpart: the reference ranks whole frames,
 * active_learning.py:682-715 -- the per-pixel measures are the same ones, :239-263)
 *
 * A region is a window of rh x rw output pixels on a grid anchored at pixel (0, 0): RY = ceil(h / rh) by RX = ceil(w / rw)
 * regions, the bottom row / right column clipped by the frame.  region_scores [n][RY][RX] float64 = the mean of the per-pixel
 * confidence over the region's pixels inside the frame, accumulated in float64 in a fixed order (csrc/ssal_regions.h) that
 * does not know the batch size, the image-group chain a frame ran on or any ssal_debug_set_knob setting.  Region outputs
 * are caller-provided; rh <= 0 or rw <= 0 is SSAL_EINVAL.
 * ---------------------------------------------------------------------------------------------- */
#define SSAL_REGION_FORM_TILES 0 /* float64 sums of 32 x 32 pixel tiles [n][ceil(h / 32)][ceil(w / 32)], row-major */
#define SSAL_REGION_FORM_PLANE 1 /* fp32 per-pixel confidence [n][h][w] */

/* host only: the region grid of an h x w frame */
int ssal_region_grid(int h, int w, int rh, int rw, int *ry, int *rx);

/* ssal_enet_score_nhwc_arith plus region scores, fused: the Final + score kernel already leaves one float64 sum per
 * 32 x 32 output tile in the workspace; one more small launch folds them into regions (tiles of a region in row-major
 * order), so rh and rw must be multiples of 32 (anything else: SSAL_EINVAL; ssal_region_means_plane serves those sizes).
 * scores_dev and the optional label / mask / conf outputs keep their meaning, and the per-image score has the bits
 * ssal_enet_score_nhwc_arith gives; with none of the optional outputs the score-only fused form runs.  The workspace is
 * ssal_enet_workspace_bytes, as for the plain entry. */
int ssal_enet_score_regions_nhwc_arith(ssal_enet *net, const void *x_dev, int x_is_u8, int n, int h, int w, int measure,
                                       float threshold, int arithmetic, int rh, int rw, double *scores_dev,
                                       double *region_scores_dev, uint8_t *label_dev, uint8_t *mask_dev, float *conf_dev,
                                       void *ws_dev, int64_t ws_bytes, void *stream);

/* stand-alone: region means of a device plane [n][h][w] fp32; any rh, rw >= 1.  Reads the plane once (16-byte loads when
 * plane_dev is 16-byte aligned and w a multiple of 4; the result has the same bits either way).  Within a region: row
 * partials first, then rows top to bottom; no floating-point atomics. */
int ssal_region_means_plane(const float *plane_dev, int n, int h, int w, int rh, int rw, double *region_scores_dev,
                            void *stream);

/* region sibling of ssal_score_logits_nhwc (which is unchanged): the same outputs plus region_scores_dev, through the
 * confidence plane and ssal_region_means_plane.  conf_dev stays optional: without it the plane lives in the workspace,
 * which is why the workspace is ssal_score_regions_workspace_bytes here. */
int64_t ssal_score_regions_workspace_bytes(int n, int h, int w);
int ssal_score_logits_regions_nhwc(const float *logits_dev, int n, int h, int w, int classes, int measure, float threshold,
                                   int rh, int rw, double *scores_dev, double *region_scores_dev, uint8_t *label_dev,
                                   uint8_t *mask_dev, float *conf_dev, void *ws_dev, int64_t ws_bytes, void *stream);

/* host only: the reduction core of the two kernels run on the CPU (the same source, csrc/ssal_regions.h).  form:
 * SSAL_REGION_FORM_*; in_host: the tiles (float64) or the plane (fp32) of n frames; region_scores_host [n][RY][RX];
 * counts_host (nullable) int64 [RY][RX]: the clipped pixel count of every region.  The tile form needs rh, rw multiples
 * of 32. */
int ssal_region_reduce_host(int form, const void *in_host, int n, int h, int w, int rh, int rw, double *region_scores_host,
                            int64_t *counts_host);

/* tensortools.metrics.confusion_mat (tensortools/metrics.py:226-257) accumulated like Metrics' assign_add (:8-27):
 * confusion_dev int64 [classes][classes] += bincount(classes * labels + pred, weights, minlength = maxlength = classes^2)
 * over `pixels` uint8 elements of pred_dev / labels_dev / weights_dev (weights_dev NULL = weight 1; a weight is its full
 * uint8 value).  Keys >= classes^2 are dropped.  classes in [2, 32].  Integer counts: bitwise reproducible. */
int64_t ssal_confusion_workspace_bytes(int classes);
int ssal_confusion_matrix(const uint8_t *pred_dev, const uint8_t *labels_dev, const uint8_t *weights_dev, int64_t pixels,
                          int classes, int64_t *confusion_dev, void *ws_dev, int64_t ws_bytes, void *stream);

/* tensortools.losses.masked_softmax_cross_entropy forward (tensortools/losses.py:3-74): label
 * smoothing, optional ENet-style class weighting (weight > 1), fp32 sum over the batch axis, float64
 * over the spatial axes, divided by the (fp32) mask sum.  labels uint8 [n,h,w], mask fp32 [n,h,w],
 * loss_dev: one float64. */
int64_t ssal_xent_workspace_bytes(int h, int w);
int ssal_masked_softmax_cross_entropy(const float *logits_dev, const uint8_t *labels_dev,
                                      const float *mask_dev, int n, int h, int w, int classes,
                                      float weight, float label_smoothing, double *loss_dev,
                                      void *ws_dev, int64_t ws_bytes, void *stream);

/* tf.nn.max_pool_with_argmax(ksize 2x2, strides 2, SAME, Targmax=int64) (enet_modules.py:927-929);
 * include_batch selects the TF<=1.13 CPU index convention (extra_ops.py:63-81). */
int ssal_max_pool_with_argmax_2x2(const float *x_dev, int n, int h, int w, int c, float *y_dev,
                                  int64_t *argmax_dev, int include_batch, void *stream);
/* xops.unpool_2d(inputs, idx, strides=[1,2,2,1])  (models/util/extra_ops.py:28-86).  Indices must be unique per
 * output element (true of pooling-derived indices, the reference's only use): tf.scatter_nd sums duplicates, this
 * scatter assigns. */
int ssal_unpool_2d(const float *x_dev, const int64_t *idx_dev, int n, int h, int w, int c,
                   int idx_has_batch, float *y_dev, void *stream);
/* xops.prelu(x, alpha)  (models/util/extra_ops.py:9-26) */
int ssal_prelu(const float *x_dev, int64_t pixels, int c, const float *alpha_dev, float *y_dev,
               void *stream);
/* xops.spatial_dropout(inputs, drop_rate)  (models/util/extra_ops.py:137-151; called, training only, at
 * enet_modules.py:591-594): tf.nn.dropout with noise_shape [N,1,1,C]: y = (x / (1-rate)) * floor((1-rate) + u[n,c]),
 * one uniform draw per (image, channel) plane.  u is a counter-based hash of (seed, n*C + c) -- TensorFlow's random
 * stream is not reproducible, the distribution and the arithmetic are.  x_dev/y_dev [n, pixels_per_image, c]. */
int ssal_spatial_dropout(const float *x_dev, int n, int64_t pixels_per_image, int c, float rate, uint64_t seed,
                         float *y_dev, void *stream);
/* xops.batch_norm(..., training=False)  (models/util/extra_ops.py:154-185) */
int ssal_batch_norm_inference(const float *x_dev, int64_t pixels, int c, const float *mean_dev,
                              const float *var_dev, const float *gamma_dev, const float *beta_dev,
                              float *y_dev, void *stream);
/* tf.nn.conv2d(x, kernel HWIO, strides [1,s,s,1], dilations [1,d,d,1], "SAME")
 * (enet_modules.py:205,538,554,559,565,581,880,895,911,1236,1267,1285) */
int ssal_conv2d_same(const float *x_dev, int n, int h, int w, int cin, const float *kernel_dev,
                     int kh, int kw, int cout, int stride, int dilation, float *y_dev, void *stream);
/* tf.nn.conv2d_transpose(x, kernel [3,3,cout,cin], strides 2, "SAME") -> [n,2h,2w,cout]
 * (enet_modules.py:1251-1255, 1376-1380) */
int ssal_conv2d_transpose_3x3_s2(const float *x_dev, int n, int h, int w, int cin,
                                 const float *kernel_dev, int cout, float *y_dev, void *stream);
/* tf.image.resize_bilinear(x, [oh,ow]) with TF-1.13 defaults (align_corners=False, legacy
 * src = dst * in/out mapping)  (inference.py:96-99) */
int ssal_resize_bilinear(const float *x_dev, int n, int h, int w, int c, int oh, int ow,
                         float *y_dev, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Prediction (inference.py:95-109): what the test-split program writes per pixel, in one kernel.
 *
 * ssal_predict_logits_nhwc: logits_dev [n,h,w,classes] fp32 -> out_dev uint8.  Per output pixel the `classes` values of
 * tf.image.resize_bilinear(logits, [oh,ow]) (ssal_resize_bilinear's mapping and expression, the same bits) are formed in
 * registers and their first maximum is taken (the lowest class wins a tie, as the score entries do); the resized logits are
 * never stored and there is no workspace.  oh == h && ow == w is a plain argmax.
 *   lut_dev == NULL, lut_channels == 0: out_dev [n,oh,ow] = the train id
 *   lut_channels == 1: lut_dev = 256 bytes,      out_dev [n,oh,ow]   = lut[id]        (reverse embedding, :101-106)
 *   lut_channels == 3: lut_dev = 256 x 3 bytes,  out_dev [n,oh,ow,3] = lut[id][0..2]  (colour map, :107-109)
 * logits_dev needs 4-byte alignment only (16-byte loads are used when classes % 4 == 0 and it is 16-byte aligned; the
 * result does not depend on it).  SSAL_EINVAL, judged before any device work: a NULL pointer, classes outside [2,32], a
 * size <= 0, lut_channels outside {0,1,3} or at odds with lut_dev, and more output tiles (32 x 8 pixels) than one launch
 * takes (n * ceil(oh / 8) * ceil(ow / 32) >= 2^31).
 *
 * ssal_label_lut: the table alone on a label plane label_dev uint8 [pixels] (the plane the fused score entries give):
 * out_dev [pixels] or [pixels][3] as above; lut_channels == 0 copies.  Same statuses. */
int ssal_predict_logits_nhwc(const float *logits_dev, int n, int h, int w, int classes, int oh, int ow,
                             const uint8_t *lut_dev, int lut_channels, uint8_t *out_dev, void *stream);
int ssal_label_lut(const uint8_t *label_dev, int64_t pixels, const uint8_t *lut_dev, int lut_channels,
                   uint8_t *out_dev, void *stream);

/* Synthetic Cityscapes-shaped frames for benchmarking/tests: frame f of the pool is a
 * pure function of (seed, f); out_dev [count,h,w,c] fp32 = uint8 pixel * (1/255)
 * (tensortools/input.py:289-290 convert_image_dtype).  Host twin: synthetic.synth_frames_u8(). */
int ssal_synth_frames_nhwc(uint64_t seed, int64_t first_frame, int count, int h, int w, int c,
                           float *out_dev, void *stream);
/* the same frames before the conversion: out_dev [count,h,w,c] uint8 */
int ssal_synth_frames_nhwc_u8(uint64_t seed, int64_t first_frame, int count, int h, int w, int c,
                              uint8_t *out_dev, void *stream);

/* The switches below (ssal_set_kernel_family, ssal_debug_set_knob, ssal_debug_set_trace, ssal_profile_*) are
 * PROCESS-GLOBAL measurement aids, not part of the re-entrant per-handle / per-stream contract stated at the top of
 * this header: set them from one host thread while no other thread is inside the library.
 *
 * Kernel-family switch for A/B measurements and cross-checks (no reference counterpart):
 * 1 = MFMA-fused bottleneck kernels on the shapes they support (default), 0 = generic kernels
 * everywhere.  Both families produce bit-identical results. */
int ssal_set_kernel_family(int use_mfma);
/* hardware-assumption probe used by the tests (v_permlane32_swap / v_permlane16_swap lane
 * semantics): writes 256 floats */
int ssal_debug_probe(float *out_dev_256, void *stream);

/* tuning / A-B knob of the fused bottleneck launchers ("bnk_tw": 16 forces 8x16 tiles, "bnk_o4": the four-workgroups-per-CU
 * form of the regular 128-channel block -- 2 (default) where the phase sub-image is at most 16 pixels wide, 1 everywhere,
 * 0 never --, "bnk_w8": eight-wave workgroups on 8x32 tiles, two per CU, for the 128-channel blocks -- 2 (default) = the
 * regular block at dilations 1..8 and the asymmetric block, 1 = the regular block only, 0 = the four-wave kernels; images above 2^28 floats always run the four-wave kernels --,
 * "bnk_xcd": 0 switches the
 * XCD-aware tile order off, "img_groups": G runs the layers selected by "img_span" (default 4 = Initial .. Final + score) as G image
 * groups on G library-owned side streams, forked from / joined into the caller's stream with events -- default 2, 1 =
 * everything on the caller's stream; "ic_front": ICNet score path, bit 0 (default 1) = conv1_sub1 + conv2_sub1 as one launch,
 * bit 1 (default 0) = conv1_1_3x3_s2 + conv1_2_3x3 as one launch; "ic_dual": ICNet score path, 1 (default) = a block's projection
 * shortcut is evaluated inside its 1x1 increase launch; "conf_reps": replicas of the confusion accumulator the evaluation
 * pass and ssal_confusion_matrix add into, 1 .. 64, default 8).  Every setting produces bit-identical results
 * (tests/test_gpu_parity.py, tests/test_icnet_gpu.py); SSAL_EINVAL for
 * an unknown name.  The product build reads no environment variable and contains no work-skipping switch: phase
 * ablation ("ablate") and the SSAL_* environment defaults exist only in -DSSAL_MEASURE builds (tools/phase_trace.py),
 * whose ssal_version() says so. */
int ssal_debug_set_knob(const char *name, int value);
/* JSON object with the state of every switch that can change what a launch does or costs: kernel_family, bnk_tw, bnk_o4,
 * bnk_w8, bnk_xcd, img_groups, img_span, fuse_ends, img_lag, ig_div, ic_front, ic_dual, conf_reps, ablate, measure_build, profiling, defaults (1 iff all are at their shipping values).  bench.py prints it
 * in its result line and refuses to time anything else. */
int ssal_debug_get_knobs(char *json_out, int64_t cap);

/* Host-only query of the layer dispatch (no handle, no device; debug aid for tests): which kernel a layer of the given form
 * would launch on an h x w input (SSAL_LAYER_INITIAL: the h x w image, asking for the Initial + Bottleneck1_0 launch) under
 * the current kernel family and knobs.  kind: SSAL_LAYER_*; cin / cout / f: input, output and bottleneck-width channels;
 * asym: the asymmetric (5,1) + (1,5) block; arithmetic: SSAL_ARITH_*.  An upsample is asked for pooling-derived indices (the
 * window-code form every whole-network call uses).  Writes SSAL_DISPATCH_* to *kernel_out: the generic kernels, the fused fp32
 * kernel, or the fused kernel of the opt-in bf16x3 mode.  The fused kernels compute offsets inside one image in 32 bits; a
 * shape beyond a fused launcher's per-image limit is dispatched to the exact fp32 kernels instead. */
#define SSAL_LAYER_INITIAL 0
#define SSAL_LAYER_REGULAR 1
#define SSAL_LAYER_DOWN    2
#define SSAL_LAYER_UP      3
#define SSAL_DISPATCH_GENERIC       0
#define SSAL_DISPATCH_FUSED         1
#define SSAL_DISPATCH_FUSED_BF16X3  2
int ssal_debug_layer_dispatch(int kind, int cin, int cout, int f, int asym, int h, int w, int arithmetic, int *kernel_out);

/* measurement aid, only functional in a -DSSAL_PHASE_TRACE build (tools/phase_trace.py; SSAL_ENOTIMPL
 * otherwise): the fused bottleneck kernels write 16 x uint64 per wave (shader-clock phase marks,
 * 100 MHz realtime of first / last mark, HW_ID, XCC_ID) into buf_dev; NULL switches it off. */
int ssal_debug_set_trace(void *buf_dev, int64_t bytes);

/* Measurement aid (no reference counterpart): when enabled, every kernel launch is bracketed by
 * HIP events on its own stream; ssal_profile_collect() returns per-kernel launch counts, total
 * milliseconds and ALGORITHMIC flops / bytes as a JSON object.  Single host thread only. */
int ssal_profile_enable(int on);
int ssal_profile_collect(char *json_out, int64_t cap);

/* ---- PNG decode (no reference counterpart: tensortools/input.py decodes with tf.image.decode_image, :246-248) ----
 * A batch of zlib payloads (the concatenated IDAT data of 8-bit, non-interlaced PNGs of colour type 0, 2, 3 or 6) is
 * inflated, unfiltered and placed straight into NHWC batch tensors on the device.  Each stream is described by
 * SSAL_PNG_DESC int64 fields:
 *   [0] payload offset, [1] payload length (bytes, in payload_dev), [2] width, [3] height, [4] bytes per pixel (1, 3, 4),
 *   [5] workspace offset (filled by ssal_png_plan), [6] destination frame, [7] role (SSAL_PNG_ROLE_*),
 *   [8] destination channel offset and [9] channel count (image role: source channels [0, count) go to channels
 *   [offset, offset + count) of the batch), [10] crop top, [11] crop left, [12] left-right flip (0 / 1), [13..15] zero.
 * The image role writes image_dev (uint8, or float32 = u8 * float32(1/255) when image_f32) and, when image_dist_dev is
 * given, clip(image * scale_dev[frame][channel], 0, 1) (float32); the label role writes channel 0 through generate_mask
 * (tensortools/input.py:17-31): label_dev = value, 0 where value == 255; mask_dev = value != 255.  All outputs are
 * [frames][height][width]([channels]) with the batch's height x width the crop window.
 * status_dev int32 [n_streams] receives one SSAL_PNG_* word per stream; a stream that is not SSAL_PNG_OK writes nothing to
 * the outputs.  Every read stays inside the stream's payload extent and every write inside its workspace slot and its
 * destination planes, whatever the payload bytes hold (descriptors out of range give SSAL_PNG_UNSUPPORTED). */
#define SSAL_PNG_DESC 16
#define SSAL_PNG_ROLE_IMAGE 0
#define SSAL_PNG_ROLE_LABEL 1
#define SSAL_PNG_OK 0
#define SSAL_PNG_TRUNCATED 1     /* the input ends before the final block or the Adler-32 trailer */
#define SSAL_PNG_BAD_CODES 2     /* invalid block type, stored length, code-length set or symbol */
#define SSAL_PNG_BAD_DISTANCE 3  /* a match reaches before the start of the output */
#define SSAL_PNG_SIZE 4          /* the output is longer (or shorter) than height * (1 + width * bpp) */
#define SSAL_PNG_ADLER 5         /* Adler-32 mismatch */
#define SSAL_PNG_BAD_FILTER 6    /* a scanline filter type > 4 */
#define SSAL_PNG_UNSUPPORTED 7   /* zlib header CM != 8 / FDICT = 1 / bad check bits, or a descriptor out of range */
/* assigns every stream its workspace slot (field [5]) and returns the workspace size in bytes; -1 on a bad descriptor */
int64_t ssal_png_plan(int64_t n_streams, int64_t *desc_host);
int ssal_png_decode_nhwc(const uint8_t *payload_dev, int64_t payload_bytes, const int64_t *desc_dev, int64_t n_streams,
                         int frames, int height, int width, int channels, const float *scale_dev, void *image_dev,
                         int image_f32, float *image_dist_dev, uint8_t *label_dev, uint8_t *mask_dev, int32_t *status_dev,
                         void *ws_dev, int64_t ws_bytes, void *stream);
/* the same inflate / unfilter source on the host, single-threaded (tests): a zlib stream into out[0, out_cap)
 * (*out_len = bytes produced), and an in-place unfilter of height rows of (1 filter byte + width * bpp); *status as above */
int ssal_inflate_host(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_cap, int64_t *out_len, int32_t *status);
int ssal_png_unfilter_host(uint8_t *raw, int height, int width, int bpp, int32_t *status);

/* ---- Output-layer training (active_learning.py:283-326 with -r/--reinitialize-output-layer, :905-909, 461-462) ----
 * The gradient of tensortools.losses.masked_softmax_cross_entropy (tensortools/losses.py:3-74, the semantics of
 * ssal_masked_softmax_cross_entropy) with respect to Final.kernel (enet_modules.py:1294-1381), and the TF-1.13
 * AdamOptimizer update that train_op = optimizer.minimize(cost) (active_learning.py:321-324) applies to it.  The trunk is
 * frozen and evaluated with training=False.
 *
 * ssal_final_grad_nhwc: features_dev [n,h,w,16] fp32 (Bottleneck5_1's output, ENet.endpoint_outputs), kernel_dev
 * [3][3][classes][16] (TF HW-O-I), labels_dev uint8 / mask_dev fp32 [n,2h,2w].  Writes loss_dev (one float64: the loss
 * the forward op gives, up to the order of its float64 sums) and grad_dev [3][3][classes][16] fp32 = d loss / d kernel
 * (TensorFlow's gradient: softmax - one_hot for the cross entropy, the derivative of the class weight through p_class when
 * weight > 1).  The logits never reach HBM; there are no float atomics (two calls give the same bits).  SSAL_EINVAL for
 * classes outside [2, 32], bad sizes, or h x w beyond the kernel's limit (2h + 1, 2w + 1 and the count of 16 x 16 tiles
 * must fit an int); ssal_final_grad_workspace_bytes then returns -1. */
int64_t ssal_final_grad_workspace_bytes(int n, int h, int w, int classes);
int ssal_final_grad_nhwc(const float *features_dev, int n, int h, int w, int classes, const float *kernel_dev,
                         const uint8_t *labels_dev, const float *mask_dev, float weight, float label_smoothing,
                         double *loss_dev, float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream);
/* The same from images x_dev [n,h,w,c_in] (fp32, or uint8 with x_is_u8): the committed trunk's launchers up to
 * Bottleneck5_1, then the gradient kernel on its output; labels_dev / mask_dev [n,h,w]; kernel_dev as above (the kernel
 * being trained: the handle's own Final weights are not used).  The workspace holds the forward workspace and the
 * gradient's partials. */
int64_t ssal_enet_train_final_workspace_bytes(const ssal_enet *net, int n, int h, int w);
int ssal_enet_train_final_nhwc(ssal_enet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                               const uint8_t *labels_dev, const float *mask_dev, const float *kernel_dev, float weight,
                               float label_smoothing, double *loss_dev, float *grad_dev, void *ws_dev, int64_t ws_bytes,
                               void *stream);
/* ---- The semi-supervised step and the training metrics (active_learning.py:226-275, 339-342) ----
 * The same gradient with the batch's targets built inside the kernel: labelled_dev uint8 [n], 1 = image i is trained on
 * the caller's labels_dev / mask_dev planes, 0 = on its own pseudo annotation (:229-275): pseudo_label = the first maximum
 * of the pixel's Final logits, pseudo_mask = confidence < threshold ? 0 : 1 with the confidence of `measure`
 * (SSAL_MEASURE_*), the arithmetic of ssal_enet_score_nhwc (a NaN confidence gives 1, as tf.math.less does).  The pseudo
 * logits are those of features_raw_dev [n,h,w,16] (Bottleneck5_1 of the undistorted frame, :231) under kernel_dev, or of
 * features_dev itself when features_raw_dev is NULL.  No gradient flows through the pseudo annotation (tf.stop_gradient,
 * :233).  labelled_dev NULL = every image labelled.  The label / mask planes of an unlabelled image are never read, and
 * labels_dev / mask_dev may be NULL when labelled_dev marks NO image as labelled -- which the library cannot verify: it is
 * the caller's contract.
 * Optional outputs (NULL to skip): confusion_dev int64 [classes][classes], the training-pass metrics of :339-342 --
 * confusion[label][argmax of the TRAINING logits] += (int)mask over every pixel of the batch (the targets actually trained
 * on; the matrix is accumulated, not overwritten, like ssal_enet_evaluate_nhwc_arith; the mask must satisfy 0 <= mask < 256
 * and is truncated like tf.cast(mask, int32); a key >= classes^2 is dropped) -- and pseudo_pixels_dev int64 [n] = the
 * count of pixels of image i whose pseudo mask is 1 (0 for a labelled image; overwritten).
 * loss_dev / grad_dev hold exactly what ssal_final_grad_nhwc gives for the composed targets; integer counts, no float
 * atomics: two calls give the same bits.  Statuses as ssal_final_grad_nhwc, plus SSAL_ENOTIMPL for an unknown measure and
 * SSAL_ENOMEM for a short workspace. */
int64_t ssal_final_grad_semi_workspace_bytes(int n, int h, int w, int classes);
int ssal_final_grad_semi_nhwc(const float *features_dev, const float *features_raw_dev, int n, int h, int w, int classes,
                              const float *kernel_dev, const uint8_t *labels_dev, const float *mask_dev,
                              const uint8_t *labelled_dev, int measure, float threshold, float weight, float label_smoothing,
                              double *loss_dev, float *grad_dev, int64_t *confusion_dev, int64_t *pseudo_pixels_dev,
                              void *ws_dev, int64_t ws_bytes, void *stream);
/* The same from images: the committed trunk up to Bottleneck5_1 on x_raw_dev first when it is given (its features stay in
 * a second slot of the workspace: with_raw = 1 in the size query), then on x_dev, then the kernel.  x_raw_dev has the shape
 * and element type of x_dev. */
int64_t ssal_enet_train_final_semi_workspace_bytes(const ssal_enet *net, int n, int h, int w, int with_raw);
int ssal_enet_train_final_semi_nhwc(ssal_enet *net, const void *x_dev, const void *x_raw_dev, int x_is_u8, int n, int h,
                                    int w, const uint8_t *labels_dev, const float *mask_dev, const uint8_t *labelled_dev,
                                    int measure, float threshold, const float *kernel_dev, float weight,
                                    float label_smoothing, double *loss_dev, float *grad_dev, int64_t *confusion_dev,
                                    int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes, void *stream);
/* Keras l1_l2(l1, l2) regulariser gradient (2 l2 w + l1 sign(w), sign(0) = 0) and TF-1.13 ApplyAdam, in place on count
 * elements of var / m / v (fp32): alpha = lr sqrt(1 - beta2_power) / (1 - beta1_power); m += (g - m)(1 - beta1);
 * v += (g^2 - v)(1 - beta2); var -= (m alpha) / (sqrt(v) + eps).  sqrt and the divisions are correctly rounded.  The
 * caller keeps the fp32 beta powers (multiplied by beta1 / beta2 after each step) and the learning rate schedule. */
int ssal_adam_apply(float *var_dev, float *m_dev, float *v_dev, const float *grad_dev, int64_t count, float lr,
                    float beta1, float beta2, float eps, float beta1_power, float beta2_power, float l1, float l2,
                    void *stream);

/* ---- Last-block training: Bottleneck5_1 + Final (enet_modules.py:526-599, 1294-1381) ----
 * The gradient of masked_softmax_cross_entropy through Final's transposed convolution and through Bottleneck5_1 in
 * inference mode: the moving means / variances are constants, there is no dropout, batch-norm is the affine map
 * y = gamma (x - mean) / sqrt(variance + 1e-3) + beta with gamma and beta trainable.  Everything below Bottleneck5_1 is
 * frozen.  PReLU is relu(x) - alpha relu(-x); at x == 0 both derivatives are 0 (TensorFlow's ReluGrad).
 *
 * The 13 trained variables (Final.kernel and the 12 of Bottleneck5_1), the six moving statistics and Final.kernel travel in ONE packed fp32 block of
 * ssal_train_block_param_floats(classes) = 400 + 144 classes floats (offsets in floats, C order inside each tensor):
 *      0  proj_kernel [16][4]        64  proj_gamma [4]      68  proj_beta [4]      72  proj_alpha [4]
 *     76  conv_kernel [3][3][4][4]  220  conv_gamma [4]     224  conv_beta [4]     228  conv_alpha [4]
 *    232  exp_kernel [4][16]        296  exp_gamma [16]     312  exp_beta [16]     328  residual_alpha [16]
 *    344  proj_mean [4]             348  proj_variance [4]  352  conv_mean [4]     356  conv_variance [4]
 *    360  exp_mean [16]             376  exp_variance [16]  392  8 floats of padding
 *    400  Final.kernel [3][3][classes][16] (TF HW-O-I)
 * grad_dev has the same layout (0 in [344, 400)), so Adam's slots can too: ssal_adam_apply runs on sub-ranges of it.
 *
 * ssal_train_block_grad_nhwc: features_dev [n,h,w,16] fp32 = Bottleneck5_0's output, labels_dev uint8 / mask_dev fp32
 * [n,2h,2w].  Writes loss_dev (one float64; the per-pixel terms are those of the forward op on ssal_enet_forward_nhwc's
 * logits) and grad_dev.  The logits and their gradient never reach HBM; dL/d(Bottleneck5_1 output) [n,h,w,16] passes
 * through the workspace once.  No float atomics: two calls give the same bits.  Limits and statuses as
 * ssal_final_grad_nhwc (the workspace query returns -1 at the same boundaries). */
int64_t ssal_train_block_param_floats(int classes);
int64_t ssal_train_block_grad_workspace_bytes(int n, int h, int w, int classes);
int ssal_train_block_grad_nhwc(const float *features_dev, int n, int h, int w, int classes, const float *params_dev,
                               const uint8_t *labels_dev, const float *mask_dev, float weight, float label_smoothing,
                               double *loss_dev, float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream);
/* The same from images x_dev [n,h,w,c_in] (fp32, or uint8 with x_is_u8): the committed trunk's launchers up to
 * Bottleneck5_0 on the caller's stream, then the training kernels on its output with params_dev (the handle's own
 * Bottleneck5_1 / Final weights are not used); labels_dev / mask_dev [n,h,w]. */
int64_t ssal_enet_train_block_workspace_bytes(const ssal_enet *net, int n, int h, int w);
int ssal_enet_train_block_nhwc(ssal_enet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                               const uint8_t *labels_dev, const float *mask_dev, const float *params_dev, float weight,
                               float label_smoothing, double *loss_dev, float *grad_dev, void *ws_dev, int64_t ws_bytes,
                               void *stream);
/* Byte offset, into the workspace of ssal_enet_forward_nhwc / ssal_enet_score_nhwc / ssal_enet_train_block_nhwc, of
 * Bottleneck5_0's output [n,h/2,w/2,16] (the features_dev of ssal_train_block_grad_nhwc); valid until the next call.
 * -1 for dims the net does not take. */
int64_t ssal_enet_train_block_features_offset(const ssal_enet *net, int n, int h, int w);

/* ---- Last-stage training: Bottleneck5_0 + Bottleneck5_1 + Final (enet_modules.py:940-1292) ----
 * The same gradient one block further down: through Bottleneck5_0, the last upsampling stage (1x1 projection 64 -> 16, 3x3
 * stride-2 transposed convolution 16 -> 8, 1x1 expansion 8 -> 16, 1x1 residual convolution 64 -> 16 + max-unpool), in
 * inference mode as above.  Everything below Bottleneck5_0 is frozen; no gradient is produced for its input.  The unpool's
 * backward is the gather of the gradient at the position each pooling index names.
 *
 * The 26 trained variables and the 12 moving statistics travel in ONE packed fp32 block of
 * ssal_train_stage_param_floats(classes) = ssal_train_block_param_floats(classes) + 3536 floats: the last-block block above,
 * unchanged, then Bottleneck5_0's part at float offset S = 400 + 144 classes (offsets from S, C order inside each tensor):
 *      0  proj_kernel [64][16]     1024  proj_gamma [16]    1040  proj_beta [16]    1056  proj_alpha [16]
 *   1072  conv_kernel [3][3][8][16] (TF HW-O-I)             2224  conv_gamma [8]    2232  conv_beta [8]    2240  conv_alpha [8]
 *   2248  exp_kernel [8][16]       2376  exp_gamma [16]     2392  exp_beta [16]
 *   2408  res_kernel [64][16]      3432  residual_alpha [16]
 *   3448  proj_mean [16]           3464  proj_variance [16] 3480  conv_mean [8]     3488  conv_variance [8]
 *   3496  exp_mean [16]            3512  exp_variance [16]  3528  8 floats of padding
 * grad_dev has the same layout (0 in the statistics and padding), so Adam's slots can too.
 *
 * ssal_train_stage_grad_nhwc: features_dev [n,h,w,64] fp32 = Bottleneck4_2's output; argmax_dev int64 [n,h,w,16] = the
 * pooling indices of Bottleneck1_0 in the reference's per-image form (y * 2w + x) * 16 + c, converted to window codes on the
 * device (an index outside its own 2x2 window and channel is taken as the window's first position: callers validate);
 * labels_dev uint8 / mask_dev fp32 [n,4h,4w].  Bottleneck5_0's output is computed by the forward path's own kernel from
 * weights folded on the device as ssal_enet_commit folds them, so loss_dev is the forward op's value on
 * ssal_enet_forward_nhwc's logits.  max_workgroups: 0 = the default, min(16x16 tiles of the [2h,2w] map, 1024); a smaller
 * positive value lowers the workgroup count of every gradient kernel (a tuning knob; the summation order, not the
 * semantics, depends on it).  No float atomics: two calls give the same bits.  The workspace query returns -1, and the
 * call SSAL_EINVAL, for classes outside [2,32] and beyond the limits of ssal_final_grad_nhwc on [2h,2w] and of the fused
 * Bottleneck5_0 kernel (64 h w < 2^31). */
int64_t ssal_train_stage_param_floats(int classes);
int64_t ssal_train_stage_grad_workspace_bytes(int n, int h, int w, int classes);
int ssal_train_stage_grad_nhwc(const float *features_dev, const int64_t *argmax_dev, int n, int h, int w, int classes,
                               const float *params_dev, const uint8_t *labels_dev, const float *mask_dev, float weight,
                               float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev,
                               int64_t ws_bytes, void *stream);
/* The same from images x_dev [n,h,w,c_in] (fp32, or uint8 with x_is_u8): the committed trunk's launchers up to
 * Bottleneck4_2 on the caller's stream, then the stage with params_dev (the handle's own Bottleneck5_0 / Bottleneck5_1 /
 * Final weights are not used) and the window codes the trunk's pooling left; labels_dev / mask_dev [n,h,w]. */
int64_t ssal_enet_train_stage_workspace_bytes(const ssal_enet *net, int n, int h, int w);
int ssal_enet_train_stage_nhwc(ssal_enet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                               const uint8_t *labels_dev, const float *mask_dev, const float *params_dev, float weight,
                               float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev,
                               int64_t ws_bytes, void *stream);
/* Byte offsets, into the workspace of ssal_enet_forward_nhwc / ssal_enet_score_nhwc / ssal_enet_train_stage_nhwc, of
 * Bottleneck4_2's output [n,h/4,w/4,64] (the features_dev of ssal_train_stage_grad_nhwc) and of the 1-byte window codes
 * [n,h/4,w/4,16] of Bottleneck1_0's pooling (ssal_enet_export_argmax(which = 1) turns them into argmax_dev); valid until the
 * next call.  -1 for dims the net does not take. */
int64_t ssal_enet_train_stage_features_offset(const ssal_enet *net, int n, int h, int w);
int64_t ssal_enet_train_stage_code_offset(const ssal_enet *net, int n, int h, int w);

/* ---- The semi-supervised step of the deeper trainers (active_learning.py:226-275, 339-342) ----
 * ssal_train_block_grad_nhwc / ssal_train_stage_grad_nhwc and their image forms with the batch's targets built inside the
 * head kernel.  labelled_dev, measure, threshold, confusion_dev and pseudo_pixels_dev mean exactly what they mean for
 * ssal_final_grad_semi_nhwc above (labelled_dev NULL = every image labelled; labels_dev / mask_dev may be NULL only when
 * labelled_dev marks no image as labelled, the caller's contract; the planes of an unlabelled image are never read; the
 * confusion matrix is accumulated; pseudo_pixels_dev is overwritten and 0 for a labelled image).  The pseudo logits are
 * those of the logits the kernel trains on, under params_dev, or -- features_raw_dev / x_raw_dev given -- those of the
 * undistorted frames: a target-only launch of the same kernel writes one byte per output pixel (label | mask << 7) into
 * the workspace first (with_raw = 1 in the size query), which the training launch reads.  The stage's raw side brings its
 * own pooling indices argmax_raw_dev (given together with features_raw_dev or not at all).  loss_dev / grad_dev hold
 * exactly what the plain entry gives for the composed targets, bit for bit; integer counts, no float atomics.  Limits
 * and statuses as the plain entries (the queries return -1 at the same boundaries), plus SSAL_ENOTIMPL for an unknown
 * measure; every argument is judged before any device work. */
int64_t ssal_train_block_grad_semi_workspace_bytes(int n, int h, int w, int classes, int with_raw);
int ssal_train_block_grad_semi_nhwc(const float *features_dev, const float *features_raw_dev, int n, int h, int w,
                                    int classes, const float *params_dev, const uint8_t *labels_dev, const float *mask_dev,
                                    const uint8_t *labelled_dev, int measure, float threshold, float weight,
                                    float label_smoothing, double *loss_dev, float *grad_dev, int64_t *confusion_dev,
                                    int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes, void *stream);
int64_t ssal_enet_train_block_semi_workspace_bytes(const ssal_enet *net, int n, int h, int w, int with_raw);
int ssal_enet_train_block_semi_nhwc(ssal_enet *net, const void *x_dev, const void *x_raw_dev, int x_is_u8, int n, int h,
                                    int w, const uint8_t *labels_dev, const float *mask_dev, const uint8_t *labelled_dev,
                                    int measure, float threshold, const float *params_dev, float weight,
                                    float label_smoothing, double *loss_dev, float *grad_dev, int64_t *confusion_dev,
                                    int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes, void *stream);
int64_t ssal_train_stage_grad_semi_workspace_bytes(int n, int h, int w, int classes, int with_raw);
int ssal_train_stage_grad_semi_nhwc(const float *features_dev, const int64_t *argmax_dev, const float *features_raw_dev,
                                    const int64_t *argmax_raw_dev, int n, int h, int w, int classes,
                                    const float *params_dev, const uint8_t *labels_dev, const float *mask_dev,
                                    const uint8_t *labelled_dev, int measure, float threshold, float weight,
                                    float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev,
                                    int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes,
                                    void *stream);
int64_t ssal_enet_train_stage_semi_workspace_bytes(const ssal_enet *net, int n, int h, int w, int with_raw);
int ssal_enet_train_stage_semi_nhwc(ssal_enet *net, const void *x_dev, const void *x_raw_dev, int x_is_u8, int n, int h,
                                    int w, const uint8_t *labels_dev, const float *mask_dev, const uint8_t *labelled_dev,
                                    int measure, float threshold, const float *params_dev, float weight,
                                    float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev,
                                    int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes,
                                    void *stream);

/* ---- Decoder-tail training: Bottleneck4_2 + Bottleneck5_0 + Bottleneck5_1 + Final (enet_modules.py:526-599; DESIGN.md
 * section 20) ----
 * The same gradient one block further down: through Bottleneck4_2, a regular 64-channel bottleneck (1x1 projection 64 -> 16,
 * 3x3 convolution 16 -> 16, 1x1 expansion 16 -> 64, identity residual), in inference mode as above.  Everything below
 * Bottleneck4_2 is frozen; no gradient is produced for its input.
 *
 * The 39 trained variables and the 18 moving statistics travel in ONE packed fp32 block of
 * ssal_train_tail_param_floats(classes) = ssal_train_stage_param_floats(classes) + 4840 floats: the stage block above,
 * unchanged, then Bottleneck4_2's part at float offset T = 3936 + 144 classes (offsets from T, C order inside each tensor):
 *      0  proj_kernel [64][16]     1024  proj_gamma [16]    1040  proj_beta [16]    1056  proj_alpha [16]
 *   1072  conv_kernel [3][3][16][16] (HWIO)                 3376  conv_gamma [16]   3392  conv_beta [16]   3408  conv_alpha [16]
 *   3424  exp_kernel [16][64]      4448  exp_gamma [64]     4512  exp_beta [64]     4576  residual_alpha [64]
 *   4640  proj_mean [16]           4656  proj_variance [16] 4672  conv_mean [16]    4688  conv_variance [16]
 *   4704  exp_mean [64]            4768  exp_variance [64]  4832  8 floats of padding
 * grad_dev has the same layout (0 in the statistics and padding), so Adam's slots can too.
 *
 * ssal_train_tail_grad_nhwc: features_dev [n,h,w,64] fp32 = Bottleneck4_1's output; argmax_dev, labels_dev, mask_dev and
 * max_workgroups as for ssal_train_stage_grad_nhwc.  Bottleneck4_2's output is computed by the forward path's own kernel from
 * weights folded on the device as ssal_enet_commit folds them, then the stage runs on it, so loss_dev is the forward op's
 * value on ssal_enet_forward_nhwc's logits.  No float atomics: two calls give the same bits.  The workspace query returns
 * -1, and the call SSAL_EINVAL, wherever the stage entries do, and beyond the limit of the fused 64-channel bottleneck
 * kernel the forward runs on (64 h w <= 2^29). */
int64_t ssal_train_tail_param_floats(int classes);
int64_t ssal_train_tail_grad_workspace_bytes(int n, int h, int w, int classes);
int ssal_train_tail_grad_nhwc(const float *features_dev, const int64_t *argmax_dev, int n, int h, int w, int classes,
                              const float *params_dev, const uint8_t *labels_dev, const float *mask_dev, float weight,
                              float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev,
                              int64_t ws_bytes, void *stream);
/* The same from images x_dev [n,h,w,c_in] (fp32, or uint8 with x_is_u8): the committed trunk's launchers up to
 * Bottleneck4_1 on the caller's stream, then the tail with params_dev (the handle's own Bottleneck4_2 / Bottleneck5_0 /
 * Bottleneck5_1 / Final weights are not used) and the window codes the trunk's pooling left; labels_dev / mask_dev [n,h,w]. */
int64_t ssal_enet_train_tail_workspace_bytes(const ssal_enet *net, int n, int h, int w);
int ssal_enet_train_tail_nhwc(ssal_enet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                              const uint8_t *labels_dev, const float *mask_dev, const float *params_dev, float weight,
                              float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev,
                              int64_t ws_bytes, void *stream);
/* Byte offset, into the workspace of ssal_enet_forward_nhwc / ssal_enet_score_nhwc / ssal_enet_train_tail_nhwc, of
 * Bottleneck4_1's output [n,h/4,w/4,64] (the features_dev of ssal_train_tail_grad_nhwc); valid until the next call.  The
 * window codes are at ssal_enet_train_stage_code_offset.  -1 for dims the net does not take. */
int64_t ssal_enet_train_tail_features_offset(const ssal_enet *net, int n, int h, int w);
/* The semi-supervised forms: arguments, meaning, limits and statuses of ssal_train_stage_grad_semi_nhwc /
 * ssal_enet_train_stage_semi_nhwc above, one block lower (features_raw_dev = Bottleneck4_1 of the undistorted frames). */
int64_t ssal_train_tail_grad_semi_workspace_bytes(int n, int h, int w, int classes, int with_raw);
int ssal_train_tail_grad_semi_nhwc(const float *features_dev, const int64_t *argmax_dev, const float *features_raw_dev,
                                   const int64_t *argmax_raw_dev, int n, int h, int w, int classes,
                                   const float *params_dev, const uint8_t *labels_dev, const float *mask_dev,
                                   const uint8_t *labelled_dev, int measure, float threshold, float weight,
                                   float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev,
                                   int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes,
                                   void *stream);
int64_t ssal_enet_train_tail_semi_workspace_bytes(const ssal_enet *net, int n, int h, int w, int with_raw);
int ssal_enet_train_tail_semi_nhwc(ssal_enet *net, const void *x_dev, const void *x_raw_dev, int x_is_u8, int n, int h,
                                   int w, const uint8_t *labels_dev, const float *mask_dev, const uint8_t *labelled_dev,
                                   int measure, float threshold, const float *params_dev, float weight,
                                   float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev,
                                   int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes,
                                   void *stream);

/* ---- Decoder-tail training, two regular blocks: Bottleneck4_1 + the tail above (enet_modules.py:526-599; DESIGN.md section
 * 21) ----
 * The same gradient one more block down: Bottleneck4_2's backward also produces its input gradient, and Bottleneck4_1, a
 * regular 64-channel bottleneck like it, is trained by a second launch of the same kernel.  Everything below Bottleneck4_1 is
 * frozen; no gradient is produced for its input.
 *
 * The 50 trained variables and the 24 moving statistics travel in ONE packed fp32 block of
 * ssal_train_tail2_param_floats(classes) = ssal_train_tail_param_floats(classes) + 4840 floats: the tail block above,
 * unchanged, then Bottleneck4_1's part at float offset T2 = 3936 + 144 classes + 4840, laid out as Bottleneck4_2's part is
 * (the offsets listed there, from T2).  grad_dev has the same layout.
 *
 * The ten entries mirror the tail's one for one: argument order, meaning, statuses, the order of the checks, the -1 /
 * SSAL_EINVAL limits (h, w are the dims of Bottleneck4_0's output; Bottleneck4_1's and Bottleneck4_2's have the same) and
 * "every argument is judged before any device work" are theirs.  features_dev / features_raw_dev [n,h,w,64] = Bottleneck4_0's
 * output; both regular blocks run forward through the forward path's own kernel from weights folded on the device, so
 * loss_dev is the forward op's value on ssal_enet_forward_nhwc's logits.  No float atomics: two calls give the same bits. */
int64_t ssal_train_tail2_param_floats(int classes);
int64_t ssal_train_tail2_grad_workspace_bytes(int n, int h, int w, int classes);
int ssal_train_tail2_grad_nhwc(const float *features_dev, const int64_t *argmax_dev, int n, int h, int w, int classes,
                               const float *params_dev, const uint8_t *labels_dev, const float *mask_dev, float weight,
                               float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev,
                               int64_t ws_bytes, void *stream);
/* From images: the committed trunk's launchers up to Bottleneck4_0, then the chain with params_dev. */
int64_t ssal_enet_train_tail2_workspace_bytes(const ssal_enet *net, int n, int h, int w);
int ssal_enet_train_tail2_nhwc(ssal_enet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                               const uint8_t *labels_dev, const float *mask_dev, const float *params_dev, float weight,
                               float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev,
                               int64_t ws_bytes, void *stream);
/* Byte offset, into the workspace of ssal_enet_train_tail2_nhwc / ssal_enet_train_tail2_semi_nhwc, of Bottleneck4_0's output
 * [n,h/4,w/4,64] (the features_dev of ssal_train_tail2_grad_nhwc) as those calls leave it; valid until the next call.  (A
 * forward or score call writes Bottleneck4_2's output to the same place.)  -1 for dims the net does not take. */
int64_t ssal_enet_train_tail2_features_offset(const ssal_enet *net, int n, int h, int w);
int64_t ssal_train_tail2_grad_semi_workspace_bytes(int n, int h, int w, int classes, int with_raw);
int ssal_train_tail2_grad_semi_nhwc(const float *features_dev, const int64_t *argmax_dev, const float *features_raw_dev,
                                    const int64_t *argmax_raw_dev, int n, int h, int w, int classes,
                                    const float *params_dev, const uint8_t *labels_dev, const float *mask_dev,
                                    const uint8_t *labelled_dev, int measure, float threshold, float weight,
                                    float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev,
                                    int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes,
                                    void *stream);
int64_t ssal_enet_train_tail2_semi_workspace_bytes(const ssal_enet *net, int n, int h, int w, int with_raw);
int ssal_enet_train_tail2_semi_nhwc(ssal_enet *net, const void *x_dev, const void *x_raw_dev, int x_is_u8, int n, int h,
                                    int w, const uint8_t *labels_dev, const float *mask_dev, const uint8_t *labelled_dev,
                                    int measure, float threshold, const float *params_dev, float weight,
                                    float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev,
                                    int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes,
                                    void *stream);

/* ---- Decoder training: Bottleneck4_0 + the two-block tail above (enet_modules.py:1217-1292) ----
 * The same gradient one more block down, through the 128 -> 64 upsampling block that opens the decoder: the trained part is
 * exactly ENet's decoder over a frozen encoder.  No gradient is produced for Bottleneck3_8's output.
 *
 * The 63 trained variables and the 30 moving statistics travel in ONE packed fp32 block of
 * ssal_train_decoder_param_floats(classes) = ssal_train_tail2_param_floats(classes) + 18488 floats: the two-block tail block
 * above, unchanged, then Bottleneck4_0's part at float offset T4 = 3936 + 144 classes + 2 * 4840, laid out in the order of
 * Bottleneck5_0's part with this block's sizes (offsets from T4): proj_kernel [128][32] 0, proj_gamma / proj_beta /
 * proj_alpha [32] 4096 / 4128 / 4160, conv_kernel [3][3][16][32] (HW-O-I) 4192, conv_gamma / conv_beta / conv_alpha [16]
 * 8800 / 8816 / 8832, exp_kernel [16][64] 8848, exp_gamma / exp_beta [64] 9872 / 9936, res_kernel [128][64] 10000,
 * residual_alpha [64] 18192; trained floats [0, 18256); proj_mean / proj_variance [32] 18256 / 18288, conv_mean /
 * conv_variance [16] 18320 / 18336, exp_mean / exp_variance [64] 18352 / 18416; 8 floats of padding.  grad_dev has the same
 * layout.
 *
 * The ten entries mirror the tail2 ones one for one: argument order, meaning, statuses, the order of the checks, the -1 /
 * SSAL_EINVAL limits and "every argument is judged before any device work" are theirs.  h, w of the features entries are the
 * dims of Bottleneck3_8's output (eighth resolution).  features_dev / features_raw_dev [n,h,w,128] = Bottleneck3_8's output;
 * argmax2_dev [n,h,w,64] = Bottleneck2_0's pooling indices (per-image index into [2h,2w,64]); argmax1_dev [n,2h,2w,16] =
 * Bottleneck1_0's, as the tail takes them.  Bottleneck4_0 runs forward through the forward path's own kernel from weights
 * folded on the device, so loss_dev is the forward op's value on ssal_enet_forward_nhwc's logits.  No float atomics: two calls
 * give the same bits. */
int64_t ssal_train_decoder_param_floats(int classes);
int64_t ssal_train_decoder_grad_workspace_bytes(int n, int h, int w, int classes);
int ssal_train_decoder_grad_nhwc(const float *features_dev, const int64_t *argmax2_dev, const int64_t *argmax1_dev, int n, int h,
                                 int w, int classes, const float *params_dev, const uint8_t *labels_dev, const float *mask_dev,
                                 float weight, float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev,
                                 void *ws_dev, int64_t ws_bytes, void *stream);
/* From images: the committed trunk's launchers up to Bottleneck3_8, then the chain with params_dev. */
int64_t ssal_enet_train_decoder_workspace_bytes(const ssal_enet *net, int n, int h, int w);
int ssal_enet_train_decoder_nhwc(ssal_enet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                                 const uint8_t *labels_dev, const float *mask_dev, const float *params_dev, float weight,
                                 float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev,
                                 int64_t ws_bytes, void *stream);
/* Byte offset, into the workspace of ssal_enet_train_decoder_nhwc / ssal_enet_train_decoder_semi_nhwc, of Bottleneck3_8's
 * output [n,h/8,w/8,128] (the features_dev of ssal_train_decoder_grad_nhwc) as those calls leave it; valid until the next call.
 * -1 for dims the net does not take. */
int64_t ssal_enet_train_decoder_features_offset(const ssal_enet *net, int n, int h, int w);
int64_t ssal_train_decoder_grad_semi_workspace_bytes(int n, int h, int w, int classes, int with_raw);
int ssal_train_decoder_grad_semi_nhwc(const float *features_dev, const int64_t *argmax2_dev, const int64_t *argmax1_dev,
                                      const float *features_raw_dev, const int64_t *argmax2_raw_dev,
                                      const int64_t *argmax1_raw_dev, int n, int h, int w, int classes,
                                      const float *params_dev, const uint8_t *labels_dev, const float *mask_dev,
                                      const uint8_t *labelled_dev, int measure, float threshold, float weight,
                                      float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev,
                                      int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes,
                                      void *stream);
int64_t ssal_enet_train_decoder_semi_workspace_bytes(const ssal_enet *net, int n, int h, int w, int with_raw);
int ssal_enet_train_decoder_semi_nhwc(ssal_enet *net, const void *x_dev, const void *x_raw_dev, int x_is_u8, int n, int h,
                                      int w, const uint8_t *labels_dev, const float *mask_dev, const uint8_t *labelled_dev,
                                      int measure, float threshold, const float *params_dev, float weight,
                                      float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev,
                                      int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes,
                                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SSAL_ENET_H */
