/*
 * ssal_icnet.h -- C ABI of libssal_hip.so for the ICNet row of the pool-scoring hot path (BASELINE config C4:
 * ICNet multi-scale 1/4, 1/2, 1 at 1024x2048, margin acquisition).
 *
 * The reference's models/icnet/icnet.py:1-7 is an EMPTY class (docstring :3 cites the ICNet paper): there is no
 * reference interface or behaviour to replace.  The network implemented here is pinned in ICNET_SPEC.md; each
 * operator uses the semantics the reference repository defines for it (SAME convolutions as
 * models/enet/enet_modules.py:205,538,565,581; batch-norm models/util/extra_ops.py:154-185; bilinear resize
 * inference.py:96-99; acquisition measures active_learning.py:239-263).  The entry points follow the pattern of
 * the ENet handle (include/ssal_enet.h): same conventions, status codes, ownership and threading rules (concurrent
 * forward / score calls on one committed handle need their own stream + workspace; one handle per device).
 */
#ifndef SSAL_ICNET_H
#define SSAL_ICNET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ssal_icnet ssal_icnet;

/* Model handle: stands where `models.ICNet(classes)` would (models/icnet/icnet.py:1-7).  Tensor names are
 * "<layer>.<attr>" with the layer names of ICNET_SPEC.md (e.g. "conv1_1_3x3_s2.kernel", "conv4_3_3x3.gamma",
 * "conv6_cls.bias"); kernels HWIO, batch-norm vectors [C]. */
int ssal_icnet_create(int c_in, int classes, ssal_icnet **out);
int ssal_icnet_destroy(ssal_icnet *net);
int ssal_icnet_num_tensors(const ssal_icnet *net);
int ssal_icnet_tensor_info(const ssal_icnet *net, int i, const char **name, int *ndim, int64_t dims[4]);
int ssal_icnet_set_tensor(ssal_icnet *net, const char *name, const float *host, int64_t numel);
/* fold the batch-norm statistics (extra_ops.py:181-184, eps = 1e-3), re-layout the kernels for the matrix-core
 * convolution and upload */
int ssal_icnet_commit(ssal_icnet *net, void *stream);
int64_t ssal_icnet_workspace_bytes(const ssal_icnet *net, int n, int h, int w);

/* ICNet.call(inputs, training=False) -> logits [n,h,w,classes] (ICNET_SPEC section 4: conv6_interp);
 * x_dev [n,h,w,c_in] fp32 (or uint8 through the _u8 form: x * f32(1/255), tensortools/input.py:289-290);
 * h, w divisible by 32. */
int ssal_icnet_forward_nhwc(ssal_icnet *net, const float *x_dev, int n, int h, int w, float *logits_dev,
                            void *ws_dev, int64_t ws_bytes, void *stream);
int ssal_icnet_forward_nhwc_u8(ssal_icnet *net, const uint8_t *x_dev, int n, int h, int w, float *logits_dev,
                               void *ws_dev, int64_t ws_bytes, void *stream);

/* forward + softmax + acquisition measure + float64 per-image mean (active_learning.py:229-263), fused: the
 * full-resolution logits never reach HBM (the 4x bilinear conv6_interp is evaluated inside the score kernel).
 * Outputs as ssal_enet_score_nhwc: scores_dev [n] float64; optional label_dev / mask_dev uint8 [n,h,w] (4-byte
 * aligned: four pixels leave per store), conf_dev fp32 [n,h,w] (16-byte aligned). */
int ssal_icnet_score_nhwc(ssal_icnet *net, const float *x_dev, int n, int h, int w, int measure, float threshold,
                          double *scores_dev, uint8_t *label_dev, uint8_t *mask_dev, float *conf_dev, void *ws_dev,
                          int64_t ws_bytes, void *stream);
int ssal_icnet_score_nhwc_u8(ssal_icnet *net, const uint8_t *x_dev, int n, int h, int w, int measure,
                             float threshold, double *scores_dev, uint8_t *label_dev, uint8_t *mask_dev,
                             float *conf_dev, void *ws_dev, int64_t ws_bytes, void *stream);

/* ssal_icnet_score_nhwc (_u8 when x_is_u8 != 0) plus region scores [n][RY][RX] float64 (include/ssal_enet.h, "Region
 * scores"); any rh, rw >= 1.  ICNet's score kernel keeps its partial sums per linear 256-pixel block, not per tile, so this
 * entry goes through the per-pixel confidence plane and ssal_region_means_plane: conf_dev stays optional, and without it
 * the plane lives behind the network's buffers in the workspace -- hence ssal_icnet_regions_workspace_bytes.  scores_dev
 * has the bits ssal_icnet_score_nhwc gives. */
int64_t ssal_icnet_regions_workspace_bytes(const ssal_icnet *net, int n, int h, int w);
int ssal_icnet_score_regions_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w, int measure,
                                  float threshold, int rh, int rw, double *scores_dev, double *region_scores_dev,
                                  uint8_t *label_dev, uint8_t *mask_dev, float *conf_dev, void *ws_dev, int64_t ws_bytes,
                                  void *stream);

/* Evaluation pass (the validation epoch of active_learning.py:277-282 with tensortools/metrics.py:226-257):
 * ssal_enet_evaluate_nhwc_arith's contract (include/ssal_enet.h) for the ICNet handle, fp32 arithmetic.  The trunk is the
 * one ssal_icnet_score_nhwc runs (same schedule, fused launches and knobs); the last launch evaluates conv6_interp, takes
 * the first maximum of the full-resolution logits (the byte ssal_icnet_score_nhwc writes to label_dev) and counts it against
 * labels_dev uint8 [n,h,w]: mask_dev[p] (uint8 [n,h,w]; NULL = weight 1) is ADDED to confusion_dev[label][prediction]
 * (int64 [classes, classes]); labels >= classes are dropped.  No softmax, no score, no per-pixel plane leaves the kernel.
 * labels_dev / mask_dev 4-byte aligned (four pixels per load).  Integer atomics only: the result does not depend on the
 * launch order.  SSAL_EINVAL: bad dims, a NULL pointer (mask_dev aside), a misaligned plane; SSAL_ENOMEM: workspace smaller
 * than ssal_icnet_eval_workspace_bytes (which returns -1 for bad dims or an uncommitted handle). */
int64_t ssal_icnet_eval_workspace_bytes(const ssal_icnet *net, int n, int h, int w);
int ssal_icnet_evaluate_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                             const uint8_t *labels_dev, const uint8_t *mask_dev, int64_t *confusion_dev, void *ws_dev,
                             int64_t ws_bytes, void *stream);

/* Named intermediate tensors of the LAST forward/score call on a workspace (every ICNET_SPEC layer output that is
 * materialised keeps its own buffer): byte offset into the workspace and NHWC dims.  SSAL_EINVAL for a name that
 * is not materialised (the 2x interpolations are evaluated inside the consuming convolution).  Every endpoint is valid
 * after a FORWARD call; a SCORE call runs conv2_2 / conv2_3 as one fused launch each and conv1_sub1 + conv2_sub1 as one
 * (k_front2, csrc/ssal_icnet_front.hip; knob "ic_front", include/ssal_enet.h), so the *_1x1_reduce / *_3x3 buffers of those
 * two blocks, conv1_sub1's and the four *_1x1_proj buffers (knob "ic_dual": the projection shortcut is evaluated inside the
 * increase launch) keep whatever an earlier call left there (stale) -- inspect layer outputs after ssal_icnet_forward_nhwc.
 * ssal_icnet_endpoint_valid_after_score answers, for one name and frame size and the knobs as they are now: 1 = a score
 * call writes it, 0 = a fused launch swallows it, -1 = unknown name / bad arguments (models.ICNet.endpoint raises on 0). */
int ssal_icnet_num_endpoints(const ssal_icnet *net);
int ssal_icnet_endpoint_name(const ssal_icnet *net, int i, const char **name);
int ssal_icnet_endpoint_info(const ssal_icnet *net, const char *name, int n, int h, int w, int64_t *offset,
                             int64_t dims[4]);
int ssal_icnet_endpoint_valid_after_score(const ssal_icnet *net, const char *name, int h, int w);

/* ---- Output-layer training (the reference's -r/--reinitialize-output-layer slice, active_learning.py:905-909, 461-462,
 * for ICNet: conv6_cls/Kernel [1,1,128,classes] and conv6_cls/Bias [classes] over a frozen trunk) ----
 * The head travels PACKED: [128 * classes | classes] floats = the kernel (HWIO, i.e. [c][k]) followed by the bias; head_dev
 * and grad_dev have that layout.  One call computes, for features sub12_sum [n,h,w,128] (1/8 resolution), labels uint8 and
 * mask fp32 [n,8h,8w]: lq = conv6_cls(resize_bilinear(sub12_sum, 2x)) by the forward path's own launch, the full-resolution
 * logits conv6_interp = resize_bilinear(lq, 4x) on the fly, masked_softmax_cross_entropy (tensortools/losses.py:3-74; weight =
 * loginverse_scaling) -> loss_dev [1] float64, and dL/d(head) -> grad_dev (without the regulariser; ssal_adam_apply of
 * include/ssal_enet.h adds it and applies the update).  max_workgroups: 0 = min(tiles, 1024), a tuning knob (>= 0).  No
 * floating-point atomics: two calls give the same bits.  SSAL_EINVAL: classes outside [2,32], n < 1, max_workgroups < 0, a
 * NULL pointer, a map beyond the kernel's limit (the _workspace_bytes query then returns -1); SSAL_ENOMEM: workspace too small. */
int64_t ssal_icnet_head_grad_workspace_bytes(int n, int h, int w, int classes);
int ssal_icnet_head_grad_nhwc(const float *sub12_dev, int n, int h, int w, int classes, const float *head_dev,
                              const uint8_t *labels_dev, const float *mask_dev, float weight, float label_smoothing,
                              int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev, int64_t ws_bytes,
                              void *stream);
/* the same from frames x_dev [n,h,w,c_in] (fp32, or uint8 when x_is_u8 != 0): the frozen trunk up to sub12_sum on the
 * caller's stream (the score path's fused launches), then the tail above; labels / mask [n,h,w].  The workspace holds the
 * network's buffers: after the call the sub12_sum endpoint is the features and conv6_cls the logits of head_dev. */
int64_t ssal_icnet_train_head_workspace_bytes(const ssal_icnet *net, int n, int h, int w);
int ssal_icnet_train_head_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                               const uint8_t *labels_dev, const float *mask_dev, const float *head_dev, float weight,
                               float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev,
                               int64_t ws_bytes, void *stream);
/* ---- The semi-supervised step of the output-layer trainer (active_learning.py:226-275, 339-342) ----
 * The two calls above with the targets built inside the gradient kernel; the argument order and every meaning are those of
 * ssal_final_grad_semi_nhwc / ssal_enet_train_final_semi_nhwc (include/ssal_enet.h).  labelled_dev uint8 [n] (NULL = every
 * image is labelled): image i with labelled_dev[i] == 0 is trained on its own pseudo annotation -- label = the first maximum
 * of its full-resolution logits under head_dev, mask = (confidence >= threshold) for `measure` (0 entropy, 1 margin,
 * 2 confidence; a NaN confidence gives 1) -- and its planes in labels_dev / mask_dev are never read; both may be NULL when
 * no image is labelled (the caller's contract).  The targets are constants: loss and gradient are those of the plain call on
 * the composed targets, bit for bit.  sub12_raw_dev / x_raw_dev (may be NULL): the features / frames of the undistorted
 * images, which the pseudo annotation is then computed from by a target-only launch that leaves one packed byte per loss
 * pixel; the training side goes through the same buffers afterwards (no second feature or logits slot; the images entry
 * runs the trunk on x_raw_dev first, and only when labelled_dev is given).  confusion_dev int64 [classes, classes] (may be
 * NULL) is ADDED the training-pass confusion matrix: (int)mask at [target label][first maximum of the training logits] for
 * every loss pixel, keys >= classes^2 dropped.  pseudo_pixels_dev int64 [n] (may be NULL) is OVERWRITTEN with the count of
 * pseudo-mask-1 pixels per image (0 for a labelled image).  Integer atomics only: two calls give the same bits.
 * with_raw != 0 sizes the workspace for a call with a raw side: one byte per loss pixel more.
 * Statuses as the plain entries', judged before any device work; an unknown measure: SSAL_ENOTIMPL. */
int64_t ssal_icnet_head_grad_semi_workspace_bytes(int n, int h, int w, int classes, int with_raw);
int ssal_icnet_head_grad_semi_nhwc(const float *sub12_dev, const float *sub12_raw_dev, int n, int h, int w, int classes,
                                   const float *head_dev, const uint8_t *labels_dev, const float *mask_dev,
                                   const uint8_t *labelled_dev, int measure, float threshold, float weight,
                                   float label_smoothing, int max_workgroups, double *loss_dev, float *grad_dev,
                                   int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes,
                                   void *stream);
int64_t ssal_icnet_train_head_semi_workspace_bytes(const ssal_icnet *net, int n, int h, int w, int with_raw);
int ssal_icnet_train_head_semi_nhwc(ssal_icnet *net, const void *x_dev, const void *x_raw_dev, int x_is_u8, int n, int h,
                                    int w, const uint8_t *labels_dev, const float *mask_dev, const uint8_t *labelled_dev,
                                    int measure, float threshold, const float *head_dev, float weight, float label_smoothing,
                                    int max_workgroups, double *loss_dev, float *grad_dev, int64_t *confusion_dev,
                                    int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes, void *stream);
/* replaces conv6_cls.kernel [128 * classes] / conv6_cls.bias [classes] (host arrays) of a COMMITTED handle in place: only
 * these two tensors are re-laid-out and uploaded (12 KB), the handle stays committed.  Synchronises the stream; as with
 * ssal_icnet_commit no call may be in flight on the handle on another stream. */
int ssal_icnet_update_head(ssal_icnet *net, const float *kernel_host, const float *bias_host, void *stream);

/* ---- Training of the last fusion stage: sub12_sum = relu(BN(conv_sub2(resize_bilinear(sub24_sum,
 * 2x))) + BN(conv3_sub1_proj(conv3_sub1))) and conv6_cls over a trunk frozen below them ----
 * The eight trained variables travel PACKED, in this order: conv_sub2.kernel [3,3,128,128] | .gamma [128] | .beta [128] |
 * conv3_sub1_proj.kernel [1,1,64,128] | .gamma [128] | .beta [128] | conv6_cls.kernel [1,1,128,classes] | .bias [classes]
 * (156160 + 129 * classes floats); params_dev and grad_dev have that layout.  Batch-norm is inference-mode: stats_dev
 * [4 * 128] = conv_sub2 mean | variance | conv3_sub1_proj mean | variance stay frozen, scale = gamma / sqrtf(variance + 1e-3f)
 * and shift = fmaf(-mean, scale, beta) are folded on the device as ssal_icnet_commit folds them.  One call computes, for
 * sub24_sum [n,h,w,128] (1/16 resolution), conv3_sub1 [n,2h,2w,64], labels uint8 and mask fp32 [n,16h,16w]: sub12_sum and lq
 * by the forward path's own launches on params_dev, the loss of ssal_icnet_head_grad_nhwc -> loss_dev [1] float64, and the
 * gradient of all eight variables -> grad_dev (without the regulariser).  Nothing below the block gets a gradient.  The
 * conv6_cls part of grad_dev and the loss are the bits ssal_icnet_head_grad_nhwc gives on the same sub12_sum.  max_workgroups:
 * 0 = the default grids, a tuning knob (>= 0).  No floating-point atomics: two calls give the same bits.  Statuses as
 * ssal_icnet_head_grad_nhwc's (the _workspace_bytes query returns -1 for a map beyond the kernels' limit). */
int64_t ssal_icnet_fusion_grad_workspace_bytes(int n, int h, int w, int classes);
int ssal_icnet_fusion_grad_nhwc(const float *sub24_dev, const float *conv3_sub1_dev, int n, int h, int w, int classes,
                                const float *params_dev, const uint8_t *labels_dev, const float *mask_dev, float weight,
                                float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream);
/* the same from frames x_dev [n,h,w,c_in] (fp32, or uint8 when x_is_u8 != 0): the frozen trunk up to sub24_sum and
 * conv3_sub1 on the caller's stream (the score path's fused launches), then the tail above; labels / mask [n,h,w].  After the
 * call the conv3_sub1_proj, sub12_sum and conv6_cls endpoints are those of params_dev. */
int64_t ssal_icnet_train_fusion_workspace_bytes(const ssal_icnet *net, int n, int h, int w);
int ssal_icnet_train_fusion_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                                 const uint8_t *labels_dev, const float *mask_dev, const float *params_dev, float weight,
                                 float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                 float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream);
/* replaces the eight trained variables (params_host: the packed vector, a host array) of a COMMITTED handle in place: only
 * conv_sub2, conv3_sub1_proj and conv6_cls are re-laid-out, folded with the handle's moving statistics and uploaded (0.7 MB),
 * the handle stays committed.  Synchronises the stream; as with ssal_icnet_commit no call may be in flight on the handle. */
int ssal_icnet_update_fusion(ssal_icnet *net, const float *params_host, void *stream);

/* ---- Training of the whole cascade head: sub24_sum = relu(BN(conv_sub4(resize_bilinear(conv5_4_k1,
 * 2x))) + BN(conv3_1_sub2_proj(conv3_1))), then the last fusion stage and conv6_cls as above, over the three frozen branches ----
 * The fourteen trained variables travel PACKED, in this order: conv_sub4.kernel [3,3,256,128] | .gamma [128] | .beta [128] |
 * conv3_1_sub2_proj.kernel [1,1,256,128] | .gamma [128] | .beta [128] | the eight of the fusion entries in their order
 * (328192 + 156160 + 129 * classes floats); params_dev and grad_dev have that layout.  stats_dev [8 * 128] = conv_sub4 mean |
 * variance | conv3_1_sub2_proj mean | variance | the four rows of the fusion entries; batch-norm as there.  One call computes,
 * for conv5_4_k1 [n,h,w,256] (1/32 resolution), conv3_1 [n,2h,2w,256], conv3_sub1 [n,4h,4w,64], labels uint8 and mask fp32
 * [n,32h,32w]: sub24_sum, sub12_sum and lq by the forward path's own launches on params_dev, the loss -> loss_dev [1] float64,
 * and the gradient of all fourteen variables -> grad_dev (without the regulariser).  Nothing below the three inputs gets a
 * gradient.  The loss and the last eight gradients are the bits ssal_icnet_fusion_grad_nhwc gives on the same sub24_sum.
 * max_workgroups, determinism and statuses as ssal_icnet_fusion_grad_nhwc's. */
int64_t ssal_icnet_cascade_grad_workspace_bytes(int n, int h, int w, int classes);
int ssal_icnet_cascade_grad_nhwc(const float *conv5_4_k1_dev, const float *conv3_1_dev, const float *conv3_sub1_dev, int n,
                                 int h, int w, int classes, const float *params_dev, const uint8_t *labels_dev,
                                 const float *mask_dev, float weight, float label_smoothing, const float *stats_dev,
                                 int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev, int64_t ws_bytes,
                                 void *stream);
/* the same from frames x_dev [n,h,w,c_in] (fp32, or uint8 when x_is_u8 != 0): the frozen trunk until conv5_4_k1, conv3_1 and
 * conv3_sub1 are written, then the tail above; labels / mask [n,h,w].  After the call the endpoints from conv3_1_sub2_proj on
 * are those of params_dev. */
int64_t ssal_icnet_train_cascade_workspace_bytes(const ssal_icnet *net, int n, int h, int w);
int ssal_icnet_train_cascade_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                                  const uint8_t *labels_dev, const float *mask_dev, const float *params_dev, float weight,
                                  float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                  float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream);
/* ssal_icnet_update_fusion for the fourteen variables: only the five trained layers are re-laid-out, folded and uploaded */
int ssal_icnet_update_cascade(ssal_icnet *net, const float *params_host, void *stream);

/* ---- Training of the pyramid head: conv5_4_k1 = relu(BN(1 x 1 conv, 1024 -> 256, of conv5_3_sum)),
 * the low-resolution branch's only path into the cascade, then the whole cascade head as above, over everything up to the
 * pyramid-pooling sum and the two other frozen branches ----
 * The seventeen trained variables travel PACKED, in this order: conv5_4_k1.kernel [1,1,1024,256] | .gamma [256] | .beta [256] |
 * the fourteen of the cascade entries in their order (262656 floats, then theirs); params_dev and grad_dev have that layout.
 * stats_dev [2 * 256 + 8 * 128] = conv5_4_k1 mean | variance | the eight rows of the cascade entries; batch-norm as there.  One
 * call computes, for conv5_3_sum [n,h,w,1024] (1/32 resolution), conv3_1 [n,2h,2w,256], conv3_sub1 [n,4h,4w,64], labels uint8
 * and mask fp32 [n,32h,32w]: conv5_4_k1 by the forward path's own launch on params_dev, the cascade head as
 * ssal_icnet_cascade_grad_nhwc does, the loss -> loss_dev [1] float64, and the gradient of all seventeen variables -> grad_dev
 * (without the regulariser).  Nothing below the three inputs gets a gradient.  The loss and the last fourteen gradients are the
 * bits ssal_icnet_cascade_grad_nhwc gives on the same conv5_4_k1.  Determinism, statuses and the order of the checks as
 * ssal_icnet_cascade_grad_nhwc's; the size query returns -1 beyond the cascade entries' limit.  max_workgroups (0: no limit)
 * caps the FIRST grid index of every launch, as there; two launches of this depth have further indices that it does not cap:
 * the data gradient through conv_sub4 runs 2 x that many workgroups (the two halves of its 256 input channels) and the weight
 * gradient of conv5_4_k1 16 x that many (8 x 2 slabs of its 1024 x 256 output) -- max_workgroups = 1 is 2 and 16 workgroups. */
int64_t ssal_icnet_pyramid_grad_workspace_bytes(int n, int h, int w, int classes);
int ssal_icnet_pyramid_grad_nhwc(const float *conv5_3_sum_dev, const float *conv3_1_dev, const float *conv3_sub1_dev, int n,
                                 int h, int w, int classes, const float *params_dev, const uint8_t *labels_dev,
                                 const float *mask_dev, float weight, float label_smoothing, const float *stats_dev,
                                 int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev, int64_t ws_bytes,
                                 void *stream);
/* the same from frames x_dev [n,h,w,c_in] (fp32, or uint8 when x_is_u8 != 0): the frozen trunk until conv5_3_sum, conv3_1 and
 * conv3_sub1 are written -- its low-resolution schedule ends after the pyramid pooling, conv5_4_k1 is not launched -- then the
 * tail above; labels / mask [n,h,w].  After the call the endpoints from conv5_4_k1 on are those of params_dev. */
int64_t ssal_icnet_train_pyramid_workspace_bytes(const ssal_icnet *net, int n, int h, int w);
int ssal_icnet_train_pyramid_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                                  const uint8_t *labels_dev, const float *mask_dev, const float *params_dev, float weight,
                                  float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                  float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream);
/* ssal_icnet_update_fusion for the seventeen variables: only the six trained layers are re-laid-out, folded and uploaded */
int ssal_icnet_update_pyramid(ssal_icnet *net, const float *params_host, void *stream);

/* ---- Training through the pyramid pooling: conv5_3 = relu(BN(1 x 1 conv, 256 -> 1024, of conv5_3_3x3) +
 * conv5_2), the increase layer of the backbone's last bottleneck, the parameter-free pyramid pooling over it (conv5_3_sum), then
 * the whole pyramid head as above, over everything below conv5_3_3x3 and conv5_2 and the two other frozen branches ----
 * The twenty trained variables travel PACKED, in this order: conv5_3_1x1_increase.kernel [1,1,256,1024] | .gamma [1024] | .beta
 * [1024] | the seventeen of the pyramid entries in their order (264192 floats, then theirs); params_dev and grad_dev have that
 * layout.  stats_dev [2 * 1024 + 2 * 256 + 8 * 128] = the increase layer's mean | variance | the rows of the pyramid entries;
 * batch-norm as there.  One call computes, for conv5_3_3x3 [n,h,w,256] and conv5_2 [n,h,w,1024] (1/32 resolution; conv5_2 is the
 * bottleneck's identity shortcut), conv3_1 [n,2h,2w,256], conv3_sub1 [n,4h,4w,64], labels uint8 and mask fp32 [n,32h,32w]:
 * conv5_3 and conv5_3_sum by the forward path's own launches on params_dev, the pyramid head as ssal_icnet_pyramid_grad_nhwc
 * does, the loss -> loss_dev [1] float64, and the gradient of all twenty variables -> grad_dev (without the regulariser).
 * Nothing below the four inputs gets a gradient.  The loss and the last seventeen gradients are the bits
 * ssal_icnet_pyramid_grad_nhwc gives on the same conv5_3_sum.  Determinism, statuses and the order of the checks as
 * ssal_icnet_pyramid_grad_nhwc's; the size query returns -1 beyond the cascade entries' limit.  max_workgroups (0: no limit)
 * caps the FIRST grid index of every launch, as there; besides the two launches named there, two launches of this depth have
 * further indices that it does not cap: the data gradient through conv5_4_k1 runs 8 x that many workgroups (the eight slabs of
 * 128 of its 1024 input channels) and the weight gradient of the increase layer 16 x that many (2 x 8 slabs of its 256 x 1024
 * output) -- max_workgroups = 1 is 8 and 16 workgroups. */
int64_t ssal_icnet_pool_grad_workspace_bytes(int n, int h, int w, int classes);
int ssal_icnet_pool_grad_nhwc(const float *conv5_3_3x3_dev, const float *conv5_2_dev, const float *conv3_1_dev,
                              const float *conv3_sub1_dev, int n, int h, int w, int classes, const float *params_dev,
                              const uint8_t *labels_dev, const float *mask_dev, float weight, float label_smoothing,
                              const float *stats_dev, int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev,
                              int64_t ws_bytes, void *stream);
/* the same from frames x_dev [n,h,w,c_in] (fp32, or uint8 when x_is_u8 != 0): the frozen trunk until conv5_3_3x3, conv5_2, conv3_1
 * and conv3_sub1 are written -- its low-resolution schedule ends inside conv5_3, behind its 3 x 3: the increase layer, the
 * pyramid pooling and conv5_4_k1 are not launched -- then the tail above; labels / mask [n,h,w].  After the call the endpoints
 * from conv5_3 on are those of params_dev. */
int64_t ssal_icnet_train_pool_workspace_bytes(const ssal_icnet *net, int n, int h, int w);
int ssal_icnet_train_pool_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w, const uint8_t *labels_dev,
                               const float *mask_dev, const float *params_dev, float weight, float label_smoothing,
                               const float *stats_dev, int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev,
                               int64_t ws_bytes, void *stream);
/* ssal_icnet_update_fusion for the twenty variables: only the seven trained layers are re-laid-out, folded and uploaded */
int ssal_icnet_update_pool(ssal_icnet *net, const float *params_host, void *stream);

/* ---- Training of the last backbone bottleneck: conv5_3_1x1_reduce = relu(BN(1 x 1 conv, 1024 -> 256, of
 * conv5_2)), conv5_3_3x3 = relu(BN(3 x 3 conv at dilation 4, 256 -> 256, SAME: four zero pixels on every side)), then everything
 * the pooling entries above train (the increase layer takes conv5_2 as its identity shortcut), over everything below conv5_2
 * and the two other frozen branches ----
 * The 26 trained variables travel PACKED, in this order: conv5_3_1x1_reduce.kernel [1,1,1024,256] | .gamma [256] | .beta [256] |
 * conv5_3_3x3.kernel [3,3,256,256] | .gamma [256] | .beta [256] | the twenty of the pooling entries in their order (852992
 * floats, then theirs); params_dev and grad_dev have that layout.  stats_dev [4 * 256 + 2 * 1024 + 2 * 256 + 8 * 128] = the
 * reduce layer's mean | variance | the 3 x 3's mean | variance | the rows of the pooling entries; batch-norm as there.  One call
 * computes, for conv5_2 [n,h,w,1024] (1/32 resolution), conv3_1 [n,2h,2w,256], conv3_sub1 [n,4h,4w,64], labels uint8 and mask
 * fp32 [n,32h,32w]: conv5_3_1x1_reduce and conv5_3_3x3 by the forward path's own launches on params_dev, everything above as
 * ssal_icnet_pool_grad_nhwc does, the loss -> loss_dev [1] float64, and the gradient of all 26 variables -> grad_dev (without the
 * regulariser).  Nothing below the three inputs gets a gradient.  The loss and the last twenty gradients are the bits
 * ssal_icnet_pool_grad_nhwc gives on the same conv5_3_3x3.  Determinism, statuses and the order of the checks as
 * ssal_icnet_pool_grad_nhwc's; the size query returns -1 beyond the cascade entries' limit.  max_workgroups (0: no limit) caps
 * the FIRST grid index of every launch, as there; besides the launches named there, four launches of this depth have further
 * indices that it does not cap: the two data gradients (through the increase layer and through the 3 x 3) run 2 x that many
 * workgroups (two slabs of 128 of their 256 input channels), the 3 x 3 weight gradient 36 x that many (9 taps x 2 x 2 slabs of
 * 128 x 128) and the reduce layer's weight gradient 16 x that many -- max_workgroups = 1 is 2, 2, 36 and 16 workgroups.  The
 * split-K partials of the 3 x 3 weight gradient are at most 16 x 2.36 MB of the workspace. */
int64_t ssal_icnet_bneck_grad_workspace_bytes(int n, int h, int w, int classes);
int ssal_icnet_bneck_grad_nhwc(const float *conv5_2_dev, const float *conv3_1_dev, const float *conv3_sub1_dev, int n, int h,
                               int w, int classes, const float *params_dev, const uint8_t *labels_dev, const float *mask_dev,
                               float weight, float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                               float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream);
/* the same from frames x_dev [n,h,w,c_in] (fp32, or uint8 when x_is_u8 != 0): the frozen trunk until conv5_2, conv3_1 and
 * conv3_sub1 are written -- its low-resolution schedule ends behind conv5_2: no layer of conv5_3, the pyramid pooling and
 * conv5_4_k1 are not launched -- then the tail above; labels / mask [n,h,w].  After the call the endpoints from
 * conv5_3_1x1_reduce on are those of params_dev. */
int64_t ssal_icnet_train_bneck_workspace_bytes(const ssal_icnet *net, int n, int h, int w);
int ssal_icnet_train_bneck_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w, const uint8_t *labels_dev,
                                const float *mask_dev, const float *params_dev, float weight, float label_smoothing,
                                const float *stats_dev, int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev,
                                int64_t ws_bytes, void *stream);
/* ssal_icnet_update_fusion for the 26 variables: only the nine trained layers are re-laid-out, folded and uploaded */
int ssal_icnet_update_bneck(ssal_icnet *net, const float *params_host, void *stream);

/* ---- Training through conv5_2, the last backbone bottleneck but one: conv5_2_1x1_reduce = relu(BN(1 x 1
 * conv, 1024 -> 256, of conv5_1)), conv5_2_3x3 = relu(BN(3 x 3 conv at dilation 4, 256 -> 256, SAME)), conv5_2 = relu(BN(1 x 1
 * conv, 256 -> 1024, of it) + conv5_1), then everything the bottleneck entries above train (conv5_3 takes conv5_2 as its input
 * and identity shortcut), over everything below conv5_1 and the two other frozen branches ----
 * The 35 trained variables travel PACKED, in this order: conv5_2_1x1_reduce.kernel [1,1,1024,256] | .gamma [256] | .beta [256] |
 * conv5_2_3x3.kernel [3,3,256,256] | .gamma [256] | .beta [256] | conv5_2_1x1_increase.kernel [1,1,256,1024] | .gamma [1024] |
 * .beta [1024] | the 26 of the bottleneck entries in their order (1117184 floats, then theirs); params_dev and grad_dev have
 * that layout.  stats_dev [4 * 256 + 2 * 1024, then the bottleneck entries' rows] = conv5_2's reduce layer's mean | variance |
 * its 3 x 3's mean | variance | its increase layer's mean | variance | the rows of the bottleneck entries; batch-norm as there.
 * One call computes, for conv5_1 [n,h,w,1024] (1/32 resolution), conv3_1 [n,2h,2w,256], conv3_sub1 [n,4h,4w,64], labels uint8
 * and mask fp32 [n,32h,32w]: the three layers of conv5_2 by the forward path's own launches on params_dev, everything above as
 * ssal_icnet_bneck_grad_nhwc does, the loss -> loss_dev [1] float64, and the gradient of all 35 variables -> grad_dev (without
 * the regulariser).  Nothing below the three inputs gets a gradient.  The loss and the last 26 gradients are the bits
 * ssal_icnet_bneck_grad_nhwc gives on the same conv5_2.  Determinism, statuses and the order of the checks as
 * ssal_icnet_bneck_grad_nhwc's; the size query returns -1 beyond the cascade entries' limit.  max_workgroups (0: no limit) caps
 * the FIRST grid index of every launch, as there; the launches of the bottleneck entries with further indices run a second
 * time for conv5_2, and two more have further indices that it does not cap: the data gradient onto conv5_2 runs 8 x that many
 * workgroups (eight slabs of 128 of its 1024 channels) and conv5_2's increase weight gradient 16 x that many.  The workspace
 * holds no split-K partials beyond the bottleneck entries': conv5_2's weight gradients reuse them. */
int64_t ssal_icnet_bneck2_grad_workspace_bytes(int n, int h, int w, int classes);
int ssal_icnet_bneck2_grad_nhwc(const float *conv5_1_dev, const float *conv3_1_dev, const float *conv3_sub1_dev, int n, int h,
                                int w, int classes, const float *params_dev, const uint8_t *labels_dev, const float *mask_dev,
                                float weight, float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream);
/* the same from frames x_dev [n,h,w,c_in] (fp32, or uint8 when x_is_u8 != 0): the frozen trunk until conv5_1, conv3_1 and
 * conv3_sub1 are written -- its low-resolution schedule ends behind conv5_1: no layer of conv5_2 or conv5_3, the pyramid
 * pooling and conv5_4_k1 are not launched -- then the tail above; labels / mask [n,h,w].  After the call the endpoints from
 * conv5_2_1x1_reduce on are those of params_dev. */
int64_t ssal_icnet_train_bneck2_workspace_bytes(const ssal_icnet *net, int n, int h, int w);
int ssal_icnet_train_bneck2_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w, const uint8_t *labels_dev,
                                 const float *mask_dev, const float *params_dev, float weight, float label_smoothing,
                                 const float *stats_dev, int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev,
                                 int64_t ws_bytes, void *stream);
/* ssal_icnet_update_fusion for the 35 variables: only the twelve trained layers are re-laid-out, folded and uploaded */
int ssal_icnet_update_bneck2(ssal_icnet *net, const float *params_host, void *stream);

/* ---- The semi-supervised step of the fusion and the cascade trainer (active_learning.py:226-275, 339-342; DESIGN.md
 * section 30) ----
 * The four gradient calls above with the targets built inside the head's gradient kernel: labelled_dev, measure, threshold,
 * confusion_dev and pseudo_pixels_dev mean what they mean in ssal_icnet_head_grad_semi_nhwc, and sit where they sit there
 * (after the mask; after the gradient).  The targets are constants: the loss and all 8 / 14 gradients are those of the plain
 * call on the composed targets, bit for bit.  The raw feature pointers (the features of the undistorted frames; shapes as
 * their counterparts) come directly after the training ones, all or none; x_raw_dev likewise after x_dev.  With a raw side
 * and labelled_dev given, the trained blocks and the head run on the raw features first, through the same workspace slots,
 * and a target-only launch leaves one packed byte per loss pixel; the training side follows (the images entries run the
 * trunk twice, up to the trainer's stop).  with_raw != 0 sizes the workspace for that byte plane: n * 16h * 16w (fusion
 * features entry), n * 32h * 32w (cascade features entry), n * h * w (images entries) bytes more.  Statuses as the plain
 * entries', judged before any device work; raw pointers given in part: SSAL_EINVAL; an unknown measure: SSAL_ENOTIMPL. */
int64_t ssal_icnet_fusion_grad_semi_workspace_bytes(int n, int h, int w, int classes, int with_raw);
int ssal_icnet_fusion_grad_semi_nhwc(const float *sub24_dev, const float *conv3_sub1_dev, const float *sub24_raw_dev,
                                     const float *conv3_sub1_raw_dev, int n, int h, int w, int classes,
                                     const float *params_dev, const uint8_t *labels_dev, const float *mask_dev,
                                     const uint8_t *labelled_dev, int measure, float threshold, float weight,
                                     float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                     float *grad_dev, int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev,
                                     int64_t ws_bytes, void *stream);
int64_t ssal_icnet_train_fusion_semi_workspace_bytes(const ssal_icnet *net, int n, int h, int w, int with_raw);
int ssal_icnet_train_fusion_semi_nhwc(ssal_icnet *net, const void *x_dev, const void *x_raw_dev, int x_is_u8, int n, int h,
                                      int w, const uint8_t *labels_dev, const float *mask_dev, const uint8_t *labelled_dev,
                                      int measure, float threshold, const float *params_dev, float weight,
                                      float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                      float *grad_dev, int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev,
                                      int64_t ws_bytes, void *stream);
int64_t ssal_icnet_cascade_grad_semi_workspace_bytes(int n, int h, int w, int classes, int with_raw);
int ssal_icnet_cascade_grad_semi_nhwc(const float *conv5_4_k1_dev, const float *conv3_1_dev, const float *conv3_sub1_dev,
                                      const float *conv5_4_k1_raw_dev, const float *conv3_1_raw_dev,
                                      const float *conv3_sub1_raw_dev, int n, int h, int w, int classes,
                                      const float *params_dev, const uint8_t *labels_dev, const float *mask_dev,
                                      const uint8_t *labelled_dev, int measure, float threshold, float weight,
                                      float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                      float *grad_dev, int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev,
                                      int64_t ws_bytes, void *stream);
int64_t ssal_icnet_train_cascade_semi_workspace_bytes(const ssal_icnet *net, int n, int h, int w, int with_raw);
int ssal_icnet_train_cascade_semi_nhwc(ssal_icnet *net, const void *x_dev, const void *x_raw_dev, int x_is_u8, int n, int h,
                                       int w, const uint8_t *labels_dev, const float *mask_dev, const uint8_t *labelled_dev,
                                       int measure, float threshold, const float *params_dev, float weight,
                                       float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                       float *grad_dev, int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev,
                                       int64_t ws_bytes, void *stream);

/* ---- Training of the high-resolution branch down to the image: conv1_sub1, conv2_sub1, conv3_sub1
 * (3 x 3, stride 2, TF SAME, batch-norm, ReLU; c_in -> 32 -> 32 -> 64), then the cascade head as above, over the two frozen
 * backbone branches ----
 * The 23 trained variables travel PACKED, in this order: conv1_sub1.kernel [3,3,c_in,32] | .gamma [32] | .beta [32] |
 * conv2_sub1.kernel [3,3,32,32] | .gamma [32] | .beta [32] | conv3_sub1.kernel [3,3,32,64] | .gamma [64] | .beta [64] | the
 * fourteen of the cascade entries in their order (288 c_in + 27904 floats, then theirs); params_dev and grad_dev have that
 * layout.  c_in is 3 or 4.  stats_dev is UNPADDED, every row at its layer's own width: conv1_sub1 mean [32] | variance [32] |
 * conv2_sub1 mean [32] | variance [32] | conv3_sub1 mean [64] | variance [64] | the eight rows of 128 of the cascade entries
 * (256 + 1024 floats); batch-norm as there.  One call computes, for conv5_4_k1 [n,h,w,256] (1/32 resolution), conv3_1
 * [n,2h,2w,256], the frames x_dev [n,32h,32w,c_in] (fp32, or uint8 when x_is_u8 != 0: float(u8) * float32(1/255)), labels uint8
 * and mask fp32 [n,32h,32w]: the branch, sub24_sum, sub12_sum and lq by the forward path's own launches on params_dev, the loss
 * -> loss_dev [1] float64, and the gradient of all 23 variables -> grad_dev (without the regulariser).  The frames and the two
 * backbone features get no gradient.  The loss and the last fourteen gradients are the bits ssal_icnet_cascade_grad_nhwc gives
 * on the same conv3_sub1.  max_workgroups, determinism and statuses as ssal_icnet_fusion_grad_nhwc's; the _workspace_bytes
 * query returns -1 beyond the cascade entries' limit or at n * 32h * 32w >= 2^27 frame pixels (the forward path's limit). */
int64_t ssal_icnet_highres_grad_workspace_bytes(int n, int h, int w, int classes);
int ssal_icnet_highres_grad_nhwc(const float *conv5_4_k1_dev, const float *conv3_1_dev, const void *x_dev, int n, int h, int w,
                                 int classes, const float *params_dev, const uint8_t *labels_dev, const float *mask_dev,
                                 float weight, float label_smoothing, const float *stats_dev, int x_is_u8, int c_in,
                                 int max_workgroups, double *loss_dev, float *grad_dev, void *ws_dev, int64_t ws_bytes,
                                 void *stream);
/* the same from the frames alone ([n,h,w,c_in] of the handle): the two frozen backbone branches until conv5_4_k1 and conv3_1 are
 * written, then the branch and the tail above; labels / mask [n,h,w].  After the call the endpoints conv1_sub1, conv2_sub1,
 * conv3_sub1 and those from conv3_1_sub2_proj on are those of params_dev. */
int64_t ssal_icnet_train_highres_workspace_bytes(const ssal_icnet *net, int n, int h, int w);
int ssal_icnet_train_highres_nhwc(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w,
                                  const uint8_t *labels_dev, const float *mask_dev, const float *params_dev, float weight,
                                  float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                  float *grad_dev, void *ws_dev, int64_t ws_bytes, void *stream);
/* ssal_icnet_update_fusion for the 23 variables: only the eight trained layers are re-laid-out, folded and uploaded */
int ssal_icnet_update_highres(ssal_icnet *net, const float *params_host, void *stream);

/* ---- The semi-supervised step of the high-resolution trainer ----
 * ssal_icnet_highres_grad_nhwc / ssal_icnet_train_highres_nhwc with the semi-supervised step of the cascade entries above
 * (ssal_icnet_cascade_grad_semi_nhwc: labelled_dev, measure, threshold, confusion_dev, pseudo_pixels_dev, their meaning,
 * determinism and statuses).  The raw side is conv5_4_k1_raw_dev, conv3_1_raw_dev and the undistorted frames x_raw_dev (the dtype
 * of x_dev), all three or none (else SSAL_EINVAL); with it the pseudo annotation of an unlabelled image comes from the logits of
 * the undistorted frames under params_dev: the branch (conv1_sub1 + conv2_sub1 as one launch where the forward path's fused
 * front applies -- knob "ic_front" bit 0 -- with the same bits as the separate launches), both fusion blocks and the head run on
 * them first, through the same workspace slots as the training frames after them.  The loss and the 23 gradients are the bits
 * the plain entries give on the composed targets.  The workspace is the plain entries' plus what the cascade semi entries add
 * to theirs at the same n, h, w, classes; the queries return -1 wherever the plain ones do. */
int64_t ssal_icnet_highres_grad_semi_workspace_bytes(int n, int h, int w, int classes, int with_raw);
int ssal_icnet_highres_grad_semi_nhwc(const float *conv5_4_k1_dev, const float *conv3_1_dev, const void *x_dev,
                                      const float *conv5_4_k1_raw_dev, const float *conv3_1_raw_dev, const void *x_raw_dev,
                                      int n, int h, int w, int classes, const float *params_dev, const uint8_t *labels_dev,
                                      const float *mask_dev, const uint8_t *labelled_dev, int measure, float threshold,
                                      float weight, float label_smoothing, const float *stats_dev, int x_is_u8, int c_in,
                                      int max_workgroups, double *loss_dev, float *grad_dev, int64_t *confusion_dev,
                                      int64_t *pseudo_pixels_dev, void *ws_dev, int64_t ws_bytes, void *stream);
int64_t ssal_icnet_train_highres_semi_workspace_bytes(const ssal_icnet *net, int n, int h, int w, int with_raw);
int ssal_icnet_train_highres_semi_nhwc(ssal_icnet *net, const void *x_dev, const void *x_raw_dev, int x_is_u8, int n, int h,
                                       int w, const uint8_t *labels_dev, const float *mask_dev, const uint8_t *labelled_dev,
                                       int measure, float threshold, const float *params_dev, float weight,
                                       float label_smoothing, const float *stats_dev, int max_workgroups, double *loss_dev,
                                       float *grad_dev, int64_t *confusion_dev, int64_t *pseudo_pixels_dev, void *ws_dev,
                                       int64_t ws_bytes, void *stream);

/* Stand-alone fused convolution (the operator every ICNet layer is built from; also the per-block parity hook):
 * y = [relu]( BN(conv2d(x, kernel HWIO, strides s, dilations d, "SAME")) [+ res] ), BN given as mean / variance /
 * gamma / beta (all NULL: no batch-norm; bias_dev optional).  upsample2x != 0 runs the conv on
 * tf.image.resize_bilinear(x, 2x) evaluated on the fly.  cin % 32 == 0 (matrix-core path) or cin in {1,3,4} with
 * a 3x3 / stride-2 / 32-channel kernel (first-layer path).  ws: ssal_conv_bn_workspace_bytes().  The kernel and the
 * batch-norm vectors are host arrays: they are folded / re-laid-out and uploaded on every call (the call synchronises
 * the stream once for that), which is what a per-operator test hook needs; the network handle does it once, at commit. */
int64_t ssal_conv_bn_workspace_bytes(int kh, int kw, int cin, int cout);
int ssal_conv_bn_act(const float *x_dev, int n, int h, int w, int cin, const float *kernel_host, int kh, int kw,
                     int cout, int stride, int dilation, const float *mean_host, const float *var_host,
                     const float *gamma_host, const float *beta_host, const float *bias_host,
                     const float *res_dev, int relu, int upsample2x, float *y_dev, void *ws_dev, int64_t ws_bytes,
                     void *stream);
/* tf.nn.max_pool(x, 3x3, strides 2, "SAME") -> [n, ceil(h/2), ceil(w/2), c];  c % 4 == 0 */
int ssal_max_pool_3x3_s2(const float *x_dev, int n, int h, int w, int c, float *y_dev, void *stream);
/* ICNET_SPEC pyramid pooling: y = x + sum over b in (1,2,3,6) of resize_bilinear(bin_average_b(x), h, w);
 * (bin average = sum over the bin's rows of the sum over its columns, divided by the count);
 * ws >= n * (50 + 12 * h) * c * 4 bytes; c % 4 == 0 */
int ssal_pyramid_pooling(const float *x_dev, int n, int h, int w, int c, float *y_dev, void *ws_dev, int64_t ws_bytes,
                         void *stream);
/* conv6_interp + score on materialised 1/4-resolution logits lq_dev [n,h,w,classes]: outputs at [n,4h,4w] */
int64_t ssal_upscore_workspace_bytes(int n, int h, int w);
int ssal_upscore_logits_nhwc(const float *lq_dev, int n, int h, int w, int classes, int measure, float threshold,
                             double *scores_dev, uint8_t *label_dev, uint8_t *mask_dev, float *conf_dev,
                             void *ws_dev, int64_t ws_bytes, void *stream);

/* ---- Opt-in arithmetic (SSAL_ARITH_* of include/ssal_enet.h) ----
 * arithmetic == SSAL_ARITH_F32 is exactly the entry without the suffix: same launches, same bits.  SSAL_ARITH_BF16X3 runs
 * every convolution that the exact path gives to the plain implicit-GEMM kernel (k_igemm<NT, 0>) on the split-operand kernel
 * k_igemm_bf16x3<NT> (csrc/ssal_icnet_bf16x3.hip) and, in the score entry, conv2_2 / conv2_3 on ENet's bf16x3 regular-block
 * kernel; the first convolutions, k_conv3x3_c32, both up-sampling forms, the projection-shortcut (dual) launches, the
 * conv6_cls head, pooling and the score kernel stay exact.  Not bit-identical to the default mode.  An unknown mode is
 * SSAL_EINVAL, judged before any device work.  x_dev is float32 (x_is_u8 == 0) or the decoded uint8 frame.  Workspaces are
 * those of the plain entries. */
int ssal_icnet_forward_nhwc_arith(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w, int arithmetic,
                                  float *logits_dev, void *ws_dev, int64_t ws_bytes, void *stream);
int ssal_icnet_score_nhwc_arith(ssal_icnet *net, const void *x_dev, int x_is_u8, int n, int h, int w, int measure,
                                float threshold, int arithmetic, double *scores_dev, uint8_t *label_dev, uint8_t *mask_dev,
                                float *conf_dev, void *ws_dev, int64_t ws_bytes, void *stream);
/* ssal_conv_bn_act with an arithmetic mode: the per-operator test hook of k_igemm_bf16x3.  The workspace of the bf16x3 mode
 * also holds the pre-split kernel (1.5x the fp32 kernel's bytes, output channels padded to 32). */
int64_t ssal_conv_bn_workspace_bytes_arith(int kh, int kw, int cin, int cout, int arithmetic);
int ssal_conv_bn_act_arith(const float *x_dev, int n, int h, int w, int cin, const float *kernel_host, int kh, int kw,
                           int cout, int stride, int dilation, const float *mean_host, const float *var_host,
                           const float *gamma_host, const float *beta_host, const float *bias_host, const float *res_dev,
                           int relu, int upsample2x, float *y_dev, void *ws_dev, int64_t ws_bytes, void *stream,
                           int arithmetic);
/* Dry query (no device, no launch; cf. ssal_debug_layer_dispatch): which kernel and which column-tile width NT the
 * convolution launcher picks for x [n,h,w,cin] (up2 != 0: the conv runs on the 2x up-sampled tensor), with the knobs and the
 * launch concurrency of the calling thread as they are now.  nt_out: 1, 2 or 4 for the implicit-GEMM kernels, 0 otherwise.
 * SSAL_EINVAL: a shape no kernel takes, an unknown mode, a NULL output. */
#define SSAL_ICNET_KERNEL_IGEMM             0  /* k_igemm<NT, 0> (either LDS-buffer count) */
#define SSAL_ICNET_KERNEL_IGEMM_UP2         1  /* k_igemm<NT, 1 | 2> */
#define SSAL_ICNET_KERNEL_CONV1X1_UP2_C128  2  /* k_conv1x1_up2_c128 */
#define SSAL_ICNET_KERNEL_CONV3X3_C32       3  /* k_conv3x3_c32 */
#define SSAL_ICNET_KERNEL_IGEMM_BF16X3      4  /* k_igemm_bf16x3<NT> */
#define SSAL_ICNET_KERNEL_CONV_FIRST        5  /* k_conv_first (cin 1, 3 or 4) */
int ssal_icnet_debug_conv_dispatch(int n, int h, int w, int cin, int cout, int kh, int kw, int stride, int dil, int up2,
                                   int has_res, int arithmetic, int *kernel_out, int *nt_out);
/* Host-only, no device is touched: which route the raw side of the semi-supervised high-resolution entries (above) takes for
 * conv1_sub1 + conv2_sub1 on n frames of 32h x 32w x c_in under the current knobs -- *fused_out = 1: one launch (k_front2),
 * 0: the two separate launches.  The statuses of the entries' dims check (SSAL_EINVAL beyond their limit or at c_in not 3 / 4). */
int ssal_icnet_debug_highres_raw_route(int c_in, int n, int h, int w, int *fused_out);

#ifdef __cplusplus
}
#endif
#endif /* SSAL_ICNET_H */
