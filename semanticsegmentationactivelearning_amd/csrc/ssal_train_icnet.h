// ssal_train_icnet.h -- training of ICNet's output layer (conv6_cls: kernel [1,1,128,K] and bias [K]) over a frozen trunk
// (ssal_train_icnet.hip).  gfx950 (MI355X / CDNA4) only.  All tensors fp32 NHWC.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ssal {

// The packed head everything here takes and gives: [128 * K | K] floats = conv6_cls/Kernel (HWIO [1,1,128,K], i.e. [c][k])
// followed by conv6_cls/Bias.
inline int64_t icnet_head_floats(int K) { return 128 * (int64_t)K + K; }

// Geometry: the features are sub12_sum [N, h8, w8, 128] (1/8 resolution), the head's logits lq [N, 2 h8, 2 w8, K] (1/4),
// the loss is taken on [N, 8 h8, 8 w8].  Every offset into a tensor is computed in 64 bits; what remains are int
// coordinates (8 h8, 8 w8 and their +1 neighbours) and the int tile index.
constexpr int IH_T = 8;          // a workgroup's tile: IH_T x IH_T pixels of lq = 32 x 32 pixels of the loss
constexpr int IH_MAX_WG = 1024;  // partial rows the finish kernel folds
bool icnet_head_fits(int h8, int w8);
// workgroups of the gradient launch: min(tiles, IH_MAX_WG[, max_workgroups when > 0])
int icnet_head_workgroups(int h8, int w8, int max_workgroups);

// What one call needs behind the features: lq (unless the caller owns it), the kernel in launch_igemm's layout with its
// scale / shift rows, the per-workgroup partials.
struct IcnetHeadWs {
    float *lq;       // [N, 2 h8, 2 w8, K]
    float *wt;       // [4][32][32] (igemm_relayout's layout for 1 x 1 x 128 x K), then scale [32], shift [32]
    float *part;     // [G][128 K + K]
    double *lpart;   // [G][2]
};
int64_t icnet_head_ws_floats_wt();  // 4 * 32 * 32 + 64
int64_t icnet_head_tiles(int h8, int w8);  // tiles of the gradient kernel per image

// conv6_cls/Kernel + Bias (packed head on the device) -> wt / scale / shift as ssal_icnet_commit lays them out
hipError_t launch_icnet_head_pack(const float *head, int K, float *wt, hipStream_t s);

// The semi-supervised side of a gradient launch; the kernel's argument as it stands.
struct IcnetHeadSemi {
    const uint8_t *labelled;    // [N], NULL = all labelled
    int measure;
    float threshold;
    const uint8_t *tgt_in;      // [N, 8 h8, 8 w8] packed pseudo targets of the undistorted frames (label in bits 0..6, mask in
                                // bit 7; launch_icnet_head_targets wrote them), NULL = from the training logits
    uint8_t *tgt_out;           // non-NULL: the target-only launch (set by launch_icnet_head_targets alone)
    unsigned long long *rep;    // confusion replicas [reps][conf_rep_stride(K * K)], zeroed by the caller; NULL = no metrics
    int reps;
    unsigned long long *pseudo_pixels;  // [N] (zeroed by the launcher), NULL = not counted
};

// The whole tail: lq = conv6_cls(resize_2x(sub12_sum)) through launch_igemm (the forward path's own launch, reading the
// packed head), then the fused loss + gradient kernel and the fold.  loss [1] float64; grad [128 K + K] fp32.
// hw_out (NULL = not written; with semi: DESIGN.md section 30): [N][icnet_head_tiles][36][K], every tile's pull-back of dL/dlq
// onto its 6 x 6 window of sub12_sum (first pixel (4 ty, 4 tx)), un-normalised; a window pixel two tiles share holds each
// one's part.
hipError_t launch_icnet_head_grad(const float *sub12, int N, int h8, int w8, int K, const float *head,
                                  const uint8_t *labels, const float *mask, float weight, float label_smoothing,
                                  int max_workgroups, const IcnetHeadWs &ws, double *loss, float *grad, hipStream_t s,
                                  const IcnetHeadSemi *semi = nullptr, float *hw_out = nullptr);

// The target-only launch on the features of the undistorted frames: packs the head, lq = conv6_cls(resize_2x(sub12_raw))
// into ws.lq, then one packed byte per loss pixel of the unlabelled images -> tgt [N, 8 h8, 8 w8].  Nothing else is
// written, so the training features can go through the same ws.lq afterwards (launch_icnet_head_grad with semi.tgt_in = tgt,
// which then does not pack the head again).  semi.labelled NULL: no launch but the pack.
hipError_t launch_icnet_head_targets(const float *sub12_raw, int N, int h8, int w8, int K, const float *head,
                                     int max_workgroups, const IcnetHeadWs &ws, const IcnetHeadSemi &semi, uint8_t *tgt,
                                     hipStream_t s);

}  // namespace ssal
