// ssal_train_icnet_highres.h -- training of ICNet's high-resolution branch down to the image: conv1_sub1, conv2_sub1 and
// conv3_sub1 (3 x 3, stride 2, TF SAME: no pad before, one zero row / column after, + inference batch-norm + ReLU,
// c_in -> 32 -> 32 -> 64), then the whole cascade head of ssal_train_icnet_cascade.h, over the two frozen backbone branches
// (ssal_train_icnet_highres.hip).  gfx950 (MI355X / CDNA4) only.  All tensors fp32 NHWC; the frame may
// be the decoded uint8 one (float(u8) * float32(1 / 255), as launch_conv_first reads it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssal_train_icnet_cascade.h"

namespace ssal {

// The packed vector everything here takes and gives (float offsets; c_in = 3 or 4 input channels):
//   conv1_sub1.kernel [3,3,c_in,32] | .gamma [32] | .beta [32] | conv2_sub1.kernel [3,3,32,32] | .gamma [32] | .beta [32] |
//   conv3_sub1.kernel [3,3,32,64] | .gamma [64] | .beta [64] | the cascade trainer's packed vector
struct IcnetHighresOff {
    int k1, g1, b1, k2, g2, b2, k3, g3, b3, cascade;
};
inline IcnetHighresOff icnet_highres_offsets(int c_in)
{
    IcnetHighresOff o;
    o.k1 = 0;
    o.g1 = 9 * c_in * 32;
    o.b1 = o.g1 + 32;
    o.k2 = o.b1 + 32;
    o.g2 = o.k2 + 9 * 32 * 32;
    o.b2 = o.g2 + 32;
    o.k3 = o.b2 + 32;
    o.g3 = o.k3 + 9 * 32 * 64;
    o.b3 = o.g3 + 64;
    o.cascade = o.b3 + 64;
    return o;
}
inline int64_t icnet_highres_floats(int c_in, int K) { return icnet_highres_offsets(c_in).cascade + icnet_cascade_floats(K); }
// The frozen moving statistics travel UNPADDED, row after row at each layer's own width: conv1_sub1 mean [32] | variance [32] |
// conv2_sub1 mean [32] | variance [32] | conv3_sub1 mean [64] | variance [64] | the cascade trainer's eight rows of 128
constexpr int HR_STATS_OWN = 4 * 32 + 2 * 64;
constexpr int HR_STATS = HR_STATS_OWN + CA_STATS;

// Geometry: the frame [N, 32 h32, 32 w32, c_in]; a_1 [N, 16 h32, 16 w32, 32], a_2 [N, 8 h32, 8 w32, 32], F3 = conv3_sub1
// [N, 4 h32, 4 w32, 64].  The weight-gradient kernels split their pixel tiles over at most HR_MAX_WG workgroups, the data
// gradients stride theirs over at most HR_DX_MAX_WG.
constexpr int HR_MAX_WG = 64;
constexpr int HR_DX_MAX_WG = 2048;
constexpr int HR_PART = (9 * 32 + 1) * 64;  // floats of the largest split-K partial: [9 taps x 32 ci, then sum_p gz][64 co]
// the cascade's guard and the forward path's 32-bit byte offsets into conv1_sub1's output (n h w < 2^27 frame pixels); the
// kernels here index with 64 bits and stride their grids over the tiles: no limit of their own
bool icnet_highres_fits(int n, int h32, int w32);

struct IcnetHighresWs {
    float *wt2;    // conv2_sub1's kernel in igemm_relayout's layout [9][1][32][32]
    float *wt3;    // conv3_sub1's [9][1][64][32]
    float *rows;   // scale_1 | shift_1 | scale_2 | shift_2 (32 each) | scale_3 | shift_3 (64 each)
    float *a1;     // [N, H/2, W/2, 32]
    float *a2;     // [N, H/4, W/4, 32]
    float *f3;     // [N, H/8, W/8, 64]  conv3_sub1
    float *gz3;    // [N, H/8, W/8, 64]  un-normalised dL/dz_3 / s_3: da_3 behind F3's ReLU
    float *gz2;    // [N, H/4, W/4, 32]
    float *gz1;    // [N, H/2, W/2, 32]
    float *part;   // [HR_MAX_WG][HR_PART], one layer after the other
    float *fold;   // [HR_PART]
    IcnetCascadeWs cascade;
};

// loss [1] float64; grad [icnet_highres_floats(c_in, K)] fp32 in the packed order.  x: the frame, fp32 or uint8.  semi
// (NULL = the plain step, launch for launch): handed on to launch_icnet_cascade_grad
hipError_t launch_icnet_highres_grad(const float *c54, const float *c31, const void *x, bool x_is_u8, int c_in, int N, int h32,
                                     int w32, int K, const float *params, const float *stats, const uint8_t *labels,
                                     const float *mask, float weight, float label_smoothing, int max_workgroups,
                                     const IcnetHighresWs &ws, double *loss, float *grad, hipStream_t s,
                                     const IcnetHeadSemi *semi = nullptr);

// The target phase on the undistorted frames x_raw and their backbone features: the pack, the branch on x_raw under the weights
// being trained -> conv3_sub1_raw in ws.f3, then launch_icnet_cascade_targets on it -> tgt [N, 32 h32, 32 w32].  Nobody reads
// the raw a_1 again, so conv1_sub1 + conv2_sub1 run as ONE launch (launch_front2, bit-identical to the two) into ws.a2 wherever
// icnet_highres_raw_fused says so, else as the training side's launches into ws.a1 / ws.a2.  The training frames go through
// the same slots afterwards (launch_icnet_highres_grad with semi.tgt_in = tgt).
hipError_t launch_icnet_highres_targets(const float *c54_raw, const float *c31_raw, const void *x_raw, bool x_is_u8, int c_in,
                                        int N, int h32, int w32, int K, const float *params, const float *stats,
                                        int max_workgroups, const IcnetHighresWs &ws, const IcnetHeadSemi &semi, uint8_t *tgt,
                                        hipStream_t s);
// the raw side's route: launch_front2's own guards (front2_supported; one frame of c_in floats below 2^31 bytes; fewer than
// 2^31 tiles of 8 x 16) on the matrix-core family, under bit 0 of the knob "ic_front".  icnet_highres_fits is the tighter
// bound (N H W < 2^27 with c_in <= 4 keeps H W c_in 4 below 2^29), so only the knob ever sends an admitted shape to the
// unfused route; the guards are restated all the same, so that no launch_front2 refusal can become an error of the step.
bool icnet_highres_raw_fused(int c_in, int N, int h32, int w32, int ic_front, bool mfma);

}  // namespace ssal
