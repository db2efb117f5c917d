// ssal_train_icnet_bneck2.h -- training of ICNet through conv5_2, the backbone's last bottleneck but one: conv5_2_1x1_reduce =
// relu(BN(1 x 1 conv (1024 -> 256) of conv5_1)), conv5_2_3x3 = relu(BN(3 x 3 conv at dilation 4 (256 -> 256) of it)), conv5_2 =
// relu(BN(1 x 1 conv (256 -> 1024) of it) + conv5_1), then everything ssal_train_icnet_bneck.h trains (the whole of conv5_3 with
// conv5_2 as input and identity shortcut, the pyramid pooling, the pyramid head), over everything below conv5_1 and the two
// other frozen branches (ssal_train_icnet_bneck2.hip).  gfx950 (MI355X / CDNA4) only.  All tensors fp32
// NHWC.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssal_train_icnet_bneck.h"

namespace ssal {

// The packed vector everything here takes and gives (float offsets):
//   conv5_2_1x1_reduce.kernel [1,1,1024,256] | .gamma [256] | .beta [256] | conv5_2_3x3.kernel [3,3,256,256] | .gamma [256] |
//   .beta [256] | conv5_2_1x1_increase.kernel [1,1,256,1024] | .gamma [1024] | .beta [1024] | the bottleneck trainer's packed vector
constexpr int B2_KR = 0, B2_GR = BK_CIN * BK_C, B2_BR = B2_GR + BK_C, B2_K3 = B2_BR + BK_C, B2_G3 = B2_K3 + 9 * BK_C * BK_C,
              B2_B3 = B2_G3 + BK_C, B2_KI = B2_B3 + BK_C, B2_GI = B2_KI + PO_CIN * PO_CO, B2_BI = B2_GI + PO_CO,
              B2_BNECK = B2_BI + PO_CO;
static_assert(B2_BNECK == 1117184, "the nine tensors of conv5_2");
inline int64_t icnet_bneck2_floats(int K) { return B2_BNECK + icnet_bneck_floats(K); }
// the frozen moving statistics: the reduce layer's mean [256] | variance [256] | the 3 x 3's mean [256] | variance [256] | the
// increase layer's mean [1024] | variance [1024] | the bottleneck trainer's rows
constexpr int B2_STATS_OWN = 4 * BK_C + 2 * PO_CO;
constexpr int B2_STATS = B2_STATS_OWN + BK_STATS;
constexpr int B2_ROWS = 4 * BK_C + 2 * PO_CO;  // scale_r | shift_r | scale_3 | shift_3 (256 each) | scale_i | shift_i (1024 each)

// Geometry: conv5_1 [N, h32, w32, 1024], conv3_1 [N, 2 h32, 2 w32, 256], conv3_sub1 [N, 4 h32, 4 w32, 64].  max_workgroups lowers
// the FIRST grid index of every launch.  Besides the bottleneck depth's launches, and conv5_2's link with the same grids a
// second time:
//   the data gradient through conv5_3's reduce layer   k_icnet_pool_dx's plan: tiles of B2_DX_PT pixels (linear over [N, h32,
//                                                      w32]) strided over at most B2_DX_MAX_WG workgroups, times 8 slabs of
//                                                      128 of the 1024 input channels: grid (G, 8)
//   conv5_2's increase weight gradient                 k_icnet_pyramid_wgrad's plan at 256 x 1024: grid (G, 2, 8), G <= PY_MAX_WG
constexpr int B2_DX_PT = 64;
constexpr int B2_DX_MAX_WG = 1024;

// The workspace.  What lives from the forward until conv5_2's backward is this struct's own: rd, a33, c52 and, from the new
// kernel on, g52.  conv5_2's backward runs when conv5_3's is over and reuses its pieces, which are dead by then, so the
// split-K partials stay bounded independently of the shape (16 x BK_PART3 + PY_MAX_WG x (BK_PARTR + PO_PART) floats, all inside
// `bneck`):
//   bneck.g3, bneck.gr                 g3 and gr of conv5_2 (gr of conv5_3 is read for the last time by the kernel that writes g52)
//   bneck.part3 / fold3, partr / foldr the 3 x 3's and the reduce layer's split-K partials and folds
//   bneck.pool.part / fold             the increase layer's
struct IcnetBneck2Ws {
    float *wt_r;    // conv5_2's reduce kernel in igemm_relayout's layout [1][32][256][32]
    float *wt_3;    // its 3 x 3 kernel [9][8][256][32]
    float *wt_i;    // its increase kernel [1][8][1024][32]
    float *rows;    // [B2_ROWS]
    float *rd;      // [N, h32, w32, 256]   conv5_2_1x1_reduce
    float *a33;     // [N, h32, w32, 256]   conv5_2_3x3
    float *c52;     // [N, h32, w32, 1024]  conv5_2 on the weights being trained
    float *g52;     // [N, h32, w32, 1024]  un-normalised dL/dconv5_2 behind its ReLU
    IcnetBneckWs bneck;
};

// loss [1] float64; grad [icnet_bneck2_floats(K)] fp32 in the packed order
hipError_t launch_icnet_bneck2_grad(const float *c51, const float *c31, const float *c3, int N, int h32, int w32, int K,
                                    const float *params, const float *stats, const uint8_t *labels, const float *mask,
                                    float weight, float label_smoothing, int max_workgroups, const IcnetBneck2Ws &ws,
                                    double *loss, float *grad, hipStream_t s);

}  // namespace ssal
