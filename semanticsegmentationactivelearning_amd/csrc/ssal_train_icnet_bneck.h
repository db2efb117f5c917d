// ssal_train_icnet_bneck.h -- training of ICNet's last backbone bottleneck: conv5_3_1x1_reduce = relu(BN(1 x 1 conv (1024 ->
// 256) of conv5_2)), conv5_3_3x3 = relu(BN(3 x 3 conv at dilation 4 (256 -> 256) of it)), then everything
// ssal_train_icnet_pool.h trains (the increase layer with conv5_2 as identity shortcut, the pyramid pooling, the pyramid head),
// over everything below conv5_2 and the two other frozen branches (ssal_train_icnet_bneck.hip).
// gfx950 (MI355X / CDNA4) only.  All tensors fp32 NHWC.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssal_train_icnet_pool.h"

namespace ssal {

// The packed vector everything here takes and gives (float offsets):
//   conv5_3_1x1_reduce.kernel [1,1,1024,256] | .gamma [256] | .beta [256] | conv5_3_3x3.kernel [3,3,256,256] | .gamma [256] |
//   .beta [256] | the pooling trainer's packed vector
constexpr int BK_CIN = 1024, BK_C = 256, BK_DIL = 4;
constexpr int BK_KR = 0, BK_GR = BK_CIN * BK_C, BK_BR = BK_GR + BK_C, BK_K3 = BK_BR + BK_C, BK_G3 = BK_K3 + 9 * BK_C * BK_C,
              BK_B3 = BK_G3 + BK_C, BK_POOL = BK_B3 + BK_C;
inline int64_t icnet_bneck_floats(int K) { return BK_POOL + icnet_pool_floats(K); }
// the frozen moving statistics: the reduce layer's mean [256] | variance [256] | the 3 x 3's mean [256] | variance [256] | the
// pooling trainer's rows
constexpr int BK_STATS_OWN = 4 * BK_C;
constexpr int BK_STATS = BK_STATS_OWN + PO_STATS;

// Geometry: conv5_2 [N, h32, w32, 1024], conv3_1 [N, 2 h32, 2 w32, 256], conv3_sub1 [N, 4 h32, 4 w32, 64].  max_workgroups
// lowers the FIRST grid index of every launch; the further indices it does not cap:
//   the data gradient through the increase layer   tiles of BK_DI_PT pixels (linear over [N, h32, w32]) strided over at most
//                                                  BK_DX_MAX_WG workgroups, times 2 slabs of 128 of its 256 input channels:
//                                                  grid (G, 2)
//   the data gradient through the dilated 3 x 3    tiles of BK_T x BK_T pixels of one image strided over at most BK_DX_MAX_WG
//                                                  workgroups, times 2 slabs of 128 input channels: grid (G, 2)
//   the 3 x 3 weight gradient                      split-K over tiles of PY_PT pixels, at most BK_W3_MAX_WG groups, times
//                                                  9 taps x 2 slabs of 128 input channels, times 2 slabs of 128 output
//                                                  channels: grid (G, 18, 2) -- 36 G workgroups run
//   the reduce layer's weight gradient             k_icnet_pyramid_wgrad's plan at 1024 x 256: grid (G, 8, 2), G <= PY_MAX_WG
constexpr int BK_DI_PT = 64;
constexpr int BK_T = 8;               // the 3 x 3 data gradient's tile: 8 x 8 pixels under a window of 16 x 16 (halo 4)
constexpr int BK_DX_MAX_WG = 1024;
constexpr int BK_W3_MAX_WG = 16;      // bounds the partials: 16 x BK_PART3 floats = 37.8 MB
constexpr int BK_PART3 = (9 * BK_C + 1) * BK_C;  // floats of one split-K partial: [9 taps][256 ci][256 co], then sum_p g3 [256]
constexpr int BK_PARTR = (BK_CIN + 1) * BK_C;    // the reduce layer's: [1024 ci, then sum_p gr][256 co]
// the pooling depth's guard: every kernel here indexes with 64 bits and strides its grid over 64-bit tile counts
bool icnet_bneck_fits(int h32, int w32);

struct IcnetBneckWs {
    float *wt_r;    // the reduce kernel in igemm_relayout's layout [1][32][256][32]
    float *wt_3;    // the 3 x 3 kernel in igemm_relayout's layout [9][8][256][32]
    float *rows;    // scale_r | shift_r | scale_3 | shift_3 (256 each)
    float *rd;      // [N, h32, w32, 256]  conv5_3_1x1_reduce
    float *a33;     // [N, h32, w32, 256]  conv5_3_3x3
    float *g3;      // [N, h32, w32, 256]  un-normalised dL/dconv5_3_3x3 behind its ReLU
    float *gr;      // [N, h32, w32, 256]  un-normalised dL/dconv5_3_1x1_reduce behind its ReLU
    float *part3;   // [BK_W3_MAX_WG][BK_PART3]
    float *fold3;   // [BK_PART3]
    float *partr;   // [PY_MAX_WG][BK_PARTR]
    float *foldr;   // [BK_PARTR]
    IcnetPoolWs pool;
};

// The backward of one Bneck(256, 1024, 1, 4) below its output gradient, as a link of a chain: the data
// gradient through the increase layer (k_icnet_bneck_dx_inc), the 3 x 3 weight gradient with its finish and gamma, the data
// gradient through the dilated 3 x 3 (k_icnet_bneck_dx_3x3) and the reduce layer's weight gradient
// (launch_icnet_wgrad_1024x256), in that order.  The increase layer's own weight gradient is the caller's.  What a block hands
// over: gr, un-normalised behind the reduce layer's ReLU -- the data gradient onto the block's input is the next depth's.
struct IcnetBneckLink {
    const float *x;                           // [N, h32, w32, 1024]  the block's input
    const float *rd, *a33;                    // [N, h32, w32, 256]   its stored 1x1_reduce and 3x3 (the fp32 forward values)
    const float *gout;                        // [N, h32, w32, 1024]  un-normalised dL/d(block output) behind its ReLU
    const float *Ki, *s_i;                    // the increase kernel [256][1024], its batch-norm scale [1024]
    const float *K3, *s_3, *mean_3, *var_3;   // the 3 x 3 kernel [9][256][256], its scale and moving statistics [256]
    const float *Kr, *s_r, *mean_r, *var_r;   // the reduce kernel [1024][256], its scale and moving statistics [256]
    const float *scale;                       // [1]  1 / sum(mask)
    float *g3, *gr, *part3, *fold3, *partr, *foldr;    // IcnetBneckWs's pieces of those names
    float *gK3, *gG3, *gB3, *gKr, *gGr, *gBr;          // the six gradient slots
    // the profile's names: dx_inc, wgrad3, finish3, gamma3, dx_3x3, then the reduce layer's wgrad, finish, gamma
    const char *const *names;
};
hipError_t launch_icnet_bneck_link(const IcnetBneckLink &L, int N, int h32, int w32, int max_workgroups, hipStream_t s);

// loss [1] float64; grad [icnet_bneck_floats(K)] fp32 in the packed order
hipError_t launch_icnet_bneck_grad(const float *c52, const float *c31, const float *c3, int N, int h32, int w32, int K,
                                   const float *params, const float *stats, const uint8_t *labels, const float *mask,
                                   float weight, float label_smoothing, int max_workgroups, const IcnetBneckWs &ws, double *loss,
                                   float *grad, hipStream_t s);

}  // namespace ssal
