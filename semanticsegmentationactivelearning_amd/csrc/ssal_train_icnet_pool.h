// ssal_train_icnet_pool.h -- training of ICNet through its pyramid pooling: conv5_3 = relu(BN(1 x 1 conv (256 -> 1024) of
// conv5_3_3x3) + conv5_2), the increase layer of the backbone's last bottleneck, the parameter-free pyramid pooling over it, then
// the whole pyramid head of ssal_train_icnet_pyramid.h, over everything below conv5_3_3x3 and conv5_2 and the two other frozen
// branches (ssal_train_icnet_pool.hip).  gfx950 (MI355X / CDNA4) only.  All tensors fp32 NHWC.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssal_train_icnet_pyramid.h"

namespace ssal {

// The packed vector everything here takes and gives (float offsets):
//   conv5_3_1x1_increase.kernel [1,1,256,1024] | .gamma [1024] | .beta [1024] | the pyramid trainer's packed vector
constexpr int PO_CIN = 256, PO_CO = 1024;
constexpr int PO_K = 0, PO_G = PO_CIN * PO_CO, PO_B = PO_G + PO_CO, PO_PYRAMID = PO_B + PO_CO;
inline int64_t icnet_pool_floats(int K) { return PO_PYRAMID + icnet_pyramid_floats(K); }
// the frozen moving statistics: the increase layer's mean [1024] | variance [1024] | the pyramid trainer's rows
constexpr int PO_STATS_OWN = 2 * PO_CO;
constexpr int PO_STATS = PO_STATS_OWN + PY_STATS;

// Geometry: conv5_3_3x3 [N, h32, w32, 256], conv5_2 [N, h32, w32, 1024], conv3_1 [N, 2 h32, 2 w32, 256], conv3_sub1
// [N, 4 h32, 4 w32, 64].  The data gradient through conv5_4_k1 takes tiles of PO_DX_PT pixels (linear over [N, h32, w32]),
// strided over at most PO_DX_MAX_WG workgroups, times 8 slabs of 128 of its 1024 input channels: grid (G, 8).  The weight
// gradient is k_icnet_pyramid_wgrad's plan at 256 x 1024: grid (G, 2, 8), G <= PY_MAX_WG.  max_workgroups lowers the first index.
constexpr int PO_DX_PT = 64;
constexpr int PO_DX_MAX_WG = 1024;
constexpr int PO_PART = (PO_CIN + 1) * PO_CO;  // floats of one split-K partial: [256 ci, then sum_p g53][1024 co]
constexpr int PO_SLOTS = 50;                   // bins of the four levels: 1 + 4 + 9 + 36
constexpr int PO_CSLOTS = 12;                  // bin columns of the four levels: 1 + 2 + 3 + 6
// the pyramid depth's guard: every kernel here indexes with 64 bits and strides its grid over 64-bit tile counts
bool icnet_pool_fits(int h32, int w32);

struct IcnetPoolWs {
    float *wt;      // the increase kernel in igemm_relayout's layout [1][8][1024][32]
    float *rows;    // scale | shift (1024 each)
    float *c53;     // [N, h32, w32, 1024]  conv5_3
    float *sum;     // [N, h32, w32, 1024]  conv5_3_sum
    float *pooled;  // launch_ppm's scratch (ppm_scratch_floats)
    float *dsum;    // [N, h32, w32, 1024]  un-normalised dL/dconv5_3_sum
    float *cols;    // [N, h32, PO_CSLOTS, 1024]  the resize adjoint's column sums, row by row
    float *gb;      // [N, PO_SLOTS, 1024]  the bin gradients, divided by the bin's pixel count
    float *g53;     // [N, h32, w32, 1024]  un-normalised dL/dconv5_3 behind the ReLU
    float *part;    // [PY_MAX_WG][PO_PART]
    float *fold;    // [PO_PART]
    IcnetPyramidWs pyramid;
};

// loss [1] float64; grad [icnet_pool_floats(K)] fp32 in the packed order
hipError_t launch_icnet_pool_grad(const float *a33, const float *c52, const float *c31, const float *c3, int N, int h32, int w32,
                                  int K, const float *params, const float *stats, const uint8_t *labels, const float *mask,
                                  float weight, float label_smoothing, int max_workgroups, const IcnetPoolWs &ws, double *loss,
                                  float *grad, hipStream_t s);

}  // namespace ssal
