// ssal_train_icnet_pyramid.h -- training of ICNet's pyramid head: conv5_4_k1 = relu(BN(1 x 1 conv (1024 -> 256) of
// conv5_3_sum)), the low-resolution branch's only path into the cascade, then the whole cascade head of
// ssal_train_icnet_cascade.h, over everything up to the pyramid-pooling sum and the two other frozen branches
// (ssal_train_icnet_pyramid.hip).  gfx950 (MI355X / CDNA4) only.  All tensors fp32 NHWC.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssal_train_icnet_cascade.h"

namespace ssal {

// The packed vector everything here takes and gives (float offsets):
//   conv5_4_k1.kernel [1,1,1024,256] | .gamma [256] | .beta [256] | the cascade trainer's packed vector
constexpr int PY_CIN = 1024, PY_CO = 256;
constexpr int PY_K = 0, PY_G = PY_CIN * PY_CO, PY_B = PY_G + PY_CO, PY_CASCADE = PY_B + PY_CO;
inline int64_t icnet_pyramid_floats(int K) { return PY_CASCADE + icnet_cascade_floats(K); }
// the frozen moving statistics: conv5_4_k1 mean [256] | variance [256] | the cascade trainer's eight rows of 128
constexpr int PY_STATS_OWN = 2 * PY_CO;
constexpr int PY_STATS = PY_STATS_OWN + CA_STATS;

// Geometry: conv5_3_sum [N, h32, w32, 1024], conv3_1 [N, 2 h32, 2 w32, 256], conv3_sub1 [N, 4 h32, 4 w32, 64].  The weight
// gradient is split-K over tiles of PY_PT pixels of conv5_4_k1, at most PY_MAX_WG groups (tiles strided over them), and over
// the 1024 x 256 output in 8 x 2 slabs of 128 x 128: grid (G, 8, 2).  max_workgroups lowers G only: 16 G workgroups run.
constexpr int PY_PT = 32;
constexpr int PY_MAX_WG = 16;
constexpr int PY_PART = (PY_CIN + 1) * PY_CO;  // floats of one split-K partial: [1024 ci, then sum_p g32][256 co]
// the cascade's guard: every kernel here indexes with 64 bits and strides its grid over 64-bit tile counts
bool icnet_pyramid_fits(int h32, int w32);

struct IcnetPyramidWs {
    float *wt;      // conv5_4_k1's kernel in igemm_relayout's layout [1][32][256][32]
    float *rows;    // scale | shift (256 each)
    float *f1;      // [N, h32, w32, 256]  conv5_4_k1
    float *du;      // [N, h16, w16, 256]  un-normalised dL/d(resize_2x(conv5_4_k1))
    float *g32;     // [N, h32, w32, 256]  un-normalised dL/dconv5_4_k1 behind the ReLU
    float *part;    // [PY_MAX_WG][PY_PART]
    float *fold;    // [PY_PART]
    IcnetCascadeWs cascade;
};

// loss [1] float64; grad [icnet_pyramid_floats(K)] fp32 in the packed order
hipError_t launch_icnet_pyramid_grad(const float *c53, const float *c31, const float *c3, int N, int h32, int w32, int K,
                                     const float *params, const float *stats, const uint8_t *labels, const float *mask,
                                     float weight, float label_smoothing, int max_workgroups, const IcnetPyramidWs &ws,
                                     double *loss, float *grad, hipStream_t s);

// k_icnet_pyramid_wgrad, its finish and its gamma kernel at 256 x 1024, for the layer below the pyramid pooling (DESIGN.md
// section 41; the profile's k_icnet_pool_wgrad / _finish / _gamma): x [pixels, 256], g [pixels, 1024] (un-normalised, behind the
// layer's ReLU, without its batch-norm scale), scale [1] = 1 / sum(mask), sl [1024] the layer's batch-norm scale, K [256][1024],
// mean / var [1024] -> part [PY_MAX_WG][257 * 1024], fold [257 * 1024], gK [256][1024], gG, gB [1024].  Grid (G, 2, 8):
// max_workgroups lowers G only, 16 G workgroups run.
hipError_t launch_icnet_wgrad_256x1024(const float *x, const float *g, long pixels, int max_workgroups, const float *scale,
                                       const float *sl, const float *K, const float *mean, const float *var, float *part,
                                       float *fold, float *gK, float *gG, float *gB, hipStream_t s,
                                       const char *const *names = nullptr);

// the same three kernels at 1024 x 256 (conv5_4_k1's own instantiations) for conv5_3's reduce layer (the
// profile's k_icnet_bneck_wgrad_r / _finish_r / _gamma_r): x [pixels, 1024], g [pixels, 256], sl / mean / var [256], K [1024][256]
// -> part [PY_MAX_WG][PY_PART], fold [PY_PART], gK [1024][256], gG, gB [256].  Grid (G, 8, 2): max_workgroups lowers G only.
// names (either launcher): the profile's names of the three launches where a further layer of the shape runs them (DESIGN.md
// section 43), else the ones above.
hipError_t launch_icnet_wgrad_1024x256(const float *x, const float *g, long pixels, int max_workgroups, const float *scale,
                                       const float *sl, const float *K, const float *mean, const float *var, float *part,
                                       float *fold, float *gK, float *gG, float *gB, hipStream_t s,
                                       const char *const *names = nullptr);

}  // namespace ssal
