// ssal_train_icnet_cascade.h -- training of ICNet's whole cascade head over frozen branches: sub24_sum = relu(BN(conv_sub4(
// resize_2x(conv5_4_k1))) + BN(conv3_1_sub2_proj(conv3_1))), then the last fusion block and conv6_cls of
// ssal_train_icnet_fusion.h (ssal_train_icnet_cascade.hip).  gfx950 (MI355X / CDNA4) only.  All tensors
// fp32 NHWC.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssal_train_icnet_fusion.h"

namespace ssal {

// The packed vector everything here takes and gives (float offsets; FusionBlock<256>, ssal_train_icnet_common.h):
//   conv_sub4.kernel [3,3,256,128] | .gamma [128] | .beta [128] | conv3_1_sub2_proj.kernel [1,1,256,128] | .gamma | .beta |
//   the fusion trainer's packed vector (ssal_train_icnet_fusion.h)
using CaBlock = FusionBlock<256>;
constexpr int CA_KC = CaBlock::KA, CA_GC = CaBlock::GA, CA_BC = CaBlock::BA, CA_KD = CaBlock::KB, CA_GD = CaBlock::GB,
              CA_BD = CaBlock::BB, CA_FUSION = CaBlock::END;
inline int64_t icnet_cascade_floats(int K) { return CA_FUSION + icnet_fusion_floats(K); }
// the frozen moving statistics: conv_sub4 mean | variance | conv3_1_sub2_proj mean | variance | the fusion trainer's four
constexpr int CA_STATS = 4 * 128 + FU_STATS;

// Geometry: conv5_4_k1 [N, h32, w32, 256], conv3_1 [N, 2 h32, 2 w32, 256], conv3_sub1 [N, 4 h32, 4 w32, 64]; the loss is
// taken on [N, 32 h32, 32 w32].  k_icnet_cascade_dx walks tiles of CA_DX_TH x CA_DX_TW pixels of du (1/8 resolution).
constexpr int CA_DX_TH = 8, CA_DX_TW = 16;
constexpr int CA_DX_MAX_WG = 2048;                  // workgroups of the data-gradient launch (tiles are strided over them)
constexpr int CA_PART = CaBlock::PART;              // floats of one split-K partial: [tap][ci][co]
constexpr int CA_MAX_WG = CaBlock::MAX_WG;          // split-K groups the finish kernel folds (x CA_TAPS x 2 workgroups)
bool icnet_cascade_fits(int h32, int w32);

// The two backward kernels of this block at 256 channels, for the layer below it (the profile's k_icnet_pyramid_dx /
// k_icnet_pyramid_g32).  k_icnet_cascade_dx<256>: the data gradient through conv_sub4, g24 [N, h16, w16,
// 128] (un-normalised, behind sub24_sum's ReLU), Kc [3,3,256,128], sc [128] its batch-norm scale -> du [N, h16, w16, 256]; grid
// (tiles strided, 2 halves of the input channels); one accumulator adds its 9 * 128 products in the order (quarter of co, tap,
// co).  k_icnet_cascade_g24<256>: the adjoint of the legacy 2x resize h16 -> h32 with the ReLU mask of f1 = conv5_4_k1
// [N, h32, w32, 256] -> g32, each element its at most 3 x 3 terms, rows then columns ascending.
// max_workgroups caps grid.x only: the data gradient launches 2 x that many workgroups.
hipError_t launch_icnet_cascade_dx256(const float *g24, const float *Kc, const float *sc, int N, int h16, int w16,
                                      int max_workgroups, float *du, hipStream_t s);
hipError_t launch_icnet_cascade_g32(const float *du, const float *f1, int N, int h32, int w32, int max_workgroups, float *g32,
                                    hipStream_t s);

struct IcnetCascadeWs {
    float *wt_c;    // conv_sub4's kernel in igemm_relayout's layout [9][8][128][32]
    float *wt_d;    // conv3_1_sub2_proj's [1][8][128][32]
    float *rows;    // scale_c | shift_c | scale_d | shift_d (128 each)
    float *proj;    // [N, h16, w16, 128]  BN(conv3_1_sub2_proj(conv3_1))
    float *sub24;   // [N, h16, w16, 128]
    float *du;      // [N, h8, w8, 128]    un-normalised dL/d(resize_2x(sub24_sum))
    float *g24;     // [N, h16, w16, 128]  un-normalised dL/dsub24_sum behind the ReLU
    float *part;    // [G][CA_PART]
    float *fold;    // [CA_PART]
    IcnetFusionWs fusion;
};

// loss [1] float64; grad [icnet_cascade_floats(K)] fp32 in the packed order.  semi (NULL = the plain
// step, launch for launch): handed on to launch_icnet_fusion_grad
hipError_t launch_icnet_cascade_grad(const float *c54, const float *c31, const float *c3, int N, int h32, int w32, int K,
                                     const float *params, const float *stats, const uint8_t *labels, const float *mask,
                                     float weight, float label_smoothing, int max_workgroups, const IcnetCascadeWs &ws,
                                     double *loss, float *grad, hipStream_t s, const IcnetHeadSemi *semi = nullptr);

// The target phase on the features of the undistorted frames: the pack and this block's two forward launches on them into
// ws.proj / ws.sub24, then launch_icnet_fusion_targets on that sub24_sum -> tgt [N, 32 h32, 32 w32].  The training features go
// through the same slots afterwards (launch_icnet_cascade_grad with semi.tgt_in = tgt).
hipError_t launch_icnet_cascade_targets(const float *c54_raw, const float *c31_raw, const float *c3_raw, int N, int h32,
                                        int w32, int K, const float *params, const float *stats, int max_workgroups,
                                        const IcnetCascadeWs &ws, const IcnetHeadSemi &semi, uint8_t *tgt, hipStream_t s);

}  // namespace ssal
