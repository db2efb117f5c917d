// ssal_train_icnet_fusion.h -- training of ICNet's last cascade-feature-fusion block together with the output layer over a
// frozen trunk: sub12_sum = relu(BN(conv_sub2(resize_2x(sub24_sum))) + BN(conv3_sub1_proj(conv3_sub1))), conv6_cls
// (ssal_train_icnet_fusion.hip).  gfx950 (MI355X / CDNA4) only.  All tensors fp32 NHWC.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssal_train_icnet.h"
#include "ssal_train_icnet_common.h"

namespace ssal {

// The packed vector everything here takes and gives (float offsets; FusionBlock<128>, ssal_train_icnet_common.h):
//   conv_sub2.kernel [3,3,128,128] | .gamma [128] | .beta [128] | conv3_sub1_proj.kernel [1,1,64,128] | .gamma | .beta |
//   conv6_cls.kernel [1,1,128,K] | conv6_cls.bias [K]
using FuBlock = FusionBlock<128>;
constexpr int FU_KA = FuBlock::KA, FU_GA = FuBlock::GA, FU_BA = FuBlock::BA, FU_KB = FuBlock::KB, FU_GB = FuBlock::GB,
              FU_BB = FuBlock::BB, FU_HEAD = FuBlock::END;
inline int64_t icnet_fusion_floats(int K) { return FU_HEAD + icnet_head_floats(K); }
// the frozen moving statistics travel next to it: conv_sub2 mean | variance | conv3_sub1_proj mean | variance
constexpr int FU_STATS = 4 * 128;

// Geometry: sub24_sum [N, h16, w16, 128], conv3_sub1 [N, h8, w8, 64] with h8 = 2 h16, w8 = 2 w16; the loss is taken on
// [N, 8 h8, 8 w8].  The weight-gradient kernel walks tiles of FU_TH x FU_TW pixels of sub12_sum.
constexpr int FU_TH = 4, FU_TW = 8;
constexpr int FU_TAPS = FuBlock::TAPS;           // the nine dilated taps, then the 1 x 1 branch (+ the row of ones: dBeta)
constexpr int FU_PART = FuBlock::PART;           // floats of one split-K partial: [tap][ci][co]
constexpr int FU_MAX_WG = FuBlock::MAX_WG;       // split-K groups the finish kernel folds (x FU_TAPS workgroups)
bool icnet_fusion_fits(int h16, int w16);
// split-K groups of a fusion block's weight gradient on a low-resolution input [n, h, w]: its FU_TH x FU_TW tiles of the output
template <int CIN>
inline int icnet_block_workgroups(int n, int h, int w, int max_workgroups)
{
    return icnet_grid((long)n * icnet_cdiv(2 * h, FU_TH) * icnet_cdiv(2 * w, FU_TW), FusionBlock<CIN>::MAX_WG, max_workgroups);
}

// The weight-gradient kernel at 256 input channels (the other fusion block): src [N, hs, ws, 256] is
// interpolated 2x on the fly, side [N, 2 hs, 2 ws, 256] is the 1 x 1 branch's input, g [N, 2 hs, 2 ws, 128].  Grid
// (G, CA_TAPS, 2): the third index picks the input-channel half; the row of ones (sum_p g) is an eleventh tap.
// part [G][CA_TAPS][256][128] ([G][tap][half][128][128]; tap 10 has its first half only, whose row 0 is sum_p g).
constexpr int CA_TAPS = FusionBlock<256>::TAPS;
hipError_t launch_icnet_fusion_wgrad256(const float *src, const float *side, const float *g, int N, int hs, int ws, int G,
                                        float *part, hipStream_t s);

struct IcnetFusionWs {
    float *wt_a;    // conv_sub2's kernel in igemm_relayout's layout [9][4][128][32]
    float *wt_b;    // conv3_sub1_proj's [1][2][128][32]
    float *rows;    // scale_a | shift_a | scale_b | shift_b (128 each)
    float *proj;    // [N, h8, w8, 128]   BN(conv3_sub1_proj(conv3_sub1))
    float *sub12;   // [N, h8, w8, 128]
    float *g;       // [N, h8, w8, 128]   un-normalised dL/dsub12_sum behind the ReLU
    float *hw;      // [N][icnet_head_tiles][36][K]
    float *part;    // [G][FU_PART]
    float *fold;    // [FU_PART] the folded partials, then the scale 1 / sum(mask)
    IcnetHeadWs head;
};

// loss [1] float64; grad [icnet_fusion_floats(K)] fp32 in the packed order.  semi (NULL = the plain
// step, launch for launch): handed to the head launch, which then builds the targets, counts the confusion replicas and the
// pseudo pixels; everything behind dL/dlogit is the plain step's.
hipError_t launch_icnet_fusion_grad(const float *sub24, const float *c3, int N, int h16, int w16, int K, const float *params,
                                    const float *stats, const uint8_t *labels, const float *mask, float weight,
                                    float label_smoothing, int max_workgroups, const IcnetFusionWs &ws, double *loss,
                                    float *grad, hipStream_t s, const IcnetHeadSemi *semi = nullptr);

// The target phase on the features of the undistorted frames: the pack, the block's two forward launches on them into
// ws.proj / ws.sub12, then launch_icnet_head_targets on that sub12_sum -> tgt [N, 16 h16, 16 w16], one packed byte per loss
// pixel of the unlabelled images.  The training features go through the same slots afterwards (launch_icnet_fusion_grad with
// semi.tgt_in = tgt).  semi.labelled NULL: no launch but the head's pack.
hipError_t launch_icnet_fusion_targets(const float *sub24_raw, const float *c3_raw, int N, int h16, int w16, int K,
                                       const float *params, const float *stats, int max_workgroups, const IcnetFusionWs &ws,
                                       const IcnetHeadSemi &semi, uint8_t *tgt, hipStream_t s);

}  // namespace ssal
