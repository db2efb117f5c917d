// ssal_train_tail.h -- training of ENet's decoder tail (Bottleneck4_2 + Bottleneck5_0 + Bottleneck5_1 + Final) over a frozen
// trunk (ssal_train_tail.hip): the packed tail block and the launcher.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssal_train_stage.h"

namespace ssal {

// The tail block = the stage block of train_stage_floats(K) floats (ssal_train_stage.h) followed by Bottleneck4_2's part of
// TT_FLOATS floats.  Float offsets INSIDE that part (include/ssal_enet.h, "Decoder-tail training"); the gradient block and
// Adam's slots use the same layout; [TT_TRAINED, TT_FLOATS) holds the moving statistics (never written, gradient 0) and 8
// floats of padding.  The layout is that of a regular 64 -> 16 -> 16 -> 64 bottleneck, whichever layer it belongs to.
constexpr int TT_WP = 0;        // proj_kernel [64][16]
constexpr int TT_PG = 1024;     // proj_gamma [16]
constexpr int TT_PB = 1040;     // proj_beta [16]
constexpr int TT_PA = 1056;     // proj_alpha [16]
constexpr int TT_WC = 1072;     // conv_kernel [3][3][16][16] (HWIO)
constexpr int TT_CG = 3376;     // conv_gamma [16]
constexpr int TT_CB = 3392;     // conv_beta [16]
constexpr int TT_CA = 3408;     // conv_alpha [16]
constexpr int TT_WE = 3424;     // exp_kernel [16][64]
constexpr int TT_EG = 4448;     // exp_gamma [64]
constexpr int TT_EB = 4512;     // exp_beta [64]
constexpr int TT_RA = 4576;     // residual_alpha [64]
constexpr int TT_TRAINED = 4640;
constexpr int TT_PM = 4640, TT_PV = 4656, TT_CM = 4672, TT_CV = 4688, TT_EM = 4704, TT_EV = 4768;  // mean / variance
constexpr int TT_FLOATS = 4840;

// the folded form k_tt_fold writes (what launch_bottleneck_mfma and the backward kernel read next to the packed block)
constexpr int TG_PS = 0, TG_PT = 16, TG_PI = 32;      // projection: s = gamma / sqrt(var + 1e-3), t = fma(-mean, s, beta), 1 / sqrt(var + 1e-3)
constexpr int TG_CS = 48, TG_CT = 64, TG_CI = 80;     // convolution
constexpr int TG_ES = 96, TG_ET = 160, TG_EI = 224;   // expansion
constexpr int TG_FLOATS = 288;

inline int64_t train_tail_floats(int K) { return train_stage_floats(K) + TT_FLOATS; }
// R regular blocks above the stage (R = 1: Bottleneck4_2; R = 2: Bottleneck4_1 below it): the tail block
// is a prefix and every further block's part of TT_FLOATS floats follows it
inline int64_t train_tail_floats(int K, int R) { return train_stage_floats(K) + (int64_t)R * TT_FLOATS; }

// H, W = the dims of Bottleneck4_1's output (quarter resolution): the stage's limit and that of the fused 64-channel
// bottleneck kernel the forward runs on
bool train_tail_fits(int H, int W);

// Workspace of one gradient call: the stage workspace, a42 [N,H,W,64] (Bottleneck4_2's output; NULL when the caller supplies
// it elsewhere), dx4 [N,H,W,64] (dL/d a4_2 before the 1 / sum(mask) factor), tfold [TG_FLOATS], part_t [G][TT_TRAINED].
// R = 2 adds the same four for Bottleneck4_1: a41 (its output), dx41 (dL/d a4_1, as dx4), tfold2, part_t2; NULL with R = 1.
struct TrainTailWs {
    TrainStageWs ts;
    float *a42, *dx4, *tfold, *part_t;
    float *a41, *dx41, *tfold2, *part_t2;
};

// x [N,H,W,64] = the input of the lowest trained block: Bottleneck4_1's output (R = 1) or Bottleneck4_0's (R = 2); argmax as
// for launch_train_stage_grad; params / grad: the block of train_tail_floats(K, R) floats; labels uint8 / mask fp32 [N,4H,4W];
// loss one double.  R = 2: Bottleneck4_1 and 4_2 forward, the stage, k_tt_block<true> on (a4_1, dx4) -> dx41, k_tt_block<false>
// on (x, dx41), k_tt_finish per block.  dx_low (may be NULL) [N,H,W,64]: the lowest block's launch is k_tt_block<true> too and
// writes its input gradient dL/dx there, before the 1 / sum(mask) factor (what the decoder trainer goes on from,
// ssal_train_decoder.h); it changes no bit of loss or grad.
hipError_t launch_train_tail_grad(const float *x, const int64_t *argmax, int N, int H, int W, int K, const float *params,
                                  const uint8_t *labels, const float *mask, float weight, float label_smoothing,
                                  int max_workgroups, const TrainTailWs &ws, double *loss, float *grad, hipStream_t s,
                                  const TrainBlockSemi *semi = nullptr, int R = 1, float *dx_low = nullptr);

// The semi-supervised step with undistorted frames: Bottleneck4_2 of x41_raw through the scoring path's kernel into ws.a42,
// then launch_train_stage_targets on it.  Uses ws.a42 and ws.tfold, which launch_train_tail_grad writes again afterwards.
// R = 2: x_raw is Bottleneck4_0 of the undistorted frames and Bottleneck4_1 runs first, into ws.a41 (with ws.tfold2).
hipError_t launch_train_tail_targets(const float *x_raw, const int64_t *argmax_raw, int N, int H, int W, int K,
                                     const float *params, int max_workgroups, const TrainTailWs &ws,
                                     const TrainBlockSemi &semi, hipStream_t s, int R = 1);

}  // namespace ssal
