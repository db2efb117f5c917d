// ssal_train_decoder.h -- training of ENet's whole decoder (Bottleneck4_0 + Bottleneck4_1 + Bottleneck4_2 + Bottleneck5_0 +
// Bottleneck5_1 + Final) over a frozen encoder (ssal_train_decoder.hip): Bottleneck4_0's part of the
// packed block and the launcher.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssal_train_tail.h"

namespace ssal {

// The decoder block = the two-block tail block of train_tail_floats(K, 2) floats (ssal_train_tail.h) followed by
// Bottleneck4_0's part of TD_FLOATS floats.  Float offsets INSIDE that part (include/ssal_enet.h, "Decoder training"): the
// order of ssal_train_stage.h with this block's sizes (128 -> 32 -> 16 -> 64); the gradient block and Adam's slots use the same
// layout; [TD_TRAINED, TD_FLOATS) holds the moving statistics (never written, gradient 0) and 8 floats of padding.
constexpr int TD_WP = 0;        // proj_kernel [128][32]
constexpr int TD_PG = 4096;     // proj_gamma [32]
constexpr int TD_PB = 4128;     // proj_beta [32]
constexpr int TD_PA = 4160;     // proj_alpha [32]
constexpr int TD_WC = 4192;     // conv_kernel [3][3][16][32] (transposed convolution: HW-O-I)
constexpr int TD_CG = 8800;     // conv_gamma [16]
constexpr int TD_CB = 8816;     // conv_beta [16]
constexpr int TD_CA = 8832;     // conv_alpha [16]
constexpr int TD_WE = 8848;     // exp_kernel [16][64]
constexpr int TD_EG = 9872;     // exp_gamma [64]
constexpr int TD_EB = 9936;     // exp_beta [64]
constexpr int TD_WR = 10000;    // res_kernel [128][64]
constexpr int TD_RA = 18192;    // residual_alpha [64]
constexpr int TD_TRAINED = 18256;
constexpr int TD_PM = 18256, TD_PV = 18288, TD_CM = 18320, TD_CV = 18336, TD_EM = 18352, TD_EV = 18416;  // mean / variance
constexpr int TD_FLOATS = 18488;

// the folded form k_td_fold writes (what launch_upsample_mfma and the backward kernel read next to the packed block)
constexpr int DF_PS = 0, DF_PT = 32;        // projection: s = gamma / sqrt(var + 1e-3), t = fma(-mean, s, beta)
constexpr int DF_CS = 64, DF_CT = 80;       // transposed convolution
constexpr int DF_ES = 96, DF_ET = 160;      // expansion
constexpr int DF_PI = 224, DF_CI = 256, DF_EI = 272;  // 1 / sqrt(var + 1e-3)
constexpr int DF_WS = 336;                  // parity-stacked transposed-convolution kernel [6][32][32] (stack_convT)
constexpr int DF_FLOATS = DF_WS + 6 * 32 * 32;

inline int64_t train_decoder_floats(int K) { return train_tail_floats(K, 2) + TD_FLOATS; }

// H, W = the dims of Bottleneck3_8's output (eighth resolution): the tail's limit on the quarter-resolution map [2H, 2W] and
// that of the fused 128-channel upsample kernel the forward runs on
bool train_decoder_fits(int H, int W);
// workgroups of Bottleneck4_0's gradient kernels: min(8 x 8 tiles of the eighth-resolution map, 1024, max_workgroups when > 0)
int train_decoder_workgroups(int H, int W, int max_workgroups);

// Workspace of one gradient call: the two-block tail workspace on the quarter-resolution map, a40 [N,2H,2W,64]
// (Bottleneck4_0's output; NULL when the caller supplies it elsewhere), dx40 [N,2H,2W,64] (dL/d a4_0 before the 1 / sum(mask)
// factor), dur [N,H,W,64] (dL/du gathered through the pooling indices), code2 [N,H,W,64] (NULL: the caller's), bad2 (one
// int), dfold [DF_FLOATS], part_d [G][TD_TRAINED].
struct TrainDecoderWs {
    TrainTailWs tt;
    float *a40, *dx40, *dur, *dfold, *part_d;
    uint8_t *code2;
    int *bad2;
};

// x38 [N,H,W,128] = Bottleneck3_8's output; argmax2 int64 [N,H,W,64] (per-image index into [2H,2W,64], Bottleneck2_0's
// pooling) is converted into ws.code2 first, or, when it is NULL, ws.code2 already holds the window codes; argmax1 as for
// launch_train_stage_grad on the [2H, 2W] map; params / grad: the decoder block of train_decoder_floats(K) floats; labels
// uint8 / mask fp32 [N,8H,8W]; loss one double.  k_td_fold, Bottleneck4_0 forward (launch_upsample_mfma, Cin = 128), the
// two-block tail on a4_0 with dx40, k_td_block, k_td_res, k_td_finish.
hipError_t launch_train_decoder_grad(const float *x38, const int64_t *argmax2, const int64_t *argmax1, int N, int H, int W,
                                     int K, const float *params, const uint8_t *labels, const float *mask, float weight,
                                     float label_smoothing, int max_workgroups, const TrainDecoderWs &ws, double *loss,
                                     float *grad, hipStream_t s, const TrainBlockSemi *semi = nullptr);

// The semi-supervised step with undistorted frames: Bottleneck4_0 of x38_raw through the scoring path's kernel into ws.a40,
// then launch_train_tail_targets (R = 2) on it.  Uses ws.a40, ws.code2 and ws.dfold, which launch_train_decoder_grad writes
// again afterwards.
hipError_t launch_train_decoder_targets(const float *x38_raw, const int64_t *argmax2_raw, const int64_t *argmax1_raw, int N,
                                        int H, int W, int K, const float *params, int max_workgroups,
                                        const TrainDecoderWs &ws, const TrainBlockSemi &semi, hipStream_t s);

}  // namespace ssal
