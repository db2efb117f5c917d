// ssal_train_stage.h -- training of ENet's last decoder stage (Bottleneck5_0 + Bottleneck5_1 + Final) over a frozen trunk
// (ssal_train_stage.hip): the packed stage block and the launcher.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssal_train_block.h"

namespace ssal {

// The stage block = the last-block block of train_block_floats(K) floats (ssal_train_block.h) followed by Bottleneck5_0's
// part of TS_FLOATS floats.  Float offsets INSIDE that part (include/ssal_enet.h, "Last-stage training"); the gradient
// block and Adam's slots use the same layout; [TS_TRAINED, TS_FLOATS) holds the moving statistics (never written,
// gradient 0) and 8 floats of padding.
constexpr int TS_WP = 0;        // proj_kernel [64][16]
constexpr int TS_PG = 1024;     // proj_gamma [16]
constexpr int TS_PB = 1040;     // proj_beta [16]
constexpr int TS_PA = 1056;     // proj_alpha [16]
constexpr int TS_WC = 1072;     // conv_kernel [3][3][8][16] (transposed convolution: HW-O-I)
constexpr int TS_CG = 2224;     // conv_gamma [8]
constexpr int TS_CB = 2232;     // conv_beta [8]
constexpr int TS_CA = 2240;     // conv_alpha [8]
constexpr int TS_WE = 2248;     // exp_kernel [8][16]
constexpr int TS_EG = 2376;     // exp_gamma [16]
constexpr int TS_EB = 2392;     // exp_beta [16]
constexpr int TS_WR = 2408;     // res_kernel [64][16]
constexpr int TS_RA = 3432;     // residual_alpha [16]
constexpr int TS_TRAINED = 3448;
constexpr int TS_PM = 3448, TS_PV = 3464, TS_CM = 3480, TS_CV = 3488, TS_EM = 3496, TS_EV = 3512;  // mean / variance
constexpr int TS_FLOATS = 3536;

// the folded form k_ts_fold writes (what launch_upsample_mfma and the backward kernel read next to the packed block)
constexpr int TF_PS = 0, TF_PT = 16;      // projection: s = gamma / sqrt(var + 1e-3), t = fma(-mean, s, beta)
constexpr int TF_CS = 32, TF_CT = 40;     // transposed convolution
constexpr int TF_ES = 48, TF_ET = 64;     // expansion
constexpr int TF_PI = 80, TF_CI = 96, TF_EI = 104;  // 1 / sqrt(var + 1e-3)
constexpr int TF_WS = 128;                // parity-stacked transposed-convolution kernel [6][16][16] (stack_convT)
constexpr int TF_FLOATS = TF_WS + 6 * 16 * 16;

inline int64_t train_stage_floats(int K) { return train_block_floats(K) + TS_FLOATS; }

// H, W = the dims of Bottleneck4_2's output (quarter resolution); the half-resolution map is [2H, 2W]
bool train_stage_fits(int H, int W);
// workgroups of a call: min(tiles of the half-resolution map, 1024, max_workgroups when that is > 0)
int train_stage_workgroups(int H, int W, int max_workgroups);

// Workspace of one gradient call: the last-block workspace on the half-resolution map, a5_0 [N,2H,2W,16] (Bottleneck5_0's
// output; NULL when the caller supplies it elsewhere), dx [N,2H,2W,16] (dL/d a5_0 before the 1 / sum(mask) factor),
// code [N,H,W,16], bad (one int), sfold [TF_FLOATS], part_s [G][TS_TRAINED].
struct TrainStageWs {
    TrainBlockWs tb;
    float *a5, *dx, *sfold, *part_s;
    uint8_t *code;
    int *bad;
};

// x4 [N,H,W,64] = Bottleneck4_2's output; argmax int64 [N,H,W,16] (per-image index into [2H,2W,16]) is converted into
// ws.code first, or, when it is NULL, ws.code already holds the window codes; params / grad: the stage block of
// train_stage_floats(K) floats; labels uint8 / mask fp32 [N,4H,4W]; loss one double.  dx4 (may be NULL) [N,H,W,64]: the
// stage's input gradient dL/d x4, before the 1 / sum(mask) factor (what the decoder-tail trainer goes on from,
// ssal_train_tail.h); it changes no bit of loss or grad.
hipError_t launch_train_stage_grad(const float *x4, const int64_t *argmax, int N, int H, int W, int K, const float *params,
                                   const uint8_t *labels, const float *mask, float weight, float label_smoothing,
                                   int max_workgroups, const TrainStageWs &ws, double *loss, float *grad, hipStream_t s,
                                   const TrainBlockSemi *semi = nullptr, float *dx4 = nullptr);

// The semi-supervised step with undistorted frames (semi as in ssal_train_block.h, on the [2H, 2W] map): x4_raw [N,H,W,64]
// and argmax_raw (NULL: ws.code already holds the raw frame's window codes) -> the packed pseudo targets semi.tgt
// [N,4H,4W].  Uses ws.code, ws.a5, ws.sfold and ws.tb.fold, all of which launch_train_stage_grad writes again afterwards.
hipError_t launch_train_stage_targets(const float *x4_raw, const int64_t *argmax_raw, int N, int H, int W, int K,
                                      const float *params, int max_workgroups, const TrainStageWs &ws,
                                      const TrainBlockSemi &semi, hipStream_t s);

}  // namespace ssal
