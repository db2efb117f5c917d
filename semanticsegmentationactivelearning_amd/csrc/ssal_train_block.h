// ssal_train_block.h -- training of ENet's last block (Bottleneck5_1 + Final) over a frozen trunk (ssal_train_block.hip,
// DESIGN.md section 17): the packed parameter / gradient block and the launcher.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ssal {

// Float offsets of the packed block (include/ssal_enet.h, "Last-block training").  The gradient block and Adam's slots use
// the same layout; [TB_TRAINED, TB_FINAL) holds the moving statistics (never written, gradient 0) and 8 floats of padding.
constexpr int TB_WP = 0;        // proj_kernel [16][4]
constexpr int TB_PG = 64;       // proj_gamma [4]
constexpr int TB_PB = 68;       // proj_beta [4]
constexpr int TB_PA = 72;       // proj_alpha [4]
constexpr int TB_WC = 76;       // conv_kernel [3][3][4][4]
constexpr int TB_CG = 220;      // conv_gamma [4]
constexpr int TB_CB = 224;      // conv_beta [4]
constexpr int TB_CA = 228;      // conv_alpha [4]
constexpr int TB_WE = 232;      // exp_kernel [4][16]
constexpr int TB_EG = 296;      // exp_gamma [16]
constexpr int TB_EB = 312;      // exp_beta [16]
constexpr int TB_RA = 328;      // residual_alpha [16]
constexpr int TB_TRAINED = 344;
constexpr int TB_PM = 344, TB_PV = 348, TB_CM = 352, TB_CV = 356, TB_EM = 360, TB_EV = 376;  // mean / variance
constexpr int TB_FINAL = 400;   // Final.kernel [3][3][K][16]
constexpr int TB_ROWS = 3;      // partial rows per workgroup of the block's backward (pixel thirds of the contractions)

inline int64_t train_block_floats(int K) { return TB_FINAL + 144 * (int64_t)K; }

// the limits and the workgroup count are those of the output-layer gradient (16 x 16 feature tiles, at most 1024 workgroups)
bool train_block_fits(int H, int W);
int train_block_workgroups(int H, int W);

// Workspace of one gradient call: fold [TB_FINAL] (the block with batch-norm folded), dy [N,H,W,16] (dL/d Bottleneck5_1's
// output, before the 1 / sum(mask) factor), part_f [G][144 K], part_b [TB_ROWS G][TB_TRAINED], lpart [G][2].
struct TrainBlockWs {
    float *fold, *dy, *part_f, *part_b;
    double *lpart;
};

// x5 [N,H,W,16] = Bottleneck5_0's output; params / grad: the packed block of train_block_floats(K) floats; labels uint8 /
// mask fp32 [N,2H,2W]; loss one double.  dx (may be NULL) [N,H,W,16]: the block's input gradient dL/d x5, before the
// 1 / sum(mask) factor (what the last-stage trainer goes on from, ssal_train_stage.h); max_workgroups > 0 lowers the
// workgroup count below train_block_workgroups(H, W).  Neither changes a bit of loss or grad at the default count.
hipError_t launch_train_block_grad(const float *x5, int N, int H, int W, int K, const float *params, const uint8_t *labels,
                                   const float *mask, float weight, float label_smoothing, const TrainBlockWs &ws,
                                   double *loss, float *grad, hipStream_t s, float *dx = nullptr, int max_workgroups = 0);

}  // namespace ssal
