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

// The semi-supervised step.  labelled [N] uint8, NULL = all labelled: an image with labelled[n] == 0 is
// trained on its pseudo annotation (argmax / confidence >= threshold of its logits for `measure`, a code of ssal_enet.h) and
// its label / mask planes are never read.  use_tgt: the pseudo annotation is read from tgt [N,2H,2W] (a byte per output
// pixel: the label in bits 0..6, the mask in bit 7), which launch_train_block_targets wrote from the undistorted frame's
// features; otherwise it comes from the training logits.  rep [reps][conf_rep_stride(K * K)] u64 (NULL = no confusion
// matrix) must be zero on entry, the caller folds it with launch_confusion_fold; pseudo_pixels [N] (NULL = not counted) is
// zeroed by launch_train_block_grad.
struct TrainBlockSemi {
    const uint8_t *labelled;
    int measure;
    float threshold;
    uint8_t *tgt;
    bool use_tgt;
    unsigned long long *rep;
    int reps;
    int64_t *pseudo_pixels;
};

// x5 [N,H,W,16] = Bottleneck5_0's output; params / grad: the packed block of train_block_floats(K) floats; labels uint8 /
// mask fp32 [N,2H,2W]; loss one double.  dx (may be NULL) [N,H,W,16]: the block's input gradient dL/d x5, before the
// 1 / sum(mask) factor (what the last-stage trainer goes on from, ssal_train_stage.h); max_workgroups > 0 lowers the
// workgroup count below train_block_workgroups(H, W).  Neither changes a bit of loss or grad at the default count.
// semi (may be NULL: the plain step, whose launches are unchanged): labels / mask may then be NULL when no image is labelled.
hipError_t launch_train_block_grad(const float *x5, int N, int H, int W, int K, const float *params, const uint8_t *labels,
                                   const float *mask, float weight, float label_smoothing, const TrainBlockWs &ws,
                                   double *loss, float *grad, hipStream_t s, float *dx = nullptr, int max_workgroups = 0,
                                   const TrainBlockSemi *semi = nullptr);

// The target-only launch of the head kernel: the packed pseudo targets of the unlabelled images of x5_raw [N,H,W,16] (the
// undistorted frames' Bottleneck5_0 output) -> semi.tgt.  Uses ws.fold only; stream-ordered before launch_train_block_grad.
hipError_t launch_train_block_targets(const float *x5_raw, int N, int H, int W, int K, const float *params,
                                      const TrainBlockSemi &semi, const TrainBlockWs &ws, hipStream_t s,
                                      int max_workgroups = 0);

}  // namespace ssal
