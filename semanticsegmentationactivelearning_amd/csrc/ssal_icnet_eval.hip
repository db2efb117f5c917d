// ssal_icnet_eval.hip -- the evaluation form of ICNet's up-sampling score kernel (k_upscore, ssal_icnet_kernels.hip):
// conv6_interp (4x bilinear) + argmax + masked confusion matrix in one launch, gfx950.  A sibling kernel in a file of its
// own: k_upscore's 62 instantiations are not touched by it (DESIGN.md section 27 holds both resource tables).
#include "ssal_confusion.h"
#include "ssal_icnet.h"
#include "ssal_internal.h"
#include "ssal_prof.h"

namespace ssal {

// lq = 1/4-resolution logits [N,H,W,K]; gt_label / gt_mask uint8 [N,4H,4W] (gt_mask NULL = weight 1), both 4-byte aligned.
// The geometry is k_upscore's: one thread per 1/4-resolution pixel = one 4 x 4 block of output pixels, 256 consecutive
// 1/4-resolution pixels of one image per workgroup (UPEVAL_TILE), grid = (ceil(H*W / 256), N).  The interpolated logit of
// class k at (dx, dy) is k_upscore's expression, operation for operation:
//     top = tl + (tr - tl) * lx,  bot = bl + (br - bl) * lx,  l = top + (bot - top) * ly
// and the prediction is pixel_score's first maximum (`l[k] > m`, k ascending), so it is the label plane's byte.  What
// differs is the loop order: the classes are the OUTER loop and the 16 running (maximum, index) pairs live in registers, so
// a thread holds 4 corner values at a time instead of 4 * K -- no softmax, no measure, no fp64 partials, no output plane.
// Every output pixel adds its mask value at (gt label, prediction) of the workgroup's u32 LDS histogram (ssal_confusion.h:
// wave-level aggregation, keys >= K * K dropped); the non-zero entries leave as u64 integer atomics into replica
// (workgroup % reps).  Threads past the image carry weight 0 and take part in the wave-level rounds.
constexpr int UPEVAL_TILE = 256;

template <int K>
__global__ __launch_bounds__(UPEVAL_TILE) void k_upeval(const float *__restrict__ lq, int H, int W,
                                                        const uint8_t *__restrict__ gt_label,
                                                        const uint8_t *__restrict__ gt_mask,
                                                        unsigned long long *__restrict__ rep, int reps)
{
    __shared__ unsigned hist[K * K];
    hist_zero(hist, K * K);
    const int n = blockIdx.y;
    const long HW = (long)H * W;
    const long q = (long)blockIdx.x * UPEVAL_TILE + threadIdx.x;
    const bool live = q < HW;
    const long qc = live ? q : HW - 1;  // a thread past the image reads the last pixel's logits and counts nothing
    const int qx = (int)(qc % W), qy = (int)(qc / W);
    const int qx1 = min(qx + 1, W - 1), qy1 = min(qy + 1, H - 1);
    // the ground truth of the 4 x 4 block first (one 4-byte load per row and plane), so that it arrives under the logits
    unsigned gl[4] = {0u, 0u, 0u, 0u}, gm[4] = {0u, 0u, 0u, 0u};
    if (live) {
        const int OW = 4 * W;
        const long obase = (long)n * 16 * HW + (long)(4 * qy) * OW + 4 * qx;
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            const long o = obase + (long)dy * OW;
            gl[dy] = *reinterpret_cast<const unsigned *>(gt_label + o);
            gm[dy] = gt_mask ? *reinterpret_cast<const unsigned *>(gt_mask + o) : 0x01010101u;
        }
    }
    const float *img = lq + (long)n * HW * K;
    const float *ptl = img + ((long)qy * W + qx) * K, *ptr_ = img + ((long)qy * W + qx1) * K;
    const float *pbl = img + ((long)qy1 * W + qx) * K, *pbr = img + ((long)qy1 * W + qx1) * K;
    float m[16];
    unsigned am[16];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float tl = ptl[k], tr = ptr_[k], bl = pbl[k], br = pbr[k];
#pragma unroll
        for (int dx = 0; dx < 4; ++dx) {
            const float lx = 0.25f * (float)dx;
            const float top = tl + (tr - tl) * lx;
            const float bot = bl + (br - bl) * lx;
#pragma unroll
            for (int dy = 0; dy < 4; ++dy) {
                const float ly = 0.25f * (float)dy;
                const float l = top + (bot - top) * ly;
                const int p = 4 * dy + dx;
                if (k == 0) {
                    m[p] = l;
                    am[p] = 0u;
                } else if (l > m[p]) {
                    m[p] = l;
                    am[p] = (unsigned)k;
                }
            }
        }
    }
    __syncthreads();  // the histogram is zero
#pragma unroll
    for (int dy = 0; dy < 4; ++dy)
#pragma unroll
        for (int dx = 0; dx < 4; ++dx)
            hist_add_wave(hist, ((gl[dy] >> (8 * dx)) & 0xFFu) * (unsigned)K + am[4 * dy + dx], (gm[dy] >> (8 * dx)) & 0xFFu,
                          (unsigned)(K * K));
    __syncthreads();
    hist_flush(hist, K * K, rep + (long)conf_rep_stride(K * K) * (((long)n * gridDim.x + blockIdx.x) % reps));
}

hipError_t launch_upeval(const float *lq, int N, int H, int W, int K, const uint8_t *gt_label, const uint8_t *gt_mask,
                         unsigned long long *rep, int reps, hipStream_t s)
{
    if (reps < 1 || reps > kConfMaxReps) return hipErrorInvalidValue;
    dim3 grid((unsigned)(((long)H * W + UPEVAL_TILE - 1) / UPEVAL_TILE), N), block(UPEVAL_TILE);
    ProfScope prof("k_upeval", 16.0 * (double)N * H * W * K * 6.0,
                   4.0 * (double)N * H * W * K + 16.0 * (double)N * H * W * (gt_mask ? 2 : 1), s);
#define SSAL_UE(KK)                                                                                          \
    case KK:                                                                                                 \
        hipLaunchKernelGGL((k_upeval<KK>), grid, block, 0, s, lq, H, W, gt_label, gt_mask, rep, reps);       \
        break;
    switch (K) {
        SSAL_UE(2) SSAL_UE(3) SSAL_UE(4) SSAL_UE(5) SSAL_UE(6) SSAL_UE(7) SSAL_UE(8) SSAL_UE(9) SSAL_UE(10)
        SSAL_UE(11) SSAL_UE(12) SSAL_UE(13) SSAL_UE(14) SSAL_UE(15) SSAL_UE(16) SSAL_UE(17) SSAL_UE(18)
        SSAL_UE(19) SSAL_UE(20) SSAL_UE(21) SSAL_UE(22) SSAL_UE(23) SSAL_UE(24) SSAL_UE(25) SSAL_UE(26)
        SSAL_UE(27) SSAL_UE(28) SSAL_UE(29) SSAL_UE(30) SSAL_UE(31) SSAL_UE(32)
    default:
        return hipErrorInvalidValue;
    }
#undef SSAL_UE
    return hipGetLastError();
}

}  // namespace ssal
