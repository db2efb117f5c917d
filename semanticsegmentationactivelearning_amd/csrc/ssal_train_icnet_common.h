// ssal_train_icnet_common.h -- what ICNet's deep trainers share (ssal_train_icnet_fusion / _cascade / _highres.hip; DESIGN.md
// section 33): the description of a cascade-feature-fusion block, the grid arithmetic of every launch, the batch-norm row fold,
// and the three small kernels around a fusion block's split-K weight gradient (pack, finish, gamma) with the device functions
// their one-layer forms in ssal_train_icnet_highres.hip are written on.  gfx950 (MI355X / CDNA4) only.
#pragma once
#include <hip/hip_runtime.h>

#include "ssal_icnet.h"
#include "ssal_score.h"

namespace ssal {

// A fusion block: out = relu(BN(3 x 3 dilated conv (CIN -> 128) of resize_2x(low)) + BN(1 x 1 conv (CB -> 128) of side)).
// CIN = 128: conv_sub2 + conv3_sub1_proj (section 28), CIN = 256: conv_sub4 + conv3_1_sub2_proj (section 29).
template <int CIN>
struct FusionBlock {
    static_assert(CIN == 128 || CIN == 256, "the two fusion blocks of ICNet");
    static constexpr int CB = CIN == 128 ? 64 : 256;  // input channels of the 1 x 1 branch
    // the block's part of the packed vector (float offsets): kernel_a [3,3,CIN,128] | gamma_a | beta_a | kernel_b [1,1,CB,128] |
    // gamma_b | beta_b
    static constexpr int KA = 0, GA = 9 * CIN * 128, BA = GA + 128, KB = BA + 128, GB = KB + CB * 128, BB = GB + 128,
                         END = BB + 128;
    // a split-K partial [TAPS][CIN][128]: the nine dilated taps, the 1 x 1 branch as tap 9, and sum_p g (dBeta) as the row the
    // weight-gradient kernel feeds with ones: behind the 64 channels of tap 9, or the first row of an eleventh tap
    static constexpr int TAPS = CIN == 128 ? 10 : 11, PART = TAPS * CIN * 128;
    static constexpr int ONES_TAP = CIN == 128 ? 9 : 10, ONES_CI = CIN == 128 ? 64 : 0;
    static constexpr int KCH = CIN / 32;                // 32-channel K chunks per tap in launch_igemm's layout
    static constexpr int MAX_WG = CIN == 128 ? 96 : 64;  // split-K groups the finish kernel folds
};

inline long icnet_cdiv(long a, long b) { return (a + b - 1) / b; }

// the grid of a launch that strides its tiles over the workgroups: the tiles, at most `cap`, at most max_workgroups (0: no
// limit), at least 1
inline int icnet_grid(long tiles, int cap, int max_workgroups)
{
    long g = tiles < cap ? tiles : cap;
    if (max_workgroups > 0 && g > max_workgroups) g = max_workgroups;
    return (int)(g < 1 ? 1 : g);
}

// where launch_igemm reads K[tap, ci, co] of a kernel with kch 32-channel chunks per tap and cout output channels
__device__ __forceinline__ int igemm_wt_index(int tap, int ci, int co, int kch, int cout)
{
    return ((tap * kch + (ci >> 5)) * cout + co) * 32 + igemm_kpos(ci & 31);
}

// the inference batch-norm as a row of scales and shifts: s = gamma / sqrtf(var + 1e-3f), t = fmaf(-mean, s, beta) as
// fold_bn_padded (sqrtf and '/' are correctly rounded under HIP's default -fhip-fp32-correctly-rounded-divide-sqrt)
__device__ __forceinline__ void icnet_bn_row(float gamma, float beta, float mean, float var, float *s, float *t)
{
    const float sg = gamma / sqrtf(var + 1e-3f);
    *s = sg;
    *t = fmaf(-mean, sg, beta);
}

// P: the block's packed vector -> its two kernels in launch_igemm's layout, rows = scale_a | shift_a | scale_b | shift_b (128
// each).  stats: mean_a | var_a | mean_b | var_b
template <int CIN>
__global__ __launch_bounds__(256) void k_icnet_block_pack(const float *__restrict__ P, const float *__restrict__ stats,
                                                          float *__restrict__ wt_a, float *__restrict__ wt_b,
                                                          float *__restrict__ rows)
{
    using B = FusionBlock<CIN>;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o < B::GA) {
        wt_a[igemm_wt_index(o / (CIN * 128), (o >> 7) & (CIN - 1), o & 127, B::KCH, 128)] = P[B::KA + o];
    } else if (o < B::GA + B::CB * 128) {
        const int e = o - B::GA;
        wt_b[igemm_wt_index(0, e >> 7, e & 127, B::CB / 32, 128)] = P[B::KB + e];
    } else if (o < B::GA + B::CB * 128 + 256) {
        const int e = o - B::GA - B::CB * 128, b = e >> 7, c = e & 127;
        icnet_bn_row(P[(b ? B::GB : B::GA) + c], P[(b ? B::BB : B::BA) + c], stats[2 * b * 128 + c],
                     stats[(2 * b + 1) * 128 + c], rows + 256 * b + c, rows + 256 * b + 128 + c);
    }
}

// (float)(1 / (double)(float)sum(mask)) from the Gh mask sums of the head kernel's lpart, as k_icnet_head_finish takes it: to
// every thread of a workgroup of 256, and from workgroup 0 into *keep
__device__ __forceinline__ float icnet_loss_scale(const double *__restrict__ lpart, int Gh, float *keep)
{
    __shared__ double red[4];
    __shared__ float scale_s;
    double b = 0.0;
    for (int i = threadIdx.x; i < Gh; i += 256) b += lpart[2 * (long)i + 1];
    const double rb = block_sum_256(b, red);
    if (threadIdx.x == 0) {
        scale_s = (float)(1.0 / (double)(float)rb);
        if (blockIdx.x == 0) *keep = scale_s;
    }
    __syncthreads();
    return scale_s;
}

// raw[o] = sum over split-K groups b = 0 .. G - 1 of part[b][o], fp32, in that order -> fold[o]; the gradients that are a
// scaled copy of it: dK_a = (raw scale) s_a[co], dK_b = (raw scale) s_b[co], dBeta_a = dBeta_b = raw[row of ones][co] scale.
// LAST (the block under the head): icnet_loss_scale, left in scale_p[0]; the blocks below read it there.
template <int CIN, bool LAST>
__global__ __launch_bounds__(256) void k_icnet_block_finish(const float *__restrict__ part, int G,
                                                            const double *__restrict__ lpart, int Gh, float *scale_p,
                                                            const float *__restrict__ rows, float *__restrict__ fold,
                                                            float *__restrict__ grad)
{
    using B = FusionBlock<CIN>;
    const float scale = LAST ? icnet_loss_scale(lpart, Gh, scale_p) : scale_p[0];
    const int o = blockIdx.x * 256 + threadIdx.x;
    const int tap = o / (CIN * 128), ci = (o >> 7) & (CIN - 1), co = o & 127;
    if (o >= B::PART || (tap > 9 && ci != B::ONES_CI)) return;  // (of an eleventh tap only the row of ones is a gradient)
    float acc = 0.0f;
    for (int gi = 0; gi < G; ++gi) acc += part[(long)gi * B::PART + o];
    fold[o] = acc;
    if (tap < 9) {
        grad[B::KA + o] = (acc * scale) * rows[co];
    } else if (tap == 9 && ci < B::CB) {
        grad[B::KB + ci * 128 + co] = (acc * scale) * rows[256 + co];
    } else if (tap == B::ONES_TAP && ci == B::ONES_CI) {
        grad[B::BA + co] = acc * scale;
        grad[B::BB + co] = acc * scale;
    }
}

// dGamma[co] = sum_p g[p, co] (acc[p, co] - mean) / sqrt(var + 1e-3) with acc = sum K u re-associated over the pixels, so that
// the pre-BN accumulators are never formed: ((sum_tap (sum_ci K[tap, ci, co] raw[tap, ci, co], ci ascending, fmaf), taps
// ascending) - mean raw_beta) rstd scale.  The three pieces:
// one tap, K and raw [CI][CO]
__device__ __forceinline__ float icnet_gamma_tap(const float *__restrict__ K, const float *__restrict__ raw, int CI, int CO,
                                                 int co)
{
    float a = 0.0f;
    for (int ci = 0; ci < CI; ++ci) a = fmaf(K[ci * CO + co], raw[ci * CO + co], a);
    return a;
}
// the nine taps of a 3 x 3 kernel, K and raw [9][CI][CO].  (A 1 x 1 kernel is icnet_gamma_tap alone, NOT this loop at one tap:
// 0.0f + a would turn a sum of -0.0f into +0.0f.)
__device__ __forceinline__ float icnet_gamma_3x3(const float *__restrict__ K, const float *__restrict__ raw, int CI, int CO,
                                                 int co)
{
    float sum = 0.0f;
    for (int tap = 0; tap < 9; ++tap) sum += icnet_gamma_tap(K + tap * CI * CO, raw + tap * CI * CO, CI, CO, co);
    return sum;
}
__device__ __forceinline__ float icnet_dgamma(float sum, float mean, float var, float rbeta, float scale)
{
    const float rstd = 1.0f / sqrtf(var + 1e-3f);
    return ((sum - mean * rbeta) * rstd) * scale;
}

// grid 2 (branch a, b) x 128 threads (co); fold: k_icnet_block_finish's
template <int CIN>
__global__ __launch_bounds__(128) void k_icnet_block_gamma(const float *__restrict__ fold, const float *__restrict__ scale_p,
                                                           const float *__restrict__ P, const float *__restrict__ stats,
                                                           float *__restrict__ grad)
{
    using B = FusionBlock<CIN>;
    const int co = threadIdx.x, b = blockIdx.x;
    const float rbeta = fold[(B::ONES_TAP * CIN + B::ONES_CI) * 128 + co], scale = scale_p[0];
    const float sum = b == 0 ? icnet_gamma_3x3(P + B::KA, fold, CIN, 128, co)
                             : icnet_gamma_tap(P + B::KB, fold + 9 * CIN * 128, B::CB, 128, co);
    grad[(b ? B::GB : B::GA) + co] = icnet_dgamma(sum, stats[2 * b * 128 + co], stats[(2 * b + 1) * 128 + co], rbeta, scale);
}

}  // namespace ssal
