// ssal_xent.h -- the per-pixel term of masked_softmax_cross_entropy (tensortools/losses.py:3-74), shared by the forward op
// (k_masked_xent, ssal_kernels.hip) and the output-layer gradient (k_final_grad, ssal_train_final.hip).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

namespace ssal {

// The reference's _EULER (e - 1) as the kernels use it: an fp32 constant
constexpr float kXentEuler = 1.718281828459045f;

struct XentPix {
    float m, S;  // max logit, sum_k exp(x_k - m)
    float pc;    // p_class = sum_k softmax_k * y_k
    float ce0;   // sum_k y_k * (log S - (x_k - m)), before the mask and the class weight
    float ce;    // ce0 * mask [* 1 / log(weight + (e - 1 - weight) * p_class) when weight > 1]
};

// y_k = on_value for k == lab, off_value otherwise (a label >= K gives the all-off row, as tf.one_hot does).
// Every sum runs over k ascending; softmax_k = expf(x_k - m) / S.
template <int K>
__device__ __forceinline__ XentPix xent_pixel(const float (&x)[K], int lab, float mk, float weight, float on_value,
                                              float off_value)
{
    XentPix r;
    float m = x[0];
#pragma unroll
    for (int k = 1; k < K; ++k) m = fmaxf(m, x[k]);
    float S = 0.0f;
#pragma unroll
    for (int k = 0; k < K; ++k) S += expf(x[k] - m);
    const float logS = logf(S);
    float ce = 0.0f, pc = 0.0f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float yk = (k == lab) ? on_value : off_value;
        const float d = x[k] - m;
        ce += yk * (logS - d);
        pc += yk * (expf(d) / S);
    }
    r.m = m;
    r.S = S;
    r.pc = pc;
    r.ce0 = ce;
    ce *= mk;
    if (weight > 1.0f) ce *= 1.0f / logf(weight + (kXentEuler - weight) * pc);
    r.ce = ce;
    return r;
}

}  // namespace ssal
