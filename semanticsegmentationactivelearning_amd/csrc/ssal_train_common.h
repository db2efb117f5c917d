// ssal_train_common.h -- device code the ENet training kernels share (ssal_train_block / _stage / _tail / _decoder.hip): PReLU
// and its derivatives, the compensated sum, and the kernel that folds a block's per-workgroup partial gradients.
#pragma once
#include "ssal_prof.h"
#include "ssal_score.h"

namespace ssal {

// PReLU is relu(x) - alpha relu(-x) (extra_ops.py:9-26)
__device__ __forceinline__ float prelu(float v, float a) { return v >= 0.0f ? v : a * v; }
// d prelu / dv and the factor of d prelu / dalpha (TensorFlow's convention at 0: both 0)
__device__ __forceinline__ float dprelu(float v, float a) { return v > 0.0f ? 1.0f : (v < 0.0f ? a : 0.0f); }
__device__ __forceinline__ float neg(float v) { return v < 0.0f ? v : 0.0f; }

// one term of a compensated (Kahan) fp32 sum in a fixed order: the folds over the 256 threads and over the up to 3072
// partial rows would otherwise be the longest rounding chains of a gradient (the library builds without fast-math and with
// -ffp-contract=off, so the compensation survives)
__device__ __forceinline__ void kahan(float &sum, float &comp, float v)
{
    const float y = v - comp, t = sum + y;
    comp = (t - sum) - y;
    sum = t;
}

// One block's part of the packed gradient, FLOATS floats of which the first TRAINED are trained:
// grad[o] = (sum over the G partial rows, in row order, compensated fp32) * (float)(1 / (double)(float)sum(mask)), the scale of
// k_tb_finish from the same Gl per-workgroup mask sums the head kernel left; the moving statistics and the padding get 0.
template <int TRAINED, int FLOATS>
__global__ __launch_bounds__(256) void k_train_finish(const float *__restrict__ part, const double *__restrict__ lpart, int G, int Gl,
                                                      float *__restrict__ grad)
{
    __shared__ double red[4];
    __shared__ float scale;
    double b = 0.0;
    for (int i = threadIdx.x; i < Gl; i += 256) b += lpart[2 * (long)i + 1];
    const double rb = block_sum_256(b, red);
    if (threadIdx.x == 0) scale = (float)(1.0 / (double)(float)rb);
    __syncthreads();
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= FLOATS) return;
    float acc = 0.0f, comp = 0.0f;
    if (o < TRAINED)
        for (long r = 0; r < G; ++r) kahan(acc, comp, part[r * TRAINED + o]);
    grad[o] = o < TRAINED ? acc * scale : 0.0f;
}

// name: the launch's row in the profile (k_ts_finish, k_tt_finish, k_td_finish)
template <int TRAINED, int FLOATS>
inline hipError_t launch_train_finish(const char *name, const float *part, const double *lpart, int G, int Gl, float *grad,
                                      hipStream_t s)
{
    ProfScope prof(name, (double)G * TRAINED, 4.0 * G * TRAINED + 16.0 * Gl, s);
    hipLaunchKernelGGL((k_train_finish<TRAINED, FLOATS>), dim3((FLOATS + 255) / 256), dim3(256), 0, s, part, lpart, G, Gl, grad);
    return hipGetLastError();
}

}  // namespace ssal
