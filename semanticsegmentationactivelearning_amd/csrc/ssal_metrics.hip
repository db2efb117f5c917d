// ssal_metrics.hip -- validation metrics on the device: the stand-alone confusion-matrix op and the fold of the
// confusion accumulator replicas, gfx950.  (The fused form, inside the Final kernel, is k_final_score<.., EVAL> in
// ssal_kernels.hip; both count through ssal_confusion.h.)
#include "ssal_confusion.h"
#include "ssal_internal.h"
#include "ssal_prof.h"

namespace ssal {

// tensortools/metrics.py:226-257 confusion_mat: bincount(K * label + pred, weights, minlength = maxlength = K * K).
// A workgroup counts CM_CHUNK consecutive pixels (so its u32 histogram holds at most 4096 * 255): every thread first loads
// its CM_PER pixels (byte loads, coalesced across the wave), then adds them one slot at a time.
constexpr int CM_PER = 16, CM_CHUNK = 256 * CM_PER;

__global__ __launch_bounds__(256) void k_confusion(const uint8_t *__restrict__ pred, const uint8_t *__restrict__ labels,
                                                   const uint8_t *__restrict__ weights, int64_t pixels, int K,
                                                   unsigned long long *__restrict__ rep, int reps)
{
    __shared__ unsigned hist[kConfMaxClasses * kConfMaxClasses];
    const int KK = K * K;
    hist_zero(hist, KK);
    const int64_t base = (int64_t)blockIdx.x * CM_CHUNK + threadIdx.x;
    unsigned key[CM_PER], wt[CM_PER];
#pragma unroll
    for (int t = 0; t < CM_PER; ++t) {
        const int64_t p = base + 256 * t;
        const bool ok = p < pixels;
        key[t] = ok ? (unsigned)labels[p] * (unsigned)K + pred[p] : 0u;
        wt[t] = ok ? (weights ? weights[p] : 1u) : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < CM_PER; ++t) hist_add_wave(hist, key[t], wt[t], (unsigned)KK);
    __syncthreads();
    hist_flush(hist, KK, rep + (int64_t)conf_rep_stride(KK) * (blockIdx.x % reps));
}

hipError_t launch_confusion(const uint8_t *pred, const uint8_t *labels, const uint8_t *weights, int64_t pixels, int K,
                            unsigned long long *rep, int reps, hipStream_t s)
{
    if (pixels <= 0) return hipSuccess;
    const int64_t blocks = (pixels + CM_CHUNK - 1) / CM_CHUNK;
    ProfScope prof("k_confusion", 0.0, (double)pixels * (weights ? 3 : 2), s);
    hipLaunchKernelGGL(k_confusion, dim3((unsigned)blocks), dim3(256), 0, s, pred, labels, weights, pixels, K, rep, reps);
    return hipGetLastError();
}

// confusion[e] += sum over the replicas of rep[r][e] (fixed order; integer sums)
__global__ __launch_bounds__(256) void k_confusion_fold(const unsigned long long *__restrict__ rep, int reps, int KK,
                                                        int64_t *__restrict__ confusion)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= KK) return;
    const int stride = conf_rep_stride(KK);
    unsigned long long v = 0ull;
    for (int r = 0; r < reps; ++r) v += rep[(int64_t)r * stride + e];
    confusion[e] += (int64_t)v;
}

hipError_t launch_confusion_fold(const unsigned long long *rep, int reps, int K, int64_t *confusion, hipStream_t s)
{
    const int KK = K * K;
    hipLaunchKernelGGL(k_confusion_fold, dim3((KK + 255) / 256), dim3(256), 0, s, rep, reps, KK, confusion);
    return hipGetLastError();
}

}  // namespace ssal
