// ssal_confusion.h -- confusion-matrix histogram pieces shared by the stand-alone op (k_confusion, ssal_metrics.hip) and
// the evaluation tail of the Final kernel (k_final_score<.., EVAL>, ssal_kernels.hip).  gfx950 only.
//
// Semantics: tf.math.bincount(K * label + pred, weights, minlength = maxlength = K * K) (tensortools/metrics.py:226-257):
// a pixel adds its weight (the mask value, not just 0 / 1) to key K * label + pred; a key >= K * K is dropped.
// Counting: a u32 histogram of K * K <= 1024 entries in LDS per workgroup, then one no-return u64 atomic add per NON-ZERO
// entry into one of R replicas of the K x K accumulator (replica = workgroup index % R, each replica on 128-byte lines of its
// own); a finishing kernel folds the replicas into the caller's int64 matrix.  Integer sums throughout: the result does
// not depend on order or schedule.
#pragma once
#include <hip/hip_runtime.h>

namespace ssal {

constexpr int kConfMaxClasses = 32;
constexpr int kConfMaxReps = 64;  // upper bound of the replica count (workspace sizes are computed with it)
constexpr int kConfPeel = 3;      // wave-level aggregation rounds before the per-lane LDS adds

// u64 elements between two replicas: K * K rounded up to whole 128-byte lines
__host__ __device__ inline int conf_rep_stride(int KK) { return (KK + 15) & ~15; }

// Adds `wt` at hist[key] for every active lane with wt != 0 and key < KK.  Most lanes of a wave share one key (the
// diagonal entry of the class the wave's pixels belong to), and ds_add_u32 on one address serialises: up to kConfPeel
// rounds take the key of the first pending lane, sum the weights of every lane holding it (popcounts of ballots, per bit
// of the u8 weight when any weight exceeds 1) and add that sum with ONE lane; what is left after them adds per lane.
__device__ __forceinline__ void hist_add_wave(unsigned *hist, unsigned key, unsigned wt, unsigned KK)
{
    bool todo = wt != 0u && key < KK;
#pragma unroll
    for (int it = 0; it < kConfPeel; ++it) {
        const unsigned long long act = __ballot(todo);
        if (act == 0ull) return;
        const int src = __builtin_ctzll(act);
        const unsigned k0 = (unsigned)__builtin_amdgcn_readlane((int)key, src);
        const bool m = todo && key == k0;
        unsigned sum;
        if (__ballot(m && wt > 1u) == 0ull) {
            sum = (unsigned)__popcll(__ballot(m));
        } else {
            sum = 0u;
#pragma unroll
            for (int b = 0; b < 8; ++b) sum += (unsigned)__popcll(__ballot(m && ((wt >> b) & 1u))) << b;
        }
        if ((int)__lane_id() == src) atomicAdd(&hist[k0], sum);
        todo = todo && !m;
    }
    if (todo) atomicAdd(&hist[key], wt);
}

__device__ __forceinline__ void hist_zero(unsigned *hist, int KK)
{
    for (int e = threadIdx.x; e < KK; e += blockDim.x) hist[e] = 0u;
}

// after a workgroup barrier: the non-zero entries of the workgroup's histogram into replica `rep`
__device__ __forceinline__ void hist_flush(const unsigned *hist, int KK, unsigned long long *rep)
{
    for (int e = threadIdx.x; e < KK; e += blockDim.x) {
        const unsigned v = hist[e];
        if (v) __hip_atomic_fetch_add(rep + e, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace ssal
