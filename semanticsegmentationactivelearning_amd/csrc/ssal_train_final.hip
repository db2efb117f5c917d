// ssal_train_final.hip -- training of ENet's output layer (Final.kernel) over a frozen trunk, gfx950:
//   k_final_grad         transposed-conv logits + softmax cross entropy + dL/dlogit, contracted with the features into
//                        per-workgroup partials of dL/dW (the logits never reach HBM)
//   k_final_grad<K, true>  (profiled as k_final_grad_semi) the same with the semi-supervised targets and the training
//                        metrics in the kernel: an unlabelled image is trained on its own pseudo annotation (argmax /
//                        confidence >= threshold of the Final logits), every pixel is counted into the confusion matrix
//   k_final_grad_finish  fixed-order fold of the partials, times 1 / sum(mask); the float64 loss
//   k_adam               the regulariser gradient and TF-1.13 ApplyAdam on (w, m, v) in place
// Semantics: tensortools/losses.py:3-74, active_learning.py:283-326; the pseudo annotation and the
// training metrics: active_learning.py:226-275, 339-342.  No floating-point atomics: two runs give the
// same bits.
#include "ssal_confusion.h"
#include "ssal_internal.h"
#include "ssal_prof.h"
#include "ssal_score.h"
#include "ssal_xent.h"
#include <type_traits>

namespace ssal {

// Workgroup = one FG_T x FG_T tile of input (feature) pixels = 2 FG_T x 2 FG_T output pixels, for ALL N images; a
// workgroup takes tiles blockIdx.x, blockIdx.x + G, ... (G = final_grad_workgroups), so the per-position fp32 batch sum of
// the loss is taken in k_masked_xent's order (images ascending) and the partial buffer holds G, not N * tiles, rows.
constexpr int FG_T = 16, FG_TP = FG_T + 1, FG_MAX_WG = 1024;

// Every offset into the features, labels, mask and partials is computed in 64 bits.  What remains are the int
// coordinates: 2H + 1 and 2W + 1 (output rows / columns) and the tile count (the tile index is an int).
bool final_grad_fits(int H, int W)
{
    if (H < 1 || W < 1 || H > (1 << 30) - 1 || W > (1 << 30) - 1) return false;
    const long tiles = (long)((H + FG_T - 1) / FG_T) * ((W + FG_T - 1) / FG_T);
    return tiles <= 0x7fffffffL;
}

int final_grad_workgroups(int H, int W)
{
    const long tiles = (long)((H + FG_T - 1) / FG_T) * ((W + FG_T - 1) / FG_T);
    return (int)(tiles < FG_MAX_WG ? tiles : FG_MAX_WG);
}

// x [N,H,W,16] (Bottleneck5_1); wk [3][3][K][16] (TF HW-O-I); labels uint8 / mask fp32 [N,2H,2W].
// part [G][9 * K * 16] fp32 (un-normalised dL/dW, TF layout), lpart [G][2] float64 (sum of the per-position batch sums
// of ce, sum of the mask).
//
// Per image of a tile: (1) stage the 17 x 17 x 16 window through LDS (zeros outside the image); (2) each thread owns
// one input pixel = one 2 x 2 output quad: logits in the tap / channel order of k_final_score and the C oracle (taps
// (kh, kw) ascending, channels ascending, one fmaf chain per class), then xent_pixel (ssal_xent.h, the code of
// k_masked_xent) and dL/dlogit into LDS gl[quad][pixel][K4]; (3) the contraction: dW[tap][k][c] += sum over the tile's
// 256 pixels (row-major) of g[quad(tap)][p][k] * x[src(tap, p)][c], one thread per 4 x 4 (class, channel) block of one
// tap, accumulators in registers across all tiles and images of the workgroup.
//
// SEMI: sa.labelled[n] == 0 replaces the label / mask of image n, which are then
// never read, by the pseudo annotation of active_learning.py:229-275 -- (conf, lab) = pixel_score (ssal_score.h, the code of
// k_final_score) of the pixel's Final logits under the kernel being trained, mask = conf < threshold ? 0 : 1 (NaN -> 1).  The
// logits are those of sa.x_raw [N,H,W,16] (the undistorted frame's features) when it is given: its window goes through `tile`
// FIRST, the four targets of the thread's quad wait in one register, then the training window is staged as usual; without
// x_raw they are the training logits the thread holds.  The targets are constants: no gradient flows through them
// (tf.stop_gradient, :233).  sa.rep: every pixel adds (int)mask at [label][first maximum of the TRAINING logits] of a u32 LDS
// histogram (ssal_confusion.h), flushed into replica (workgroup % reps) at the end.  sa.pseudo_pixels[n] += the image's
// pixels with pseudo mask 1 (one integer atomic per wave, tile and unlabelled image).
struct FinalGradSemi {
    const float *x_raw;         // NULL: the pseudo logits are the training logits
    const uint8_t *labelled;    // [N], NULL = all labelled
    int measure;
    float threshold;
    unsigned long long *rep;    // confusion replicas, NULL = no metrics
    int reps;
    unsigned long long *pseudo_pixels;  // [N] (zeroed by the launcher), NULL = not counted
};

// The pseudo targets of one thread's quad from the undistorted frame's features: the window of image n of sa.x_raw goes
// through `tile` (which the caller stages the training window into afterwards), the logits are k_final_grad's own (the same
// taps, the same order).  Returns a byte per output pixel: the label in bits 0..6, the mask in bit 7.  Called by the whole
// workgroup (two barriers inside).
template <int K>
__device__ __forceinline__ unsigned pseudo_targets_raw(const FinalGradSemi &sa, const float *__restrict__ wk, int n, int H,
                                                       int W, int i0, int j0, bool valid, float inv_logK, float *tile)
{
    const int tid = threadIdx.x, ti = tid / FG_T, tj = tid % FG_T;
    unsigned tgt = 0u;
    __syncthreads();  // the previous contraction is done with tile
    for (int e = tid; e < FG_TP * FG_TP * 4; e += 256) {
        const int pi = (e >> 2) / FG_TP, pj = (e >> 2) % FG_TP;
        const int gi = i0 - 1 + pi, gj = j0 - 1 + pj;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gi >= 0 && gi < H && gj >= 0 && gj < W)
            v = reinterpret_cast<const float4 *>(sa.x_raw + (((long)n * H + gi) * W + gj) * 16)[e & 3];
        reinterpret_cast<float4 *>(tile)[e] = v;
    }
    __syncthreads();
    if (valid) {
        float va[16], vb[16], vc[16], vd[16];  // a = own pixel, b = above, c = left, d = above-left
        const float *la = tile + ((ti + 1) * FG_TP + tj + 1) * 16;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            va[c] = la[c];
            vb[c] = la[c - FG_TP * 16];
            vc[c] = la[c - 16];
            vd[c] = la[c - FG_TP * 16 - 16];
        }
        auto tap = [&](float (&xl)[K], const float (&v)[16], int kh, int kw) {
            const float *wt = wk + (kh * 3 + kw) * K * 16;
#pragma unroll
            for (int c = 0; c < 16; ++c)
#pragma unroll
                for (int k = 0; k < K; ++k) xl[k] = fmaf(v[c], wt[k * 16 + c], xl[k]);
        };
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {
            float lr[K];
#pragma unroll
            for (int k = 0; k < K; ++k) lr[k] = 0.0f;
            if (q == 0) { tap(lr, va, 0, 0); tap(lr, vc, 0, 2); tap(lr, vb, 2, 0); tap(lr, vd, 2, 2); }
            else if (q == 1) { tap(lr, va, 0, 1); tap(lr, vb, 2, 1); }
            else if (q == 2) { tap(lr, va, 1, 0); tap(lr, vc, 1, 2); }
            else { tap(lr, va, 1, 1); }
            int lab;
            const float conf = pixel_score<K>(lr, sa.measure, inv_logK, lab);
            tgt |= ((unsigned)lab | (conf < sa.threshold ? 0u : 0x80u)) << (8 * q);
        }
    }
    return tgt;
}

struct FinalGradPlain {};  // SEMI = false: no argument

template <int K, bool SEMI>
__global__ __launch_bounds__(256) void k_final_grad(const float *__restrict__ x, int N, int H, int W,
                                                    const float *__restrict__ wk, const uint8_t *__restrict__ labels,
                                                    const float *__restrict__ mask, float weight, float on_value,
                                                    float off_value, float *__restrict__ part, double *__restrict__ lpart,
                                                    std::conditional_t<SEMI, FinalGradSemi, FinalGradPlain> sa)
{
    constexpr int K4 = (K + 3) / 4 * 4, KB = K4 / 4;
    constexpr int NB = 9 * KB * 4, BPT = (NB + 255) / 256;  // 4 x 4 blocks, blocks per thread
    __shared__ double red[4];
    __shared__ __attribute__((aligned(16))) float tile[FG_TP * FG_TP * 16];
    __shared__ __attribute__((aligned(16))) float gl[4 * 256 * K4];
    __shared__ unsigned hist[SEMI ? K * K : 1];  // (never referenced, so not allocated, without SEMI)
    const int tid = threadIdx.x;
    const int tiles_x = (W + FG_T - 1) / FG_T, tiles = tiles_x * ((H + FG_T - 1) / FG_T);
    const int ti = tid / FG_T, tj = tid % FG_T;
    const long Ho = 2L * H, Wo = 2L * W;
    float acc[BPT][16];
#pragma unroll
    for (int bb = 0; bb < BPT; ++bb)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[bb][e] = 0.0f;
    double loss = 0.0, msum = 0.0;
    float wc = 1.0f, dwc_cw = 0.0f;  // class weight constants (weight > 1): c_w = e - 1 - weight
    const float cw = kXentEuler - weight;
    const float inv_logK = 1.0f / __logf((float)K);
    if constexpr (SEMI) {
        if (sa.rep) hist_zero(hist, K * K);  // (ordered before the first add by the barriers of the first image)
    }
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int i0 = (t / tiles_x) * FG_T, j0 = (t % tiles_x) * FG_T;
        const int i = i0 + ti, j = j0 + tj;
        const bool valid = i < H && j < W;
        float bsum[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // tf.reduce_sum(loss, axis=0) in fp32, per output pixel of the quad
        for (int n = 0; n < N; ++n) {
            // SEMI: image n is pseudo-annotated (workgroup-uniform); tgt = its four targets from x_raw, a byte per output
            // pixel: the label in bits 0..6, the mask in bit 7
            bool pseudo = false;
            unsigned tgt = 0u;
            int npseudo = 0;
            if constexpr (SEMI) {
                pseudo = sa.labelled && sa.labelled[n] == 0;
                if (pseudo && sa.x_raw) tgt = pseudo_targets_raw<K>(sa, wk, n, H, W, i0, j0, valid, inv_logK, tile);
            }
            __syncthreads();  // the previous contraction (or the pseudo pass) is done with tile / gl
            for (int e = tid; e < FG_TP * FG_TP * 4; e += 256) {
                const int pi = (e >> 2) / FG_TP, pj = (e >> 2) % FG_TP;
                const int gi = i0 - 1 + pi, gj = j0 - 1 + pj;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (gi >= 0 && gi < H && gj >= 0 && gj < W)
                    v = reinterpret_cast<const float4 *>(x + (((long)n * H + gi) * W + gj) * 16)[e & 3];
                reinterpret_cast<float4 *>(tile)[e] = v;
            }
            __syncthreads();
            if (valid) {
                float va[16], vb[16], vc[16], vd[16];  // a = own pixel, b = above, c = left, d = above-left
                const float *la = tile + ((ti + 1) * FG_TP + tj + 1) * 16;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    va[c] = la[c];
                    vb[c] = la[c - FG_TP * 16];
                    vc[c] = la[c - 16];
                    vd[c] = la[c - FG_TP * 16 - 16];
                }
                auto tap = [&](float (&xl)[K], const float (&v)[16], int kh, int kw) {
                    const float *wt = wk + (kh * 3 + kw) * K * 16;
#pragma unroll
                    for (int c = 0; c < 16; ++c)
#pragma unroll
                        for (int k = 0; k < K; ++k) xl[k] = fmaf(v[c], wt[k * 16 + c], xl[k]);
                };
#pragma unroll 1
                for (int q = 0; q < 4; ++q) {
                    float xl[K];
#pragma unroll
                    for (int k = 0; k < K; ++k) xl[k] = 0.0f;
                    if (q == 0) { tap(xl, va, 0, 0); tap(xl, vc, 0, 2); tap(xl, vb, 2, 0); tap(xl, vd, 2, 2); }
                    else if (q == 1) { tap(xl, va, 0, 1); tap(xl, vb, 2, 1); }
                    else if (q == 2) { tap(xl, va, 1, 0); tap(xl, vc, 1, 2); }
                    else { tap(xl, va, 1, 1); }
                    const long op = ((long)n * Ho + 2 * i + (q >> 1)) * Wo + 2 * j + (q & 1);
                    int lab;
                    float mk;
                    if constexpr (SEMI) {
                        if (pseudo) {
                            if (sa.x_raw) {
                                lab = (int)((tgt >> (8 * q)) & 0x7Fu);
                                mk = ((tgt >> (8 * q)) & 0x80u) ? 1.0f : 0.0f;
                            } else {
                                mk = pixel_score<K>(xl, sa.measure, inv_logK, lab) < sa.threshold ? 0.0f : 1.0f;
                            }
                            npseudo += mk != 0.0f;
                        } else {
                            lab = labels[op];
                            mk = mask[op];
                        }
                        if (sa.rep) {  // train_pred = tf.math.argmax(train_logits): the first maximum
                            float pm = xl[0];
                            int pred = 0;
#pragma unroll
                            for (int k = 1; k < K; ++k)
                                if (xl[k] > pm) { pm = xl[k]; pred = k; }
                            hist_add_wave(hist, (unsigned)lab * K + (unsigned)pred, (unsigned)(int)mk, K * K);
                        }
                    } else {
                        lab = labels[op];
                        mk = mask[op];
                    }
                    const XentPix r = xent_pixel<K>(xl, lab, mk, weight, on_value, off_value);
                    bsum[q] += r.ce;
                    msum += (double)mk;
                    // dL/dx_k (before the 1 / sum(mask) factor): TF's gradient of softmax_cross_entropy_with_logits is
                    // softmax - y; the class weight w(p_class) = 1 / log(weight + c_w p_class) has no stop_gradient:
                    //   g_k = mask (w (s_k - y_k) + ce0 w' s_k (y_k - p_class)),  w' = -w^2 c_w / u
                    if (weight > 1.0f) {
                        const float u = weight + cw * r.pc;
                        wc = 1.0f / logf(u);
                        dwc_cw = -(wc * wc) * cw / u;
                    }
                    const float a1 = mk * wc, a2 = mk * r.ce0 * dwc_cw;
                    float *gq = gl + (q * 256 + tid) * K4;
#pragma unroll
                    for (int k = 0; k < K4; ++k) {
                        float g = 0.0f;
                        if (k < K) {
                            const float yk = (k == lab) ? on_value : off_value;
                            const float sk = expf(xl[k] - r.m) / r.S;
                            g = a1 * (sk - yk) + a2 * (sk * (yk - r.pc));
                        }
                        gq[k] = g;
                    }
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int k = 0; k < K4; ++k) gl[(q * 256 + tid) * K4 + k] = 0.0f;
            }
            if constexpr (SEMI) {
                if (pseudo && sa.pseudo_pixels) {
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) npseudo += __shfl_down(npseudo, off, 64);
                    if ((tid & 63) == 0 && npseudo) atomicAdd(sa.pseudo_pixels + n, (unsigned long long)npseudo);
                }
            }
            __syncthreads();
#pragma unroll
            for (int bb = 0; bb < BPT; ++bb) {
                const int b = tid + 256 * bb;
                if (NB % 256 == 0 || b < NB) {
                    const int cb = b & 3, kb = (b >> 2) % KB, tp = (b >> 2) / KB;
                    const int kh = tp / 3, kw = tp % 3;
                    const int q = (kh == 1 ? 2 : 0) + (kw == 1 ? 1 : 0);
                    const int src0 = (1 - (kh == 2 ? 1 : 0)) * FG_TP + 1 - (kw == 2 ? 1 : 0);
                    const float4 *g4 = reinterpret_cast<const float4 *>(gl + q * 256 * K4) + kb;
                    const float4 *f4 = reinterpret_cast<const float4 *>(tile) + cb;
#pragma unroll 4
                    for (int p = 0; p < 256; ++p) {
                        const float4 g = g4[p * KB];
                        const float4 f = f4[(src0 + (p / FG_T) * FG_TP + p % FG_T) * 4];
                        const float gk[4] = {g.x, g.y, g.z, g.w}, fc[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                        for (int a = 0; a < 4; ++a)
#pragma unroll
                            for (int c = 0; c < 4; ++c) acc[bb][a * 4 + c] = fmaf(gk[a], fc[c], acc[bb][a * 4 + c]);
                    }
                }
            }
        }
        if (valid)
#pragma unroll
            for (int q = 0; q < 4; ++q) loss += (double)bsum[q];
    }
    float *pw = part + (long)blockIdx.x * (9 * K * 16);
#pragma unroll
    for (int bb = 0; bb < BPT; ++bb) {
        const int b = tid + 256 * bb;
        if (NB % 256 == 0 || b < NB) {
            const int cb = b & 3, kb = (b >> 2) % KB, tp = (b >> 2) / KB;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int k = kb * 4 + a;
                if (k < K)
#pragma unroll
                    for (int c = 0; c < 4; ++c) pw[(tp * K + k) * 16 + cb * 4 + c] = acc[bb][a * 4 + c];
            }
        }
    }
    const double r0 = block_sum_256(loss, red);
    __syncthreads();
    const double r1 = block_sum_256(msum, red);
    if (tid == 0) {
        lpart[2 * (long)blockIdx.x] = r0;
        lpart[2 * (long)blockIdx.x + 1] = r1;
    }
    if constexpr (SEMI) {
        if (sa.rep) {
            __syncthreads();
            hist_flush(hist, K * K, sa.rep + (long)conf_rep_stride(K * K) * (blockIdx.x % sa.reps));
        }
    }
}

// grad[o] = (sum over workgroups g = 0, 1, .. G-1 of part[g][o], fp32, in that order) * (float)(1 / (double)(float)sum(mask));
// loss = (sum of the lpart sums) / (double)(float)sum(mask), as k_xent_finish.  Every block folds the G mask sums itself.
__global__ __launch_bounds__(256) void k_final_grad_finish(const float *__restrict__ part, const double *__restrict__ lpart,
                                                           int G, int count, double *__restrict__ loss_out,
                                                           float *__restrict__ grad)
{
    __shared__ double red[4];
    __shared__ float scale;
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < G; i += 256) { a += lpart[2 * (long)i]; b += lpart[2 * (long)i + 1]; }
    const double ra = block_sum_256(a, red);
    __syncthreads();
    const double rb = block_sum_256(b, red);
    if (threadIdx.x == 0) {
        const double msum = (double)(float)rb;  // tf.cast(tf.reduce_sum(_mask) [fp32], float64)
        scale = (float)(1.0 / msum);            // d loss / d (batch sum), cast back to fp32 by the gradient of tf.cast
        if (blockIdx.x == 0) loss_out[0] = ra / msum;
    }
    __syncthreads();
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o < count) {
        float acc = 0.0f;
        for (int g = 0; g < G; ++g) acc += part[(long)g * count + o];
        grad[o] = acc * scale;
    }
}

hipError_t launch_final_grad(const float *x, int N, int H, int W, const float *wk, int K, const uint8_t *labels,
                             const float *mask, float weight, float label_smoothing, float *part, double *lpart,
                             double *loss, float *grad, hipStream_t s)
{
    if (N < 1 || !final_grad_fits(H, W)) return hipErrorInvalidValue;
    const int G = final_grad_workgroups(H, W);
    const float on_value = 1.0f - label_smoothing, off_value = label_smoothing / ((float)K - 1.0f);
    const double pix = (double)N * H * W;
    {
        ProfScope prof("k_final_grad", 2.0 * 2.0 * pix * 9 * 16 * K,
                       4.0 * pix * 16 + 4.0 * pix * (1 + 4) + 4.0 * G * 9.0 * 16 * K, s);
#define SSAL_FG(KK)                                                                                                    \
    case KK:                                                                                                           \
        hipLaunchKernelGGL((k_final_grad<KK, false>), dim3(G), dim3(256), 0, s, x, N, H, W, wk, labels, mask, weight,   \
                           on_value, off_value, part, lpart, FinalGradPlain{});                                        \
        break;
        switch (K) {
            SSAL_FG(2) SSAL_FG(3) SSAL_FG(4) SSAL_FG(5) SSAL_FG(6) SSAL_FG(7) SSAL_FG(8) SSAL_FG(9)
            SSAL_FG(10) SSAL_FG(11) SSAL_FG(12) SSAL_FG(13) SSAL_FG(14) SSAL_FG(15) SSAL_FG(16)
            SSAL_FG(17) SSAL_FG(18) SSAL_FG(19) SSAL_FG(20) SSAL_FG(21) SSAL_FG(22) SSAL_FG(23)
            SSAL_FG(24) SSAL_FG(25) SSAL_FG(26) SSAL_FG(27) SSAL_FG(28) SSAL_FG(29) SSAL_FG(30)
            SSAL_FG(31) SSAL_FG(32)
        default:
            return hipErrorInvalidValue;
        }
#undef SSAL_FG
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int count = 9 * K * 16;
    ProfScope prof("k_final_grad_finish", (double)G * count, 4.0 * G * count + 16.0 * G, s);
    hipLaunchKernelGGL(k_final_grad_finish, dim3((count + 255) / 256), dim3(256), 0, s, part, lpart, G, count, loss, grad);
    return hipGetLastError();
}

// The semi-supervised form: x_raw / labelled / rep / pseudo_pixels may each be NULL (FinalGradSemi).  rep [reps][conf_rep_stride(K * K)]
// u64 must be zero on entry (the caller folds it with launch_confusion_fold); pseudo_pixels [N] is zeroed here.
hipError_t launch_final_grad_semi(const float *x, const float *x_raw, int N, int H, int W, const float *wk, int K,
                                  const uint8_t *labels, const float *mask, const uint8_t *labelled, int measure,
                                  float threshold, float weight, float label_smoothing, float *part, double *lpart,
                                  double *loss, float *grad, unsigned long long *rep, int reps, int64_t *pseudo_pixels,
                                  hipStream_t s)
{
    if (N < 1 || !final_grad_fits(H, W) || measure < 0 || measure > 2 || (rep && reps < 1)) return hipErrorInvalidValue;
    const int G = final_grad_workgroups(H, W);
    const float on_value = 1.0f - label_smoothing, off_value = label_smoothing / ((float)K - 1.0f);
    const double pix = (double)N * H * W;
    if (pseudo_pixels) {
        hipError_t e = hipMemsetAsync(pseudo_pixels, 0, (size_t)N * sizeof(int64_t), s);
        if (e != hipSuccess) return e;
    }
    const FinalGradSemi sa = {x_raw, labelled, measure, threshold, rep, reps, (unsigned long long *)pseudo_pixels};
    {
        ProfScope prof("k_final_grad_semi", 2.0 * 2.0 * pix * 9 * 16 * K * (x_raw ? 1.5 : 1.0),
                       4.0 * pix * 16 * (x_raw ? 2 : 1) + 4.0 * pix * (1 + 4) + 4.0 * G * 9.0 * 16 * K, s);
#define SSAL_FG(KK)                                                                                                    \
    case KK:                                                                                                           \
        hipLaunchKernelGGL((k_final_grad<KK, true>), dim3(G), dim3(256), 0, s, x, N, H, W, wk, labels, mask, weight,      \
                           on_value, off_value, part, lpart, sa);                                                      \
        break;
        switch (K) {
            SSAL_FG(2) SSAL_FG(3) SSAL_FG(4) SSAL_FG(5) SSAL_FG(6) SSAL_FG(7) SSAL_FG(8) SSAL_FG(9)
            SSAL_FG(10) SSAL_FG(11) SSAL_FG(12) SSAL_FG(13) SSAL_FG(14) SSAL_FG(15) SSAL_FG(16)
            SSAL_FG(17) SSAL_FG(18) SSAL_FG(19) SSAL_FG(20) SSAL_FG(21) SSAL_FG(22) SSAL_FG(23)
            SSAL_FG(24) SSAL_FG(25) SSAL_FG(26) SSAL_FG(27) SSAL_FG(28) SSAL_FG(29) SSAL_FG(30)
            SSAL_FG(31) SSAL_FG(32)
        default:
            return hipErrorInvalidValue;
        }
#undef SSAL_FG
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int count = 9 * K * 16;
    ProfScope prof("k_final_grad_finish", (double)G * count, 4.0 * G * count + 16.0 * G, s);
    hipLaunchKernelGGL(k_final_grad_finish, dim3((count + 255) / 256), dim3(256), 0, s, part, lpart, G, count, loss, grad);
    return hipGetLastError();
}

// TF-1.13 ApplyAdam (training_ops.cc, use_nesterov = false) after the Keras l1_l2 regulariser gradient:
//   g += l2 * (2 w) + l1 * sign(w)           (sign(0) = 0)
//   alpha = lr * sqrt(1 - beta2_power) / (1 - beta1_power)
//   m += (g - m) * (1 - beta1);  v += (g^2 - v) * (1 - beta2);  w -= (m * alpha) / (sqrt(v) + eps)
// sqrt and the two divisions are correctly rounded: sqrtf and '/' under HIP's default
// -fhip-fp32-correctly-rounded-divide-sqrt.  (Not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the HIP headers map it
// to __ocml_native_sqrt_f32, the ~1 ulp v_sqrt_f32, and w then missed the numpy restatement by an ulp.)  The library builds
// with -ffp-contract=off, so no product is fused into an add: numpy float32 gives the same bits.
__global__ __launch_bounds__(256) void k_adam(float *__restrict__ var, float *__restrict__ m, float *__restrict__ v,
                                              const float *__restrict__ grad, long count, float lr, float beta1,
                                              float beta2, float eps, float beta1_power, float beta2_power, float l1,
                                              float l2)
{
    const long o = (long)blockIdx.x * 256 + threadIdx.x;
    if (o >= count) return;
    const float alpha = lr * sqrtf(1.0f - beta2_power) / (1.0f - beta1_power);
    const float w = var[o];
    const float sgn = w > 0.0f ? 1.0f : (w < 0.0f ? -1.0f : 0.0f);
    const float g = grad[o] + (l2 * (2.0f * w) + l1 * sgn);
    float mo = m[o], vo = v[o];
    mo += (g - mo) * (1.0f - beta1);
    vo += (g * g - vo) * (1.0f - beta2);
    m[o] = mo;
    v[o] = vo;
    var[o] = w - (mo * alpha) / (sqrtf(vo) + eps);
}

hipError_t launch_adam(float *var, float *m, float *v, const float *grad, long count, float lr, float beta1, float beta2,
                       float eps, float beta1_power, float beta2_power, float l1, float l2, hipStream_t s)
{
    if (count <= 0 || (count + 255) / 256 > 0x7fffffffL) return hipErrorInvalidValue;
    ProfScope prof("k_adam", 12.0 * count, 4.0 * 7 * count, s);
    hipLaunchKernelGGL(k_adam, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, var, m, v, grad, count, lr, beta1,
                       beta2, eps, beta1_power, beta2_power, l1, l2);
    return hipGetLastError();
}

}  // namespace ssal
