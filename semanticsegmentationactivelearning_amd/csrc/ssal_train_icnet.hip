// ssal_train_icnet.hip -- training of ICNet's output layer (conv6_cls/Kernel [1,1,128,K], conv6_cls/Bias [K]) over a frozen
// trunk, gfx950:
//   k_icnet_head_pack    the packed head [128 K | K] -> the kernel in launch_igemm's layout + its scale / shift rows, so that
//                        the FORWARD path's own launch (k_conv1x1_up2_c128) computes lq from the weights being trained
//   k_icnet_head_grad    conv6_interp (4x legacy bilinear of lq) + softmax cross entropy + dL/dlogit, pulled back through the
//                        4x and the 2x resize and contracted with sub12_sum into per-workgroup partials of dL/dKernel and
//                        dL/dBias (neither the full-resolution logits nor sub12_sum_interp reach HBM)
//   k_icnet_head_finish  fixed-order fold of the partials, times 1 / sum(mask); the float64 loss
// Semantics: ICNET_SPEC.md sections 4 and 6, tensortools/losses.py:3-74, active_learning.py:283-326 (DESIGN.md sections 15
// and 23).  No floating-point atomics: two runs give the same bits.
// The semi-supervised step (active_learning.py:226-275, 339-342) is k_icnet_head_grad<K, true>: the
// targets of an unlabelled image are built from the logits the kernel holds, the training-pass confusion matrix and the
// pseudo-pixel counts leave through integer atomics.  k_icnet_head_grad<K, true, true> is that step with the pull-back
// windows of the fusion and the cascade trainer.
#include <type_traits>

#include "ssal_confusion.h"
#include "ssal_icnet.h"
#include "ssal_internal.h"
#include "ssal_prof.h"
#include "ssal_score.h"
#include "ssal_train_icnet.h"
#include "ssal_xent.h"

namespace ssal {

constexpr int IH_TP = IH_T + 1, IH_WP = IH_TP * IH_TP;  // the 9 x 9 window of lq a tile's 32 x 32 loss pixels read
constexpr int IH_SS = IH_T / 2 + 2, IH_SP = IH_SS * IH_SS;  // the 6 x 6 window of sub12_sum those 81 pixels read
constexpr int IH_OT = 4 * IH_T;  // loss pixels per tile side

bool icnet_head_fits(int h8, int w8)
{
    if (h8 < 1 || w8 < 1 || h8 > (1 << 27) || w8 > (1 << 27)) return false;  // 8 h8 + 1, 8 w8 + 1 are ints
    const long tiles = (long)((2 * h8 + IH_T - 1) / IH_T) * ((2 * w8 + IH_T - 1) / IH_T);
    return tiles <= 0x7fffffffL;
}

int icnet_head_workgroups(int h8, int w8, int max_workgroups)
{
    long g = (long)((2 * h8 + IH_T - 1) / IH_T) * ((2 * w8 + IH_T - 1) / IH_T);
    if (g > IH_MAX_WG) g = IH_MAX_WG;
    if (max_workgroups > 0 && g > max_workgroups) g = max_workgroups;
    return (int)g;
}

int64_t icnet_head_ws_floats_wt() { return 4 * 32 * 32 + 64; }

int64_t icnet_head_tiles(int h8, int w8) { return (int64_t)((2 * h8 + IH_T - 1) / IH_T) * ((2 * w8 + IH_T - 1) / IH_T); }

// wt [128 / 32][32][32] as igemm_relayout writes a 1 x 1 x 128 x K kernel (rows co >= K zero), scale (1 / 0), shift (bias / 0)
__global__ __launch_bounds__(256) void k_icnet_head_pack(const float *__restrict__ head, int K, float *__restrict__ wt)
{
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o < 4096) {
        const int ci = o >> 5, co = o & 31;
        wt[((ci >> 5) * 32 + co) * 32 + igemm_kpos(ci & 31)] = co < K ? head[ci * K + co] : 0.0f;
    } else if (o < 4096 + 32) {
        wt[o] = (o - 4096) < K ? 1.0f : 0.0f;
    } else if (o < 4096 + 64) {
        const int co = o - 4096 - 32;
        wt[o] = co < K ? head[128 * K + co] : 0.0f;
    }
}

hipError_t launch_icnet_head_pack(const float *head, int K, float *wt, hipStream_t s)
{
    if (K < 2 || K > 32) return hipErrorInvalidValue;
    ProfScope prof("k_icnet_head_pack", 0.0, 4.0 * (129.0 * K + 4160.0), s);
    hipLaunchKernelGGL(k_icnet_head_pack, dim3((4096 + 64 + 255) / 256), dim3(256), 0, s, head, K, wt);
    return hipGetLastError();
}

// The weight the legacy resize by `f` (4: lq -> loss pixels, 2: sub12_sum -> lq) gives source index `src` in destination
// index `dst` along one axis of `size` source entries: dst reads src0 = dst / f with 1 - l and min(src0 + 1, size - 1) with
// l = (dst % f) / f -- the clamped tap folds onto the last entry exactly as the forward reads it.  Exact in fp32.
__device__ __forceinline__ float resize_weight(int dst, int src, int size, int f)
{
    const int s0 = dst / f, s1 = min(s0 + 1, size - 1);
    const float l = (float)(dst % f) * (1.0f / (float)f);
    return (s0 == src ? 1.0f - l : 0.0f) + (s1 == src ? l : 0.0f);
}

// x = sub12_sum [N,h8,w8,128]; lq [N,2 h8,2 w8,K] (the forward launch's output); labels uint8 / mask fp32 [N,8 h8,8 w8].
// part [G][128 K + K] fp32 (un-normalised dL/dKernel as [c][k], then dL/dBias), lpart [G][2] float64 (sum of the
// per-position batch sums of ce, sum of the mask).
//
// Workgroup = tiles blockIdx.x, blockIdx.x + G, ... of 8 x 8 pixels of lq = 32 x 32 loss pixels, for ALL N images, so the
// per-position fp32 batch sum of the loss is taken in k_masked_xent's order (images ascending).  Per image of a tile:
//   (1) the 9 x 9 x K window of lq -> LDS (zeros outside the map: the clamped taps never read them);
//   (2) four bands of 8 x 32 loss pixels, one pixel per thread: the K logits in launch_resize_bilinear's arithmetic
//       (top = tl + (tr - tl) xl, bot likewise, top + (bot - top) yl), xent_pixel (ssal_xent.h, the code of k_masked_xent),
//       dL/dlogit -> LDS gl; then a GATHER, not a scatter: one thread per (window pixel of the band's three window rows,
//       class quad) adds the weighted dL/dlogit of the band's pixels that read it, rows then columns ascending, to
//       gw [81][K] = dL/dlq of this tile's pixels (a window pixel on a tile border is completed by the neighbouring tile;
//       dKernel and dBias are sums over pixels, so the partial sums need not meet);
//   (3) the same gather once more, through the 2x resize: hw [36][K] = the pull-back of gw onto the 6 x 6 window of
//       sub12_sum, which is staged next to it.  sum_q f(q, c) gw(q, k) with f = resize_2x(sub12_sum) is, re-associated,
//       sum_s x(s, c) hw(s, k): f is never formed, and the contraction runs over 36 instead of 81 pixels;
//   (4) the contraction: one thread per 4 x 4 (channel, class) block, dKernel[c][k] += sum_s x(s, c) hw(s, k), s row-major,
//       accumulators in registers across all tiles and images of the workgroup; dBias[k] += sum_s hw(s, k) (the resize
//       weights of a pixel sum to 1) in the threads of channel block 0.
//
// SEMI: sa.labelled[n] == 0 replaces the label / mask of image n, which are then never read, by the
// pseudo annotation of active_learning.py:229-275 -- (conf, lab) = pixel_score (ssal_score.h, the code of k_upscore) of the
// interpolated logits the thread holds, mask = conf < threshold ? 0 : 1 (NaN -> 1).  The targets are constants
// (tf.stop_gradient, :233): the loss, dL/dlogit, both gathers and the contraction do not change.  With sa.tgt_in the targets
// of an unlabelled image come from that plane instead (a byte per loss pixel: the label in bits 0..6, the mask in bit 7),
// which a TARGET-ONLY launch (sa.tgt_out, lq = the head's output on the undistorted frame's features) wrote: phase (1) and
// the logits of phase (2) for the unlabelled images, nothing else -- no gradient, no partials, no sums.  sa.rep: every loss
// pixel adds (int)mask at [label][first maximum of the TRAINING logits] of a u32 LDS histogram (ssal_confusion.h), flushed
// into replica (workgroup % reps) at the end; a loss pixel belongs to exactly one tile.  sa.pseudo_pixels[n] += the image's
// pixels with pseudo mask 1 (one integer atomic per wave, tile and unlabelled image).
struct IcnetHeadPlain {};  // SEMI = false: no argument
// HWOUT: every tile also leaves its pull-back window hw [36][K] as it stands -- partial sums where
// the window overlaps a neighbouring tile's -- at hw[(n tiles + tile) 36 K], for the fusion trainer's gather into
// dL/dsub12_sum.  Nothing else changes: loss, dKernel and dBias are the bits of the plain instantiation.
struct IcnetHeadHw { float *hw; };
// SEMI and HWOUT: the semi-supervised step of the fusion and the cascade trainer.  The targets are
// constants, so the window is the plain one's on the composed targets; a target-only launch never takes this form.
struct IcnetHeadSemiHw : IcnetHeadSemi { float *hw; };
template <bool SEMI, bool HWOUT>
using IcnetHeadArg = std::conditional_t<SEMI, std::conditional_t<HWOUT, IcnetHeadSemiHw, IcnetHeadSemi>,
                                        std::conditional_t<HWOUT, IcnetHeadHw, IcnetHeadPlain>>;

template <int K, bool SEMI, bool HWOUT = false>
__global__ __launch_bounds__(256) void k_icnet_head_grad(const float *__restrict__ x, const float *__restrict__ lq, int N,
                                                         int h8, int w8, const uint8_t *__restrict__ labels,
                                                         const float *__restrict__ mask, float weight, float on_value,
                                                         float off_value, float *__restrict__ part,
                                                         double *__restrict__ lpart, IcnetHeadArg<SEMI, HWOUT> sa)
{
    constexpr int K4 = (K + 3) / 4 * 4, KB = K4 / 4;
    constexpr int KLD = K4 % 8 == 0 ? K4 + 4 : K4;  // row stride of the LDS planes: quads of neighbouring rows on other banks
    constexpr int BIG = 256 * KLD > IH_SP * (128 + KLD) ? 256 * KLD : IH_SP * (128 + KLD);
    static_assert(3 * IH_TP * KB <= 256 && 32 * KB <= 256, "one gather / contraction item per thread");
    __shared__ double red[4];
    __shared__ __attribute__((aligned(16))) float lqw[IH_WP * KLD];
    __shared__ __attribute__((aligned(16))) float gw[IH_WP * KLD];
    __shared__ __attribute__((aligned(16))) float big[BIG];
    __shared__ unsigned hist[SEMI ? K * K : 1];  // (never referenced, so not allocated, without SEMI)
    float *gl = big;                  // (2): dL/dlogit of a band [256][KLD]
    float *xw = big;                  // (3), (4): the sub12_sum window [36][128] ...
    float *hw = big + IH_SP * 128;    // ... and the pull-back [36][KLD]
    const int tid = threadIdx.x;
    const int Hq = 2 * h8, Wq = 2 * w8;
    const long Ho = 8L * h8, Wo = 8L * w8;
    const int tiles_x = (Wq + IH_T - 1) / IH_T, tiles = tiles_x * ((Hq + IH_T - 1) / IH_T);
    const int ry = tid >> 5, cx = tid & 31;  // (2): the thread's loss pixel inside a band
    const int cb = tid & 31, kbc = tid >> 5;  // (4): the thread's channel quad and class quad
    float acc[16], bacc[4];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e) bacc[e] = 0.0f;
    double loss = 0.0, msum = 0.0;
    float wc = 1.0f, dwc_cw = 0.0f;  // class weight constants (weight > 1): c_w = e - 1 - weight
    const float cw = kXentEuler - weight;
    bool tgt_only = false;
    if constexpr (SEMI) {
        tgt_only = sa.tgt_out != nullptr;
        if (sa.rep) hist_zero(hist, K * K);  // (ordered before the first add by the barriers of the first image)
    }
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int i0 = (t / tiles_x) * IH_T, j0 = (t % tiles_x) * IH_T;  // the tile's first pixel of lq
        float bsum[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // tf.reduce_sum(loss, axis=0) in fp32, per loss pixel of the thread
        for (int n = 0; n < N; ++n) {
            // SEMI: image n is pseudo-annotated (workgroup-uniform)
            bool pseudo = false;
            int npseudo = 0;
            if constexpr (SEMI) {
                pseudo = sa.labelled && sa.labelled[n] == 0;
                if (tgt_only && !pseudo) continue;  // a labelled image needs no pseudo targets
            }
            __syncthreads();  // the previous contraction is done with xw / hw, the previous gather with gw
            for (int e = tid; e < IH_WP * KB; e += 256) {
                const int wp = e / KB, kb = e % KB;
                const int gi = i0 + wp / IH_TP, gj = j0 + wp % IH_TP;
                float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (gi < Hq && gj < Wq) {
                    const float *src = lq + (((long)n * Hq + gi) * Wq + gj) * K + 4 * kb;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
                        if (K % 4 == 0 || 4 * kb + a < K) v[a] = src[a];
                }
                *reinterpret_cast<float4 *>(lqw + wp * KLD + 4 * kb) = make_float4(v[0], v[1], v[2], v[3]);
                *reinterpret_cast<float4 *>(gw + wp * KLD + 4 * kb) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            __syncthreads();
#pragma unroll 1
            for (int b = 0; b < 4; ++b) {
                const int oy = 8 * b + ry;  // the loss pixel (oy, cx) of the tile
                const long y = 4L * i0 + oy, xo = 4L * j0 + cx;
                float *gq = gl + tid * KLD;
                if (y < Ho && xo < Wo) {
                    const int r0 = oy >> 2, c0 = cx >> 2;
                    const int r1 = i0 + r0 + 1 <= Hq - 1 ? r0 + 1 : r0, c1 = j0 + c0 + 1 <= Wq - 1 ? c0 + 1 : c0;
                    const float ly = (float)(oy & 3) * 0.25f, lx = (float)(cx & 3) * 0.25f;
                    const float *ptl = lqw + (r0 * IH_TP + c0) * KLD, *ptr = lqw + (r0 * IH_TP + c1) * KLD;
                    const float *pbl = lqw + (r1 * IH_TP + c0) * KLD, *pbr = lqw + (r1 * IH_TP + c1) * KLD;
                    float xl[K];
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const float top = ptl[k] + (ptr[k] - ptl[k]) * lx;
                        const float bot = pbl[k] + (pbr[k] - pbl[k]) * lx;
                        xl[k] = top + (bot - top) * ly;
                    }
                    const long op = ((long)n * Ho + y) * Wo + xo;
                    int lab;
                    float mk;
                    if constexpr (SEMI) {
                        if (tgt_only) {
                            const float conf = pixel_score<K>(xl, sa.measure, 1.0f / __logf((float)K), lab);
                            sa.tgt_out[op] = (uint8_t)((unsigned)lab | (conf < sa.threshold ? 0u : 0x80u));
                            continue;
                        }
                        if (pseudo) {
                            if (sa.tgt_in) {
                                const unsigned tb = sa.tgt_in[op];
                                lab = (int)(tb & 0x7Fu);
                                mk = (tb & 0x80u) ? 1.0f : 0.0f;
                            } else {
                                mk = pixel_score<K>(xl, sa.measure, 1.0f / __logf((float)K), lab) < sa.threshold ? 0.0f : 1.0f;
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
                    bsum[b] += r.ce;
                    msum += (double)mk;
                    // dL/dx_k (before the 1 / sum(mask) factor), as k_final_grad:
                    //   g_k = mask (w (s_k - y_k) + ce0 w' s_k (y_k - p_class)),  w' = -w^2 c_w / u
                    if (weight > 1.0f) {
                        const float u = weight + cw * r.pc;
                        wc = 1.0f / logf(u);
                        dwc_cw = -(wc * wc) * cw / u;
                    }
                    const float a1 = mk * wc, a2 = mk * r.ce0 * dwc_cw;
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
                } else {
#pragma unroll
                    for (int k = 0; k < K4; ++k) gq[k] = 0.0f;
                }
                if constexpr (SEMI) {
                    if (tgt_only) continue;  // (workgroup-uniform: no barrier is skipped by a part of the workgroup)
                }
                __syncthreads();
                if (tid < 3 * IH_TP * KB) {  // the band's pixels read the window rows 2b, 2b + 1, 2b + 2
                    const int kb = tid % KB, wr = 2 * b + (tid / KB) / IH_TP, wcn = (tid / KB) % IH_TP;
                    const int gi = i0 + wr, gj = j0 + wcn;
                    if (gi < Hq && gj < Wq) {
                        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        const int c_lo = max(4 * (wcn - 1), 0), c_hi = min(4 * wcn + 3, IH_OT - 1);
                        for (int r2 = 0; r2 < 8; ++r2) {
                            const float wy = resize_weight(4 * i0 + 8 * b + r2, gi, Hq, 4);
                            if (wy == 0.0f) continue;
                            for (int c2 = c_lo; c2 <= c_hi; ++c2) {
                                const float wx = resize_weight(4 * j0 + c2, gj, Wq, 4);
                                if (wx == 0.0f) continue;
                                const float wgt = wy * wx;
                                const float4 g = *reinterpret_cast<const float4 *>(gl + (r2 * 32 + c2) * KLD + 4 * kb);
                                a.x = fmaf(wgt, g.x, a.x);
                                a.y = fmaf(wgt, g.y, a.y);
                                a.z = fmaf(wgt, g.z, a.z);
                                a.w = fmaf(wgt, g.w, a.w);
                            }
                        }
                        float4 *dst = reinterpret_cast<float4 *>(gw + (wr * IH_TP + wcn) * KLD + 4 * kb);
                        const float4 o = *dst;
                        *dst = make_float4(o.x + a.x, o.y + a.y, o.z + a.z, o.w + a.w);
                    }
                }
                __syncthreads();  // gl is free for the next band (or for xw / hw), gw is complete up to this band
            }
            if constexpr (SEMI) {
                if (tgt_only) continue;
                if (pseudo && sa.pseudo_pixels) {
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) npseudo += __shfl_down(npseudo, off, 64);
                    if ((tid & 63) == 0 && npseudo) atomicAdd(sa.pseudo_pixels + n, (unsigned long long)npseudo);
                }
            }
            const int s0 = i0 >> 1, t0 = j0 >> 1;  // the window's first pixel of sub12_sum
            for (int e = tid; e < IH_SP * 32; e += 256) {
                const int p = e >> 5;
                const int gr = s0 + p / IH_SS, gc = t0 + p % IH_SS;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (gr < h8 && gc < w8) v = reinterpret_cast<const float4 *>(x + (((long)n * h8 + gr) * w8 + gc) * 128)[e & 31];
                reinterpret_cast<float4 *>(xw)[e] = v;
            }
            for (int e = tid; e < IH_SP * KB; e += 256) {
                const int p = e / KB, kb = e % KB;
                const int gr = s0 + p / IH_SS, gc = t0 + p % IH_SS;
                float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (gr < h8 && gc < w8) {
                    for (int wr = 0; wr < IH_TP && i0 + wr < Hq; ++wr) {
                        const float wy = resize_weight(i0 + wr, gr, h8, 2);
                        if (wy == 0.0f) continue;
                        for (int wcn = 0; wcn < IH_TP && j0 + wcn < Wq; ++wcn) {
                            const float wx = resize_weight(j0 + wcn, gc, w8, 2);
                            if (wx == 0.0f) continue;
                            const float wgt = wy * wx;
                            const float4 g = *reinterpret_cast<const float4 *>(gw + (wr * IH_TP + wcn) * KLD + 4 * kb);
                            a.x = fmaf(wgt, g.x, a.x);
                            a.y = fmaf(wgt, g.y, a.y);
                            a.z = fmaf(wgt, g.z, a.z);
                            a.w = fmaf(wgt, g.w, a.w);
                        }
                    }
                }
                *reinterpret_cast<float4 *>(hw + p * KLD + 4 * kb) = a;
            }
            __syncthreads();
            if constexpr (HWOUT) {
                float *dst = sa.hw + ((long)n * tiles + t) * (IH_SP * K);
                for (int e = tid; e < IH_SP * K; e += 256) dst[e] = hw[(e / K) * KLD + e % K];
            }
            if (tid < 32 * KB) {
                const float4 *f4 = reinterpret_cast<const float4 *>(xw) + cb;
                const float *hp = hw + 4 * kbc;
#pragma unroll 4
                for (int p = 0; p < IH_SP; ++p) {
                    const float4 f = f4[p * 32];
                    const float4 g = *reinterpret_cast<const float4 *>(hp + p * KLD);
                    const float gk[4] = {g.x, g.y, g.z, g.w}, fc[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[a * 4 + c] = fmaf(gk[a], fc[c], acc[a * 4 + c]);
                        bacc[a] += gk[a];
                    }
                }
            }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) loss += (double)bsum[b];  // (0 where the thread's pixel lies outside the map)
    }
    if constexpr (SEMI) {
        if (tgt_only) return;
    }
    float *pw = part + (long)blockIdx.x * (129 * K);
    if (tid < 32 * KB) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int k = kbc * 4 + a;
            if (K % 4 == 0 || k < K) {
#pragma unroll
                for (int c = 0; c < 4; ++c) pw[(cb * 4 + c) * K + k] = acc[a * 4 + c];
                if (cb == 0) pw[128 * K + k] = bacc[a];
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
// loss = (sum of the lpart sums) / (double)(float)sum(mask), as k_xent_finish and k_final_grad_finish
__global__ __launch_bounds__(256) void k_icnet_head_finish(const float *__restrict__ part, const double *__restrict__ lpart,
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
        const double msum = (double)(float)rb;
        scale = (float)(1.0 / msum);
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

// the K switch of one launch of the template
#define SSAL_IH_CASES                                                                                                  \
    SSAL_IH(2) SSAL_IH(3) SSAL_IH(4) SSAL_IH(5) SSAL_IH(6) SSAL_IH(7) SSAL_IH(8) SSAL_IH(9) SSAL_IH(10) SSAL_IH(11)      \
    SSAL_IH(12) SSAL_IH(13) SSAL_IH(14) SSAL_IH(15) SSAL_IH(16) SSAL_IH(17) SSAL_IH(18) SSAL_IH(19) SSAL_IH(20)         \
    SSAL_IH(21) SSAL_IH(22) SSAL_IH(23) SSAL_IH(24) SSAL_IH(25) SSAL_IH(26) SSAL_IH(27) SSAL_IH(28) SSAL_IH(29)         \
    SSAL_IH(30) SSAL_IH(31) SSAL_IH(32)

static bool icnet_head_semi_ok(const IcnetHeadSemi *semi)
{
    return !semi || (semi->measure >= 0 && semi->measure <= 2 && (!semi->rep || semi->reps >= 1));
}

// sub12_sum_interp (2x) + conv6_cls (1x1, bias) on the packed head in ws.wt: the launch of the forward path
// (ssal_icnet_api.hip, run_trunk)
static hipError_t launch_icnet_head_lq(const float *sub12, int N, int h8, int w8, int K, const IcnetHeadWs &ws, hipStream_t s)
{
    return launch_igemm(sub12, N, h8, w8, 128, ws.wt, 1, 1, K, 1, 1, ws.wt + 4096, ws.wt + 4096 + 32, nullptr, false, true,
                        ws.lq, s);
}

hipError_t launch_icnet_head_targets(const float *sub12_raw, int N, int h8, int w8, int K, const float *head,
                                     int max_workgroups, const IcnetHeadWs &ws, const IcnetHeadSemi &semi, uint8_t *tgt,
                                     hipStream_t s)
{
    if (N < 1 || K < 2 || K > 32 || max_workgroups < 0 || !icnet_head_fits(h8, w8) || !icnet_head_semi_ok(&semi) || !tgt ||
        !sub12_raw)
        return hipErrorInvalidValue;
    hipError_t e = launch_icnet_head_pack(head, K, ws.wt, s);
    if (e != hipSuccess) return e;
    if (!semi.labelled) return hipSuccess;  // every image is labelled: no pseudo target is read
    const int G = icnet_head_workgroups(h8, w8, max_workgroups);
    e = launch_icnet_head_lq(sub12_raw, N, h8, w8, K, ws, s);
    if (e != hipSuccess) return e;
    IcnetHeadSemi sa = semi;
    sa.tgt_in = nullptr;
    sa.tgt_out = tgt;
    sa.rep = nullptr;
    sa.pseudo_pixels = nullptr;
    const double pix = (double)N * h8 * w8;
    // the interpolation and the score of every loss pixel (counted for all images), one byte out
    ProfScope prof("k_icnet_head_targets", 64.0 * pix * 12.0 * K, 4.0 * 4 * pix * K + 64.0 * pix, s);
#define SSAL_IH(KK)                                                                                                    \
    case KK:                                                                                                           \
        hipLaunchKernelGGL((k_icnet_head_grad<KK, true>), dim3(G), dim3(256), 0, s, sub12_raw, ws.lq, N, h8, w8,        \
                           nullptr, nullptr, 0.0f, 1.0f, 0.0f, ws.part, ws.lpart, sa);                                 \
        break;
    switch (K) {
        SSAL_IH_CASES
    default:
        return hipErrorInvalidValue;
    }
#undef SSAL_IH
    return hipGetLastError();
}

hipError_t launch_icnet_head_grad(const float *sub12, int N, int h8, int w8, int K, const float *head,
                                  const uint8_t *labels, const float *mask, float weight, float label_smoothing,
                                  int max_workgroups, const IcnetHeadWs &ws, double *loss, float *grad, hipStream_t s,
                                  const IcnetHeadSemi *semi, float *hw_out)
{
    if (N < 1 || K < 2 || K > 32 || max_workgroups < 0 || !icnet_head_fits(h8, w8) || !icnet_head_semi_ok(semi))
        return hipErrorInvalidValue;
    const int G = icnet_head_workgroups(h8, w8, max_workgroups);
    hipError_t e;
    if (semi && semi->pseudo_pixels) {
        e = hipMemsetAsync(semi->pseudo_pixels, 0, (size_t)N * sizeof(int64_t), s);
        if (e != hipSuccess) return e;
    }
    if (!(semi && semi->tgt_in)) {  // (the target launch before this one packed the same head into ws.wt)
        e = launch_icnet_head_pack(head, K, ws.wt, s);
        if (e != hipSuccess) return e;
    }
    e = launch_icnet_head_lq(sub12, N, h8, w8, K, ws, s);
    if (e != hipSuccess) return e;
    const float on_value = 1.0f - label_smoothing, off_value = label_smoothing / ((float)K - 1.0f);
    const double pix = (double)N * h8 * w8;
    if (hw_out && !semi) {
        ProfScope prof("k_icnet_head_grad_hw", 64.0 * pix * 12.0 * K + 2.0 * pix * 128 * K,
                       4.0 * pix * 128 + 4.0 * 4 * pix * K + 64.0 * pix * (1 + 4) + 4.0 * G * 129.0 * K +
                           4.0 * N * icnet_head_tiles(h8, w8) * IH_SP * K, s);
#define SSAL_IH(KK)                                                                                                    \
    case KK:                                                                                                           \
        hipLaunchKernelGGL((k_icnet_head_grad<KK, false, true>), dim3(G), dim3(256), 0, s, sub12, ws.lq, N, h8, w8,     \
                           labels, mask, weight, on_value, off_value, ws.part, ws.lpart, IcnetHeadHw{hw_out});         \
        break;
        switch (K) {
            SSAL_IH_CASES
        default:
            return hipErrorInvalidValue;
        }
#undef SSAL_IH
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    } else if (!semi) {
        ProfScope prof("k_icnet_head_grad", 64.0 * pix * 12.0 * K + 2.0 * pix * 128 * K,
                       4.0 * pix * 128 + 4.0 * 4 * pix * K + 64.0 * pix * (1 + 4) + 4.0 * G * 129.0 * K, s);
#define SSAL_IH(KK)                                                                                                    \
    case KK:                                                                                                           \
        hipLaunchKernelGGL((k_icnet_head_grad<KK, false>), dim3(G), dim3(256), 0, s, sub12, ws.lq, N, h8, w8, labels,   \
                           mask, weight, on_value, off_value, ws.part, ws.lpart, IcnetHeadPlain{});                    \
        break;
        switch (K) {
            SSAL_IH_CASES
        default:
            return hipErrorInvalidValue;
        }
#undef SSAL_IH
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    } else if (hw_out) {
        IcnetHeadSemiHw sa;
        static_cast<IcnetHeadSemi &>(sa) = *semi;
        sa.tgt_out = nullptr;
        if (!sa.labelled) sa.tgt_in = nullptr;
        sa.hw = hw_out;
        ProfScope prof("k_icnet_head_grad_semi_hw", 64.0 * pix * 12.0 * K + 2.0 * pix * 128 * K,
                       4.0 * pix * 128 + 4.0 * 4 * pix * K + 64.0 * pix * (1 + 4) + 4.0 * G * 129.0 * K +
                           4.0 * N * icnet_head_tiles(h8, w8) * IH_SP * K, s);
#define SSAL_IH(KK)                                                                                                    \
    case KK:                                                                                                           \
        hipLaunchKernelGGL((k_icnet_head_grad<KK, true, true>), dim3(G), dim3(256), 0, s, sub12, ws.lq, N, h8, w8,      \
                           labels, mask, weight, on_value, off_value, ws.part, ws.lpart, sa);                          \
        break;
        switch (K) {
            SSAL_IH_CASES
        default:
            return hipErrorInvalidValue;
        }
#undef SSAL_IH
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    } else {
        IcnetHeadSemi sa = *semi;
        sa.tgt_out = nullptr;
        if (!sa.labelled) sa.tgt_in = nullptr;
        ProfScope prof("k_icnet_head_grad_semi", 64.0 * pix * 12.0 * K + 2.0 * pix * 128 * K,
                       4.0 * pix * 128 + 4.0 * 4 * pix * K + 64.0 * pix * (1 + 4) + 4.0 * G * 129.0 * K, s);
#define SSAL_IH(KK)                                                                                                    \
    case KK:                                                                                                           \
        hipLaunchKernelGGL((k_icnet_head_grad<KK, true>), dim3(G), dim3(256), 0, s, sub12, ws.lq, N, h8, w8, labels,    \
                           mask, weight, on_value, off_value, ws.part, ws.lpart, sa);                                  \
        break;
        switch (K) {
            SSAL_IH_CASES
        default:
            return hipErrorInvalidValue;
        }
#undef SSAL_IH
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int count = 129 * K;
    ProfScope prof("k_icnet_head_finish", (double)G * count, 4.0 * G * count + 16.0 * G, s);
    hipLaunchKernelGGL(k_icnet_head_finish, dim3((count + 255) / 256), dim3(256), 0, s, ws.part, ws.lpart, G, count, loss,
                       grad);
    return hipGetLastError();
}
#undef SSAL_IH_CASES

}  // namespace ssal
