// ssal_train_block.hip -- training of ENet's last block (Bottleneck5_1 + Final.kernel) over a frozen trunk, gfx950:
//   k_tb_fold    the packed block with batch-norm folded (s = gamma / sqrt(var + 1e-3), t = fma(-mean, s, beta), as
//                ssal_enet_commit folds it on the host) and 1 / sqrt(var + 1e-3) in the variance slots
//   k_tb_head    Bottleneck5_1's forward on an 18 x 18 window, the Final logits, the masked softmax cross entropy and
//                dL/dlogit on a 17 x 17 window of 2 x 2 output quads; dL/dW of Final.kernel as per-workgroup partials and
//                dL/d(Bottleneck5_1 output) to HBM (neither the logits nor dL/dlogit reach HBM)
//   k_tb_head<K, true>  (profiled as k_tb_head_semi) the same with the semi-supervised targets and the training metrics in
//                the kernel: an unlabelled image is trained on its own pseudo annotation, the
//                tile's pixels are counted into the confusion matrix; as a target-only launch it writes the packed pseudo
//                targets of the undistorted frame instead
//   k_tb_block   Bottleneck5_1's forward again and its backward: per-workgroup partials of the 13 block gradients
//   k_tb_finish  fixed-order fold of the partials, times 1 / sum(mask); the float64 loss
// Semantics: enet_modules.py:526-599 in inference mode (moving statistics are constants, no dropout), Final's transposed
// convolution, tensortools/losses.py:3-74.  PReLU is relu(x) - alpha relu(-x) (extra_ops.py:9-26):
// at x == 0 TensorFlow's ReluGrad gives 0 on both branches, so d/dx = 0 and d/dalpha = 0 there.  No floating-point atomics:
// two runs give the same bits.
#include "ssal_confusion.h"
#include "ssal_internal.h"
#include "ssal_prof.h"
#include "ssal_score.h"
#include "ssal_train_block.h"
#include "ssal_train_common.h"
#include "ssal_xent.h"
#include <type_traits>

namespace ssal {

namespace {

constexpr int TB_T = 16;        // feature pixels per tile side (FG_T of the output-layer gradient)
constexpr int TB_GW = TB_T + 1;  // dL/dlogit window: the tile plus one row below and one column to the right
constexpr int TB_AW = TB_T + 2;  // Bottleneck5_1 output window: one more row above and column to the left
constexpr int TB_PW = TB_T + 4;  // projected window
constexpr int TB_SEG = 86;       // pixels per third of the block contractions (3 x 86 >= 256)

// one pixel of x5 [H,W,16] with clamped coordinates; ok = inside the image
__device__ __forceinline__ bool tb_load16(const float *__restrict__ x5, int H, int W, int gi, int gj, float (&v)[16])
{
    const bool ok = gi >= 0 && gi < H && gj >= 0 && gj < W;
    const float4 *xp = reinterpret_cast<const float4 *>(x5 + ((long)min(max(gi, 0), H - 1) * W + min(max(gj, 0), W - 1)) * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 t = xp[q];
        v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
    return ok;
}

// projection 16 -> 4 (the fmaf chain of k_bottleneck16 / k_final_score<F51>: ci ascending)
__device__ __forceinline__ void tb_proj(const float (&xv)[16], const float *__restrict__ f, float (&acc)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = 0.0f;
#pragma unroll
    for (int ci = 0; ci < 16; ++ci)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(xv[ci], f[TB_WP + ci * 4 + k], acc[k]);
}

// phase P: the projected tensor (BN + PReLU; exact zeros outside the image: SAME padding applies to it) on the
// TB_PW x TB_PW window whose corner is image pixel (i0 - 2, j0 - 2)
__device__ __forceinline__ void tb_phase_p(const float *__restrict__ x5, int H, int W, int i0, int j0,
                                           const float *__restrict__ f, float *p1)
{
#pragma unroll 1
    for (int e = threadIdx.x; e < TB_PW * TB_PW; e += 256) {
        float xv[16], acc[4];
        const bool ok = tb_load16(x5, H, W, i0 - 2 + e / TB_PW, j0 - 2 + e % TB_PW, xv);
        tb_proj(xv, f, acc);
        float4 o;
        o.x = ok ? prelu(fmaf(acc[0], f[TB_PG + 0], f[TB_PB + 0]), f[TB_PA + 0]) : 0.0f;
        o.y = ok ? prelu(fmaf(acc[1], f[TB_PG + 1], f[TB_PB + 1]), f[TB_PA + 1]) : 0.0f;
        o.z = ok ? prelu(fmaf(acc[2], f[TB_PG + 2], f[TB_PB + 2]), f[TB_PA + 2]) : 0.0f;
        o.w = ok ? prelu(fmaf(acc[3], f[TB_PG + 3], f[TB_PB + 3]), f[TB_PA + 3]) : 0.0f;
        reinterpret_cast<float4 *>(p1)[e] = o;
    }
}

// the rest of the block at one pixel whose 3 x 3 projected neighbourhood starts at p1 index (pi, pj): conv 3x3 (taps and
// channels ascending), BN, PReLU, expansion, BN, + x, (PReLU left to the caller: u is its input)
struct TbPix {
    float accc[4], yc[4], qv[4], ev[16], u[16];
};
__device__ __forceinline__ void tb_conv_exp(const float *p1, int pi, int pj, const float *__restrict__ f,
                                            const float (&xres)[16], TbPix &r)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) r.accc[k] = 0.0f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const float4 pv = reinterpret_cast<const float4 *>(p1)[(pi + kh) * TB_PW + (pj + kw)];
            const float pc[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
            for (int ci = 0; ci < 4; ++ci)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    r.accc[k] = fmaf(pc[ci], f[TB_WC + ((kh * 3 + kw) * 4 + ci) * 4 + k], r.accc[k]);
        }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r.yc[k] = fmaf(r.accc[k], f[TB_CG + k], f[TB_CB + k]);
        r.qv[k] = prelu(r.yc[k], f[TB_CA + k]);
    }
#pragma unroll
    for (int co = 0; co < 16; ++co) {
        float ev = 0.0f;
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) ev = fmaf(r.qv[ci], f[TB_WE + ci * 16 + co], ev);
        r.ev[co] = ev;
        r.u[co] = fmaf(ev, f[TB_EG + co], f[TB_EB + co]) + xres[co];
    }
}

}  // namespace

bool train_block_fits(int H, int W) { return final_grad_fits(H, W); }
int train_block_workgroups(int H, int W) { return final_grad_workgroups(H, W); }

__global__ __launch_bounds__(512) void k_tb_fold(const float *__restrict__ params, float *__restrict__ fold)
{
    const int i = threadIdx.x;
    if (i >= TB_FINAL) return;
    float v = params[i];
    int g = -1, pv = 0, pm = 0, pb = 0;  // gamma slot, variance, mean, beta of the channel this slot belongs to
    if (i >= TB_PG && i < TB_PA) { const int j = (i - TB_PG) & 3; g = TB_PG + j; pv = TB_PV + j; pm = TB_PM + j; pb = TB_PB + j; }
    if (i >= TB_CG && i < TB_CA) { const int j = (i - TB_CG) & 3; g = TB_CG + j; pv = TB_CV + j; pm = TB_CM + j; pb = TB_CB + j; }
    if (i >= TB_EG && i < TB_RA) { const int j = (i - TB_EG) & 15; g = TB_EG + j; pv = TB_EV + j; pm = TB_EM + j; pb = TB_EB + j; }
    if (g >= 0) {
        const float sg = params[g] / sqrtf(params[pv] + 1e-3f);
        v = i == g ? sg : fmaf(-params[pm], sg, params[pb]);
    }
    if ((i >= TB_PV && i < TB_CM) || (i >= TB_CV && i < TB_EM) || (i >= TB_EV && i < TB_EV + 16))
        v = 1.0f / sqrtf(v + 1e-3f);
    fold[i] = v;
}

// Workgroup = one 16 x 16 tile of feature pixels for ALL N images, tiles blockIdx.x, blockIdx.x + G, ... (the loss' per-
// position fp32 batch sum runs over the images in ascending order, as in k_masked_xent and k_final_grad).  Per image:
//   P, C  Bottleneck5_1 on the 18 x 18 window (i0 - 1 .., j0 - 1 ..) -> tile (zeros outside the image)
//   per output quad q = 0 .. 3 (parity of the output row, column):
//     (a) thread = feature pixel (and threads 0 .. 32 a second time for the 33 pixels of the row below and the column to
//         the right, where only the quads the tile's pixels feed are taken): the logits of the quad in k_final_score's
//         tap / channel order, xent_pixel, dL/dlogit -> gl[17 x 17][K4]; loss and mask sums from the tile's pixels only
//     (b) Final.kernel: dW[tap][k][c] += sum over the tile's 256 pixels (row-major) of gl[p][k] * tile[src(tap, p)][c] for
//         the taps of quad q, one thread per 4 x 4 (class, channel) block, accumulators in registers across tiles, images
//     (c) dL/dx[p][c] += sum_k gl[p'][k] * wk[tap][k][c] over the (pixel, tap) pairs of quad q that read pixel p
//   then dL/dx of the tile's pixels -> dy.
//
// SEMI: sa.labelled[n] == 0 replaces the label / mask of image n, which are then never read, by the
// pseudo annotation of active_learning.py:229-275 -- (conf, lab) = pixel_score (ssal_score.h, the code of k_final_score) of
// the logits the thread holds, mask = conf < threshold ? 0 : 1 (NaN -> 1) -- for the tile's own pixels and the 33 second-pass
// pixels alike.  The targets are constants (tf.stop_gradient, :233): nothing else in (a), (b), (c) changes.  With sa.tgt_in
// the targets of an unlabelled image come from that plane instead (a byte per output pixel: the label in bits 0..6, the mask
// in bit 7), which a TARGET-ONLY launch (sa.tgt_out, x5 = the undistorted frame's features) wrote: P, C and the logits of
// the own pixels of the unlabelled images, nothing else -- no gradient, no partials, no sums.  sa.rep: every OWN pixel adds
// (int)mask at [label][first maximum of the TRAINING logits] of a u32 LDS histogram (ssal_confusion.h), flushed into
// replica (workgroup % reps) at the end; a second-pass pixel is another tile's own pixel and is counted there.
// sa.pseudo_pixels[n] += the image's own pixels with pseudo mask 1 (one integer atomic per wave, tile and unlabelled image).
struct TbHeadSemi {
    const uint8_t *labelled;    // [N], NULL = all labelled
    int measure;
    float threshold;
    const uint8_t *tgt_in;      // [N,2H,2W] packed pseudo targets of the undistorted frames, NULL = from the training logits
    uint8_t *tgt_out;           // non-NULL: the target-only launch
    unsigned long long *rep;    // confusion replicas, NULL = no metrics
    int reps;
    unsigned long long *pseudo_pixels;  // [N] (zeroed by the launcher), NULL = not counted
};

struct TbHeadPlain {};  // SEMI = false: no argument

template <int K, bool SEMI>
__global__ __launch_bounds__(256) void k_tb_head(const float *__restrict__ x5, int N, int H, int W,
                                                 const float *__restrict__ fold, const float *__restrict__ wk,
                                                 const uint8_t *__restrict__ labels, const float *__restrict__ mask,
                                                 float weight, float on_value, float off_value, float *__restrict__ dy,
                                                 float *__restrict__ part, double *__restrict__ lpart,
                                                 std::conditional_t<SEMI, TbHeadSemi, TbHeadPlain> sa)
{
    constexpr int K4 = (K + 3) / 4 * 4, KB = K4 / 4;
    constexpr int NB = 9 * KB * 4, BPT = (NB + 255) / 256;
    __shared__ double red[4];
    __shared__ __attribute__((aligned(16))) float p1[TB_PW * TB_PW * 4];
    __shared__ __attribute__((aligned(16))) float tile[TB_AW * TB_AW * 16];
    __shared__ __attribute__((aligned(16))) float gl[TB_GW * TB_GW * K4];
    __shared__ unsigned hist[SEMI ? K * K : 1];  // (never referenced, so not allocated, without SEMI)
    const int tid = threadIdx.x;
    const int tiles_x = (W + TB_T - 1) / TB_T, tiles = tiles_x * ((H + TB_T - 1) / TB_T);
    const int ti = tid / TB_T, tj = tid % TB_T;
    // the second pixel of threads 0 .. 32: the row below the tile, the column to its right, the corner
    const int hi = tid < 16 ? 16 : (tid < 32 ? tid - 16 : 16), hj = tid < 16 ? tid : 16;
    const long Ho = 2L * H, Wo = 2L * W, HW = (long)H * W;
    float acc[BPT][16];
#pragma unroll
    for (int bb = 0; bb < BPT; ++bb)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[bb][e] = 0.0f;
    double loss = 0.0, msum = 0.0;
    float wc = 1.0f, dwc_cw = 0.0f;
    const float cw = kXentEuler - weight;
    bool tgt_only = false;
    if constexpr (SEMI) {
        tgt_only = sa.tgt_out != nullptr;
        if (sa.rep) hist_zero(hist, K * K);  // (ordered before the first add by the barriers of the first image)
    }
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int i0 = (t / tiles_x) * TB_T, j0 = (t % tiles_x) * TB_T;
        const bool valid = i0 + ti < H && j0 + tj < W;
        float bsum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int n = 0; n < N; ++n) {
            // SEMI: image n is pseudo-annotated (workgroup-uniform)
            bool pseudo = false;
            int npseudo = 0;
            if constexpr (SEMI) {
                pseudo = sa.labelled && sa.labelled[n] == 0;
                if (tgt_only && !pseudo) continue;  // a labelled image needs no pseudo targets
            }
            const float *xn = x5 + (long)n * HW * 16;
            __syncthreads();  // the previous image is done with p1 / tile / gl
            tb_phase_p(xn, H, W, i0, j0, fold, p1);
            __syncthreads();
#pragma unroll 1
            for (int e = tid; e < TB_AW * TB_AW; e += 256) {
                const int pi = e / TB_AW, pj = e % TB_AW;
                float xres[16];
                const bool ok = tb_load16(xn, H, W, i0 - 1 + pi, j0 - 1 + pj, xres);
                TbPix r;
                tb_conv_exp(p1, pi, pj, fold, xres, r);
                float out[16];
#pragma unroll
                for (int co = 0; co < 16; ++co) out[co] = ok ? prelu(r.u[co], fold[TB_RA + co]) : 0.0f;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    reinterpret_cast<float4 *>(tile)[e * 4 + q] = make_float4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
            }
            __syncthreads();
            float dyv[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) dyv[c] = 0.0f;
#pragma unroll 1
            for (int q = 0; q < 4; ++q) {
                // ---- (a)
#pragma unroll 1
                for (int ps = 0; ps < 2; ++ps) {
                    if (ps == 1 && (tid >= 2 * TB_T + 1 || tgt_only)) break;
                    const int gi = ps ? hi : ti, gj = ps ? hj : tj;
                    const bool own = ps == 0;
                    // a pixel below / right of the tile: only the quads that read a pixel of the tile
                    const bool need = own || (gi == TB_T && gj == TB_T ? q == 0 : (gi == TB_T ? q < 2 : (q & 1) == 0));
                    const int i = i0 + gi, j = j0 + gj;
                    float *gq = gl + (gi * TB_GW + gj) * K4;
                    if (need && i < H && j < W) {
                        const float *la = tile + ((gi + 1) * TB_AW + gj + 1) * 16;  // a = own, b = above, c = left, d = above-left
                        float xl[K];
#pragma unroll
                        for (int k = 0; k < K; ++k) xl[k] = 0.0f;
                        auto tap = [&](const float *v, int kh, int kw) __attribute__((always_inline)) {
                            const float *wt = wk + (kh * 3 + kw) * K * 16;
                            float vv[16];
#pragma unroll
                            for (int c4 = 0; c4 < 4; ++c4) {
                                const float4 t4 = reinterpret_cast<const float4 *>(v)[c4];
                                vv[4 * c4] = t4.x; vv[4 * c4 + 1] = t4.y; vv[4 * c4 + 2] = t4.z; vv[4 * c4 + 3] = t4.w;
                            }
#pragma unroll
                            for (int c = 0; c < 16; ++c)
#pragma unroll
                                for (int k = 0; k < K; ++k) xl[k] = fmaf(vv[c], wt[k * 16 + c], xl[k]);
                        };
                        const float *lb = la - TB_AW * 16, *lc = la - 16, *ld = la - TB_AW * 16 - 16;
                        if (q == 0) { tap(la, 0, 0); tap(lc, 0, 2); tap(lb, 2, 0); tap(ld, 2, 2); }
                        else if (q == 1) { tap(la, 0, 1); tap(lb, 2, 1); }
                        else if (q == 2) { tap(la, 1, 0); tap(lc, 1, 2); }
                        else { tap(la, 1, 1); }
                        const long op = ((long)n * Ho + 2 * i + (q >> 1)) * Wo + 2 * j + (q & 1);
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
                                    const unsigned b = sa.tgt_in[op];
                                    lab = (int)(b & 0x7Fu);
                                    mk = (b & 0x80u) ? 1.0f : 0.0f;
                                } else {
                                    mk = pixel_score<K>(xl, sa.measure, 1.0f / __logf((float)K), lab) < sa.threshold ? 0.0f : 1.0f;
                                }
                                if (own) npseudo += mk != 0.0f;
                            } else {
                                lab = labels[op];
                                mk = mask[op];
                            }
                            if (sa.rep && own) {  // train_pred = tf.math.argmax(train_logits): the first maximum
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
                        if (own) {
                            bsum[q] += r.ce;
                            msum += (double)mk;
                        }
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
                }
                if constexpr (SEMI) {
                    if (tgt_only) continue;  // (workgroup-uniform: no barrier is skipped by a part of the workgroup)
                }
                __syncthreads();
                // ---- (b)
#pragma unroll
                for (int bb = 0; bb < BPT; ++bb) {
                    const int b = tid + 256 * bb;
                    const int cb = b & 3, kb = (b >> 2) % KB, tp = (b >> 2) / KB;
                    const int kh = tp / 3, kw = tp % 3;
                    if ((NB % 256 == 0 || b < NB) && (kh == 1 ? 2 : 0) + (kw == 1 ? 1 : 0) == q) {
                        const int src0 = (1 - (kh == 2 ? 1 : 0)) * TB_AW + 1 - (kw == 2 ? 1 : 0);
                        const float4 *g4 = reinterpret_cast<const float4 *>(gl) + kb;
                        const float4 *f4 = reinterpret_cast<const float4 *>(tile) + cb;
#pragma unroll 4
                        for (int p = 0; p < 256; ++p) {
                            const float4 g = g4[((p / TB_T) * TB_GW + p % TB_T) * KB];
                            const float4 f = f4[(src0 + (p / TB_T) * TB_AW + p % TB_T) * 4];
                            const float gk[4] = {g.x, g.y, g.z, g.w}, fc[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                            for (int a = 0; a < 4; ++a)
#pragma unroll
                                for (int c = 0; c < 4; ++c) acc[bb][a * 4 + c] = fmaf(gk[a], fc[c], acc[bb][a * 4 + c]);
                        }
                    }
                }
                // ---- (c)
                if (valid) {
                    auto back = [&](int di, int dj, int tp) __attribute__((always_inline)) {
                        const float *g = gl + ((ti + di) * TB_GW + tj + dj) * K4;
                        const float *wt = wk + tp * K * 16;
#pragma unroll
                        for (int kq = 0; kq < KB; ++kq) {
                            const float4 g4 = reinterpret_cast<const float4 *>(g)[kq];
                            const float gk[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
                            for (int a = 0; a < 4; ++a)
                                if (kq * 4 + a < K)
#pragma unroll
                                    for (int c = 0; c < 16; ++c) dyv[c] = fmaf(gk[a], wt[(kq * 4 + a) * 16 + c], dyv[c]);
                        }
                    };
                    if (q == 0) { back(0, 0, 0); back(0, 1, 2); back(1, 0, 6); back(1, 1, 8); }
                    else if (q == 1) { back(0, 0, 1); back(1, 0, 7); }
                    else if (q == 2) { back(0, 0, 3); back(0, 1, 5); }
                    else { back(0, 0, 4); }
                }
                __syncthreads();
            }
            if constexpr (SEMI) {
                if (tgt_only) continue;
                if (pseudo && sa.pseudo_pixels) {
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) npseudo += __shfl_down(npseudo, off, 64);
                    if ((tid & 63) == 0 && npseudo) atomicAdd(sa.pseudo_pixels + n, (unsigned long long)npseudo);
                }
            }
            if (valid) {
                float4 *o = reinterpret_cast<float4 *>(dy + (((long)n * H + i0 + ti) * W + j0 + tj) * 16);
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = make_float4(dyv[4 * q], dyv[4 * q + 1], dyv[4 * q + 2], dyv[4 * q + 3]);
            }
        }
        if (valid)
#pragma unroll
            for (int q = 0; q < 4; ++q) loss += (double)bsum[q];
    }
    if constexpr (SEMI) {
        if (tgt_only) return;
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

// packed-block slot of the elementwise (per-channel) gradient number e of k_tb_block
__device__ __forceinline__ int tb_elem_slot(int e)
{
    if (e < 16) return TB_EG + e;
    if (e < 32) return TB_EB + e - 16;
    if (e < 48) return TB_RA + e - 32;
    if (e < 52) return TB_CG + e - 48;
    if (e < 56) return TB_CB + e - 52;
    if (e < 60) return TB_CA + e - 56;
    if (e < 64) return TB_PG + e - 60;
    if (e < 68) return TB_PB + e - 64;
    if (e < 72) return TB_PA + e - 68;
    return -1;
}

// Bottleneck5_1's backward.  Tiling as k_tb_head.  Per image of a tile:
//   P  the projected 20 x 20 window -> p1
//   C  18 x 18 pixels (the tile plus a ring of one): the forward up to the residual sum u, dy of the pixel, back through the
//      residual PReLU, the expansion and the convolution's BN + PReLU: dL/d(conv accumulator) -> dac (zeros outside the
//      image).  Pixels of the tile add their per-channel terms (exp_gamma, exp_beta, residual_alpha, conv_gamma, conv_beta,
//      conv_alpha) to the thread's registers and leave qv [4] and dL/d(exp accumulator) [16] in LDS.
//   D  thread = pixel of the tile: dL/dp = the convolution's input gradient from dac, back through the projection's PReLU and
//      BN (per-channel terms in registers); x [16] and dL/d(proj accumulator) [4] -> LDS
//   E  the three kernel gradients as contractions over the tile's pixels in row-major order: 68 threads (16 rows of
//      proj_kernel, 36 of conv_kernel, 16 quarter-rows of exp_kernel) x 3 thirds of the pixels, four accumulators each, kept
//      in registers across all tiles and images.
// gamma / beta gradients are produced directly: d gamma = sum dL/dy (acc - mean) / sqrt(var + 1e-3), d beta = sum dL/dy.
// part [TB_ROWS gridDim.x][TB_TRAINED] (zeroed by the launcher): row 3 g + third; the per-channel sums (folded over the 256
// threads in thread order) go to row 3 g.
// DX (the last-stage trainer): the block's INPUT gradient of the tile's pixels -> dx [N,H,W,16]: the
// residual path (dL/du, handed from C to D through lx) plus the projection's input gradient through BN and PReLU.
template <bool DX>
__global__ __launch_bounds__(256) void k_tb_block(const float *__restrict__ x5, const float *__restrict__ dy, int N, int H,
                                                  int W, const float *__restrict__ fold, float *__restrict__ part,
                                                  float *__restrict__ dx)
{
    __shared__ __attribute__((aligned(16))) float p1[TB_PW * TB_PW * 4];
    __shared__ __attribute__((aligned(16))) float dac[TB_AW * TB_AW * 4];
    __shared__ __attribute__((aligned(16))) float lq[256 * 4];
    __shared__ __attribute__((aligned(16))) float lde[256 * 16];
    __shared__ __attribute__((aligned(16))) float lx[256 * 16];
    __shared__ __attribute__((aligned(16))) float ldp[256 * 4];
    const int tid = threadIdx.x;
    const int tiles_x = (W + TB_T - 1) / TB_T, tiles = tiles_x * ((H + TB_T - 1) / TB_T);
    const int ti = tid / TB_T, tj = tid % TB_T;
    const long HW = (long)H * W;
    float el[72];  // per-channel sums: tb_elem_slot order
#pragma unroll
    for (int e = 0; e < 72; ++e) el[e] = 0.0f;
    float ka[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int grp = tid / 68, o = tid % 68;  // grp 3 (threads 204 ..) takes no part in E
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int i0 = (t / tiles_x) * TB_T, j0 = (t % tiles_x) * TB_T;
        const bool valid = i0 + ti < H && j0 + tj < W;
        for (int n = 0; n < N; ++n) {
            const float *xn = x5 + (long)n * HW * 16;
            const float *dyn = dy + (long)n * HW * 16;
            __syncthreads();  // E of the previous image is done with the LDS arrays
            tb_phase_p(xn, H, W, i0, j0, fold, p1);
            __syncthreads();
            // ---- C
#pragma unroll 1
            for (int e = tid; e < TB_AW * TB_AW; e += 256) {
                const int pi = e / TB_AW, pj = e % TB_AW;
                const int gi = i0 - 1 + pi, gj = j0 - 1 + pj;
                float xres[16], dv[16];
                const bool ok = tb_load16(xn, H, W, gi, gj, xres);
                tb_load16(dyn, H, W, gi, gj, dv);
                TbPix r;
                tb_conv_exp(p1, pi, pj, fold, xres, r);
                const bool own = pi >= 1 && pi <= TB_T && pj >= 1 && pj <= TB_T;
                const bool acc_own = own && ok;
                float de[16], dq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int co = 0; co < 16; ++co) {
                    const float d = ok ? dv[co] : 0.0f;
                    const float du = d * dprelu(r.u[co], fold[TB_RA + co]);
                    if (acc_own) {
                        el[co] += du * ((r.ev[co] - fold[TB_EM + co]) * fold[TB_EV + co]);
                        el[16 + co] += du;
                        el[32 + co] += d * neg(r.u[co]);
                    }
                    de[co] = du * fold[TB_EG + co];
                }
#pragma unroll
                for (int ci = 0; ci < 4; ++ci)
#pragma unroll
                    for (int co = 0; co < 16; ++co) dq[ci] = fmaf(de[co], fold[TB_WE + ci * 16 + co], dq[ci]);
                float da[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float dyc = dq[k] * dprelu(r.yc[k], fold[TB_CA + k]);
                    if (acc_own) {
                        el[48 + k] += dyc * ((r.accc[k] - fold[TB_CM + k]) * fold[TB_CV + k]);
                        el[52 + k] += dyc;
                        el[56 + k] += dq[k] * neg(r.yc[k]);
                    }
                    da[k] = dyc * fold[TB_CG + k];
                }
                reinterpret_cast<float4 *>(dac)[e] = make_float4(da[0], da[1], da[2], da[3]);  // (zeros outside: d = 0)
                if (own) {
                    const int p = (pi - 1) * TB_T + pj - 1;
                    reinterpret_cast<float4 *>(lq)[p] = ok ? make_float4(r.qv[0], r.qv[1], r.qv[2], r.qv[3])
                                                           : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        reinterpret_cast<float4 *>(lde)[p * 4 + q] = make_float4(de[4 * q], de[4 * q + 1], de[4 * q + 2], de[4 * q + 3]);
                    if constexpr (DX) {  // dL/du of the pixel: lx is free until D writes x into it
#pragma unroll
                        for (int co = 0; co < 16; ++co)
                            lx[p * 16 + co] = (ok ? dv[co] : 0.0f) * dprelu(r.u[co], fold[TB_RA + co]);
                    }
                }
            }
            __syncthreads();
            // ---- D
            {
                float xv[16], accp[4], dp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                tb_load16(xn, H, W, i0 + ti, j0 + tj, xv);
                tb_proj(xv, fold, accp);
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const float4 d4 = reinterpret_cast<const float4 *>(dac)[(ti + 2 - kh) * TB_AW + tj + 2 - kw];
                        const float dk[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                        for (int ci = 0; ci < 4; ++ci)
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                dp[ci] = fmaf(dk[k], fold[TB_WC + ((kh * 3 + kw) * 4 + ci) * 4 + k], dp[ci]);
                    }
                float dap[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float yp = fmaf(accp[k], fold[TB_PG + k], fold[TB_PB + k]);
                    const float dyp = dp[k] * dprelu(yp, fold[TB_PA + k]);
                    if (valid) {
                        el[60 + k] += dyp * ((accp[k] - fold[TB_PM + k]) * fold[TB_PV + k]);
                        el[64 + k] += dyp;
                        el[68 + k] += dp[k] * neg(yp);
                    }
                    dap[k] = valid ? dyp * fold[TB_PG + k] : 0.0f;
                }
                reinterpret_cast<float4 *>(ldp)[tid] = make_float4(dap[0], dap[1], dap[2], dap[3]);
                if constexpr (DX) {
                    if (valid) {
                        float4 *o4 = reinterpret_cast<float4 *>(dx + (((long)n * H + i0 + ti) * W + j0 + tj) * 16);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            float g[4];
#pragma unroll
                            for (int c = 0; c < 4; ++c) {
                                float a = 0.0f;
#pragma unroll
                                for (int k = 0; k < 4; ++k) a = fmaf(dap[k], fold[TB_WP + (4 * q + c) * 4 + k], a);
                                g[c] = lx[tid * 16 + 4 * q + c] + a;
                            }
                            o4[q] = make_float4(g[0], g[1], g[2], g[3]);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    reinterpret_cast<float4 *>(lx)[tid * 4 + q] = make_float4(xv[4 * q], xv[4 * q + 1], xv[4 * q + 2], xv[4 * q + 3]);
            }
            __syncthreads();
            // ---- E
            if (grp < TB_ROWS) {
                const int pb = grp * TB_SEG, pe = min(256, pb + TB_SEG);
                if (o < 16) {
                    for (int p = pb; p < pe; ++p) {
                        const float a = lx[p * 16 + o];
                        const float4 d = reinterpret_cast<const float4 *>(ldp)[p];
                        ka[0] = fmaf(a, d.x, ka[0]); ka[1] = fmaf(a, d.y, ka[1]);
                        ka[2] = fmaf(a, d.z, ka[2]); ka[3] = fmaf(a, d.w, ka[3]);
                    }
                } else if (o < 52) {
                    const int tp = (o - 16) >> 2, ci = (o - 16) & 3, kh = tp / 3, kw = tp % 3;
                    for (int p = pb; p < pe; ++p) {
                        const int pi = p / TB_T, pj = p % TB_T;
                        const float a = p1[((pi + 1 + kh) * TB_PW + pj + 1 + kw) * 4 + ci];
                        const float4 d = reinterpret_cast<const float4 *>(dac)[(pi + 1) * TB_AW + pj + 1];
                        ka[0] = fmaf(a, d.x, ka[0]); ka[1] = fmaf(a, d.y, ka[1]);
                        ka[2] = fmaf(a, d.z, ka[2]); ka[3] = fmaf(a, d.w, ka[3]);
                    }
                } else {
                    const int ci = (o - 52) >> 2, cq = (o - 52) & 3;
                    for (int p = pb; p < pe; ++p) {
                        const float a = lq[p * 4 + ci];
                        const float4 d = reinterpret_cast<const float4 *>(lde)[p * 4 + cq];
                        ka[0] = fmaf(a, d.x, ka[0]); ka[1] = fmaf(a, d.y, ka[1]);
                        ka[2] = fmaf(a, d.z, ka[2]); ka[3] = fmaf(a, d.w, ka[3]);
                    }
                }
            }
        }
    }
    if (grp < TB_ROWS) {
        float *pw = part + ((long)blockIdx.x * TB_ROWS + grp) * TB_TRAINED;
        const int base = o < 16 ? TB_WP + o * 4
                                : (o < 52 ? TB_WC + (o - 16) * 4 : TB_WE + ((o - 52) >> 2) * 16 + ((o - 52) & 3) * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) pw[base + k] = ka[k];
    }
    // the per-channel sums: 16 numbers at a time through lx ([16][256]), thread e sums its row in thread order
    float *row0 = part + (long)blockIdx.x * TB_ROWS * TB_TRAINED;
#pragma unroll
    for (int ch = 0; ch < 5; ++ch) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; ++e) lx[e * 256 + tid] = ch * 16 + e < 72 ? el[(ch * 16 + e) % 72] : 0.0f;
        __syncthreads();
        const int slot = tid < 16 ? tb_elem_slot(ch * 16 + tid) : -1;
        if (slot >= 0) {
            float sum = 0.0f, comp = 0.0f;
            for (int p = 0; p < 256; ++p) kahan(sum, comp, lx[tid * 256 + p]);
            row0[slot] = sum;
        }
    }
}

// grad[o] = (sum over the partial rows, in row order, compensated fp32) * (float)(1 / (double)(float)sum(mask)); the moving statistics
// and the padding get 0; loss as k_final_grad_finish.
__global__ __launch_bounds__(256) void k_tb_finish(const float *__restrict__ part_f, const float *__restrict__ part_b,
                                                   const double *__restrict__ lpart, int G, int K,
                                                   double *__restrict__ loss_out, float *__restrict__ grad)
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
    const int o = blockIdx.x * 256 + threadIdx.x, cf = 9 * K * 16;
    if (o >= TB_FINAL + cf) return;
    float acc = 0.0f, comp = 0.0f;
    if (o >= TB_FINAL) {
        for (int g = 0; g < G; ++g) kahan(acc, comp, part_f[(long)g * cf + (o - TB_FINAL)]);
    } else if (o < TB_TRAINED) {
        for (long g = 0; g < (long)G * TB_ROWS; ++g) kahan(acc, comp, part_b[g * TB_TRAINED + o]);
    }
    // the statistics and the padding are 0 whatever the scale is (an all-zero mask makes it inf)
    grad[o] = (o >= TB_TRAINED && o < TB_FINAL) ? 0.0f : acc * scale;
}

// the head launch: plain (semi NULL), semi-supervised, or the target-only launch (tgt_out non-NULL: x5 = the undistorted
// frame's features; nothing but tgt_out is written)
static hipError_t launch_tb_head(const float *x5, int N, int H, int W, int K, int G, const float *params, const uint8_t *labels,
                                 const float *mask, float weight, float label_smoothing, const TrainBlockWs &ws,
                                 const TrainBlockSemi *semi, uint8_t *tgt_out, hipStream_t s)
{
    const float on_value = 1.0f - label_smoothing, off_value = label_smoothing / ((float)K - 1.0f);
    const double pix = (double)N * H * W;
    const float *wk = params + TB_FINAL;
    if (!semi) {
        // logits, the Final.kernel contraction and the input gradient: 144 K FMAs per feature pixel each; the block: 272
        ProfScope prof("k_tb_head", 2.0 * pix * (3.0 * 144 * K + 272.0 * 1.6),
                       4.0 * pix * 16 * 2 + 4.0 * pix * (1 + 4) + 4.0 * G * 9.0 * 16 * K, s);
#define SSAL_TB(KK)                                                                                                    \
    case KK:                                                                                                           \
        hipLaunchKernelGGL((k_tb_head<KK, false>), dim3(G), dim3(256), 0, s, x5, N, H, W, ws.fold, wk, labels, mask,   \
                           weight, on_value, off_value, ws.dy, ws.part_f, ws.lpart, TbHeadPlain{});                    \
        break;
        switch (K) {
            SSAL_TB(2) SSAL_TB(3) SSAL_TB(4) SSAL_TB(5) SSAL_TB(6) SSAL_TB(7) SSAL_TB(8) SSAL_TB(9)
            SSAL_TB(10) SSAL_TB(11) SSAL_TB(12) SSAL_TB(13) SSAL_TB(14) SSAL_TB(15) SSAL_TB(16)
            SSAL_TB(17) SSAL_TB(18) SSAL_TB(19) SSAL_TB(20) SSAL_TB(21) SSAL_TB(22) SSAL_TB(23)
            SSAL_TB(24) SSAL_TB(25) SSAL_TB(26) SSAL_TB(27) SSAL_TB(28) SSAL_TB(29) SSAL_TB(30)
            SSAL_TB(31) SSAL_TB(32)
        default:
            return hipErrorInvalidValue;
        }
#undef SSAL_TB
        return hipGetLastError();
    }
    TbHeadSemi sa;
    sa.labelled = semi->labelled;
    sa.measure = semi->measure;
    sa.threshold = semi->threshold;
    sa.tgt_in = tgt_out ? nullptr : (semi->use_tgt ? semi->tgt : nullptr);
    sa.tgt_out = tgt_out;
    sa.rep = tgt_out ? nullptr : semi->rep;
    sa.reps = semi->reps;
    sa.pseudo_pixels = tgt_out ? nullptr : (unsigned long long *)semi->pseudo_pixels;
    // the target-only launch: the block and the logits (the own pixels of the unlabelled images; counted for all)
    ProfScope prof(tgt_out ? "k_tb_head_targets" : "k_tb_head_semi",
                   tgt_out ? 2.0 * pix * (144.0 * K + 272.0 * 1.6) : 2.0 * pix * (3.0 * 144 * K + 272.0 * 1.6),
                   tgt_out ? 4.0 * pix * 16 * 2 + 4.0 * pix
                           : 4.0 * pix * 16 * 2 + 4.0 * pix * (1 + 4) + 4.0 * G * 9.0 * 16 * K, s);
#define SSAL_TB(KK)                                                                                                    \
    case KK:                                                                                                           \
        hipLaunchKernelGGL((k_tb_head<KK, true>), dim3(G), dim3(256), 0, s, x5, N, H, W, ws.fold, wk, labels, mask,    \
                           weight, on_value, off_value, ws.dy, ws.part_f, ws.lpart, sa);                               \
        break;
    switch (K) {
        SSAL_TB(2) SSAL_TB(3) SSAL_TB(4) SSAL_TB(5) SSAL_TB(6) SSAL_TB(7) SSAL_TB(8) SSAL_TB(9)
        SSAL_TB(10) SSAL_TB(11) SSAL_TB(12) SSAL_TB(13) SSAL_TB(14) SSAL_TB(15) SSAL_TB(16)
        SSAL_TB(17) SSAL_TB(18) SSAL_TB(19) SSAL_TB(20) SSAL_TB(21) SSAL_TB(22) SSAL_TB(23)
        SSAL_TB(24) SSAL_TB(25) SSAL_TB(26) SSAL_TB(27) SSAL_TB(28) SSAL_TB(29) SSAL_TB(30)
        SSAL_TB(31) SSAL_TB(32)
    default:
        return hipErrorInvalidValue;
    }
#undef SSAL_TB
    return hipGetLastError();
}

static bool train_block_semi_ok(const TrainBlockSemi *semi)
{
    return !semi || (semi->measure >= 0 && semi->measure <= 2 && (!semi->rep || semi->reps >= 1));
}

hipError_t launch_train_block_targets(const float *x5_raw, int N, int H, int W, int K, const float *params,
                                      const TrainBlockSemi &semi, const TrainBlockWs &ws, hipStream_t s, int max_workgroups)
{
    if (N < 1 || K < 2 || K > 32 || !train_block_fits(H, W) || !train_block_semi_ok(&semi) || !semi.tgt || !x5_raw)
        return hipErrorInvalidValue;
    if (!semi.labelled) return hipSuccess;  // every image is labelled: no pseudo target is read
    int G = train_block_workgroups(H, W);
    if (max_workgroups > 0 && max_workgroups < G) G = max_workgroups;
    hipLaunchKernelGGL(k_tb_fold, dim3(1), dim3(512), 0, s, params, ws.fold);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_tb_head(x5_raw, N, H, W, K, G, params, nullptr, nullptr, 0.0f, 0.0f, ws, &semi, semi.tgt, s);
}

hipError_t launch_train_block_grad(const float *x5, int N, int H, int W, int K, const float *params, const uint8_t *labels,
                                   const float *mask, float weight, float label_smoothing, const TrainBlockWs &ws,
                                   double *loss, float *grad, hipStream_t s, float *dx, int max_workgroups,
                                   const TrainBlockSemi *semi)
{
    if (N < 1 || K < 2 || K > 32 || !train_block_fits(H, W) || !train_block_semi_ok(semi)) return hipErrorInvalidValue;
    int G = train_block_workgroups(H, W);
    if (max_workgroups > 0 && max_workgroups < G) G = max_workgroups;
    const double pix = (double)N * H * W;
    hipError_t e;
    if (semi && semi->pseudo_pixels) {
        e = hipMemsetAsync(semi->pseudo_pixels, 0, (size_t)N * sizeof(int64_t), s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_tb_fold, dim3(1), dim3(512), 0, s, params, ws.fold);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(ws.part_b, 0, (size_t)G * TB_ROWS * TB_TRAINED * sizeof(float), s);
    if (e != hipSuccess) return e;
    e = launch_tb_head(x5, N, H, W, K, G, params, labels, mask, weight, label_smoothing, ws, semi, nullptr, s);
    if (e != hipSuccess) return e;
    {
        ProfScope prof("k_tb_block", 2.0 * pix * (272.0 * 1.6 + 272.0 * 2 + 64.0), 4.0 * pix * 16 * 2 + 4.0 * G * TB_ROWS * TB_TRAINED, s);
        if (dx) hipLaunchKernelGGL(k_tb_block<true>, dim3(G), dim3(256), 0, s, x5, ws.dy, N, H, W, ws.fold, ws.part_b, dx);
        else    hipLaunchKernelGGL(k_tb_block<false>, dim3(G), dim3(256), 0, s, x5, ws.dy, N, H, W, ws.fold, ws.part_b, dx);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int count = (int)train_block_floats(K);
    ProfScope prof("k_tb_finish", (double)G * count, 4.0 * G * (9.0 * 16 * K + TB_ROWS * TB_TRAINED) + 16.0 * G, s);
    hipLaunchKernelGGL(k_tb_finish, dim3((count + 255) / 256), dim3(256), 0, s, ws.part_f, ws.part_b, ws.lpart, G, K, loss, grad);
    return hipGetLastError();
}

}  // namespace ssal
