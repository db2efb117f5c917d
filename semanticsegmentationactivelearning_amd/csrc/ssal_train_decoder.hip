// ssal_train_decoder.hip -- training of ENet's whole decoder (Bottleneck4_0 + the two-block tail above it) over a frozen
// encoder, gfx950:
//   k_td_fold    Bottleneck4_0's batch-norms folded as ssal_enet_commit folds them on the host (s = gamma / sqrt(var + 1e-3),
//                t = fma(-mean, s, beta)), 1 / sqrt(var + 1e-3), and the parity-stacked transposed-convolution kernel
//                (stack_convT of ssal_api.hip): what k_upsample_mfma reads, built on the device from the packed block
//   (forward)    a4_0 = the library's own Bottleneck4_0 forward, launch_upsample_mfma (Cin = 128), on those weights
//   (tail)       launch_train_tail_grad (R = 2) on a4_0, whose lowest block also writes dL/d a4_0
//   k_td_block   Bottleneck4_0's forward again on the window a tile needs, and its backward: per-workgroup partials of twelve
//                gradients (all but res_kernel), and dL/du gathered through the pooling indices -> dur
//   k_td_res     res_kernel's gradient: the contraction of the block's input with dur, into the same partial rows
//   k_td_finish  (the profile's name of k_train_finish, ssal_train_common.h) fixed-order compensated fold of the partials,
//                times 1 / sum(mask)
// Semantics: enet_modules.py:1217-1292 in inference mode (moving statistics are constants, no dropout); PReLU and its
// derivative at 0 as in ssal_train_block.hip.  The unpool's backward is the gather of dL/du at the position the window code
// names.  Plain fmaf contractions (fp32 MFMA runs at the vector rate on this part, DESIGN.md section 6, and the fmaf form
// keeps one summation order for every operand).  No floating-point atomics: two runs give the same bits.
#include "ssal_internal.h"
#include "ssal_prof.h"
#include "ssal_score.h"
#include "ssal_train_common.h"
#include "ssal_train_decoder.h"

namespace ssal {

namespace {

constexpr int TD_Q = 8;    // eighth-resolution pixels per tile side
constexpr int TD_T = 16;   // quarter-resolution pixels per tile side
constexpr int TD_CW = 17;  // dL/d(convT accumulator) window: the tile plus one row below and one column to the right
constexpr int TD_PW = 10;  // projected window (eighth resolution): the 8 x 8 patch plus a ring of one
constexpr int TD_RW = 9;   // residual / window-code window (eighth resolution): the patch plus one row / column
constexpr int TD_CPIX = TD_CW * TD_CW;   // 289 pixels of the convolution window
constexpr int TD_CITEMS = TD_CPIX * 4;   // (pixel of the convolution window, channel quarter)
constexpr int TD_PASSES = (TD_CITEMS + 255) / 256;  // C2 runs 64 pixels at a time
// C2 exchanges partial sums among the four lanes of a pixel inside a branch on the item number: a pixel's lanes must be
// active together
static_assert(TD_CITEMS % 4 == 0 && 256 % 4 == 0, "the four lanes of a pixel are active together");
// k_td_block's LDS copy of the per-channel scalars: the folded ones [0, DF_WS) as k_td_fold lays them out (the stacked kernel
// that follows them there is not copied), then proj_alpha, conv_alpha, residual_alpha and the three moving means from the
// packed block
constexpr int LD_PA = DF_WS, LD_CA = LD_PA + 32, LD_RA = LD_CA + 16, LD_PM = LD_RA + 64, LD_CM = LD_PM + 32, LD_EM = LD_CM + 16;
constexpr int LD_FLOATS = LD_EM + 64;

// offset, inside Bottleneck4_0's part of the packed block, of per-channel gradient number r of a thread whose channel
// quarter is kq (k_td_block's el order: exp_gamma, exp_beta, residual_alpha of the quarter's 16 channels; conv_gamma,
// conv_beta, conv_alpha of its four; proj_gamma, proj_beta, proj_alpha of its eight)
__device__ __forceinline__ int td_elem_slot(int r, int kq)
{
    if (r < 16) return TD_EG + 16 * kq + r;
    if (r < 32) return TD_EB + 16 * kq + r - 16;
    if (r < 48) return TD_RA + 16 * kq + r - 32;
    if (r < 52) return TD_CG + 4 * kq + r - 48;
    if (r < 56) return TD_CB + 4 * kq + r - 52;
    if (r < 60) return TD_CA + 4 * kq + r - 56;
    if (r < 68) return TD_PG + 8 * kq + r - 60;
    if (r < 76) return TD_PB + 8 * kq + r - 68;
    if (r < 84) return TD_PA + 8 * kq + r - 76;
    return -1;
}

}  // namespace

bool train_decoder_fits(int H, int W)
{
    if (H < 1 || W < 1 || H >= (1 << 28) || W >= (1 << 28)) return false;
    return train_tail_fits(2 * H, 2 * W) && upsample_mfma_fits(128, H, W);
}

int train_decoder_workgroups(int H, int W, int max_workgroups)
{
    const long tiles = (long)((H + TD_Q - 1) / TD_Q) * ((W + TD_Q - 1) / TD_Q);
    const int G = tiles < 1024 ? (int)tiles : 1024;
    return max_workgroups > 0 && max_workgroups < G ? max_workgroups : G;
}

// P = Bottleneck4_0's part of the packed block
__global__ __launch_bounds__(256) void k_td_fold(const float *__restrict__ P, float *__restrict__ F)
{
    for (int i = threadIdx.x; i < DF_FLOATS; i += 256) {
        float v;
        if (i < DF_PI) {
            int j, g, b, m, vr;
            bool shift;
            if (i < DF_CS) { j = i & 31; g = TD_PG; b = TD_PB; m = TD_PM; vr = TD_PV; shift = i >= DF_PT; }
            else if (i < DF_ES) { j = i & 15; g = TD_CG; b = TD_CB; m = TD_CM; vr = TD_CV; shift = i >= DF_CT; }
            else { j = (i - DF_ES) & 63; g = TD_EG; b = TD_EB; m = TD_EM; vr = TD_EV; shift = i >= DF_ET; }
            const float sg = P[g + j] / sqrtf(P[vr + j] + 1e-3f);
            v = shift ? fmaf(-P[m + j], sg, P[b + j]) : sg;
        } else if (i < DF_CI) {
            v = 1.0f / sqrtf(P[TD_PV + i - DF_PI] + 1e-3f);
        } else if (i < DF_EI) {
            v = 1.0f / sqrtf(P[TD_CV + i - DF_CI] + 1e-3f);
        } else if (i < DF_WS) {
            v = 1.0f / sqrtf(P[TD_EV + i - DF_EI] + 1e-3f);
        } else {
            // ws[slot][ci][row]: rows [0, 16) = first parity class of the slot, [16, 32) = second (stack_convT)
            const int idx = i - DF_WS, sl = idx >> 10, ci = (idx >> 5) & 31, row = idx & 31, half = row >> 4, co = row & 15;
            const int t = half == 0 ? (sl == 0 ? 0 : sl == 1 ? 2 : sl == 2 ? 6 : sl == 3 ? 8 : sl == 4 ? 3 : 5)
                                    : (sl == 0 ? 1 : sl == 2 ? 7 : sl == 4 ? 4 : -1);
            v = t < 0 ? 0.0f : P[TD_WC + (t * 16 + co) * 32 + ci];
        }
        F[i] = v;
    }
}

// Bottleneck4_0's backward but for res_kernel.  H, W = the dims of x (eighth resolution); g = dL/d a4_0 [N,2H,2W,64].  A
// workgroup owns one 8 x 8 tile of eighth-resolution pixels (= 16 x 16 quarter-resolution pixels) for all N images and takes
// tiles blockIdx.x + G i.  Per image:
//   P   wave w = projected channels 8w .. 8w + 7 and residual channels 16w .. 16w + 15 (weights in scalar registers), lane =
//       pixel of the 10 x 10 eighth-resolution window whose corner is (i0 - 1, j0 - 1): the projection 128 -> 32 with BN + PReLU
//       -> lp (zeros outside the image: such a pixel feeds nothing into the transposed convolution), its accumulator for the
//       patch's pixels -> lpa; the residual 1 x 1 convolution and the window codes on the 9 x 9 window (i0 .., j0 ..) -> lr, lcode
//   C1  item = (pixel of the 17 x 17 quarter-resolution window whose corner is the tile's, four convolution outputs): the
//       transposed convolution (taps by the parity of the pixel: out[2 i + kh][2 j + kw] += p[i][j] W[kh][kw]) -> lca, BN + PReLU
//       -> lq
//   C2  64 window pixels at a time, item = (pixel, 16 of the 64 outputs): the expansion, BN, + the unpooled residual = u, back
//       through the residual PReLU (dL/du goes to dur where the window code names the pixel: the unpool's backward, a gather)
//       and the expansion's BN -> lde (zeros for the row below and the column to the right), the expansion's input gradient as
//       four partial sums that the four lanes of a pixel add in a fixed order, then, lane = four convolution channels, back
//       through the convolution's BN + PReLU: dL/d(convT accumulator) -> ldc (zeros outside the image); then exp_kernel's
//       contraction over the 64 pixels (thread = input channel x four outputs)
//   D   thread = (pixel of the patch, eight projected channels): the transposed convolution's input gradient over the nine taps
//       (rows 2 i + kh of ldc: the tap that falls off the bottom / right edge of the map meets the zeros C2 left there), back
//       through the projection's PReLU and BN -> lpa
//   E   proj_kernel (thread = input channel x 16 outputs, over the patch's 64 pixels) and conv_kernel (thread = input channel x
//       two outputs, nine taps) as contractions in a fixed order, accumulators in registers across all tiles and images.
// The 84 per-channel sums of a thread (its channel quarter is tid & 3 in C2 and D alike) accumulate in registers and are folded
// over the 64 threads of a quarter in thread order, compensated, at the end.  gamma / beta gradients are produced directly, as
// in k_tb_block.  part [gridDim.x][TD_TRAINED]: every slot outside res_kernel's is written (k_td_res writes those).
__global__ __launch_bounds__(256) void k_td_block(const float *__restrict__ x, const uint8_t *__restrict__ code,
                                                  const float *__restrict__ g, int N, int H, int W,
                                                  const float *__restrict__ P, const float *__restrict__ F,
                                                  float *__restrict__ part, float *__restrict__ dur)
{
    __shared__ __attribute__((aligned(16))) float lwc[9 * 16 * 32];
    __shared__ __attribute__((aligned(16))) float lwe[16 * 64];
    __shared__ __attribute__((aligned(16))) float lk[LD_FLOATS];
    __shared__ __attribute__((aligned(16))) float lp[TD_PW * TD_PW * 32];
    __shared__ __attribute__((aligned(16))) float lpa[64 * 32];  // P -> D: the projection's accumulator; D -> E: dL/d(that)
    __shared__ __attribute__((aligned(16))) float lr[TD_RW * TD_RW * 64];
    __shared__ unsigned lcode[TD_RW * TD_RW * 16];
    __shared__ __attribute__((aligned(16))) float lca[TD_CPIX * 16];
    __shared__ __attribute__((aligned(16))) float lq[TD_CPIX * 16];
    __shared__ __attribute__((aligned(16))) float ldc[TD_CPIX * 16];
    __shared__ __attribute__((aligned(16))) float lde[64 * 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = tid & 3;
    const int H2 = 2 * H, W2 = 2 * W;
    const int tiles_x = (W + TD_Q - 1) / TD_Q, tiles = tiles_x * ((H + TD_Q - 1) / TD_Q);
    const long HW = (long)H * W;
    float el[84];  // per-channel sums, td_elem_slot order
#pragma unroll
    for (int e = 0; e < 84; ++e) el[e] = 0.0f;
    float kwp[16], kwc[18];
    float kwe[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 16; ++j) kwp[j] = 0.0f;
#pragma unroll
    for (int j = 0; j < 18; ++j) kwc[j] = 0.0f;
    for (int i = tid; i < 9 * 16 * 32; i += 256) lwc[i] = P[TD_WC + i];
    for (int i = tid; i < 16 * 64; i += 256) lwe[i] = P[TD_WE + i];
    for (int j = tid; j < LD_FLOATS; j += 256) {
        lk[j] = j < LD_PA ? F[j] : (j < LD_CA ? P[TD_PA + j - LD_PA] : (j < LD_RA ? P[TD_CA + j - LD_CA] : (j < LD_PM ? P[TD_RA + j - LD_RA]
                : (j < LD_CM ? P[TD_PM + j - LD_PM] : (j < LD_EM ? P[TD_CM + j - LD_CM] : P[TD_EM + j - LD_EM])))));
    }
    const int dqp = tid >> 2, dil = dqp >> 3, djl = dqp & 7;  // D: the thread's pixel of the patch
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int i0 = (t / tiles_x) * TD_Q, j0 = (t % tiles_x) * TD_Q, I0 = 2 * i0, J0 = 2 * j0;
        for (int n = 0; n < N; ++n) {
            const float *xn = x + (long)n * HW * 128;
            const uint8_t *cn = code + (long)n * HW * 64;
            const float *gn = g + (long)n * HW * 4 * 64;
            float *durn = dur + (long)n * HW * 64;
            __syncthreads();  // E of the previous image is done with the LDS arrays (and the weights are in place)
            // ---- P
#pragma unroll 1
            for (int e = lane; e < TD_PW * TD_PW; e += 64) {
                const int pi = e / TD_PW, pj = e % TD_PW;
                const int qi = i0 - 1 + pi, qj = j0 - 1 + pj;
                const bool ok = qi >= 0 && qi < H && qj >= 0 && qj < W;
                const long pix = (long)min(max(qi, 0), H - 1) * W + min(max(qj, 0), W - 1);
                const float4 *xp = reinterpret_cast<const float4 *>(xn + pix * 128);
                float ap[8], ar[16];
#pragma unroll
                for (int k = 0; k < 8; ++k) ap[k] = 0.0f;
#pragma unroll
                for (int k = 0; k < 16; ++k) ar[k] = 0.0f;
#pragma unroll 1
                for (int c4 = 0; c4 < 32; ++c4) {
                    const float4 x4 = xp[c4];
                    const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) ap[k] = fmaf(xv[c], P[TD_WP + (4 * c4 + c) * 32 + 8 * wv + k], ap[k]);
#pragma unroll
                        for (int k = 0; k < 16; ++k) ar[k] = fmaf(xv[c], P[TD_WR + (4 * c4 + c) * 64 + 16 * wv + k], ar[k]);
                    }
                }
                float pv[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int ch = 8 * wv + k;
                    pv[k] = ok ? prelu(fmaf(ap[k], lk[DF_PS + ch], lk[DF_PT + ch]), lk[LD_PA + ch]) : 0.0f;
                }
                reinterpret_cast<float4 *>(lp)[e * 8 + 2 * wv] = make_float4(pv[0], pv[1], pv[2], pv[3]);
                reinterpret_cast<float4 *>(lp)[e * 8 + 2 * wv + 1] = make_float4(pv[4], pv[5], pv[6], pv[7]);
                if (pi >= 1 && pj >= 1) {
                    if (pi <= TD_Q && pj <= TD_Q) {
                        float4 *ap4 = reinterpret_cast<float4 *>(lpa) + ((pi - 1) * TD_Q + pj - 1) * 8 + 2 * wv;
                        ap4[0] = make_float4(ap[0], ap[1], ap[2], ap[3]);
                        ap4[1] = make_float4(ap[4], ap[5], ap[6], ap[7]);
                    }
                    const int re = (pi - 1) * TD_RW + pj - 1;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        reinterpret_cast<float4 *>(lr)[re * 16 + 4 * wv + q] =
                            ok ? make_float4(ar[4 * q], ar[4 * q + 1], ar[4 * q + 2], ar[4 * q + 3]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        // (no code matches 0xff: a pixel outside the map unpools nothing)
                        lcode[re * 16 + 4 * wv + q] = ok ? *reinterpret_cast<const unsigned *>(cn + pix * 64 + 16 * wv + 4 * q) : 0xffffffffu;
                    }
                }
            }
            __syncthreads();
            // ---- C1
#pragma unroll 1
            for (int it = tid; it < TD_CITEMS; it += 256) {
                const int e = it >> 2, ci_ = e / TD_CW, cj = e % TD_CW;
                float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
                for (int ab = 0; ab < 4; ++ab) {
                    const int a = ab >> 1, b = ab & 1;
                    // even row: taps kh = 0 (eighth row ci_ / 2) and kh = 2 (the row above); odd row: kh = 1 only
                    if ((a == 1 && (ci_ & 1)) || (b == 1 && (cj & 1))) continue;
                    const int kh = (ci_ & 1) ? 1 : 2 * a, kw = (cj & 1) ? 1 : 2 * b;
                    const int pi = (ci_ >> 1) + 1 - a, pj = (cj >> 1) + 1 - b;
                    const float4 *pp = reinterpret_cast<const float4 *>(lp) + (pi * TD_PW + pj) * 8;
                    const float4 *wt = reinterpret_cast<const float4 *>(lwc) + ((kh * 3 + kw) * 16 + 4 * kq) * 8;
#pragma unroll
                    for (int c4 = 0; c4 < 8; ++c4) {
                        const float4 p4 = pp[c4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float4 w4 = wt[k * 8 + c4];
                            acc[k] = fmaf(p4.x, w4.x, acc[k]);
                            acc[k] = fmaf(p4.y, w4.y, acc[k]);
                            acc[k] = fmaf(p4.z, w4.z, acc[k]);
                            acc[k] = fmaf(p4.w, w4.w, acc[k]);
                        }
                    }
                }
                float qv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int ch = 4 * kq + k;
                    qv[k] = prelu(fmaf(acc[k], lk[DF_CS + ch], lk[DF_CT + ch]), lk[LD_CA + ch]);
                }
                reinterpret_cast<float4 *>(lca)[it] = make_float4(acc[0], acc[1], acc[2], acc[3]);
                reinterpret_cast<float4 *>(lq)[it] = make_float4(qv[0], qv[1], qv[2], qv[3]);
            }
            // ---- C2 (TD_CITEMS and 256 are multiples of 4: the four lanes of a pixel are active together)
#pragma unroll 1
            for (int ps = 0; ps < TD_PASSES; ++ps) {
                __syncthreads();  // C1's lq / lca are in place; the previous pass' contraction is done with lde
                const int it = ps * 256 + tid;
                if (it < TD_CITEMS) {
                    const int e = it >> 2, ci_ = e / TD_CW, cj = e % TD_CW;
                    const int Y = I0 + ci_, X = J0 + cj;
                    const bool ok = Y < H2 && X < W2;
                    const bool own = ci_ < TD_T && cj < TD_T;
                    const bool acc_own = own && ok;
                    const float4 *gr = reinterpret_cast<const float4 *>(gn + ((long)min(Y, H2 - 1) * W2 + min(X, W2 - 1)) * 64 + 16 * kq);
                    const int rq = (ci_ >> 1) * TD_RW + (cj >> 1);
                    const unsigned cls = (unsigned)((ci_ & 1) * 2 + (cj & 1));
                    // (acc_own: the eighth-resolution pixel is inside the map, since 2 i <= Y < 2 H)
                    float *dup = durn + ((long)min(i0 + (ci_ >> 1), H - 1) * W + min(j0 + (cj >> 1), W - 1)) * 64 + 16 * kq;
                    float qv[16], dq[16];
#pragma unroll
                    for (int c4 = 0; c4 < 4; ++c4) {
                        const float4 q4 = reinterpret_cast<const float4 *>(lq)[e * 4 + c4];
                        qv[4 * c4] = q4.x; qv[4 * c4 + 1] = q4.y; qv[4 * c4 + 2] = q4.z; qv[4 * c4 + 3] = q4.w;
                    }
#pragma unroll
                    for (int ci = 0; ci < 16; ++ci) dq[ci] = 0.0f;
#pragma unroll
                    for (int c4 = 0; c4 < 4; ++c4) {
                        const float4 g4 = gr[c4];
                        const float4 r4 = reinterpret_cast<const float4 *>(lr)[rq * 16 + 4 * kq + c4];
                        const unsigned cd = lcode[rq * 16 + 4 * kq + c4];
                        const float gv[4] = {g4.x, g4.y, g4.z, g4.w}, rv[4] = {r4.x, r4.y, r4.z, r4.w};
                        float ev[4] = {0.0f, 0.0f, 0.0f, 0.0f}, de[4];
#pragma unroll
                        for (int ci = 0; ci < 16; ++ci) {
                            const float4 w4 = reinterpret_cast<const float4 *>(lwe)[ci * 16 + 4 * kq + c4];
                            ev[0] = fmaf(qv[ci], w4.x, ev[0]);
                            ev[1] = fmaf(qv[ci], w4.y, ev[1]);
                            ev[2] = fmaf(qv[ci], w4.z, ev[2]);
                            ev[3] = fmaf(qv[ci], w4.w, ev[3]);
                        }
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const int lc = 4 * c4 + c, co = 16 * kq + lc;
                            const bool hit = ((cd >> (8 * c)) & 0xffu) == cls;
                            const float u = fmaf(ev[c], lk[DF_ES + co], lk[DF_ET + co]) + (hit ? rv[c] : 0.0f);
                            const float d = ok ? gv[c] : 0.0f;
                            const float du = d * dprelu(u, lk[LD_RA + co]);
                            if (acc_own) {
                                el[lc] += du * ((ev[c] - lk[LD_EM + co]) * lk[DF_EI + co]);
                                el[16 + lc] += du;
                                el[32 + lc] += d * neg(u);
                                if (hit) dup[lc] = du;
                            }
                            de[c] = du * lk[DF_ES + co];
                        }
                        // (the row below and the column to the right go on to dL/dq, but not into exp_kernel's contraction)
                        reinterpret_cast<float4 *>(lde)[(e - 64 * ps) * 16 + 4 * kq + c4] =
                            own ? make_float4(de[0], de[1], de[2], de[3]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                        for (int ci = 0; ci < 16; ++ci) {
                            const float4 w4 = reinterpret_cast<const float4 *>(lwe)[ci * 16 + 4 * kq + c4];
                            dq[ci] = fmaf(de[0], w4.x, dq[ci]);
                            dq[ci] = fmaf(de[1], w4.y, dq[ci]);
                            dq[ci] = fmaf(de[2], w4.z, dq[ci]);
                            dq[ci] = fmaf(de[3], w4.w, dq[ci]);
                        }
                    }
                    // the four partial sums of a pixel (lanes 4 j .. 4 j + 3) in a fixed order; every lane gets every sum
#pragma unroll
                    for (int ci = 0; ci < 16; ++ci) {
                        dq[ci] += __shfl_xor(dq[ci], 1);
                        dq[ci] += __shfl_xor(dq[ci], 2);
                    }
                    const float4 a4 = reinterpret_cast<const float4 *>(lca)[it];
                    const float accc[4] = {a4.x, a4.y, a4.z, a4.w};
                    float da[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int ch = 4 * kq + k;
                        const float dqk = kq == 0 ? dq[k] : (kq == 1 ? dq[4 + k] : (kq == 2 ? dq[8 + k] : dq[12 + k]));
                        const float yc = fmaf(accc[k], lk[DF_CS + ch], lk[DF_CT + ch]);
                        const float dyc = dqk * dprelu(yc, lk[LD_CA + ch]);
                        if (acc_own) {
                            el[48 + k] += dyc * ((accc[k] - lk[LD_CM + ch]) * lk[DF_CI + ch]);
                            el[52 + k] += dyc;
                            el[56 + k] += dqk * neg(yc);
                        }
                        da[k] = dyc * lk[DF_CS + ch];
                    }
                    reinterpret_cast<float4 *>(ldc)[it] = make_float4(da[0], da[1], da[2], da[3]);  // (zeros outside the map: d = 0)
                }
                __syncthreads();
                {
                    const int cnt = min(64, TD_CPIX - 64 * ps), ci = tid >> 4, co = tid & 15;
#pragma unroll 4
                    for (int p = 0; p < cnt; ++p) {
                        const float a = lq[(64 * ps + p) * 16 + ci];
                        const float4 d = reinterpret_cast<const float4 *>(lde)[p * 16 + co];
                        kwe[0] = fmaf(a, d.x, kwe[0]); kwe[1] = fmaf(a, d.y, kwe[1]);
                        kwe[2] = fmaf(a, d.z, kwe[2]); kwe[3] = fmaf(a, d.w, kwe[3]);
                    }
                }
            }
            __syncthreads();
            // ---- D
            {
                const bool valid = i0 + dil < H && j0 + djl < W;
                float dp[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) dp[k] = 0.0f;
#pragma unroll 1
                for (int tp = 0; tp < 9; ++tp) {
                    const int kh = tp / 3, kw = tp % 3;
                    const float4 *dcp = reinterpret_cast<const float4 *>(ldc) + ((2 * dil + kh) * TD_CW + 2 * djl + kw) * 4;
                    const float4 *wt = reinterpret_cast<const float4 *>(lwc) + tp * 16 * 8 + 2 * kq;
#pragma unroll
                    for (int c4 = 0; c4 < 4; ++c4) {
                        const float4 d4 = dcp[c4];
                        const float dk[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const float4 w0 = wt[(4 * c4 + c) * 8], w1 = wt[(4 * c4 + c) * 8 + 1];
                            dp[0] = fmaf(dk[c], w0.x, dp[0]); dp[1] = fmaf(dk[c], w0.y, dp[1]);
                            dp[2] = fmaf(dk[c], w0.z, dp[2]); dp[3] = fmaf(dk[c], w0.w, dp[3]);
                            dp[4] = fmaf(dk[c], w1.x, dp[4]); dp[5] = fmaf(dk[c], w1.y, dp[5]);
                            dp[6] = fmaf(dk[c], w1.z, dp[6]); dp[7] = fmaf(dk[c], w1.w, dp[7]);
                        }
                    }
                }
                float4 *ap4 = reinterpret_cast<float4 *>(lpa) + dqp * 8 + 2 * kq;
                const float4 a0 = ap4[0], a1 = ap4[1];
                const float accp[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                float dap[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int ch = 8 * kq + k;
                    const float yp = fmaf(accp[k], lk[DF_PS + ch], lk[DF_PT + ch]);
                    const float dyp = dp[k] * dprelu(yp, lk[LD_PA + ch]);
                    if (valid) {
                        el[60 + k] += dyp * ((accp[k] - lk[LD_PM + ch]) * lk[DF_PI + ch]);
                        el[68 + k] += dyp;
                        el[76 + k] += dp[k] * neg(yp);
                    }
                    dap[k] = valid ? dyp * lk[DF_PS + ch] : 0.0f;
                }
                ap4[0] = make_float4(dap[0], dap[1], dap[2], dap[3]);
                ap4[1] = make_float4(dap[4], dap[5], dap[6], dap[7]);
            }
            __syncthreads();
            // ---- E
            {
                const int c = tid >> 1, half = tid & 1;
#pragma unroll 2
                for (int p = 0; p < 64; ++p) {
                    const long pix = (long)min(i0 + (p >> 3), H - 1) * W + min(j0 + (p & 7), W - 1);
                    const float a = xn[pix * 128 + c];
                    const float4 *dp4 = reinterpret_cast<const float4 *>(lpa) + p * 8 + 4 * half;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float4 d = dp4[q];
                        kwp[4 * q] = fmaf(a, d.x, kwp[4 * q]); kwp[4 * q + 1] = fmaf(a, d.y, kwp[4 * q + 1]);
                        kwp[4 * q + 2] = fmaf(a, d.z, kwp[4 * q + 2]); kwp[4 * q + 3] = fmaf(a, d.w, kwp[4 * q + 3]);
                    }
                }
            }
            {
                const int ci = tid >> 3, cp = tid & 7;
#pragma unroll 2
                for (int p = 0; p < 64; ++p) {
                    const int il = p >> 3, jl = p & 7;
                    const float a = lp[((il + 1) * TD_PW + jl + 1) * 32 + ci];  // (zero outside the map)
#pragma unroll
                    for (int tp = 0; tp < 9; ++tp) {
                        const float2 d = reinterpret_cast<const float2 *>(ldc)[((2 * il + tp / 3) * TD_CW + 2 * jl + tp % 3) * 8 + cp];
                        kwc[2 * tp] = fmaf(a, d.x, kwc[2 * tp]);
                        kwc[2 * tp + 1] = fmaf(a, d.y, kwc[2 * tp + 1]);
                    }
                }
            }
        }
    }
    float *row = part + (long)blockIdx.x * TD_TRAINED;
    {
        const int c = tid >> 1, half = tid & 1, ci = tid >> 3, cp = tid & 7, ce = tid >> 4, co = tid & 15;
#pragma unroll
        for (int j = 0; j < 16; ++j) row[TD_WP + c * 32 + 16 * half + j] = kwp[j];
#pragma unroll
        for (int tp = 0; tp < 9; ++tp) {
            row[TD_WC + (tp * 16 + 2 * cp) * 32 + ci] = kwc[2 * tp];
            row[TD_WC + (tp * 16 + 2 * cp + 1) * 32 + ci] = kwc[2 * tp + 1];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) row[TD_WE + ce * 64 + 4 * co + k] = kwe[k];
    }
    // the per-channel sums: 16 numbers at a time through lde ([16][256]); thread (e, quarter) sums the 64 threads of its
    // quarter in thread order
#pragma unroll
    for (int ch = 0; ch < 6; ++ch) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; ++e) lde[e * 256 + tid] = ch * 16 + e < 84 ? el[(ch * 16 + e) % 84] : 0.0f;
        __syncthreads();
        const int slot = tid < 64 ? td_elem_slot(ch * 16 + (tid >> 2), kq) : -1;
        if (slot >= 0) {
            float sum = 0.0f, comp = 0.0f;
            for (int j = 0; j < 64; ++j) kahan(sum, comp, lde[(tid >> 2) * 256 + 4 * j + kq]);
            row[slot] = sum;
        }
    }
}

// res_kernel's gradient: dW_res[ci][co] = sum over pixels of x[ci] dur[co] (dur = dL/du at the position the pixel's window code
// names, k_td_block's).  The tiles, their order and the workgroup's row of part are k_td_block's; thread = input channel x 32
// outputs, the tile's x and dur in LDS (zeros for the pixels of a ragged tile that lie outside the map), one fmaf chain per
// element over tiles, images and pixels in that order.
__global__ __launch_bounds__(256) void k_td_res(const float *__restrict__ x, const float *__restrict__ dur, int N, int H, int W,
                                                float *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float lx[64 * 128];
    __shared__ __attribute__((aligned(16))) float ld[64 * 64];
    const int tid = threadIdx.x, ci = tid >> 1, half = tid & 1;
    const int tiles_x = (W + TD_Q - 1) / TD_Q, tiles = tiles_x * ((H + TD_Q - 1) / TD_Q);
    const long HW = (long)H * W;
    float acc[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) acc[j] = 0.0f;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int i0 = (t / tiles_x) * TD_Q, j0 = (t % tiles_x) * TD_Q;
        for (int n = 0; n < N; ++n) {
            __syncthreads();
            for (int i = tid; i < 64 * 32; i += 256) {
                const int p = i >> 5, qi = i0 + (p >> 3), qj = j0 + (p & 7);
                const long pix = (long)n * HW + (long)min(qi, H - 1) * W + min(qj, W - 1);
                reinterpret_cast<float4 *>(lx)[i] = reinterpret_cast<const float4 *>(x + pix * 128)[i & 31];
            }
            for (int i = tid; i < 64 * 16; i += 256) {
                const int p = i >> 4, qi = i0 + (p >> 3), qj = j0 + (p & 7);
                const long pix = (long)n * HW + (long)min(qi, H - 1) * W + min(qj, W - 1);
                reinterpret_cast<float4 *>(ld)[i] = qi < H && qj < W ? reinterpret_cast<const float4 *>(dur + pix * 64)[i & 15]
                                                                     : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            __syncthreads();
#pragma unroll 2
            for (int p = 0; p < 64; ++p) {
                const float a = lx[p * 128 + ci];
                const float4 *dp = reinterpret_cast<const float4 *>(ld) + p * 16 + 8 * half;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float4 d = dp[q];
                    acc[4 * q] = fmaf(a, d.x, acc[4 * q]); acc[4 * q + 1] = fmaf(a, d.y, acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(a, d.z, acc[4 * q + 2]); acc[4 * q + 3] = fmaf(a, d.w, acc[4 * q + 3]);
                }
            }
        }
    }
    float *row = part + (long)blockIdx.x * TD_TRAINED + TD_WR + ci * 64 + 32 * half;
#pragma unroll
    for (int j = 0; j < 32; ++j) row[j] = acc[j];
}

// Bottleneck4_0's forward as the scoring path runs it, on the block's own weights: PD = its part of the packed block
static hipError_t decoder_forward(const float *x38, const int64_t *argmax2, int N, int H, int W, const float *PD,
                                  const TrainDecoderWs &ws, hipStream_t s)
{
    hipError_t e;
    if (argmax2) {
        e = launch_argmax_to_codes(argmax2, N, H, W, 64, ws.code2, ws.bad2, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_td_fold, dim3(1), dim3(256), 0, s, PD, ws.dfold);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const float *F = ws.dfold;
    return launch_upsample_mfma(x38, ws.a40, ws.code2, N, H, W, 128, PD + TD_WP, F + DF_PS, F + DF_PT, PD + TD_PA, F + DF_WS,
                                F + DF_CS, F + DF_CT, PD + TD_CA, PD + TD_WE, F + DF_ES, F + DF_ET, PD + TD_WR, PD + TD_RA, s);
}

hipError_t launch_train_decoder_grad(const float *x38, const int64_t *argmax2, const int64_t *argmax1, int N, int H, int W,
                                     int K, const float *params, const uint8_t *labels, const float *mask, float weight,
                                     float label_smoothing, int max_workgroups, const TrainDecoderWs &ws, double *loss,
                                     float *grad, hipStream_t s, const TrainBlockSemi *semi)
{
    if (N < 1 || K < 2 || K > 32 || !train_decoder_fits(H, W)) return hipErrorInvalidValue;
    const int G = train_decoder_workgroups(H, W, max_workgroups);
    const int Gl = train_stage_workgroups(2 * H, 2 * W, max_workgroups);  // rows of the mask sums the head kernel leaves
    const float *PD = params + train_tail_floats(K, 2);
    hipError_t e = decoder_forward(x38, argmax2, N, H, W, PD, ws, s);
    if (e != hipSuccess) return e;
    e = launch_train_tail_grad(ws.a40, argmax1, N, 2 * H, 2 * W, K, params, labels, mask, weight, label_smoothing,
                               max_workgroups, ws.tt, loss, grad, s, semi, 2, ws.dx40);
    if (e != hipSuccess) return e;
    const double pix = (double)N * H * W;
    {
        // per eighth-resolution pixel: projection + residual conv on a 10 x 10 window for an 8 x 8 patch (12288 FMAs x 1.56),
        // four quarter-resolution pixels of forward (convT 1152 average, exp 1024) and backward (exp 1024) on a 17 x 17 window
        // for 16 x 16 (x 1.13), the convT input gradient 4608, the contractions 4096 + 4608 + 4 x 1024
        ProfScope prof("k_td_block", 2.0 * pix * (12288.0 * 1.5625 + 4.0 * 1.13 * (1152.0 + 2048.0) + 4608.0 + 12800.0),
                       4.0 * pix * (128.0 * 2 + 4.0 * 64 + 64.0) + pix * 64 + 4.0 * G * (TD_TRAINED - 8192), s);
        hipLaunchKernelGGL(k_td_block, dim3(G), dim3(256), 0, s, x38, ws.code2, ws.dx40, N, H, W, PD, ws.dfold, ws.part_d, ws.dur);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    {
        ProfScope prof("k_td_res", 2.0 * pix * 8192.0, 4.0 * pix * (128.0 + 64.0) + 4.0 * G * 8192, s);
        hipLaunchKernelGGL(k_td_res, dim3(G), dim3(256), 0, s, x38, ws.dur, N, H, W, ws.part_d);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return launch_train_finish<TD_TRAINED, TD_FLOATS>("k_td_finish", ws.part_d, ws.tt.ts.tb.lpart, G, Gl,
                                                      grad + train_tail_floats(K, 2), s);
}

hipError_t launch_train_decoder_targets(const float *x38_raw, const int64_t *argmax2_raw, const int64_t *argmax1_raw, int N,
                                        int H, int W, int K, const float *params, int max_workgroups,
                                        const TrainDecoderWs &ws, const TrainBlockSemi &semi, hipStream_t s)
{
    if (N < 1 || K < 2 || K > 32 || !train_decoder_fits(H, W) || !x38_raw) return hipErrorInvalidValue;
    if (!semi.labelled) return hipSuccess;  // every image is labelled: no pseudo target is read
    const hipError_t e = decoder_forward(x38_raw, argmax2_raw, N, H, W, params + train_tail_floats(K, 2), ws, s);
    if (e != hipSuccess) return e;
    return launch_train_tail_targets(ws.a40, argmax1_raw, N, 2 * H, 2 * W, K, params, max_workgroups, ws.tt, semi, s, 2);
}

}  // namespace ssal
