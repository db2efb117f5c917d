// ssal_train_stage.hip -- training of ENet's last decoder stage (Bottleneck5_0 + Bottleneck5_1 + Final.kernel) over a frozen
// trunk, gfx950:
//   k_ts_fold    Bottleneck5_0's batch-norms folded as ssal_enet_commit folds them on the host (s = gamma / sqrt(var + 1e-3),
//                t = fma(-mean, s, beta)), 1 / sqrt(var + 1e-3), and the parity-stacked transposed-convolution kernel
//                (stack_convT of ssal_api.hip): what k_upsample16 reads, built on the device from the packed block
//   (forward)    a5_0 = the library's own Bottleneck5_0 forward, launch_upsample_mfma -> k_upsample16, on those weights
//   (last block) launch_train_block_grad on a5_0 (ssal_train_block.hip) with k_tb_block<true>, which also writes dL/d a5_0
//   k_ts_block   Bottleneck5_0's forward again on the window a tile needs, and its backward: per-workgroup partials of the
//                13 gradients
//   k_ts_finish  (the profile's name of k_train_finish, ssal_train_common.h) fixed-order compensated fold of the partials,
//                times 1 / sum(mask)
// Semantics: enet_modules.py:1217-1292 in inference mode (moving statistics are constants, no dropout); PReLU and its
// derivative at 0 as in ssal_train_block.hip.  The unpool's backward is the gather of dL/du at the position the window code
// names.  No floating-point atomics: two runs give the same bits.
#include "ssal_internal.h"
#include "ssal_prof.h"
#include "ssal_score.h"
#include "ssal_train_common.h"
#include "ssal_train_stage.h"

namespace ssal {

namespace {

constexpr int TS_T = 16;   // half-resolution pixels per tile side (the tile of ssal_train_block.hip)
constexpr int TS_Q = 8;    // quarter-resolution pixels per tile side
constexpr int TS_CW = 17;  // dL/d(convT accumulator) window: the tile plus one row below and one column to the right
constexpr int TS_PW = 10;  // projected window (quarter resolution): the 8 x 8 patch plus a ring of one
constexpr int TS_RW = 9;   // residual / window-code window (quarter resolution): the patch plus one row / column
// k_ts_block's LDS copy of what every thread reads at the same address: the folded scalars [0, TF_WS) as k_ts_fold lays them
// out, then proj_alpha, conv_alpha, exp_kernel, residual_alpha and the six moving statistics from the packed block
constexpr int LK_PA = TF_WS, LK_CA = LK_PA + 16, LK_WE = LK_CA + 8, LK_RA = LK_WE + 128, LK_PM = LK_RA + 16;
constexpr int LK_FLOATS = LK_PM + (TS_FLOATS - 8 - TS_PM);

// offset, inside Bottleneck5_0's part of the stage block, of per-channel gradient number e of k_ts_block
__device__ __forceinline__ int ts_elem_slot(int e)
{
    if (e < 16) return TS_EG + e;
    if (e < 32) return TS_EB + e - 16;
    if (e < 48) return TS_RA + e - 32;
    if (e < 56) return TS_CG + e - 48;
    if (e < 64) return TS_CB + e - 56;
    if (e < 72) return TS_CA + e - 64;
    if (e < 88) return TS_PG + e - 72;
    if (e < 104) return TS_PB + e - 88;
    if (e < 120) return TS_PA + e - 104;
    return -1;
}

}  // namespace

bool train_stage_fits(int H, int W)
{
    if (H < 1 || W < 1 || H >= (1 << 29) || W >= (1 << 29)) return false;
    return final_grad_fits(2 * H, 2 * W) && upsample_mfma_fits(64, H, W);
}

int train_stage_workgroups(int H, int W, int max_workgroups)
{
    const int G = train_block_workgroups(2 * H, 2 * W);
    return max_workgroups > 0 && max_workgroups < G ? max_workgroups : G;
}

// P = Bottleneck5_0's part of the packed block
__global__ __launch_bounds__(256) void k_ts_fold(const float *__restrict__ P, float *__restrict__ F)
{
    for (int i = threadIdx.x; i < TF_FLOATS; i += 256) {
        float v = 0.0f;
        if (i < TF_PI) {
            int j, g, b, m, vr;
            bool shift;
            if (i < TF_CS) { j = i & 15; g = TS_PG; b = TS_PB; m = TS_PM; vr = TS_PV; shift = i >= TF_PT; }
            else if (i < TF_ES) { j = i & 7; g = TS_CG; b = TS_CB; m = TS_CM; vr = TS_CV; shift = i >= TF_CT; }
            else { j = i & 15; g = TS_EG; b = TS_EB; m = TS_EM; vr = TS_EV; shift = i >= TF_ET; }
            const float sg = P[g + j] / sqrtf(P[vr + j] + 1e-3f);
            v = shift ? fmaf(-P[m + j], sg, P[b + j]) : sg;
        } else if (i < TF_CI) {
            v = 1.0f / sqrtf(P[TS_PV + i - TF_PI] + 1e-3f);
        } else if (i < TF_EI) {
            v = 1.0f / sqrtf(P[TS_CV + i - TF_CI] + 1e-3f);
        } else if (i < TF_EI + 16) {
            v = 1.0f / sqrtf(P[TS_EV + i - TF_EI] + 1e-3f);
        } else if (i >= TF_WS) {
            // ws[slot][ci][row]: rows [0, 8) = first parity class of the slot, [8, 16) = second (stack_convT)
            const int idx = i - TF_WS, sl = idx >> 8, ci = (idx >> 4) & 15, row = idx & 15, half = row >> 3, co = row & 7;
            const int t = half == 0 ? (sl == 0 ? 0 : sl == 1 ? 2 : sl == 2 ? 6 : sl == 3 ? 8 : sl == 4 ? 3 : 5)
                                    : (sl == 0 ? 1 : sl == 2 ? 7 : sl == 4 ? 4 : -1);
            v = t < 0 ? 0.0f : P[TS_WC + (t * 8 + co) * 16 + ci];
        }
        F[i] = v;
    }
}

// Bottleneck5_0's backward.  H, W = the dims of x4 (quarter resolution); g = dL/d a5_0 [N,2H,2W,16].  A workgroup owns one
// 16 x 16 tile of half-resolution pixels (= an 8 x 8 patch of x4) for all N images and takes tiles blockIdx.x + G i.  Per image:
//   P  wave w = channels 4w .. 4w + 3 (weights in scalar registers), lane = pixel of the 10 x 10 quarter-resolution window whose
//      corner is (i0 - 1, j0 - 1): the projection 64 -> 16 with BN + PReLU -> lp (zeros outside the image: such a pixel feeds
//      nothing into the transposed convolution), its accumulator for the patch's pixels -> lpa; the residual 1 x 1 convolution
//      and the window codes on the 9 x 9 window (i0 .., j0 ..) -> lr, lcode
//   C  thread = pixel of the tile, and threads 0 .. 32 a second time for the row below and the column to the right: the
//      transposed convolution (taps by the parity of the pixel: out[2 i + kh][2 j + kw] += p[i][j] W[kh][kw]), BN, PReLU, the
//      expansion, BN, + the unpooled residual = u; back through the residual PReLU, the expansion and the convolution's BN + PReLU:
//      dL/d(convT accumulator) -> ldc (zeros outside the image).  Pixels of the tile add their per-channel terms to the thread's
//      registers, leave q [8] and dL/d(exp accumulator) [16] in LDS and, where the window code names them, dL/du -> ldr (the
//      unpool's backward: a gather).
//   D  thread = (pixel of the patch, four projected channels): the transposed convolution's input gradient over the nine taps
//      (rows 2 i + kh of ldc: the tap that falls off the bottom / right edge of the map meets the zeros C left there), back
//      through the projection's PReLU and BN -> ldpa; per-channel terms in registers
//   E  the four kernel gradients as contractions in a fixed order, accumulators in registers across all tiles and images:
//      proj_kernel and res_kernel (thread = input channel x four outputs, over the patch's 64 pixels), conv_kernel (144 threads =
//      tap x output x half of the inputs), exp_kernel (threads 128 .. 255 = one element each, over the tile's 256 pixels).
// gamma / beta gradients are produced directly, as in k_tb_block.  part [gridDim.x][TS_TRAINED]: every slot is written.
// DX (the decoder-tail trainer): the block's INPUT gradient of the patch's pixels -> dx4 [N,H,W,64],
// written once between D and E: the projection's input gradient sum_k dL/d(proj acc)[k] W_p[ci][k] (BN and PReLU are inside ldpa) plus
// the residual 1 x 1 convolution's sum_c dL/du_gathered[c] W_res[ci][c].
template <bool DX>
__global__ __launch_bounds__(256) void k_ts_block(const float *__restrict__ x4, const uint8_t *__restrict__ code,
                                                  const float *__restrict__ g, int N, int H, int W,
                                                  const float *__restrict__ P, const float *__restrict__ F,
                                                  float *__restrict__ part, float *__restrict__ dx4)
{
    __shared__ __attribute__((aligned(16))) float lwc[9 * 8 * 16];
    __shared__ __attribute__((aligned(16))) float lp[TS_PW * TS_PW * 16];
    __shared__ __attribute__((aligned(16))) float lr[TS_RW * TS_RW * 16];
    __shared__ unsigned lcode[TS_RW * TS_RW * 4];
    __shared__ __attribute__((aligned(16))) float lk[LK_FLOATS];  // the folded scalars, the block's per-channel variables, exp_kernel
    __shared__ __attribute__((aligned(16))) float ldc[TS_CW * TS_CW * 8];
    __shared__ __attribute__((aligned(16))) float lq[256 * 8];
    __shared__ __attribute__((aligned(16))) float lde[256 * 16];
    __shared__ __attribute__((aligned(16))) float ldpa[64 * 16];  // P -> D: the projection's accumulator; D -> E: dL/d(that)
    __shared__ __attribute__((aligned(16))) float ldr[64 * 16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H2 = 2 * H, W2 = 2 * W;
    const int tiles_x = (W2 + TS_T - 1) / TS_T, tiles = tiles_x * ((H2 + TS_T - 1) / TS_T);
    const long HW = (long)H * W;
    float el[72];  // per-channel sums, ts_elem_slot order: exp_gamma, exp_beta, residual_alpha [16]; conv_gamma, conv_beta, conv_alpha [8]
#pragma unroll
    for (int e = 0; e < 72; ++e) el[e] = 0.0f;
    float elp[12];  // proj_gamma, proj_beta, proj_alpha of the thread's four channels
#pragma unroll
    for (int e = 0; e < 12; ++e) elp[e] = 0.0f;
    float kwp[4] = {0.0f, 0.0f, 0.0f, 0.0f}, kwr[4] = {0.0f, 0.0f, 0.0f, 0.0f}, kwe = 0.0f;
    float kwc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) kwc[j] = 0.0f;
    for (int i = tid; i < 9 * 8 * 16; i += 256) lwc[i] = P[TS_WC + i];
    for (int i = tid; i < LK_FLOATS; i += 256)
        lk[i] = i < LK_PA ? F[i] : (i < LK_CA ? P[TS_PA + i - LK_PA] : (i < LK_WE ? P[TS_CA + i - LK_CA] : (i < LK_RA ? P[TS_WE + i - LK_WE]
                : (i < LK_PM ? P[TS_RA + i - LK_RA] : P[TS_PM + i - LK_PM]))));
    // D: the thread's pixel of the patch and its channel group
    const int dqp = tid >> 2, dcg = tid & 3, dil = dqp >> 3, djl = dqp & 7;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int I0 = (t / tiles_x) * TS_T, J0 = (t % tiles_x) * TS_T, i0 = I0 >> 1, j0 = J0 >> 1;
        for (int n = 0; n < N; ++n) {
            const float *xn = x4 + (long)n * HW * 64;
            const uint8_t *cn = code + (long)n * HW * 16;
            const float *gn = g + (long)n * HW * 4 * 16;
            __syncthreads();  // E of the previous image is done with the LDS arrays (and lwc is in place)
            // ---- P
#pragma unroll 1
            for (int e = lane; e < TS_PW * TS_PW; e += 64) {
                const int pi = e / TS_PW, pj = e % TS_PW;
                const int qi = i0 - 1 + pi, qj = j0 - 1 + pj;
                const bool ok = qi >= 0 && qi < H && qj >= 0 && qj < W;
                const long pix = (long)min(max(qi, 0), H - 1) * W + min(max(qj, 0), W - 1);
                const float4 *xp = reinterpret_cast<const float4 *>(xn + pix * 64);
                float ap[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ar[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
                for (int c4 = 0; c4 < 16; ++c4) {
                    const float4 x = xp[c4];
                    const float xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                    for (int c = 0; c < 4; ++c)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            ap[k] = fmaf(xv[c], P[TS_WP + (4 * c4 + c) * 16 + 4 * wv + k], ap[k]);
                            ar[k] = fmaf(xv[c], P[TS_WR + (4 * c4 + c) * 16 + 4 * wv + k], ar[k]);
                        }
                }
                float pv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int ch = 4 * wv + k;
                    pv[k] = ok ? prelu(fmaf(ap[k], lk[TF_PS + ch], lk[TF_PT + ch]), lk[LK_PA + ch]) : 0.0f;
                }
                reinterpret_cast<float4 *>(lp)[e * 4 + wv] = make_float4(pv[0], pv[1], pv[2], pv[3]);
                if (pi >= 1 && pj >= 1) {
                    if (pi <= TS_Q && pj <= TS_Q)
                        reinterpret_cast<float4 *>(ldpa)[((pi - 1) * TS_Q + pj - 1) * 4 + wv] = make_float4(ap[0], ap[1], ap[2], ap[3]);
                    const int re = (pi - 1) * TS_RW + pj - 1;
                    reinterpret_cast<float4 *>(lr)[re * 4 + wv] = ok ? make_float4(ar[0], ar[1], ar[2], ar[3])
                                                                     : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    // (no code matches 0xff: a pixel outside the map unpools nothing)
                    lcode[re * 4 + wv] = ok ? *reinterpret_cast<const unsigned *>(cn + pix * 16 + 4 * wv) : 0xffffffffu;
                }
            }
            __syncthreads();
            // ---- C
#pragma unroll 1
            for (int ps = 0; ps < 2; ++ps) {
                if (ps == 1 && tid >= 2 * TS_T + 1) break;
                const int ci_ = ps == 0 ? tid / TS_T : (tid < 16 ? 16 : (tid < 32 ? tid - 16 : 16));
                const int cj = ps == 0 ? tid % TS_T : (tid < 16 ? tid : 16);
                const bool own = ps == 0;
                const int Y = I0 + ci_, X = J0 + cj;
                const bool ok = Y < H2 && X < W2;
                const bool acc_own = own && ok;
                float cacc[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) cacc[k] = 0.0f;
#pragma unroll 1
                for (int a = 0; a < 2; ++a)
#pragma unroll 1
                    for (int b = 0; b < 2; ++b) {
                        // even row: taps kh = 0 (quarter row ci_ / 2) and kh = 2 (the row above); odd row: kh = 1 only
                        if ((a == 1 && (ci_ & 1)) || (b == 1 && (cj & 1))) continue;
                        const int kh = (ci_ & 1) ? 1 : 2 * a, kw = (cj & 1) ? 1 : 2 * b;
                        const int pi = (ci_ >> 1) + 1 - a, pj = (cj >> 1) + 1 - b;
                        const float4 *pp = reinterpret_cast<const float4 *>(lp) + (pi * TS_PW + pj) * 4;
                        const float4 *wt = reinterpret_cast<const float4 *>(lwc) + (kh * 3 + kw) * 8 * 4;
#pragma unroll
                        for (int c4 = 0; c4 < 4; ++c4) {
                            const float4 p4 = pp[c4];
#pragma unroll
                            for (int co = 0; co < 8; ++co) {
                                const float4 w4 = wt[co * 4 + c4];
                                cacc[co] = fmaf(p4.x, w4.x, cacc[co]);
                                cacc[co] = fmaf(p4.y, w4.y, cacc[co]);
                                cacc[co] = fmaf(p4.z, w4.z, cacc[co]);
                                cacc[co] = fmaf(p4.w, w4.w, cacc[co]);
                            }
                        }
                    }
                float yc[8], qv[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    yc[k] = fmaf(cacc[k], lk[TF_CS + k], lk[TF_CT + k]);
                    qv[k] = prelu(yc[k], lk[LK_CA + k]);
                }
                const int rq = (ci_ >> 1) * TS_RW + (cj >> 1);
                const unsigned cls = (unsigned)((ci_ & 1) * 2 + (cj & 1));
                const float4 *gp = reinterpret_cast<const float4 *>(gn + ((long)min(Y, H2 - 1) * W2 + min(X, W2 - 1)) * 16);
                float de[16], dq[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) dq[k] = 0.0f;
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    const float4 g4 = gp[c4];
                    const float4 r4 = reinterpret_cast<const float4 *>(lr)[rq * 4 + c4];
                    const unsigned cd = lcode[rq * 4 + c4];
                    const float gv[4] = {g4.x, g4.y, g4.z, g4.w}, rv[4] = {r4.x, r4.y, r4.z, r4.w};
                    float duv[4];
                    bool hit[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int co = 4 * c4 + c;
                        float ev = 0.0f;
#pragma unroll
                        for (int ci = 0; ci < 8; ++ci) ev = fmaf(qv[ci], lk[LK_WE + ci * 16 + co], ev);
                        hit[c] = ((cd >> (8 * c)) & 0xffu) == cls;
                        const float u = fmaf(ev, lk[TF_ES + co], lk[TF_ET + co]) + (hit[c] ? rv[c] : 0.0f);
                        const float d = ok ? gv[c] : 0.0f;
                        const float du = d * dprelu(u, lk[LK_RA + co]);
                        if (acc_own) {
                            el[co] += du * ((ev - lk[LK_PM + TS_EM - TS_PM + co]) * lk[TF_EI + co]);
                            el[16 + co] += du;
                            el[32 + co] += d * neg(u);
                        }
                        duv[c] = du;
                        de[co] = du * lk[TF_ES + co];
                    }
                    if (acc_own) {
                        float *rp = ldr + (((ci_ >> 1) * TS_Q + (cj >> 1)) * 16 + 4 * c4);
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (hit[c]) rp[c] = duv[c];
                    }
                }
#pragma unroll
                for (int ci = 0; ci < 8; ++ci)
#pragma unroll
                    for (int co = 0; co < 16; ++co) dq[ci] = fmaf(de[co], lk[LK_WE + ci * 16 + co], dq[ci]);
                float da[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float dyc = dq[k] * dprelu(yc[k], lk[LK_CA + k]);
                    if (acc_own) {
                        el[48 + k] += dyc * ((cacc[k] - lk[LK_PM + TS_CM - TS_PM + k]) * lk[TF_CI + k]);
                        el[56 + k] += dyc;
                        el[64 + k] += dq[k] * neg(yc[k]);
                    }
                    da[k] = dyc * lk[TF_CS + k];
                }
                float4 *dcp = reinterpret_cast<float4 *>(ldc) + (ci_ * TS_CW + cj) * 2;  // (zeros outside the map: d = 0)
                dcp[0] = make_float4(da[0], da[1], da[2], da[3]);
                dcp[1] = make_float4(da[4], da[5], da[6], da[7]);
                if (own) {
                    float4 *qp = reinterpret_cast<float4 *>(lq) + tid * 2;
                    qp[0] = ok ? make_float4(qv[0], qv[1], qv[2], qv[3]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    qp[1] = ok ? make_float4(qv[4], qv[5], qv[6], qv[7]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        reinterpret_cast<float4 *>(lde)[tid * 4 + q] = make_float4(de[4 * q], de[4 * q + 1], de[4 * q + 2], de[4 * q + 3]);
                }
            }
            __syncthreads();
            // ---- D
            {
                const bool valid = i0 + dil < H && j0 + djl < W;
                float dp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const float4 *dcp = reinterpret_cast<const float4 *>(ldc) + ((2 * dil + kh) * TS_CW + 2 * djl + kw) * 2;
                        const float4 d0 = dcp[0], d1 = dcp[1];
                        const float dk[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
                        for (int co = 0; co < 8; ++co) {
                            const float4 w4 = reinterpret_cast<const float4 *>(lwc)[((kh * 3 + kw) * 8 + co) * 4 + dcg];
                            dp[0] = fmaf(dk[co], w4.x, dp[0]);
                            dp[1] = fmaf(dk[co], w4.y, dp[1]);
                            dp[2] = fmaf(dk[co], w4.z, dp[2]);
                            dp[3] = fmaf(dk[co], w4.w, dp[3]);
                        }
                    }
                const float4 a4 = reinterpret_cast<const float4 *>(ldpa)[dqp * 4 + dcg];
                const float accp[4] = {a4.x, a4.y, a4.z, a4.w};
                float dap[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int ch = 4 * dcg + k;
                    const float yp = fmaf(accp[k], lk[TF_PS + ch], lk[TF_PT + ch]);
                    const float dyp = dp[k] * dprelu(yp, lk[LK_PA + ch]);
                    if (valid) {
                        elp[k] += dyp * ((accp[k] - lk[LK_PM + TS_PM - TS_PM + ch]) * lk[TF_PI + ch]);
                        elp[4 + k] += dyp;
                        elp[8 + k] += dp[k] * neg(yp);
                    }
                    dap[k] = valid ? dyp * lk[TF_PS + ch] : 0.0f;
                }
                reinterpret_cast<float4 *>(ldpa)[dqp * 4 + dcg] = make_float4(dap[0], dap[1], dap[2], dap[3]);
                if (!valid) reinterpret_cast<float4 *>(ldr)[dqp * 4 + dcg] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
            __syncthreads();
            if constexpr (DX) {
                // lane = pixel of the patch, wave = 16 input channels with both kernels' rows in scalar registers
                const int qi = i0 + (lane >> 3), qj = j0 + (lane & 7);
                const bool inside = qi < H && qj < W;
                float dv[32];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 d = reinterpret_cast<const float4 *>(ldpa)[lane * 4 + q];
                    const float4 r = reinterpret_cast<const float4 *>(ldr)[lane * 4 + q];
                    dv[4 * q] = d.x; dv[4 * q + 1] = d.y; dv[4 * q + 2] = d.z; dv[4 * q + 3] = d.w;
                    dv[16 + 4 * q] = r.x; dv[17 + 4 * q] = r.y; dv[18 + 4 * q] = r.z; dv[19 + 4 * q] = r.w;
                }
                float *dxp = dx4 + ((long)n * HW + (long)min(qi, H - 1) * W + min(qj, W - 1)) * 64;
#pragma unroll 1
                for (int ci = 16 * wv; ci < 16 * wv + 16; ++ci) {
                    float v = 0.0f;
#pragma unroll
                    for (int k = 0; k < 16; ++k) v = fmaf(dv[k], P[TS_WP + ci * 16 + k], v);
#pragma unroll
                    for (int k = 0; k < 16; ++k) v = fmaf(dv[16 + k], P[TS_WR + ci * 16 + k], v);
                    if (inside) dxp[ci] = v;
                }
            }
            // ---- E
            {
                const int c = tid >> 2, kq = tid & 3;
#pragma unroll 8
                for (int p = 0; p < 64; ++p) {
                    const long pix = (long)min(i0 + (p >> 3), H - 1) * W + min(j0 + (p & 7), W - 1);
                    const float a = xn[pix * 64 + c];
                    const float4 d = reinterpret_cast<const float4 *>(ldpa)[p * 4 + kq];
                    const float4 r = reinterpret_cast<const float4 *>(ldr)[p * 4 + kq];
                    kwp[0] = fmaf(a, d.x, kwp[0]); kwp[1] = fmaf(a, d.y, kwp[1]);
                    kwp[2] = fmaf(a, d.z, kwp[2]); kwp[3] = fmaf(a, d.w, kwp[3]);
                    kwr[0] = fmaf(a, r.x, kwr[0]); kwr[1] = fmaf(a, r.y, kwr[1]);
                    kwr[2] = fmaf(a, r.z, kwr[2]); kwr[3] = fmaf(a, r.w, kwr[3]);
                }
            }
            if (tid < 144) {
                const int tp = tid >> 4, co = (tid >> 1) & 7, half = tid & 1, kh = tp / 3, kw = tp % 3;
                for (int p = 0; p < 64; ++p) {
                    const int il = p >> 3, jl = p & 7;
                    const float4 *ap = reinterpret_cast<const float4 *>(lp) + ((il + 1) * TS_PW + jl + 1) * 4 + 2 * half;
                    const float4 a0 = ap[0], a1 = ap[1];
                    const float d = ldc[((2 * il + kh) * TS_CW + 2 * jl + kw) * 8 + co];
                    kwc[0] = fmaf(a0.x, d, kwc[0]); kwc[1] = fmaf(a0.y, d, kwc[1]);
                    kwc[2] = fmaf(a0.z, d, kwc[2]); kwc[3] = fmaf(a0.w, d, kwc[3]);
                    kwc[4] = fmaf(a1.x, d, kwc[4]); kwc[5] = fmaf(a1.y, d, kwc[5]);
                    kwc[6] = fmaf(a1.z, d, kwc[6]); kwc[7] = fmaf(a1.w, d, kwc[7]);
                }
            }
            if (tid >= 128) {
                const int ci = (tid - 128) >> 4, co = tid & 15;
                for (int p = 0; p < 256; ++p) kwe = fmaf(lq[p * 8 + ci], lde[p * 16 + co], kwe);
            }
        }
    }
    float *row = part + (long)blockIdx.x * TS_TRAINED;
    {
        const int c = tid >> 2, kq = tid & 3;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            row[TS_WP + c * 16 + 4 * kq + k] = kwp[k];
            row[TS_WR + c * 16 + 4 * kq + k] = kwr[k];
        }
    }
    if (tid < 144) {
        const int tp = tid >> 4, co = (tid >> 1) & 7, half = tid & 1;
#pragma unroll
        for (int j = 0; j < 8; ++j) row[TS_WC + (tp * 8 + co) * 16 + 8 * half + j] = kwc[j];
    }
    if (tid >= 128) row[TS_WE + tid - 128] = kwe;
    // the per-channel sums: 16 numbers at a time through lde ([16][256]), thread e sums its row in thread order
#pragma unroll
    for (int ch = 0; ch < 8; ++ch) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int sl = ch * 16 + e;
            float v = 0.0f;
            if (sl < 72) v = el[sl < 72 ? sl : 0];
            else if (sl < 120 && (((sl - 72) & 15) >> 2) == dcg) v = elp[sl < 120 ? ((sl - 72) >> 4) * 4 + ((sl - 72) & 3) : 0];
            lde[e * 256 + tid] = v;
        }
        __syncthreads();
        const int slot = tid < 16 ? ts_elem_slot(ch * 16 + tid) : -1;
        if (slot >= 0) {
            float sum = 0.0f, comp = 0.0f;
            for (int p = 0; p < 256; ++p) kahan(sum, comp, lde[tid * 256 + p]);
            row[slot] = sum;
        }
    }
}

hipError_t launch_train_stage_grad(const float *x4, const int64_t *argmax, int N, int H, int W, int K, const float *params,
                                   const uint8_t *labels, const float *mask, float weight, float label_smoothing,
                                   int max_workgroups, const TrainStageWs &ws, double *loss, float *grad, hipStream_t s,
                                   const TrainBlockSemi *semi, float *dx4)
{
    if (N < 1 || K < 2 || K > 32 || !train_stage_fits(H, W)) return hipErrorInvalidValue;
    const int G = train_stage_workgroups(H, W, max_workgroups);
    const float *P = params + train_block_floats(K), *F = ws.sfold;
    hipError_t e;
    if (argmax) {
        e = launch_argmax_to_codes(argmax, N, H, W, 16, ws.code, ws.bad, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ts_fold, dim3(1), dim3(256), 0, s, P, ws.sfold);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the forward of the scoring path, on the block's own weights
    e = launch_upsample_mfma(x4, ws.a5, ws.code, N, H, W, 64, P + TS_WP, F + TF_PS, F + TF_PT, P + TS_PA, F + TF_WS, F + TF_CS,
                             F + TF_CT, P + TS_CA, P + TS_WE, F + TF_ES, F + TF_ET, P + TS_WR, P + TS_RA, s);
    if (e != hipSuccess) return e;
    e = launch_train_block_grad(ws.a5, N, 2 * H, 2 * W, K, params, labels, mask, weight, label_smoothing, ws.tb, loss, grad, s,
                                ws.dx, G, semi);
    if (e != hipSuccess) return e;
    const double qpix = (double)N * H * W;
    {
        // per quarter-resolution pixel: projection + residual conv on a 10 x 10 window for an 8 x 8 patch (2048 FMAs x 1.56),
        // four half-resolution pixels of forward (convT 288 average, exp 128) and backward (exp 128, + the terms), the convT
        // input gradient 1152, the contractions 2048 + 1152 + 4 x 128
        ProfScope prof("k_ts_block", 2.0 * qpix * (2048.0 * 1.5625 + 4.0 * 1.13 * (288.0 + 256.0) + 1152.0 + 3712.0),
                       4.0 * qpix * (64.0 * 2 + 4.0 * 16) + qpix * 16 + 4.0 * G * TS_TRAINED, s);
        if (dx4) hipLaunchKernelGGL(k_ts_block<true>, dim3(G), dim3(256), 0, s, x4, ws.code, ws.dx, N, H, W, P, F, ws.part_s, dx4);
        else     hipLaunchKernelGGL(k_ts_block<false>, dim3(G), dim3(256), 0, s, x4, ws.code, ws.dx, N, H, W, P, F, ws.part_s, dx4);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return launch_train_finish<TS_TRAINED, TS_FLOATS>("k_ts_finish", ws.part_s, ws.tb.lpart, G, G, grad + train_block_floats(K), s);
}

// The pseudo targets of the undistorted frames: their window codes and Bottleneck5_0 through the
// scoring path's kernel into ws.code / ws.a5 (which the training call overwrites afterwards, in stream order), then the
// target-only launch of the head kernel -> semi.tgt.
hipError_t launch_train_stage_targets(const float *x4_raw, const int64_t *argmax_raw, int N, int H, int W, int K,
                                      const float *params, int max_workgroups, const TrainStageWs &ws,
                                      const TrainBlockSemi &semi, hipStream_t s)
{
    if (N < 1 || K < 2 || K > 32 || !train_stage_fits(H, W) || !x4_raw) return hipErrorInvalidValue;
    if (!semi.labelled) return hipSuccess;  // every image is labelled: no pseudo target is read
    const int G = train_stage_workgroups(H, W, max_workgroups);
    const float *P = params + train_block_floats(K), *F = ws.sfold;
    hipError_t e;
    if (argmax_raw) {
        e = launch_argmax_to_codes(argmax_raw, N, H, W, 16, ws.code, ws.bad, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ts_fold, dim3(1), dim3(256), 0, s, P, ws.sfold);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_upsample_mfma(x4_raw, ws.a5, ws.code, N, H, W, 64, P + TS_WP, F + TF_PS, F + TF_PT, P + TS_PA, F + TF_WS, F + TF_CS,
                             F + TF_CT, P + TS_CA, P + TS_WE, F + TF_ES, F + TF_ET, P + TS_WR, P + TS_RA, s);
    if (e != hipSuccess) return e;
    return launch_train_block_targets(ws.a5, N, 2 * H, 2 * W, K, params, semi, ws.tb, s, G);
}

}  // namespace ssal
