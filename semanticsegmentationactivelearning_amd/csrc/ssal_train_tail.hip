// ssal_train_tail.hip -- training of ENet's decoder tail (Bottleneck4_2 + Bottleneck5_0 + Bottleneck5_1 + Final.kernel) over a
// frozen trunk, gfx950:
//   k_tt_fold    a regular 64-channel bottleneck's batch-norms folded as ssal_enet_commit folds them on the host
//                (s = gamma / sqrt(var + 1e-3), t = fma(-mean, s, beta)) and 1 / sqrt(var + 1e-3): what the scoring path's
//                kernel reads, built on the device from the packed block
//   (forward)    a4_2 = the library's own Bottleneck4_2 forward, launch_bottleneck_mfma (Cin = 64), on those weights
//   (stage)      launch_train_stage_grad on a4_2 (ssal_train_stage.hip) with k_ts_block<true>, which also writes dL/d a4_2
//   k_tt_block   the bottleneck's forward again on the window a tile needs, and its backward: per-workgroup partials of the
//                12 gradients; <true> also writes the block's input gradient, which makes it a link of a chain: with
//                R = 2 Bottleneck4_1 below Bottleneck4_2 is a second fold, forward and launch
//   k_tt_finish  (the profile's name of k_train_finish, ssal_train_common.h) fixed-order compensated fold of the partials,
//                times 1 / sum(mask)
// Semantics: enet_modules.py:526-599 in inference mode (moving statistics are constants, no dropout); PReLU and its
// derivative at 0 as in ssal_train_block.hip.  Nothing in the two kernels names the layer: they take the block's part of
// the packed parameters, its input and its output gradient, so another regular 64-channel bottleneck is another launch.
// No floating-point atomics: two runs give the same bits.
#include "ssal_internal.h"
#include "ssal_prof.h"
#include "ssal_score.h"
#include "ssal_train_common.h"
#include "ssal_train_tail.h"

namespace ssal {

namespace {

constexpr int TT_Q = 8;    // pixels per tile side (the stage's 8 x 8 patch)
constexpr int TT_CW = 10;  // convolution window: the tile plus a ring of one
constexpr int TT_PW = 12;  // projected window: one more ring
constexpr int TT_UW = 65;  // k_tt_block<true>'s ldu: floats per channel row (64 pixels and one of padding)
constexpr int TT_CITEMS = TT_CW * TT_CW * 4;  // (pixel of the convolution window, channel quarter)
// k_tt_block's LDS copy of the per-channel scalars: the folded ones [0, TG_FLOATS) as k_tt_fold lays them out, then
// proj_alpha, conv_alpha, residual_alpha and the three moving means from the packed block
constexpr int LT_PA = TG_FLOATS, LT_CA = LT_PA + 16, LT_RA = LT_CA + 16, LT_PM = LT_RA + 64, LT_CM = LT_PM + 16, LT_EM = LT_CM + 16;
constexpr int LT_FLOATS = LT_EM + 64;

// offset, inside the bottleneck's part of the packed block, of per-channel gradient number r of a thread whose channel
// quarter is kq (k_tt_block's el order: exp_gamma, exp_beta, residual_alpha of the quarter's 16 channels; conv_gamma,
// conv_beta, conv_alpha and proj_gamma, proj_beta, proj_alpha of its four)
__device__ __forceinline__ int tt_elem_slot(int r, int kq)
{
    if (r < 16) return TT_EG + 16 * kq + r;
    if (r < 32) return TT_EB + 16 * kq + r - 16;
    if (r < 48) return TT_RA + 16 * kq + r - 32;
    if (r < 52) return TT_CG + 4 * kq + r - 48;
    if (r < 56) return TT_CB + 4 * kq + r - 52;
    if (r < 60) return TT_CA + 4 * kq + r - 56;
    if (r < 64) return TT_PG + 4 * kq + r - 60;
    if (r < 68) return TT_PB + 4 * kq + r - 64;
    if (r < 72) return TT_PA + 4 * kq + r - 68;
    return -1;
}

}  // namespace

bool train_tail_fits(int H, int W) { return train_stage_fits(H, W) && bottleneck_mfma_fits(64, H, W); }

// P = the bottleneck's part of the packed block
__global__ __launch_bounds__(256) void k_tt_fold(const float *__restrict__ P, float *__restrict__ F)
{
    for (int i = threadIdx.x; i < TG_FLOATS; i += 256) {
        int j, kind, g, b, m, vr;
        if (i < TG_CS) { j = i & 15; kind = i >> 4; g = TT_PG; b = TT_PB; m = TT_PM; vr = TT_PV; }
        else if (i < TG_ES) { j = (i - TG_CS) & 15; kind = (i - TG_CS) >> 4; g = TT_CG; b = TT_CB; m = TT_CM; vr = TT_CV; }
        else { j = (i - TG_ES) & 63; kind = (i - TG_ES) >> 6; g = TT_EG; b = TT_EB; m = TT_EM; vr = TT_EV; }
        const float sg = P[g + j] / sqrtf(P[vr + j] + 1e-3f);
        F[i] = kind == 0 ? sg : (kind == 1 ? fmaf(-P[m + j], sg, P[b + j]) : 1.0f / sqrtf(P[vr + j] + 1e-3f));
    }
}

// The backward of a regular 64 -> 16 -> 16 -> 64 bottleneck.  x [N,H,W,64] = its input, g = dL/d(its output) [N,H,W,64].  A
// workgroup owns one 8 x 8 tile of pixels for all N images and takes tiles blockIdx.x + G i (the stage's tiles).  Per image:
//   P   wave w = projected channels 4w .. 4w + 3 (weights in scalar registers), lane = pixel of the 12 x 12 window whose corner
//       is (i0 - 2, j0 - 2): the projection with BN + PReLU -> lp (zeros outside the image: the 3 x 3 convolution's SAME
//       padding), its accumulator for the tile's pixels -> lpa
//   C1  item = (pixel of the 10 x 10 window, four convolution outputs): the 3 x 3 convolution -> lca, BN + PReLU -> lq
//   C2  item = (pixel of the 10 x 10 window, 16 of the 64 outputs): the expansion, BN, + x, back through the residual PReLU and
//       the expansion's BN -> lde (tile pixels), the expansion's input gradient as four partial sums that the four lanes of a
//       pixel add in a fixed order, then, lane = four convolution channels, back through the convolution's BN + PReLU:
//       dL/d(conv accumulator) -> ldc (zeros outside the image)
//   D   thread = (pixel of the tile, four projected channels): the convolution's input gradient over the nine taps, back
//       through the projection's PReLU and BN -> lpa
//   E   the three kernel gradients as contractions over the tile's 64 pixels in a fixed order, accumulators in registers across
//       all tiles and images: proj_kernel (thread = input channel x four outputs), conv_kernel (thread = (ci, co), nine taps),
//       exp_kernel (thread = input channel x four outputs).
// The 72 per-channel sums of a thread (its channel quarter is tid & 3 in C2 and D alike) accumulate in registers and are
// folded over the 64 threads of a quarter in thread order, compensated, at the end.  gamma / beta gradients are produced
// directly, as in k_tb_block.  part [gridDim.x][TT_TRAINED]: every slot is written.
// DX (a block with another trained block below it): the block's INPUT gradient of the tile's pixels ->
// dx [N,H,W,64], written once between D and E, before the 1 / sum(mask) factor as g is: dL/du (the identity residual; C2 leaves
// it in ldu, channel-major with a row of 65 so that neither side meets a bank twice) plus the projection's input gradient
// sum_k dL/d(proj acc)[k] W_p[ci][k] (BN and PReLU are inside lpa), one fmaf chain that starts at dL/du and takes k = 0 .. 15.
template <bool DX>
__global__ __launch_bounds__(256) void k_tt_block(const float *__restrict__ x, const float *__restrict__ g, int N, int H, int W,
                                                  const float *__restrict__ P, const float *__restrict__ F,
                                                  float *__restrict__ part, float *__restrict__ dx)
{
    __shared__ __attribute__((aligned(16))) float lwc[9 * 16 * 16];
    __shared__ __attribute__((aligned(16))) float lwe[16 * 64];
    __shared__ __attribute__((aligned(16))) float lk[LT_FLOATS];
    __shared__ __attribute__((aligned(16))) float lp[TT_PW * TT_PW * 16];
    __shared__ __attribute__((aligned(16))) float lpa[64 * 16];  // P -> D: the projection's accumulator; D -> E: dL/d(that)
    __shared__ __attribute__((aligned(16))) float lca[TT_CW * TT_CW * 16];
    __shared__ __attribute__((aligned(16))) float lq[TT_CW * TT_CW * 16];
    __shared__ __attribute__((aligned(16))) float ldc[TT_CW * TT_CW * 16];
    __shared__ __attribute__((aligned(16))) float lde[64 * 64];
    __shared__ float ldu[DX ? 64 * TT_UW : 1];  // C2 -> DX: dL/du of the tile's pixels, [channel][pixel]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = tid & 3;
    const int tiles_x = (W + TT_Q - 1) / TT_Q, tiles = tiles_x * ((H + TT_Q - 1) / TT_Q);
    const long HW = (long)H * W;
    float el[72];  // per-channel sums, tt_elem_slot order
#pragma unroll
    for (int e = 0; e < 72; ++e) el[e] = 0.0f;
    float kwp[4] = {0.0f, 0.0f, 0.0f, 0.0f}, kwe[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float kwc[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) kwc[j] = 0.0f;
    for (int i = tid; i < 9 * 16 * 16; i += 256) lwc[i] = P[TT_WC + i];
    for (int i = tid; i < 16 * 64; i += 256) lwe[i] = P[TT_WE + i];
    for (int i = tid; i < LT_FLOATS; i += 256)
        lk[i] = i < LT_PA ? F[i] : (i < LT_CA ? P[TT_PA + i - LT_PA] : (i < LT_RA ? P[TT_CA + i - LT_CA] : (i < LT_PM ? P[TT_RA + i - LT_RA]
                : (i < LT_CM ? P[TT_PM + i - LT_PM] : (i < LT_EM ? P[TT_CM + i - LT_CM] : P[TT_EM + i - LT_EM])))));
    const int dqp = tid >> 2, dil = dqp >> 3, djl = dqp & 7;  // D: the thread's pixel of the tile
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int i0 = (t / tiles_x) * TT_Q, j0 = (t % tiles_x) * TT_Q;
        for (int n = 0; n < N; ++n) {
            const float *xn = x + (long)n * HW * 64;
            const float *gn = g + (long)n * HW * 64;
            __syncthreads();  // E of the previous image is done with the LDS arrays (and the weights are in place)
            // ---- P
#pragma unroll 1
            for (int e = lane; e < TT_PW * TT_PW; e += 64) {
                const int pi = e / TT_PW, pj = e % TT_PW;
                const int qi = i0 - 2 + pi, qj = j0 - 2 + pj;
                const bool ok = qi >= 0 && qi < H && qj >= 0 && qj < W;
                const long pix = (long)min(max(qi, 0), H - 1) * W + min(max(qj, 0), W - 1);
                const float4 *xp = reinterpret_cast<const float4 *>(xn + pix * 64);
                float ap[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
                for (int c4 = 0; c4 < 16; ++c4) {
                    const float4 x4 = xp[c4];
                    const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
                    for (int c = 0; c < 4; ++c)
#pragma unroll
                        for (int k = 0; k < 4; ++k) ap[k] = fmaf(xv[c], P[TT_WP + (4 * c4 + c) * 16 + 4 * wv + k], ap[k]);
                }
                float pv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int ch = 4 * wv + k;
                    pv[k] = ok ? prelu(fmaf(ap[k], lk[TG_PS + ch], lk[TG_PT + ch]), lk[LT_PA + ch]) : 0.0f;
                }
                reinterpret_cast<float4 *>(lp)[e * 4 + wv] = make_float4(pv[0], pv[1], pv[2], pv[3]);
                if (pi >= 2 && pi < 2 + TT_Q && pj >= 2 && pj < 2 + TT_Q)
                    reinterpret_cast<float4 *>(lpa)[((pi - 2) * TT_Q + pj - 2) * 4 + wv] = make_float4(ap[0], ap[1], ap[2], ap[3]);
            }
            __syncthreads();
            // ---- C1
#pragma unroll 1
            for (int it = tid; it < TT_CITEMS; it += 256) {
                const int e = it >> 2, pi = e / TT_CW, pj = e % TT_CW;
                float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
                for (int tp = 0; tp < 9; ++tp) {
                    const int kh = tp / 3, kw = tp % 3;
                    const float4 *pp = reinterpret_cast<const float4 *>(lp) + ((pi + kh) * TT_PW + pj + kw) * 4;
                    const float4 *wt = reinterpret_cast<const float4 *>(lwc) + tp * 16 * 4 + kq;
#pragma unroll
                    for (int c4 = 0; c4 < 4; ++c4) {
                        const float4 p4 = pp[c4];
                        const float pvv[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const float4 w4 = wt[(4 * c4 + c) * 4];
                            acc[0] = fmaf(pvv[c], w4.x, acc[0]);
                            acc[1] = fmaf(pvv[c], w4.y, acc[1]);
                            acc[2] = fmaf(pvv[c], w4.z, acc[2]);
                            acc[3] = fmaf(pvv[c], w4.w, acc[3]);
                        }
                    }
                }
                float qv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int ch = 4 * kq + k;
                    qv[k] = prelu(fmaf(acc[k], lk[TG_CS + ch], lk[TG_CT + ch]), lk[LT_CA + ch]);
                }
                reinterpret_cast<float4 *>(lca)[it] = make_float4(acc[0], acc[1], acc[2], acc[3]);
                reinterpret_cast<float4 *>(lq)[it] = make_float4(qv[0], qv[1], qv[2], qv[3]);
            }
            __syncthreads();
            // ---- C2 (TT_CITEMS and 256 are multiples of 4: the four lanes of a pixel are active together)
#pragma unroll 1
            for (int it = tid; it < TT_CITEMS; it += 256) {
                const int e = it >> 2, pi = e / TT_CW, pj = e % TT_CW;
                const int gi = i0 - 1 + pi, gj = j0 - 1 + pj;
                const bool ok = gi >= 0 && gi < H && gj >= 0 && gj < W;
                const bool own = pi >= 1 && pi <= TT_Q && pj >= 1 && pj <= TT_Q;
                const bool acc_own = own && ok;
                const long pix = (long)min(max(gi, 0), H - 1) * W + min(max(gj, 0), W - 1);
                const float4 *xr = reinterpret_cast<const float4 *>(xn + pix * 64 + 16 * kq);
                const float4 *gr = reinterpret_cast<const float4 *>(gn + pix * 64 + 16 * kq);
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
                    const float4 x4 = xr[c4], g4 = gr[c4];
                    const float xv[4] = {x4.x, x4.y, x4.z, x4.w}, gv[4] = {g4.x, g4.y, g4.z, g4.w};
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
                        const float u = fmaf(ev[c], lk[TG_ES + co], lk[TG_ET + co]) + xv[c];
                        const float d = ok ? gv[c] : 0.0f;
                        const float du = d * dprelu(u, lk[LT_RA + co]);
                        if (acc_own) {
                            el[lc] += du * ((ev[c] - lk[LT_EM + co]) * lk[TG_EI + co]);
                            el[16 + lc] += du;
                            el[32 + lc] += d * neg(u);
                        }
                        de[c] = du * lk[TG_ES + co];
                        if constexpr (DX)
                            if (own) ldu[co * TT_UW + (pi - 1) * TT_Q + pj - 1] = du;
                    }
                    if (own)
                        reinterpret_cast<float4 *>(lde)[((pi - 1) * TT_Q + pj - 1) * 16 + 4 * kq + c4] = make_float4(de[0], de[1], de[2], de[3]);
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
                    const float yc = fmaf(accc[k], lk[TG_CS + ch], lk[TG_CT + ch]);
                    const float dyc = dqk * dprelu(yc, lk[LT_CA + ch]);
                    if (acc_own) {
                        el[48 + k] += dyc * ((accc[k] - lk[LT_CM + ch]) * lk[TG_CI + ch]);
                        el[52 + k] += dyc;
                        el[56 + k] += dqk * neg(yc);
                    }
                    da[k] = dyc * lk[TG_CS + ch];
                }
                reinterpret_cast<float4 *>(ldc)[it] = make_float4(da[0], da[1], da[2], da[3]);  // (zeros outside the map: d = 0)
            }
            __syncthreads();
            // ---- D
            {
                const bool valid = i0 + dil < H && j0 + djl < W;
                float dp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
                for (int tp = 0; tp < 9; ++tp) {
                    const int kh = tp / 3, kw = tp % 3;
                    const float4 *dcp = reinterpret_cast<const float4 *>(ldc) + ((dil + 2 - kh) * TT_CW + djl + 2 - kw) * 4;
                    const float4 *wt = reinterpret_cast<const float4 *>(lwc) + (tp * 16 + 4 * kq) * 4;
#pragma unroll
                    for (int c4 = 0; c4 < 4; ++c4) {
                        const float4 d4 = dcp[c4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float4 w4 = wt[k * 4 + c4];
                            dp[k] = fmaf(d4.x, w4.x, dp[k]);
                            dp[k] = fmaf(d4.y, w4.y, dp[k]);
                            dp[k] = fmaf(d4.z, w4.z, dp[k]);
                            dp[k] = fmaf(d4.w, w4.w, dp[k]);
                        }
                    }
                }
                const float4 a4 = reinterpret_cast<const float4 *>(lpa)[tid];
                const float accp[4] = {a4.x, a4.y, a4.z, a4.w};
                float dap[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int ch = 4 * kq + k;
                    const float yp = fmaf(accp[k], lk[TG_PS + ch], lk[TG_PT + ch]);
                    const float dyp = dp[k] * dprelu(yp, lk[LT_PA + ch]);
                    if (valid) {
                        el[60 + k] += dyp * ((accp[k] - lk[LT_PM + ch]) * lk[TG_PI + ch]);
                        el[64 + k] += dyp;
                        el[68 + k] += dp[k] * neg(yp);
                    }
                    dap[k] = valid ? dyp * lk[TG_PS + ch] : 0.0f;
                }
                reinterpret_cast<float4 *>(lpa)[tid] = make_float4(dap[0], dap[1], dap[2], dap[3]);
            }
            __syncthreads();
            if constexpr (DX) {
                // lane = pixel of the tile, wave = 16 input channels with proj_kernel's rows in scalar registers
                const int qi = i0 + (lane >> 3), qj = j0 + (lane & 7);
                const bool inside = qi < H && qj < W;
                float dv[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 d = reinterpret_cast<const float4 *>(lpa)[lane * 4 + q];
                    dv[4 * q] = d.x; dv[4 * q + 1] = d.y; dv[4 * q + 2] = d.z; dv[4 * q + 3] = d.w;
                }
                float *dxp = dx + ((long)n * HW + (long)min(qi, H - 1) * W + min(qj, W - 1)) * 64;
#pragma unroll 1
                for (int ci = 16 * wv; ci < 16 * wv + 16; ++ci) {
                    float v = ldu[ci * TT_UW + lane];
#pragma unroll
                    for (int k = 0; k < 16; ++k) v = fmaf(dv[k], P[TT_WP + ci * 16 + k], v);
                    if (inside) dxp[ci] = v;
                }
            }
            // ---- E
            {
                const int c = tid >> 2;
#pragma unroll 8
                for (int p = 0; p < 64; ++p) {
                    const long pix = (long)min(i0 + (p >> 3), H - 1) * W + min(j0 + (p & 7), W - 1);
                    const float a = xn[pix * 64 + c];
                    const float4 d = reinterpret_cast<const float4 *>(lpa)[p * 4 + kq];
                    kwp[0] = fmaf(a, d.x, kwp[0]); kwp[1] = fmaf(a, d.y, kwp[1]);
                    kwp[2] = fmaf(a, d.z, kwp[2]); kwp[3] = fmaf(a, d.w, kwp[3]);
                }
            }
            {
                const int ci = tid >> 4, co = tid & 15;
#pragma unroll 2
                for (int p = 0; p < 64; ++p) {
                    const int il = p >> 3, jl = p & 7;
                    const float d = ldc[((il + 1) * TT_CW + jl + 1) * 16 + co];
#pragma unroll
                    for (int tp = 0; tp < 9; ++tp)
                        kwc[tp] = fmaf(lp[((il + 1 + tp / 3) * TT_PW + jl + 1 + tp % 3) * 16 + ci], d, kwc[tp]);
                }
#pragma unroll 4
                for (int p = 0; p < 64; ++p) {
                    const float a = lq[(((p >> 3) + 1) * TT_CW + (p & 7) + 1) * 16 + ci];
                    const float4 d = reinterpret_cast<const float4 *>(lde)[p * 16 + co];
                    kwe[0] = fmaf(a, d.x, kwe[0]); kwe[1] = fmaf(a, d.y, kwe[1]);
                    kwe[2] = fmaf(a, d.z, kwe[2]); kwe[3] = fmaf(a, d.w, kwe[3]);
                }
            }
        }
    }
    float *row = part + (long)blockIdx.x * TT_TRAINED;
    {
        const int c = tid >> 2, ci = tid >> 4, co = tid & 15;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            row[TT_WP + c * 16 + 4 * kq + k] = kwp[k];
            row[TT_WE + ci * 64 + 4 * co + k] = kwe[k];
        }
#pragma unroll
        for (int tp = 0; tp < 9; ++tp) row[TT_WC + (tp * 16 + ci) * 16 + co] = kwc[tp];
    }
    // the per-channel sums: 16 numbers at a time through lde ([16][256]); thread (e, quarter) sums the 64 threads of its
    // quarter in thread order
#pragma unroll
    for (int ch = 0; ch < 5; ++ch) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; ++e) lde[e * 256 + tid] = ch * 16 + e < 72 ? el[(ch * 16 + e) % 72] : 0.0f;
        __syncthreads();
        const int slot = tid < 64 ? tt_elem_slot(ch * 16 + (tid >> 2), kq) : -1;
        if (slot >= 0) {
            float sum = 0.0f, comp = 0.0f;
            for (int j = 0; j < 64; ++j) kahan(sum, comp, lde[(tid >> 2) * 256 + 4 * j + kq]);
            row[slot] = sum;
        }
    }
}

// the bottleneck's forward as the scoring path runs it, on the block's own weights: PT = its part of the packed block
static hipError_t tail_forward(const float *x41, float *a42, int N, int H, int W, const float *PT, float *F, hipStream_t s)
{
    hipLaunchKernelGGL(k_tt_fold, dim3(1), dim3(256), 0, s, PT, F);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_bottleneck_mfma(x41, a42, N, H, W, 64, 1, PT + TT_WP, F + TG_PS, F + TG_PT, PT + TT_PA, PT + TT_WC, nullptr,
                                  F + TG_CS, F + TG_CT, PT + TT_CA, PT + TT_WE, F + TG_ES, F + TG_ET, PT + TT_RA, s);
}

// one regular block's backward: x = its input, g = dL/d(its output), PT / F = its part of the packed block and its folded
// form; dx not NULL: its input gradient goes there (k_tt_block<true>)
static hipError_t tail_block_grad(const float *x, const float *g, int N, int H, int W, int G, const float *PT, const float *F,
                                  float *part, float *dx, hipStream_t s)
{
    const double pix = (double)N * H * W;
    // per pixel: the projection on a 12 x 12 window for an 8 x 8 tile (1024 FMAs x 2.25), the convolution and the expansion
    // forward and backward on the 10 x 10 window ((2304 + 2 x 1024) x 1.5625), the convolution's input gradient 2304, the
    // contractions 1024 + 2304 + 1024; the input gradient another 1024 and its 64 floats
    ProfScope prof(dx ? "k_tt_block<dx>" : "k_tt_block",
                   2.0 * pix * (1024.0 * 2.25 + 4352.0 * 1.5625 + 2304.0 + 4352.0 + (dx ? 1024.0 : 0.0)),
                   4.0 * pix * 64.0 * (dx ? 3 : 2) + 4.0 * G * TT_TRAINED, s);
    if (dx)
        hipLaunchKernelGGL(k_tt_block<true>, dim3(G), dim3(256), 0, s, x, g, N, H, W, PT, F, part, dx);
    else
        hipLaunchKernelGGL(k_tt_block<false>, dim3(G), dim3(256), 0, s, x, g, N, H, W, PT, F, part, dx);
    return hipGetLastError();
}

hipError_t launch_train_tail_grad(const float *x, const int64_t *argmax, int N, int H, int W, int K, const float *params,
                                  const uint8_t *labels, const float *mask, float weight, float label_smoothing,
                                  int max_workgroups, const TrainTailWs &ws, double *loss, float *grad, hipStream_t s,
                                  const TrainBlockSemi *semi, int R, float *dx_low)
{
    if (N < 1 || K < 2 || K > 32 || R < 1 || R > 2 || !train_tail_fits(H, W)) return hipErrorInvalidValue;
    const int G = train_stage_workgroups(H, W, max_workgroups);
    const float *PT = params + train_stage_floats(K), *PT1 = PT + TT_FLOATS;  // Bottleneck4_2's part, Bottleneck4_1's
    hipError_t e;
    const float *x41 = x;
    if (R == 2) {
        e = tail_forward(x, ws.a41, N, H, W, PT1, ws.tfold2, s);
        if (e != hipSuccess) return e;
        x41 = ws.a41;
    }
    e = tail_forward(x41, ws.a42, N, H, W, PT, ws.tfold, s);
    if (e != hipSuccess) return e;
    e = launch_train_stage_grad(ws.a42, argmax, N, H, W, K, params, labels, mask, weight, label_smoothing, max_workgroups, ws.ts,
                                loss, grad, s, semi, ws.dx4);
    if (e != hipSuccess) return e;
    e = tail_block_grad(x41, ws.dx4, N, H, W, G, PT, ws.tfold, ws.part_t, R == 2 ? ws.dx41 : dx_low, s);
    if (e != hipSuccess) return e;
    if (R == 2) {
        e = tail_block_grad(x, ws.dx41, N, H, W, G, PT1, ws.tfold2, ws.part_t2, dx_low, s);
        if (e != hipSuccess) return e;
    }
    for (int r = 0; r < R; ++r) {
        e = launch_train_finish<TT_TRAINED, TT_FLOATS>("k_tt_finish", r ? ws.part_t2 : ws.part_t, ws.ts.tb.lpart, G, G,
                                                       grad + train_stage_floats(K) + r * TT_FLOATS, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_train_tail_targets(const float *x_raw, const int64_t *argmax_raw, int N, int H, int W, int K,
                                     const float *params, int max_workgroups, const TrainTailWs &ws,
                                     const TrainBlockSemi &semi, hipStream_t s, int R)
{
    if (N < 1 || K < 2 || K > 32 || R < 1 || R > 2 || !train_tail_fits(H, W) || !x_raw) return hipErrorInvalidValue;
    if (!semi.labelled) return hipSuccess;  // every image is labelled: no pseudo target is read
    const float *PT = params + train_stage_floats(K);
    const float *x41_raw = x_raw;
    if (R == 2) {
        const hipError_t e1 = tail_forward(x_raw, ws.a41, N, H, W, PT + TT_FLOATS, ws.tfold2, s);
        if (e1 != hipSuccess) return e1;
        x41_raw = ws.a41;
    }
    const hipError_t e = tail_forward(x41_raw, ws.a42, N, H, W, PT, ws.tfold, s);
    if (e != hipSuccess) return e;
    return launch_train_stage_targets(ws.a42, argmax_raw, N, H, W, K, params, max_workgroups, ws.ts, semi, s);
}

}  // namespace ssal
