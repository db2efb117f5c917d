// ssal_train_icnet_bneck2.hip -- training of ICNet through conv5_2: the three layers of the backbone's last bottleneck but one
// (Bneck(256, 1024, 1, 4), the shape of conv5_3) under everything the bottleneck trainer trains, over everything below conv5_1
// and the two other frozen branches, gfx950.  Behind the forward path's own launches on the weights being
// trained (launch_igemm three times) and the bottleneck trainer's gradient (ssal_train_icnet_bneck.hip, which leaves gr =
// dL/dconv5_3_1x1_reduce behind its ReLU, g53 = dL/dconv5_3 behind its ReLU, the reduce layer's batch-norm row and 1 / sum(mask)):
//   k_icnet_bneck2_pack     the packed vector -> the three kernels in launch_igemm's layouts, their folded batch-norm rows
//   k_icnet_bneck2_dx_red   the data gradient through conv5_3's reduce layer on the fp32 matrix cores, the bottleneck's join in
//                           the epilogue: g52 = relu'(conv5_2) (g53 + (s_r gr) K_r^T)
//   k_icnet_pyramid_wgrad<256, 1024>, its finish and gamma (ssal_train_icnet_pyramid.hip) for conv5_2's increase layer
//   launch_icnet_bneck_link (ssal_train_icnet_bneck.hip) a second time, for conv5_2
// g52 is un-normalised, as g53 and gr are.  No floating-point atomics, no inline assembly, 64-bit offsets, grids strided over the
// tiles: two runs give the same bits.
#include "ssal_icnet.h"
#include "ssal_internal.h"
#include "ssal_mfma.h"
#include "ssal_prof.h"
#include "ssal_train_icnet_bneck2.h"

namespace ssal {

// P: reduce kernel [1024][256] | gamma | beta | 3 x 3 kernel [9][256][256] | gamma | beta | increase kernel [256][1024] | gamma |
// beta; stats: mean_r | var_r | mean_3 | var_3 (256 each) | mean_i | var_i (1024 each).  rows: icnet_bn_row's s_r | t_r | s_3 |
// t_3 | s_i | t_i
__global__ __launch_bounds__(256) void k_icnet_bneck2_pack(const float *__restrict__ P, const float *__restrict__ stats,
                                                           float *__restrict__ wt_r, float *__restrict__ wt_3,
                                                           float *__restrict__ wt_i, float *__restrict__ rows)
{
    constexpr int KR = BK_CIN * BK_C, K3 = 9 * BK_C * BK_C, KI = PO_CIN * PO_CO;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o < KR) {
        wt_r[igemm_wt_index(0, o >> 8, o & 255, BK_CIN / 32, BK_C)] = P[B2_KR + o];
    } else if (o < KR + K3) {
        const int e = o - KR;
        wt_3[igemm_wt_index(e >> 16, (e >> 8) & 255, e & 255, BK_C / 32, BK_C)] = P[B2_K3 + e];
    } else if (o < KR + K3 + KI) {
        const int e = o - KR - K3;
        wt_i[igemm_wt_index(0, e >> 10, e & 1023, PO_CIN / 32, PO_CO)] = P[B2_KI + e];
    } else if (o < KR + K3 + KI + 2 * BK_C) {
        const int e = o - KR - K3 - KI, b = e >> 8, c = e & 255;
        icnet_bn_row(P[(b ? B2_G3 : B2_GR) + c], P[(b ? B2_B3 : B2_BR) + c], stats[2 * b * BK_C + c],
                     stats[(2 * b + 1) * BK_C + c], rows + 2 * b * BK_C + c, rows + (2 * b + 1) * BK_C + c);
    } else if (o < KR + K3 + KI + 2 * BK_C + PO_CO) {
        const int c = o - KR - K3 - KI - 2 * BK_C;
        icnet_bn_row(P[B2_GI + c], P[B2_BI + c], stats[4 * BK_C + c], stats[4 * BK_C + PO_CO + c], rows + 4 * BK_C + c,
                     rows + 4 * BK_C + PO_CO + c);
    }
}

// g52[p, ci] = c52[p, ci] > 0 ? g53[p, ci] + sum_co (s_r[co] gr[p, co]) K_r[ci, co] : 0: dL/dconv5_2 behind its ReLU, the join of
// conv5_3's identity shortcut with the data gradient of its reduce layer (1 x 1, 1024 -> 256).  gr [pixels, 256] un-normalised
// behind conv5_3_1x1_reduce's ReLU, K_r [1024][256], s_r [256] its batch-norm scale, g53 [pixels, 1024] un-normalised behind
// conv5_3's ReLU, c52 = conv5_2 [pixels, 1024] (the fp32 forward values) -> g52 [pixels, 1024]; the un-masked sum never reaches
// memory.
// grid (G, 8): k_icnet_pool_dx's plan (ssal_train_icnet_pool.hip), a kernel of its own for the epilogue.  Workgroup (b, y) owns
// the input channels ci = 128 y .. + 127 and takes the tiles b, b + G, ... of B2_DX_PT = 64 pixels (linear over [N, h32, w32]);
// wave w keeps D[pixel 32 j .. + 31][ci = 128 y + 32 w .. + 31], j = 0, 1, in two v_mfma_f32_32x32x2_f32 accumulators.  Per
// tile, for each of the 8 chunks of 32 output channels (ascending): s_r gr of the chunk (the product rounded once, here; zeros
// behind the last pixel) -> LDS as [co][pixel], K_r's chunk -> LDS as [co][ci] (every global load a float4 of a 128-byte row
// piece), then 16 steps of two co each: lane (r = lane & 31, h = lane >> 5) feeds gs[pixel 32 j + r][2 s + h] and
// K_r[32 w + r][2 s + h].  One accumulator therefore adds its 256 products in ascending co, two per instruction; the epilogue
// adds g53 to the finished sum, once, and masks.
// Epilogue: accumulator register i of lane (r, h) is pixel 32 j + (i & 3) + 8 (i >> 2) + 4 h, channel 32 w + r -- g53 and c52
// are read, and g52 written, at that very offset: per register the 32 lanes of a half wave touch 128 consecutive bytes of one
// pixel's row.
// LDS banking, as k_icnet_pool_dx states it (32 banks and groups of 32 lanes for 4-byte accesses): an MFMA operand read is 32
// consecutive floats per lane group, free of conflicts at any leading dimension; a staging store's lane group holds 8 quads q x
// 4 rows, at (4 q + i) LD + row, so an odd LD (4 LD = 4 mod 32) puts its 32 lanes on 32 banks.
constexpr int B2_CC = 32;    // output channels of the reduce layer per chunk
constexpr int B2_LDG = 65;   // 64 pixels + 1
constexpr int B2_LDK = 129;  // 128 ci + 1
__global__ __launch_bounds__(256) void k_icnet_bneck2_dx_red(const float *__restrict__ gr, const float *__restrict__ Kr,
                                                             const float *__restrict__ sr, const float *__restrict__ g53,
                                                             const float *__restrict__ c52, long pixels,
                                                             float *__restrict__ g52)
{
    __shared__ float Gs[B2_CC * B2_LDG];
    __shared__ float Ks[B2_CC * B2_LDK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int ci0 = 128 * blockIdx.y;
    const long tiles = (pixels + B2_DX_PT - 1) / B2_DX_PT;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long p0 = t * B2_DX_PT;
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][i] = 0.0f;
        for (int cc = 0; cc < BK_C / B2_CC; ++cc) {
            __syncthreads();  // the previous chunk's MFMAs are done with Gs / Ks
            for (int e = tid; e < B2_DX_PT * (B2_CC / 4); e += 256) {
                const int pl = e >> 3, q = e & 7;
                const long p = p0 + pl;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (p < pixels) {
                    const float4 gv = reinterpret_cast<const float4 *>(gr + p * BK_C + B2_CC * cc)[q];
                    const float4 sv = reinterpret_cast<const float4 *>(sr + B2_CC * cc)[q];
                    v = make_float4(sv.x * gv.x, sv.y * gv.y, sv.z * gv.z, sv.w * gv.w);
                }
                Gs[(4 * q + 0) * B2_LDG + pl] = v.x;
                Gs[(4 * q + 1) * B2_LDG + pl] = v.y;
                Gs[(4 * q + 2) * B2_LDG + pl] = v.z;
                Gs[(4 * q + 3) * B2_LDG + pl] = v.w;
            }
            for (int e = tid; e < 128 * (B2_CC / 4); e += 256) {
                const int ci = e >> 3, q = e & 7;
                const float4 v = reinterpret_cast<const float4 *>(Kr + (long)(ci0 + ci) * BK_C + B2_CC * cc)[q];
                Ks[(4 * q + 0) * B2_LDK + ci] = v.x;
                Ks[(4 * q + 1) * B2_LDK + ci] = v.y;
                Ks[(4 * q + 2) * B2_LDK + ci] = v.z;
                Ks[(4 * q + 3) * B2_LDK + ci] = v.w;
            }
            __syncthreads();
            const float *ap = Gs + hh * B2_LDG + r;
            const float *bp = Ks + hh * B2_LDK + 32 * wave + r;
#pragma unroll 4
            for (int s = 0; s < B2_CC / 2; ++s) {
                const float b = bp[2 * s * B2_LDK];
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = mfma32(ap[2 * s * B2_LDG + 32 * j], b, acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const long p = p0 + 32 * j + (i & 3) + 8 * (i >> 2) + 4 * hh;
                if (p < pixels) {
                    const long o = p * BK_CIN + ci0 + 32 * wave + r;
                    g52[o] = c52[o] > 0.0f ? g53[o] + acc[j][i] : 0.0f;
                }
            }
    }
}

hipError_t launch_icnet_bneck2_grad(const float *c51, const float *c31, const float *c3, int N, int h32, int w32, int K,
                                    const float *params, const float *stats, const uint8_t *labels, const float *mask,
                                    float weight, float label_smoothing, int max_workgroups, const IcnetBneck2Ws &ws,
                                    double *loss, float *grad, hipStream_t s)
{
    if (N < 1 || K < 2 || K > 32 || max_workgroups < 0 || !icnet_bneck_fits(h32, w32)) return hipErrorInvalidValue;
    const long pixels = (long)N * h32 * w32;
    const double pix32 = (double)pixels;
    constexpr int PACK = BK_CIN * BK_C + 9 * BK_C * BK_C + PO_CIN * PO_CO + 2 * BK_C + PO_CO;
    const float *s_r = ws.rows, *s_3 = ws.rows + 2 * BK_C, *s_i = ws.rows + 4 * BK_C;
    const IcnetBneckWs &up = ws.bneck;
    hipError_t e;
    // ---- forward: the pack, then run_trunk's three launches of conv5_2 on the weights being trained ----
    {
        ProfScope prof("k_icnet_bneck2_pack", 0.0, 8.0 * PACK, s);
        hipLaunchKernelGGL(k_icnet_bneck2_pack, dim3(icnet_cdiv(PACK, 256)), dim3(256), 0, s, params, stats, ws.wt_r, ws.wt_3,
                           ws.wt_i, ws.rows);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    e = launch_igemm(c51, N, h32, w32, BK_CIN, ws.wt_r, 1, 1, BK_C, 1, 1, s_r, s_r + BK_C, nullptr, true, false, ws.rd, s);
    if (e != hipSuccess) return e;
    e = launch_igemm(ws.rd, N, h32, w32, BK_C, ws.wt_3, 3, 3, BK_C, 1, BK_DIL, s_3, s_3 + BK_C, nullptr, true, false, ws.a33, s);
    if (e != hipSuccess) return e;
    e = launch_igemm(ws.a33, N, h32, w32, PO_CIN, ws.wt_i, 1, 1, PO_CO, 1, 1, s_i, s_i + PO_CO, c51, true, false, ws.c52, s);
    if (e != hipSuccess) return e;
    // section 42 as it stands, on that conv5_2: conv5_3, the pyramid pooling, the pyramid head, the loss, its 26 gradients; gr behind
    // conv5_3_1x1_reduce's ReLU and g53 behind conv5_3's
    e = launch_icnet_bneck_grad(ws.c52, c31, c3, N, h32, w32, K, params + B2_BNECK, stats + B2_STATS_OWN, labels, mask, weight,
                                label_smoothing, max_workgroups, up, loss, grad + B2_BNECK, s);
    if (e != hipSuccess) return e;
    const float *scale = up.pool.pyramid.cascade.fusion.fold + FU_PART;  // 1 / sum(mask), as the fusion trainer's finish left it
    // ---- backward: onto conv5_2, then conv5_2 as a link.  conv5_3's g3, gr, partials and folds are dead from here on ----
    {
        const int G = icnet_grid(icnet_cdiv(pixels, B2_DX_PT), B2_DX_MAX_WG, max_workgroups);
        ProfScope prof("k_icnet_bneck2_dx_red", 2.0 * pix32 * BK_CIN * BK_C,
                       4.0 * pix32 * (BK_C + 3.0 * BK_CIN) + 4.0 * (double)icnet_cdiv(pixels, B2_DX_PT) * BK_CIN * BK_C, s);
        hipLaunchKernelGGL(k_icnet_bneck2_dx_red, dim3(G, BK_CIN / 128), dim3(256), 0, s, up.gr, params + B2_BNECK + BK_KR, up.rows,
                           up.pool.g53, ws.c52, pixels, ws.g52);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    static const char *const wi[] = {"k_icnet_bneck2_wgrad_i", "k_icnet_bneck2_finish_i", "k_icnet_bneck2_gamma_i"};
    e = launch_icnet_wgrad_256x1024(ws.a33, ws.g52, pixels, max_workgroups, scale, s_i, params + B2_KI, stats + 4 * BK_C,
                                    stats + 4 * BK_C + PO_CO, up.pool.part, up.pool.fold, grad + B2_KI, grad + B2_GI, grad + B2_BI, s,
                                    wi);
    if (e != hipSuccess) return e;
    static const char *const names[] = {"k_icnet_bneck2_dx_inc", "k_icnet_bneck2_wgrad3", "k_icnet_bneck2_finish3",
                                        "k_icnet_bneck2_gamma3", "k_icnet_bneck2_dx_3x3", "k_icnet_bneck2_wgrad_r",
                                        "k_icnet_bneck2_finish_r", "k_icnet_bneck2_gamma_r"};
    const IcnetBneckLink L = {c51, ws.rd, ws.a33, ws.g52, params + B2_KI, s_i, params + B2_K3, s_3, stats + 2 * BK_C,
                              stats + 3 * BK_C, params + B2_KR, s_r, stats, stats + BK_C, scale, up.g3, up.gr, up.part3, up.fold3,
                              up.partr, up.foldr, grad + B2_K3, grad + B2_G3, grad + B2_B3, grad + B2_KR, grad + B2_GR,
                              grad + B2_BR, names};
    return launch_icnet_bneck_link(L, N, h32, w32, max_workgroups, s);
}

}  // namespace ssal
