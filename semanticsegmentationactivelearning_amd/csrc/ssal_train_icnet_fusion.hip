// ssal_train_icnet_fusion.hip -- training of ICNet's last fusion stage and its output layer over a frozen trunk, gfx950
// (DESIGN.md section 28):
//   k_icnet_block_pack<128>  (ssal_train_icnet_common.h; the profile's k_icnet_fusion_pack) the packed vector -> conv_sub2 /
//                          conv3_sub1_proj in launch_igemm's layout with their folded batch-norm rows, so that the FORWARD
//                          path's own launches compute sub12_sum from the weights being trained (the head:
//                          k_icnet_head_pack, the loss and dL/d(head): k_icnet_head_grad<K, false, true>)
//   k_icnet_fusion_g       g = relu'(sub12_sum) (hw Wcls^T): the head kernel's per-tile pull-back windows gathered in a fixed
//                          order into the complete per-pixel plane
//   k_icnet_fusion_wgrad   the weight-gradient implicit GEMM on the fp32 matrix cores: sum_p u[p + tap, ci] g[p, co] for the
//                          nine dilated taps (u = resize_2x(sub24_sum), interpolated from a staged window, never written),
//                          sum_p conv3_sub1[p, ci] g[p, co] and sum_p g[p, co] as a tenth tap; split-K over workgroups
//   k_icnet_block_finish<128, true>  (common; k_icnet_fusion_finish) fixed-order fold of the partials, the batch-norm scale,
//                          1 / sum(mask)
//   k_icnet_block_gamma<128>  (common; k_icnet_fusion_gamma) dGamma = (sum K dKraw - mean dBeta) / sqrt(var + eps): sum_p g acc
//                          re-associated, so the pre-BN accumulators are never formed
// No floating-point atomics, no inline assembly, 64-bit offsets: two runs give the same bits.
#include "ssal_icnet.h"
#include "ssal_internal.h"
#include "ssal_mfma.h"
#include "ssal_prof.h"
#include "ssal_score.h"
#include "ssal_train_icnet_fusion.h"

namespace ssal {

constexpr int FU_LD = 160;  // LDS row stride of the operand tiles [32 pixels][128 + pad]: the two lane halves of a
                            // ds_read_b32 (pixels 2s, 2s + 1) fall on the two halves of the 64 banks
constexpr int FU_WR = 3, FU_WC = 5;  // the window of sub24_sum behind a tile's 4 x 8 pixels of u (the +1 taps included)

bool icnet_fusion_fits(int h16, int w16)
{
    if (h16 < 1 || w16 < 1 || h16 > (1 << 26) || w16 > (1 << 26)) return false;  // 2 h16 <= 2^27: icnet_head_fits' limit
    return icnet_head_fits(2 * h16, 2 * w16);  // its 4 x 4 tiles of sub12_sum outnumber the 4 x 8 ones here
}

// hwp [N][tiles][36][K]: tile (ty, tx) of k_icnet_head_grad holds the pull-back of its own loss pixels onto the window of
// sub12_sum whose first pixel is (4 ty, 4 tx).  Pixel (r, c) lies in the windows of tiles ty in {r / 4 - 1 (when r % 4 < 2),
// r / 4} and tx likewise: at most four partial sums, added rows then columns ascending.  g[p, ch] = x[p, ch] > 0 ?
// sum_k hw[p, k] W[ch, k] : 0 (k ascending, fmaf), un-normalised.  64 pixels per workgroup.
__global__ __launch_bounds__(256) void k_icnet_fusion_g(const float *__restrict__ hwp, const float *__restrict__ x,
                                                        const float *__restrict__ head, int N, int h8, int w8, int K,
                                                        float *__restrict__ g)
{
    __shared__ __attribute__((aligned(16))) float Wt[32 * 128];  // [k][channel]
    __shared__ float hs[64 * 32];                                // [pixel][k]
    const int tid = threadIdx.x;
    for (int e = tid; e < 128 * K; e += 256) Wt[(e % K) * 128 + e / K] = head[e];
    const long total = (long)N * h8 * w8, p0 = (long)blockIdx.x * 64;
    const int txh = (w8 + 3) / 4, tyh = (h8 + 3) / 4;
    const long tiles = (long)txh * tyh;
    for (int e = tid; e < 64 * K; e += 256) {
        const int pl = e / K, k = e % K;
        const long p = p0 + pl;
        float a = 0.0f;
        if (p < total) {
            const int c = (int)(p % w8), r = (int)((p / w8) % h8);
            const long n = p / ((long)w8 * h8);
            for (int ty = r / 4 - 1; ty <= r / 4; ++ty) {
                const int wr = r - 4 * ty;
                if (ty < 0 || wr > 5) continue;
                for (int tx = c / 4 - 1; tx <= c / 4; ++tx) {
                    const int wc = c - 4 * tx;
                    if (tx < 0 || wc > 5) continue;
                    a += hwp[((n * tiles + (long)ty * txh + tx) * 36 + wr * 6 + wc) * K + k];
                }
            }
        }
        hs[pl * 32 + k] = a;
    }
    __syncthreads();
    for (int e = tid; e < 64 * 32; e += 256) {
        const int pl = e >> 5, cq = e & 31;
        const long p = p0 + pl;
        if (p >= total) continue;
        const float4 xv = reinterpret_cast<const float4 *>(x + p * 128)[cq];
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int k = 0; k < K; ++k) {
            const float h = hs[pl * 32 + k];
            const float4 w = *reinterpret_cast<const float4 *>(Wt + k * 128 + 4 * cq);
            o.x = fmaf(h, w.x, o.x);
            o.y = fmaf(h, w.y, o.y);
            o.z = fmaf(h, w.z, o.z);
            o.w = fmaf(h, w.w, o.w);
        }
        reinterpret_cast<float4 *>(g + p * 128)[cq] =
            make_float4(xv.x > 0.0f ? o.x : 0.0f, xv.y > 0.0f ? o.y : 0.0f, xv.z > 0.0f ? o.z : 0.0f, xv.w > 0.0f ? o.w : 0.0f);
    }
}

// grid (G, FU_TAPS), 256 threads.  Workgroup (b, tap) takes the pixel tiles b, b + G, ... (4 x 8 pixels of sub12_sum, image
// after image) and keeps D[ci][co] = sum_p A[p][ci] B[p][co] for its tap in registers: wave w owns the rows ci = 32 w ..
// 32 w + 31 and all 128 columns, four v_mfma_f32_32x32x2_f32 accumulators.  Per tile:
//   B = g[tile] [32][128] -> LDS (zeros outside the map);
//   tap < 9: the 3 x 5 window of sub24_sum behind the tile's shifted pixels of u -> LDS (rows / columns clamped to the map as
//     the legacy resize clamps its +1 tap), then A[p][ci] = u[p + 2 (kh - 1, kw - 1), ci] in launch_resize_bilinear's
//     arithmetic (top = tl + (tr - tl) xl, bot likewise, top + (bot - top) yl), 0 where TF's SAME padding lies;
//   tap 9: A[p][ci] = conv3_sub1[p, ci] for ci < 64, 1 for ci = 64 (that row of D is sum_p g = dBeta), 0 beyond;
//   16 steps of two pixels each: lane (r = lane & 31, h = lane >> 5) feeds A[2 s + h][32 w + r] and B[2 s + h][32 j + r].
// part [G][FU_TAPS][128][128].
// CIN = 256 (the other fusion block, section 29): grid (G, CA_TAPS, 2), blockIdx.z picks the half of the input channels a
// workgroup owns; tap 9 is the 1 x 1 branch on all 256 channels of its input, tap 10 (half 0 only) the row of ones in
// row 0.  part [G][CA_TAPS][2][128][128].  CIN = 128 compiles to the kernel it was before the parameter.
template <int CIN>
__global__ __launch_bounds__(256) void k_icnet_fusion_wgrad(const float *__restrict__ s24, const float *__restrict__ c3,
                                                            const float *__restrict__ g, int N, int h16, int w16,
                                                            float *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float As[32 * FU_LD];
    __shared__ __attribute__((aligned(16))) float Bs[32 * FU_LD];
    __shared__ __attribute__((aligned(16))) float win[FU_WR * FU_WC * 128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int tap = blockIdx.y;
    constexpr int TAPS = FusionBlock<CIN>::TAPS;
    const int half = CIN == 128 ? 0 : (int)blockIdx.z, cb = 128 * half;
    if (CIN != 128 && tap == 10 && half) return;
    const int h8 = 2 * h16, w8 = 2 * w16;
    const int tx = (w8 + FU_TW - 1) / FU_TW, ty = (h8 + FU_TH - 1) / FU_TH;
    const long per_image = (long)tx * ty, tiles = (long)N * per_image;
    const int dy = tap < 9 ? 2 * (tap / 3 - 1) : 0, dx = tap < 9 ? 2 * (tap % 3 - 1) : 0;
    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.0f;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long n = t / per_image;
        const int rem = (int)(t % per_image);
        const int y0 = (rem / tx) * FU_TH, x0 = (rem % tx) * FU_TW;
        __syncthreads();  // the previous tile's MFMAs are done with As / Bs
        for (int e = tid; e < 32 * 32; e += 256) {
            const int p = e >> 5, q = e & 31;
            const int y = y0 + (p >> 3), xx = x0 + (p & 7);
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (y < h8 && xx < w8) v = reinterpret_cast<const float4 *>(g + ((n * h8 + y) * w8 + xx) * 128)[q];
            *reinterpret_cast<float4 *>(Bs + p * FU_LD + 4 * q) = v;
        }
        if (tap < 9) {
            const int sr0 = (y0 + dy) / 2, sc0 = (x0 + dx) / 2;  // (even numerators: exact, -1 for the padding rows)
            for (int e = tid; e < FU_WR * FU_WC * 32; e += 256) {
                const int wp = e >> 5, q = e & 31;
                const int sr = min(sr0 + wp / FU_WC, h16 - 1), sc = min(sc0 + wp % FU_WC, w16 - 1);
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (sr >= 0 && sc >= 0) v = reinterpret_cast<const float4 *>(s24 + ((n * h16 + sr) * w16 + sc) * CIN + cb)[q];
                *reinterpret_cast<float4 *>(win + wp * 128 + 4 * q) = v;
            }
            __syncthreads();
            for (int e = tid; e < 32 * 32; e += 256) {
                const int p = e >> 5, q = e & 31;
                const int uy = y0 + (p >> 3) + dy, ux = x0 + (p & 7) + dx;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (uy >= 0 && uy < h8 && ux >= 0 && ux < w8) {
                    const int r0 = (uy >> 1) - sr0, c0 = (ux >> 1) - sc0;  // 0..1 and 0..3; the +1 taps: r0 + 1, c0 + 1
                    const float ly = (float)(uy & 1) * 0.5f, lx = (float)(ux & 1) * 0.5f;
                    const float4 tl = *reinterpret_cast<const float4 *>(win + (r0 * FU_WC + c0) * 128 + 4 * q);
                    const float4 tr = *reinterpret_cast<const float4 *>(win + (r0 * FU_WC + c0 + 1) * 128 + 4 * q);
                    const float4 bl = *reinterpret_cast<const float4 *>(win + ((r0 + 1) * FU_WC + c0) * 128 + 4 * q);
                    const float4 br = *reinterpret_cast<const float4 *>(win + ((r0 + 1) * FU_WC + c0 + 1) * 128 + 4 * q);
                    float top, bot;
                    top = tl.x + (tr.x - tl.x) * lx; bot = bl.x + (br.x - bl.x) * lx; v.x = top + (bot - top) * ly;
                    top = tl.y + (tr.y - tl.y) * lx; bot = bl.y + (br.y - bl.y) * lx; v.y = top + (bot - top) * ly;
                    top = tl.z + (tr.z - tl.z) * lx; bot = bl.z + (br.z - bl.z) * lx; v.z = top + (bot - top) * ly;
                    top = tl.w + (tr.w - tl.w) * lx; bot = bl.w + (br.w - bl.w) * lx; v.w = top + (bot - top) * ly;
                }
                *reinterpret_cast<float4 *>(As + p * FU_LD + 4 * q) = v;
            }
        } else {
            for (int e = tid; e < 32 * 32; e += 256) {
                const int p = e >> 5, q = e & 31;
                const int y = y0 + (p >> 3), xx = x0 + (p & 7);
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (y < h8 && xx < w8) {
                    if (CIN == 128) {
                        if (q < 16) v = reinterpret_cast<const float4 *>(c3 + ((n * h8 + y) * w8 + xx) * 64)[q];
                        else if (q == 16) v.x = 1.0f;
                    } else if (tap == 9) {
                        v = reinterpret_cast<const float4 *>(c3 + ((n * h8 + y) * w8 + xx) * CIN + cb)[q];
                    } else if (q == 0) {
                        v.x = 1.0f;
                    }
                }
                *reinterpret_cast<float4 *>(As + p * FU_LD + 4 * q) = v;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int s = 0; s < 16; ++s) {
            const float a = As[(2 * s + hh) * FU_LD + 32 * wave + r];
            const float *bp = Bs + (2 * s + hh) * FU_LD + r;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = mfma32(a, bp[32 * j], acc[j]);
        }
    }
    float *pw = part + (((long)blockIdx.x * TAPS + tap) * (CIN / 128) + half) * (128 * 128);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * hh;
            pw[(32 * wave + row) * 128 + 32 * j + r] = acc[j][i];
        }
}

// the pack, then the forward path's own launches (ssal_icnet_api.hip, run_trunk) on the weights being trained:
// ws.proj = BN(conv3_sub1_proj(c3)), ws.sub12 = sub12_sum
static hipError_t fusion_forward(const float *sub24, const float *c3, int N, int h16, int w16, const float *params,
                                 const float *stats, const IcnetFusionWs &ws, hipStream_t s)
{
    const int h8 = 2 * h16, w8 = 2 * w16;
    hipError_t e;
    {
        ProfScope prof("k_icnet_fusion_pack", 0.0, 8.0 * FU_HEAD, s);
        hipLaunchKernelGGL(k_icnet_block_pack<128>, dim3(icnet_cdiv(FU_GA + 64 * 128 + 256, 256)), dim3(256), 0, s, params,
                           stats, ws.wt_a, ws.wt_b, ws.rows);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    e = launch_igemm(c3, N, h8, w8, 64, ws.wt_b, 1, 1, 128, 1, 1, ws.rows + 256, ws.rows + 384, nullptr, false, false,
                     ws.proj, s);
    if (e != hipSuccess) return e;
    return launch_igemm(sub24, N, h16, w16, 128, ws.wt_a, 3, 3, 128, 1, 2, ws.rows, ws.rows + 128, ws.proj, true, true,
                        ws.sub12, s);
}

hipError_t launch_icnet_fusion_targets(const float *sub24_raw, const float *c3_raw, int N, int h16, int w16, int K,
                                       const float *params, const float *stats, int max_workgroups, const IcnetFusionWs &ws,
                                       const IcnetHeadSemi &semi, uint8_t *tgt, hipStream_t s)
{
    if (N < 1 || K < 2 || K > 32 || max_workgroups < 0 || !icnet_fusion_fits(h16, w16) || !sub24_raw || !c3_raw)
        return hipErrorInvalidValue;
    if (semi.labelled) {  // (every image labelled: no pseudo target is read, the head launcher below only packs)
        const hipError_t e = fusion_forward(sub24_raw, c3_raw, N, h16, w16, params, stats, ws, s);
        if (e != hipSuccess) return e;
    }
    return launch_icnet_head_targets(ws.sub12, N, 2 * h16, 2 * w16, K, params + FU_HEAD, max_workgroups, ws.head, semi, tgt, s);
}

hipError_t launch_icnet_fusion_grad(const float *sub24, const float *c3, int N, int h16, int w16, int K, const float *params,
                                    const float *stats, const uint8_t *labels, const float *mask, float weight,
                                    float label_smoothing, int max_workgroups, const IcnetFusionWs &ws, double *loss,
                                    float *grad, hipStream_t s, const IcnetHeadSemi *semi)
{
    if (N < 1 || K < 2 || K > 32 || max_workgroups < 0 || !icnet_fusion_fits(h16, w16)) return hipErrorInvalidValue;
    const int h8 = 2 * h16, w8 = 2 * w16;
    const double pix = (double)N * h8 * w8;
    hipError_t e = fusion_forward(sub24, c3, N, h16, w16, params, stats, ws, s);
    if (e != hipSuccess) return e;
    // head, loss, dL/d(head) into the packed gradient's tail, the per-tile pull-back windows
    e = launch_icnet_head_grad(ws.sub12, N, h8, w8, K, params + FU_HEAD, labels, mask, weight, label_smoothing,
                               max_workgroups, ws.head, loss, grad + FU_HEAD, s, semi, ws.hw);
    if (e != hipSuccess) return e;
    {
        ProfScope prof("k_icnet_fusion_g", 2.0 * pix * 128 * K, 4.0 * pix * (256 + 2.25 * K), s);
        const long blocks = icnet_cdiv((long)N * h8 * w8, 64);
        if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_icnet_fusion_g, dim3((unsigned)blocks), dim3(256), 0, s, ws.hw, ws.sub12, params + FU_HEAD, N, h8,
                           w8, K, ws.g);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const int G = icnet_block_workgroups<128>(N, h16, w16, max_workgroups);
    {
        ProfScope prof("k_icnet_fusion_wgrad", 2.0 * pix * (9 * 128 + 64) * 128,
                       4.0 * (FU_TAPS * pix * 128 + pix * (32 + 64)) + 4.0 * G * FU_PART, s);
        hipLaunchKernelGGL(k_icnet_fusion_wgrad<128>, dim3(G, FU_TAPS), dim3(256), 0, s, sub24, c3, ws.g, N, h16, w16, ws.part);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    {
        ProfScope prof("k_icnet_fusion_finish", (double)G * FU_PART, 4.0 * (G + 2.0) * FU_PART, s);
        hipLaunchKernelGGL((k_icnet_block_finish<128, true>), dim3(icnet_cdiv(FU_PART, 256)), dim3(256), 0, s, ws.part, G,
                           ws.head.lpart, icnet_head_workgroups(h8, w8, max_workgroups), ws.fold + FU_PART, ws.rows, ws.fold,
                           grad);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    ProfScope prof("k_icnet_fusion_gamma", 2.0 * (FU_GA + 64 * 128), 8.0 * FU_PART, s);
    hipLaunchKernelGGL(k_icnet_block_gamma<128>, dim3(2), dim3(128), 0, s, ws.fold, ws.fold + FU_PART, params, stats, grad);
    return hipGetLastError();
}

hipError_t launch_icnet_fusion_wgrad256(const float *src, const float *side, const float *g, int N, int hs, int ws, int G,
                                        float *part, hipStream_t s)
{
    if (N < 1 || G < 1 || G > 0xffff || !icnet_fusion_fits(hs, ws)) return hipErrorInvalidValue;
    const double pix = 4.0 * N * hs * ws;
    ProfScope prof("k_icnet_fusion_wgrad<256>", 2.0 * pix * (10 * 256 + 1) * 128,
                   4.0 * (2.0 * CA_TAPS * pix * 128 + pix * (9 * 64 + 256)) + 4.0 * G * (CA_TAPS * 256 * 128), s);
    hipLaunchKernelGGL(k_icnet_fusion_wgrad<256>, dim3(G, CA_TAPS, 2), dim3(256), 0, s, src, side, g, N, hs, ws, part);
    return hipGetLastError();
}

}  // namespace ssal
