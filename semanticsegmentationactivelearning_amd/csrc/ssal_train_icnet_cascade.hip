// ssal_train_icnet_cascade.hip -- training of ICNet's whole cascade head (both fusion blocks and conv6_cls) over frozen
// branches, gfx950.  Behind the forward path's own launches on the weights being trained and the
// fusion trainer's gradient (ssal_train_icnet_fusion.hip, which leaves g = dL/dsub12_sum behind its ReLU):
//   k_icnet_block_pack<256> (ssal_train_icnet_common.h; the profile's k_icnet_cascade_pack) the packed vector -> conv_sub4 /
//                           conv3_1_sub2_proj in launch_igemm's layout, folded batch-norm rows
//   k_icnet_cascade_dx      the data gradient through conv_sub2 as an implicit GEMM on the fp32 matrix cores:
//                           du[p, ci] = sum_tap sum_co K_a[tap, ci, co] (s_a[co] g[p - 2 (tap - 1), co])
//   k_icnet_cascade_g24     the adjoint of the legacy 2x resize in gather form and the ReLU mask: du -> dL/dsub24_sum
//   k_icnet_fusion_wgrad<256>  (ssal_train_icnet_fusion.hip) the weight gradients of the block, split-K
//   k_icnet_block_finish<256, false>  (common; k_icnet_cascade_finish) fixed-order fold of the partials, the batch-norm scale,
//                           the 1 / sum(mask) the fusion trainer's finish left behind
//   k_icnet_block_gamma<256>  (common; k_icnet_cascade_gamma) dGamma contracted from the folded weight gradient
// No floating-point atomics, no inline assembly, 64-bit offsets: two runs give the same bits.
#include "ssal_icnet.h"
#include "ssal_internal.h"
#include "ssal_mfma.h"
#include "ssal_prof.h"
#include "ssal_train_icnet_cascade.h"

namespace ssal {

constexpr int DX_WH = CA_DX_TH + 4, DX_WW = CA_DX_TW + 4;  // a tile's window of g: two pixels of halo on every side
constexpr int DX_CO = 32;      // output channels of conv_sub2 (the GEMM's K) staged at a time
constexpr int DX_LDA = 36;     // LDS row stride of the window [pixel][32 co + pad]
constexpr int DX_LDB = 160;    // and of the weights [co][128 ci + pad] (FU_LD's reasoning)

bool icnet_cascade_fits(int h32, int w32)
{
    if (h32 < 1 || w32 < 1 || h32 > (1 << 25) || w32 > (1 << 25)) return false;  // 2 h32 <= 2^26: icnet_fusion_fits' limit
    return icnet_fusion_fits(2 * h32, 2 * w32);  // every grid here is strided over 64-bit tile counts: no limit of its own
}

// du[p, ci] = sum_co sum_tap K[tap, ci, co] gs[p - 2 (kh - 1, kw - 1), co], gs = s[co] g, zero outside the map: the transposed
// dilated 3 x 3 convolution through conv_sub2 as a GEMM of pixels x (9 * 128) x 128.  A workgroup takes the tiles b, b + G, ...
// (8 x 16 pixels, image after image); wave w owns the input channels ci = 32 w .. 32 w + 31 of all 128 pixels: four
// v_mfma_f32_32x32x2_f32 accumulators D[pixel][ci].  Per tile, for each quarter of the output channels (co ascending):
//   the 12 x 20 window of gs behind the tile -> LDS (the product s g is rounded once, here);
//   for each tap (ascending): K[tap, :, quarter] -> LDS as [co][ci]; 16 steps of two co each: lane (r = lane & 31,
//   h = lane >> 5) feeds gs[pixel 32 j + r shifted by the tap][2 s + h] and K[2 s + h][32 w + r].
// One accumulator therefore adds its 1152 products in the order (quarter, tap, co): the chain of section 29's bound.
// CIN: the input channels of the convolution (K [9][CIN][128], du [.., CIN]).  128: conv_sub2, the kernel as it always was;
// 256: conv_sub4 at 1/16 resolution -- blockIdx.y picks the half of 128 input channels a workgroup owns.
template <int CIN>
__global__ __launch_bounds__(256) void k_icnet_cascade_dx(const float *__restrict__ g, const float *__restrict__ Ka,
                                                          const float *__restrict__ sa, int N, int h8, int w8,
                                                          float *__restrict__ du)
{
    static_assert(CIN == 128 || CIN == 256, "the two fusion blocks of ICNet");
    const int cb = CIN == 128 ? 0 : 128 * (int)blockIdx.y;  // first input channel of this workgroup
    __shared__ __attribute__((aligned(16))) float win[DX_WH * DX_WW * DX_LDA];
    __shared__ __attribute__((aligned(16))) float Wb[DX_CO * DX_LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int tx = (w8 + CA_DX_TW - 1) / CA_DX_TW, ty = (h8 + CA_DX_TH - 1) / CA_DX_TH;
    const long per_image = (long)tx * ty, tiles = (long)N * per_image;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long n = t / per_image;
        const int rem = (int)(t % per_image);
        const int y0 = (rem / tx) * CA_DX_TH, x0 = (rem % tx) * CA_DX_TW;
        f32x16 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][i] = 0.0f;
        for (int cc = 0; cc < 128 / DX_CO; ++cc) {
            __syncthreads();  // the previous quarter's (tile's) MFMAs are done with win / Wb
            for (int e = tid; e < DX_WH * DX_WW * (DX_CO / 4); e += 256) {
                const int wp = e >> 3, q = e & 7;
                const int y = y0 - 2 + wp / DX_WW, xx = x0 - 2 + wp % DX_WW;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (y >= 0 && y < h8 && xx >= 0 && xx < w8) {
                    const float4 gv = reinterpret_cast<const float4 *>(g + ((n * h8 + y) * w8 + xx) * 128 + DX_CO * cc)[q];
                    const float4 sv = reinterpret_cast<const float4 *>(sa + DX_CO * cc)[q];
                    v = make_float4(sv.x * gv.x, sv.y * gv.y, sv.z * gv.z, sv.w * gv.w);
                }
                *reinterpret_cast<float4 *>(win + wp * DX_LDA + 4 * q) = v;
            }
            for (int tap = 0; tap < 9; ++tap) {
                if (tap) __syncthreads();  // the previous tap's MFMAs are done with Wb
                for (int e = tid; e < 128 * (DX_CO / 4); e += 256) {
                    const int ci = e >> 3, q = e & 7;
                    const float4 v = reinterpret_cast<const float4 *>(Ka + (tap * CIN + cb + ci) * 128 + DX_CO * cc)[q];
                    Wb[(4 * q + 0) * DX_LDB + ci] = v.x;
                    Wb[(4 * q + 1) * DX_LDB + ci] = v.y;
                    Wb[(4 * q + 2) * DX_LDB + ci] = v.z;
                    Wb[(4 * q + 3) * DX_LDB + ci] = v.w;
                }
                __syncthreads();
                // window pixel of gs[p - 2 (kh - 1, kw - 1)] for tile pixel p: p + 2 (the halo) - 2 (k - 1)
                const int oy = 4 - 2 * (tap / 3), ox = 4 - 2 * (tap % 3);
                const float *ap = win + ((oy + (r >> 4)) * DX_WW + ox + (r & 15)) * DX_LDA + hh;
                const float *bp = Wb + hh * DX_LDB + 32 * wave + r;
#pragma unroll 4
                for (int s = 0; s < DX_CO / 2; ++s) {
                    const float b = bp[2 * s * DX_LDB];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = mfma32(ap[2 * j * DX_WW * DX_LDA + 2 * s], b, acc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int p = 32 * j + (i & 3) + 8 * (i >> 2) + 4 * hh;
                const int y = y0 + (p >> 4), xx = x0 + (p & 15);
                if (y < h8 && xx < w8) du[((n * h8 + y) * w8 + xx) * CIN + cb + 32 * wave + r] = acc[j][i];
            }
    }
}

// g24[q, ci] = sub24_sum[q, ci] > 0 ? sum_{p'} w(p', q) du[p', ci] : 0: the adjoint of launch_resize_bilinear's exact 2x (even
// rows / columns copy, odd ones average with the +1 tap clamped to the map, so the last row / column collects its clamped tap
// twice: weight 1/2 + 1/2).  Every pixel of sub24_sum gathers its at most 3 x 3 pixels of du, rows then columns ascending,
// fmaf; the weights are powers of two.  One float4 of channels per thread.  C: the channels of du and of the map below
// (128: sub24_sum, the kernel as it always was; 256: conv5_4_k1).
template <int C>
__global__ __launch_bounds__(256) void k_icnet_cascade_g24(const float *__restrict__ du, const float *__restrict__ s24, int N,
                                                           int h16, int w16, float *__restrict__ g24)
{
    const int h8 = 2 * h16, w8 = 2 * w16;
    constexpr int Q = C / 4, QS = C == 128 ? 5 : 6;
    const long total = (long)N * h16 * w16 * Q;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int q = (int)(e & (Q - 1));
        const long p = e >> QS;
        const int c = (int)(p % w16), r = (int)((p / w16) % h16);
        const long n = p / ((long)w16 * h16);
        float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int dy = -1; dy <= 1; ++dy) {
            const int y = 2 * r + dy;
            if (y < 0) continue;
            const float wy = dy == 0 || (dy == 1 && r == h16 - 1) ? 1.0f : 0.5f;
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = 2 * c + dx;
                if (xx < 0) continue;
                const float w = wy * (dx == 0 || (dx == 1 && c == w16 - 1) ? 1.0f : 0.5f);
                const float4 v = reinterpret_cast<const float4 *>(du + ((n * h8 + y) * w8 + xx) * C)[q];
                o.x = fmaf(w, v.x, o.x);
                o.y = fmaf(w, v.y, o.y);
                o.z = fmaf(w, v.z, o.z);
                o.w = fmaf(w, v.w, o.w);
            }
        }
        const float4 xv = reinterpret_cast<const float4 *>(s24 + p * C)[q];
        reinterpret_cast<float4 *>(g24 + p * C)[q] =
            make_float4(xv.x > 0.0f ? o.x : 0.0f, xv.y > 0.0f ? o.y : 0.0f, xv.z > 0.0f ? o.z : 0.0f, xv.w > 0.0f ? o.w : 0.0f);
    }
}

// The two kernels at 256 channels (ssal_train_icnet_cascade.h): conv_sub4's data gradient and the resize adjoint below it
hipError_t launch_icnet_cascade_dx256(const float *g24, const float *Kc, const float *sc, int N, int h16, int w16,
                                      int max_workgroups, float *du, hipStream_t s)
{
    if (N < 1 || max_workgroups < 0 || h16 < 2 || w16 < 2 || !icnet_cascade_fits(h16 / 2, w16 / 2)) return hipErrorInvalidValue;
    const double pix16 = (double)N * h16 * w16;
    const long tiles = (long)N * icnet_cdiv(h16, CA_DX_TH) * icnet_cdiv(w16, CA_DX_TW);
    ProfScope prof("k_icnet_pyramid_dx", 2.0 * pix16 * 9 * 128 * 256, 4.0 * pix16 * (2 * 128 + 256) + 4.0 * (double)tiles * 9 * 256 * 128,
                   s);
    hipLaunchKernelGGL(k_icnet_cascade_dx<256>, dim3(icnet_grid(tiles, CA_DX_MAX_WG, max_workgroups), 2), dim3(256), 0, s, g24, Kc,
                       sc, N, h16, w16, du);
    return hipGetLastError();
}

hipError_t launch_icnet_cascade_g32(const float *du, const float *f1, int N, int h32, int w32, int max_workgroups, float *g32,
                                    hipStream_t s)
{
    if (N < 1 || max_workgroups < 0 || !icnet_cascade_fits(h32, w32)) return hipErrorInvalidValue;
    const double pix32 = (double)N * h32 * w32;
    const int B = icnet_grid(icnet_cdiv((long)N * h32 * w32 * 64, 256), 65536, max_workgroups);
    ProfScope prof("k_icnet_pyramid_g32", 18.0 * pix32 * 256, 4.0 * (4.0 * pix32 + 2.0 * pix32) * 256, s);
    hipLaunchKernelGGL(k_icnet_cascade_g24<256>, dim3(B), dim3(256), 0, s, du, f1, N, h32, w32, g32);
    return hipGetLastError();
}

// the pack, then the forward path's own launches (ssal_icnet_api.hip, run_trunk) on the weights being trained:
// ws.proj = BN(conv3_1_sub2_proj(c31)), ws.sub24 = sub24_sum
static hipError_t cascade_forward(const float *c54, const float *c31, int N, int h32, int w32, const float *params,
                                  const float *stats, const IcnetCascadeWs &ws, hipStream_t s)
{
    const int h16 = 2 * h32, w16 = 2 * w32;
    hipError_t e;
    {
        ProfScope prof("k_icnet_cascade_pack", 0.0, 8.0 * CA_FUSION, s);
        hipLaunchKernelGGL(k_icnet_block_pack<256>, dim3(icnet_cdiv(CA_GC + 256 * 128 + 256, 256)), dim3(256), 0, s, params,
                           stats, ws.wt_c, ws.wt_d, ws.rows);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    e = launch_igemm(c31, N, h16, w16, 256, ws.wt_d, 1, 1, 128, 1, 1, ws.rows + 256, ws.rows + 384, nullptr, false, false,
                     ws.proj, s);
    if (e != hipSuccess) return e;
    return launch_igemm(c54, N, h32, w32, 256, ws.wt_c, 3, 3, 128, 1, 2, ws.rows, ws.rows + 128, ws.proj, true, true, ws.sub24,
                        s);
}

hipError_t launch_icnet_cascade_targets(const float *c54_raw, const float *c31_raw, const float *c3_raw, int N, int h32,
                                        int w32, int K, const float *params, const float *stats, int max_workgroups,
                                        const IcnetCascadeWs &ws, const IcnetHeadSemi &semi, uint8_t *tgt, hipStream_t s)
{
    if (N < 1 || K < 2 || K > 32 || max_workgroups < 0 || !icnet_cascade_fits(h32, w32) || !c54_raw || !c31_raw)
        return hipErrorInvalidValue;
    if (semi.labelled) {  // (every image labelled: no pseudo target is read)
        const hipError_t e = cascade_forward(c54_raw, c31_raw, N, h32, w32, params, stats, ws, s);
        if (e != hipSuccess) return e;
    }
    return launch_icnet_fusion_targets(ws.sub24, c3_raw, N, 2 * h32, 2 * w32, K, params + CA_FUSION, stats + 4 * 128,
                                       max_workgroups, ws.fusion, semi, tgt, s);
}

hipError_t launch_icnet_cascade_grad(const float *c54, const float *c31, const float *c3, int N, int h32, int w32, int K,
                                     const float *params, const float *stats, const uint8_t *labels, const float *mask,
                                     float weight, float label_smoothing, int max_workgroups, const IcnetCascadeWs &ws,
                                     double *loss, float *grad, hipStream_t s, const IcnetHeadSemi *semi)
{
    if (N < 1 || K < 2 || K > 32 || max_workgroups < 0 || !icnet_cascade_fits(h32, w32)) return hipErrorInvalidValue;
    const int h16 = 2 * h32, w16 = 2 * w32, h8 = 2 * h16, w8 = 2 * w16;
    const double pix8 = (double)N * h8 * w8, pix16 = (double)N * h16 * w16;
    hipError_t e = cascade_forward(c54, c31, N, h32, w32, params, stats, ws, s);
    if (e != hipSuccess) return e;
    // section 28 as it stands: sub12_sum, the head, the loss, its eight gradients, and g behind sub12_sum's ReLU
    e = launch_icnet_fusion_grad(ws.sub24, c3, N, h16, w16, K, params + CA_FUSION, stats + 4 * 128, labels, mask, weight,
                                 label_smoothing, max_workgroups, ws.fusion, loss, grad + CA_FUSION, s, semi);
    if (e != hipSuccess) return e;
    {
        const long tiles = (long)N * icnet_cdiv(h8, CA_DX_TH) * icnet_cdiv(w8, CA_DX_TW);
        ProfScope prof("k_icnet_cascade_dx", 2.0 * pix8 * 9 * 128 * 128, 8.0 * pix8 * 128 + 4.0 * (double)tiles * 9 * 128 * 128,
                       s);
        hipLaunchKernelGGL(k_icnet_cascade_dx<128>, dim3(icnet_grid(tiles, CA_DX_MAX_WG, max_workgroups)), dim3(256), 0, s,
                           ws.fusion.g, params + CA_FUSION + FU_KA, ws.fusion.rows, N, h8, w8, ws.du);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    {
        const int B = icnet_grid(icnet_cdiv((long)N * h16 * w16 * 32, 256), 65536, max_workgroups);
        ProfScope prof("k_icnet_cascade_g24", 18.0 * pix16 * 128, 4.0 * (pix8 + 2.0 * pix16) * 128, s);
        hipLaunchKernelGGL(k_icnet_cascade_g24<128>, dim3(B), dim3(256), 0, s, ws.du, ws.sub24, N, h16, w16, ws.g24);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const int G = icnet_block_workgroups<256>(N, h32, w32, max_workgroups);
    if ((e = launch_icnet_fusion_wgrad256(c54, c31, ws.g24, N, h32, w32, G, ws.part, s)) != hipSuccess) return e;
    float *scale = ws.fusion.fold + FU_PART;  // 1 / sum(mask), as the fusion trainer's finish left it
    {
        ProfScope prof("k_icnet_cascade_finish", (double)G * CA_PART, 4.0 * (G + 2.0) * CA_PART, s);
        hipLaunchKernelGGL((k_icnet_block_finish<256, false>), dim3(icnet_cdiv(CA_PART, 256)), dim3(256), 0, s, ws.part, G,
                           nullptr, 0, scale, ws.rows, ws.fold, grad);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    ProfScope prof("k_icnet_cascade_gamma", 2.0 * (CA_GC + 256 * 128), 8.0 * CA_PART, s);
    hipLaunchKernelGGL(k_icnet_block_gamma<256>, dim3(2), dim3(128), 0, s, ws.fold, scale, params, stats, grad);
    return hipGetLastError();
}

}  // namespace ssal
