// ssal_train_icnet_pyramid.hip -- training of ICNet's pyramid head: conv5_4_k1 (1 x 1, 1024 -> 256, batch-norm, ReLU over the
// pyramid-pooling sum) with the whole cascade head, over everything below conv5_3_sum and the two other frozen branches, gfx950
// (DESIGN.md section 39).  Behind the forward path's own launch on the weights being trained (launch_igemm) and the cascade
// trainer's gradient (ssal_train_icnet_cascade.hip, which leaves g24 = dL/dsub24_sum behind its ReLU and the scale 1 / sum(mask)):
//   k_icnet_pyramid_pack     the packed vector -> conv5_4_k1 in launch_igemm's layout, its folded batch-norm row
//   k_icnet_cascade_dx<256>  (ssal_train_icnet_cascade.hip; the profile's k_icnet_pyramid_dx) the data gradient through conv_sub4
//   k_icnet_cascade_g24<256> (likewise; k_icnet_pyramid_g32) the adjoint of the legacy 2x resize and the ReLU mask of conv5_4_k1
//   k_icnet_pyramid_wgrad    the 1024 x 256 weight gradient on the fp32 matrix cores, split-K over pixel tiles and split over
//                            8 x 2 slabs of the output
//   k_icnet_pyramid_finish   fixed-order fold of the partials, the batch-norm scale, 1 / sum(mask); dBeta
//   k_icnet_pyramid_gamma    dGamma contracted from the folded weight gradient (section 28's re-association)
// The last two are the one-layer 1 x 1 forms of the fusion blocks' finish and gamma, written on ssal_train_icnet_common.h's
// device functions as ssal_train_icnet_highres.hip's 3 x 3 forms are.
// g32 is un-normalised and WITHOUT conv5_4_k1's batch-norm scale: the scale is applied once, by the finish kernel.
// No floating-point atomics, no inline assembly, 64-bit offsets, grids strided over the tiles: two runs give the same bits.
#include "ssal_icnet.h"
#include "ssal_internal.h"
#include "ssal_mfma.h"
#include "ssal_prof.h"
#include "ssal_train_icnet_pyramid.h"

namespace ssal {

bool icnet_pyramid_fits(int h32, int w32) { return icnet_cascade_fits(h32, w32); }

// P: conv5_4_k1.kernel [1024][256] | gamma | beta; stats: mean | variance.  rows: icnet_bn_row's s | t (256 each)
__global__ __launch_bounds__(256) void k_icnet_pyramid_pack(const float *__restrict__ P, const float *__restrict__ stats,
                                                            float *__restrict__ wt, float *__restrict__ rows)
{
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o < PY_G) {
        wt[igemm_wt_index(0, o >> 8, o & 255, PY_CIN / 32, PY_CO)] = P[PY_K + o];
    } else if (o < PY_G + PY_CO) {
        const int c = o - PY_G;
        icnet_bn_row(P[PY_G + c], P[PY_B + c], stats[c], stats[PY_CO + c], rows + c, rows + PY_CO + c);
    }
}

// part[b][ci][co] = sum over the pixel tiles of group b, sum_p x[p, ci] g[p, co]; part[b][1024][co] = sum_p g[p, co].
// grid (G, 8, 2): workgroup (b, y, z) owns the slab ci = 128 y .. + 127, co = 128 z .. + 127 of the output and takes the tiles b,
// b + G, ... of PY_PT = 32 pixels (linear over [N, h32, w32]); wave w keeps D[ci = 128 y + 32 w .. + 31][co] in four
// v_mfma_f32_32x32x2_f32 accumulators.  Per tile: x[tile][slab of ci] and g[tile][slab of co] -> LDS as [pixel][128 + pad]
// (zeros behind the last pixel; every global load is a float4 of a 512-byte row piece, each read by one workgroup column), then
// 16 steps of two pixels each: lane (r = lane & 31, h = lane >> 5) feeds x[pixel 2 s + h][32 w + r] and g[pixel 2 s + h][32 j + r].
// One accumulator so adds the products of its group's pixels in ascending order.  The y = 0 workgroups also add the rows of g
// (threads 0 .. 127, one co each, pixels ascending): dBeta's partial.
// CIN x CO: the layer (1024 x 256: conv5_4_k1, the kernel as it always was, grid (G, 8, 2); 256 x 1024: conv5_3's increase
// layer, DESIGN.md section 41, grid (G, 2, 8)); PART = (CIN + 1) CO floats per partial
constexpr int PW_LD = 160;  // 2 pixels = 320 floats: the lane halves (pixel 2 s, 2 s + 1) fall on the two bank halves
template <int CIN, int CO>
__global__ __launch_bounds__(256) void k_icnet_pyramid_wgrad(const float *__restrict__ x, const float *__restrict__ g,
                                                             long pixels, float *__restrict__ part)
{
    constexpr int PART = (CIN + 1) * CO;
    __shared__ __attribute__((aligned(16))) float As[PY_PT * PW_LD];
    __shared__ __attribute__((aligned(16))) float Bs[PY_PT * PW_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int ci0 = 128 * blockIdx.y, co0 = 128 * blockIdx.z;
    const bool ones = blockIdx.y == 0 && tid < 128;
    const long tiles = (pixels + PY_PT - 1) / PY_PT;
    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.0f;
    float gsum = 0.0f;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long p0 = t * PY_PT;
        __syncthreads();  // the previous tile's MFMAs are done with As / Bs
        for (int e = tid; e < PY_PT * 32; e += 256) {
            const int pl = e >> 5, q = e & 31;
            const long p = p0 + pl;
            float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
            if (p < pixels) {
                a = reinterpret_cast<const float4 *>(x + p * CIN + ci0)[q];
                b = reinterpret_cast<const float4 *>(g + p * CO + co0)[q];
            }
            *reinterpret_cast<float4 *>(As + pl * PW_LD + 4 * q) = a;
            *reinterpret_cast<float4 *>(Bs + pl * PW_LD + 4 * q) = b;
        }
        __syncthreads();
        const float *ap = As + hh * PW_LD + 32 * wave + r;
        const float *bp = Bs + hh * PW_LD + r;
#pragma unroll 4
        for (int s = 0; s < PY_PT / 2; ++s) {
            const float a = ap[2 * s * PW_LD];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = mfma32(a, bp[2 * s * PW_LD + 32 * j], acc[j]);
        }
        if (ones)
            for (int p = 0; p < PY_PT; ++p) gsum += Bs[p * PW_LD + tid];
    }
    float *pw = part + (long)blockIdx.x * PART;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * hh;
            pw[(ci0 + 32 * wave + row) * CO + co0 + 32 * j + r] = acc[j][i];
        }
    if (ones) pw[CIN * CO + co0 + tid] = gsum;
}

// The one-layer 1 x 1 form of k_icnet_block_finish (ssal_train_icnet_common.h): raw[o] = sum over split-K groups b = 0 .. G - 1
// of part[b][o], fp32, in that order -> fold[o] ([1024 + 1][256]); dK = (raw scale) s[co], dBeta = raw[1024][co] scale; scale:
// the one the fusion trainer's finish took from the head kernel's lpart
template <int CIN, int CO>
__global__ __launch_bounds__(256) void k_icnet_pyramid_finish(const float *__restrict__ part, int G,
                                                              const float *__restrict__ scale_p, const float *__restrict__ sl,
                                                              float *__restrict__ fold, float *__restrict__ gK,
                                                              float *__restrict__ gB)
{
    constexpr int PART = (CIN + 1) * CO;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= PART) return;
    const float scale = scale_p[0];
    float acc = 0.0f;
    for (int gi = 0; gi < G; ++gi) acc += part[(long)gi * PART + o];
    fold[o] = acc;
    const int co = o & (CO - 1);
    if (o < CIN * CO) gK[o] = (acc * scale) * sl[co];
    else gB[co] = acc * scale;
}

// The one-layer 1 x 1 form of k_icnet_block_gamma: its 1 x 1 branch (icnet_gamma_tap alone).  CO / 256 workgroups of 256 threads (co).
template <int CIN, int CO>
__global__ __launch_bounds__(256) void k_icnet_pyramid_gamma(const float *__restrict__ fold, const float *__restrict__ scale_p,
                                                             const float *__restrict__ K, const float *__restrict__ mean,
                                                             const float *__restrict__ var, float *__restrict__ gG)
{
    const int co = (CO > 256 ? (int)blockIdx.x * 256 : 0) + (int)threadIdx.x;
    gG[co] = icnet_dgamma(icnet_gamma_tap(K, fold, CIN, CO, co), mean[co], var[co], fold[CIN * CO + co], scale_p[0]);
}

hipError_t launch_icnet_pyramid_grad(const float *c53, const float *c31, const float *c3, int N, int h32, int w32, int K,
                                     const float *params, const float *stats, const uint8_t *labels, const float *mask,
                                     float weight, float label_smoothing, int max_workgroups, const IcnetPyramidWs &ws,
                                     double *loss, float *grad, hipStream_t s)
{
    if (N < 1 || K < 2 || K > 32 || max_workgroups < 0 || !icnet_pyramid_fits(h32, w32)) return hipErrorInvalidValue;
    const long pixels = (long)N * h32 * w32;
    const double pix32 = (double)pixels;
    hipError_t e;
    // ---- forward: the pack, then run_trunk's launch of conv5_4_k1 on the weights being trained ----
    {
        ProfScope prof("k_icnet_pyramid_pack", 0.0, 8.0 * (PY_G + PY_CO), s);
        hipLaunchKernelGGL(k_icnet_pyramid_pack, dim3(icnet_cdiv(PY_G + PY_CO, 256)), dim3(256), 0, s, params, stats, ws.wt,
                           ws.rows);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    e = launch_igemm(c53, N, h32, w32, PY_CIN, ws.wt, 1, 1, PY_CO, 1, 1, ws.rows, ws.rows + PY_CO, nullptr, true, false, ws.f1, s);
    if (e != hipSuccess) return e;
    // section 29 as it stands: both fusion blocks, the head, the loss, its fourteen gradients, g24 behind sub24_sum's ReLU
    e = launch_icnet_cascade_grad(ws.f1, c31, c3, N, h32, w32, K, params + PY_CASCADE, stats + PY_STATS_OWN, labels, mask, weight,
                                  label_smoothing, max_workgroups, ws.cascade, loss, grad + PY_CASCADE, s);
    if (e != hipSuccess) return e;
    const float *scale = ws.cascade.fusion.fold + FU_PART;  // 1 / sum(mask), as the fusion trainer's finish left it
    // ---- backward ----
    e = launch_icnet_cascade_dx256(ws.cascade.g24, params + PY_CASCADE + CA_KC, ws.cascade.rows, N, 2 * h32, 2 * w32,
                                   max_workgroups, ws.du, s);
    if (e != hipSuccess) return e;
    if ((e = launch_icnet_cascade_g32(ws.du, ws.f1, N, h32, w32, max_workgroups, ws.g32, s)) != hipSuccess) return e;
    const int G = icnet_grid(icnet_cdiv(pixels, PY_PT), PY_MAX_WG, max_workgroups);
    {
        ProfScope prof("k_icnet_pyramid_wgrad", 2.0 * pix32 * PY_PART, 4.0 * pix32 * (PY_CIN + PY_CO) + 4.0 * G * PY_PART, s);
        hipLaunchKernelGGL((k_icnet_pyramid_wgrad<PY_CIN, PY_CO>), dim3(G, PY_CIN / 128, PY_CO / 128), dim3(256), 0, s, c53, ws.g32,
                           pixels, ws.part);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    {
        ProfScope prof("k_icnet_pyramid_finish", (double)G * PY_PART, 4.0 * (G + 2.0) * PY_PART, s);
        hipLaunchKernelGGL((k_icnet_pyramid_finish<PY_CIN, PY_CO>), dim3(icnet_cdiv(PY_PART, 256)), dim3(256), 0, s, ws.part, G, scale,
                           ws.rows, ws.fold, grad + PY_K, grad + PY_B);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    ProfScope prof("k_icnet_pyramid_gamma", 2.0 * PY_G, 8.0 * PY_PART, s);
    hipLaunchKernelGGL((k_icnet_pyramid_gamma<PY_CIN, PY_CO>), dim3(PY_CO / 256), dim3(256), 0, s, ws.fold, scale, params + PY_K, stats,
                       stats + PY_CO, grad + PY_G);
    return hipGetLastError();
}

// The three kernels at 256 x 1024 (ssal_train_icnet_pyramid.h): the weight gradient of conv5_3's increase layer, its fold and
// finish, its dGamma
hipError_t launch_icnet_wgrad_256x1024(const float *x, const float *g, long pixels, int max_workgroups, const float *scale,
                                       const float *sl, const float *K, const float *mean, const float *var, float *part,
                                       float *fold, float *gK, float *gG, float *gB, hipStream_t s, const char *const *names)
{
    constexpr int CIN = 256, CO = 1024, PART = (CIN + 1) * CO;
    if (pixels < 1 || max_workgroups < 0) return hipErrorInvalidValue;
    hipError_t e;
    const int G = icnet_grid(icnet_cdiv(pixels, PY_PT), PY_MAX_WG, max_workgroups);
    {
        ProfScope prof(names ? names[0] : "k_icnet_pool_wgrad", 2.0 * (double)pixels * PART, 4.0 * (double)pixels * (CIN + CO) + 4.0 * G * PART, s);
        hipLaunchKernelGGL((k_icnet_pyramid_wgrad<CIN, CO>), dim3(G, CIN / 128, CO / 128), dim3(256), 0, s, x, g, pixels, part);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    {
        ProfScope prof(names ? names[1] : "k_icnet_pool_finish", (double)G * PART, 4.0 * (G + 2.0) * PART, s);
        hipLaunchKernelGGL((k_icnet_pyramid_finish<CIN, CO>), dim3(icnet_cdiv(PART, 256)), dim3(256), 0, s, part, G, scale, sl, fold,
                           gK, gB);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    ProfScope prof(names ? names[2] : "k_icnet_pool_gamma", 2.0 * CIN * CO, 8.0 * PART, s);
    hipLaunchKernelGGL((k_icnet_pyramid_gamma<CIN, CO>), dim3(CO / 256), dim3(256), 0, s, fold, scale, K, mean, var, gG);
    return hipGetLastError();
}

// The three kernels at 1024 x 256 for a second layer of that shape (ssal_train_icnet_pyramid.h): the weight gradient of conv5_3's
// reduce layer, its fold and finish, its dGamma
hipError_t launch_icnet_wgrad_1024x256(const float *x, const float *g, long pixels, int max_workgroups, const float *scale,
                                       const float *sl, const float *K, const float *mean, const float *var, float *part,
                                       float *fold, float *gK, float *gG, float *gB, hipStream_t s, const char *const *names)
{
    if (pixels < 1 || max_workgroups < 0) return hipErrorInvalidValue;
    hipError_t e;
    const int G = icnet_grid(icnet_cdiv(pixels, PY_PT), PY_MAX_WG, max_workgroups);
    {
        ProfScope prof(names ? names[0] : "k_icnet_bneck_wgrad_r", 2.0 * (double)pixels * PY_PART, 4.0 * (double)pixels * (PY_CIN + PY_CO) + 4.0 * G * PY_PART,
                       s);
        hipLaunchKernelGGL((k_icnet_pyramid_wgrad<PY_CIN, PY_CO>), dim3(G, PY_CIN / 128, PY_CO / 128), dim3(256), 0, s, x, g, pixels,
                           part);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    {
        ProfScope prof(names ? names[1] : "k_icnet_bneck_finish_r", (double)G * PY_PART, 4.0 * (G + 2.0) * PY_PART, s);
        hipLaunchKernelGGL((k_icnet_pyramid_finish<PY_CIN, PY_CO>), dim3(icnet_cdiv(PY_PART, 256)), dim3(256), 0, s, part, G, scale, sl,
                           fold, gK, gB);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    ProfScope prof(names ? names[2] : "k_icnet_bneck_gamma_r", 2.0 * PY_G, 8.0 * PY_PART, s);
    hipLaunchKernelGGL((k_icnet_pyramid_gamma<PY_CIN, PY_CO>), dim3(PY_CO / 256), dim3(256), 0, s, fold, scale, K, mean, var, gG);
    return hipGetLastError();
}

}  // namespace ssal
