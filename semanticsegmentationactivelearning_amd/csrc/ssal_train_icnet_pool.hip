// ssal_train_icnet_pool.hip -- training of ICNet through its pyramid pooling: conv5_3's increase layer (1 x 1, 256 -> 1024,
// batch-norm, + conv5_2, ReLU), the parameter-free pyramid pooling over it and the whole pyramid head, over everything below
// conv5_3_3x3 and conv5_2 and the two other frozen branches, gfx950.  Behind the forward path's own
// launches on the weights being trained (launch_igemm, launch_ppm) and the pyramid trainer's gradient
// (ssal_train_icnet_pyramid.hip, which leaves g32 = dL/dconv5_4_k1 behind its ReLU, conv5_4_k1's batch-norm row and the scale
// 1 / sum(mask)):
//   k_icnet_pool_pack       the packed vector -> the increase kernel in launch_igemm's layout, its folded batch-norm row
//   k_icnet_pool_dx         the data gradient through conv5_4_k1 on the fp32 matrix cores: dsum = (s1 g32) K1^T
//   k_icnet_ppm_adj_rows    the column half of the four resize adjoints, row by row (the adjoint of k_ppm_sum's PpmLevel::init)
//   k_icnet_ppm_adj_bins    the row half: the 50 bin gradients, each divided by its bin's pixel count
//   k_icnet_ppm_adj_sum     g53 = relu'(conv5_3) (dsum + the bin gradients of every bin that holds the pixel)
//   k_icnet_pyramid_wgrad<256, 1024>, its finish and gamma (ssal_train_icnet_pyramid.hip; the profile's k_icnet_pool_wgrad, ...)
// dsum, the bin gradients and g53 are un-normalised and WITHOUT the increase layer's batch-norm scale: the finish kernel applies
// both once.  No floating-point atomics, no inline assembly, 64-bit offsets, grids strided over the tiles: two runs give the same
// bits.
#include "ssal_icnet.h"
#include "ssal_internal.h"
#include "ssal_mfma.h"
#include "ssal_prof.h"
#include "ssal_train_icnet_pool.h"

namespace ssal {

bool icnet_pool_fits(int h32, int w32) { return icnet_pyramid_fits(h32, w32); }

// the pyramid's four levels as k_ppm_pool numbers them: bins per side, first slot of the 50, first column slot of the 12
__device__ __host__ constexpr int po_bins(int k) { return k == 0 ? 1 : k == 1 ? 2 : k == 2 ? 3 : 6; }
__device__ __host__ constexpr int po_base(int k) { return k == 0 ? 0 : k == 1 ? 1 : k == 2 ? 5 : 14; }
__device__ __host__ constexpr int po_cbase(int k) { return k == 0 ? 0 : k == 1 ? 1 : k == 2 ? 3 : 6; }
static_assert(po_base(3) + 36 == PO_SLOTS && po_cbase(3) + 6 == PO_CSLOTS, "1 + 4 + 9 + 36 bins, 1 + 2 + 3 + 6 columns");

// what pixel o of a side of S pixels reads from bin t of a level with B bins per side under the legacy mapping, as
// PpmLevel::init / add form it (src = o * (B / S) in fp32, t0 = floor, t1 = min(t0 + 1, B - 1), l = src - t0;
// value = v[t0] + (v[t1] - v[t0]) l): 1 - l from t0 and l from t1; where the two coincide the forward value is v[t0] itself.
// -> false where the pixel does not read the bin
__device__ __forceinline__ bool po_weight(int o, int S, int B, int t, float *wgt)
{
    const float src = (float)o * ((float)B / (float)S);
    const int t0 = (int)floorf(src);
    const int t1 = min(t0 + 1, B - 1);
    const float l = src - (float)t0;
    if (t0 == t1) {
        *wgt = 1.0f;
        return t == t0;
    }
    *wgt = t == t0 ? 1.0f - l : l;
    return t == t0 || t == t1;
}

// P: the increase kernel [256][1024] | gamma | beta; stats: mean | variance.  rows: icnet_bn_row's s | t (1024 each)
__global__ __launch_bounds__(256) void k_icnet_pool_pack(const float *__restrict__ P, const float *__restrict__ stats,
                                                         float *__restrict__ wt, float *__restrict__ rows)
{
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o < PO_G) {
        wt[igemm_wt_index(0, o >> 10, o & 1023, PO_CIN / 32, PO_CO)] = P[PO_K + o];
    } else if (o < PO_G + PO_CO) {
        const int c = o - PO_G;
        icnet_bn_row(P[PO_G + c], P[PO_B + c], stats[c], stats[PO_CO + c], rows + c, rows + PO_CO + c);
    }
}

// dsum[p, ci] = sum_co (s1[co] g32[p, co]) K1[ci, co]: the data gradient of conv5_4_k1 (1 x 1, 1024 -> 256).  g32 [pixels, 256]
// un-normalised behind conv5_4_k1's ReLU, K1 [1024][256], s1 [256] its batch-norm scale -> dsum [pixels, 1024].
// grid (G, 8): workgroup (b, y) owns the input channels ci = 128 y .. + 127 and takes the tiles b, b + G, ... of PO_DX_PT = 64
// pixels (linear over [N, h32, w32]); wave w keeps D[pixel 32 j .. + 31][ci = 128 y + 32 w .. + 31], j = 0, 1, in two
// v_mfma_f32_32x32x2_f32 accumulators.  Per tile, for each of the 8 chunks of 32 output channels (ascending): s1 g32 of the chunk
// (the product rounded once, here; zeros behind the last pixel) -> LDS as [co][pixel], K1's chunk -> LDS as [co][ci] (every global
// load a float4 of a 128-byte row piece), then 16 steps of two co each: lane (r = lane & 31, h = lane >> 5) feeds
// gs[pixel 32 j + r][2 s + h] and K1[32 w + r][2 s + h].  One accumulator therefore adds its 256 products in ascending co, two
// per instruction.
// LDS banking (32 banks and groups of 32 lanes for 4-byte accesses): an MFMA operand read is 32 consecutive floats per lane
// group, free of conflicts at any leading dimension; a staging store's lane group holds 8 quads q x 4 rows, at (4 q + i) LD + row,
// so an odd LD (4 LD = 4 mod 32) puts its 32 lanes on 32 banks.
constexpr int PD_CC = 32;    // output channels of conv5_4_k1 per chunk
constexpr int PD_LDG = 65;   // 64 pixels + 1
constexpr int PD_LDK = 129;  // 128 ci + 1
__global__ __launch_bounds__(256) void k_icnet_pool_dx(const float *__restrict__ g32, const float *__restrict__ K1,
                                                       const float *__restrict__ s1, long pixels, float *__restrict__ dsum)
{
    __shared__ float Gs[PD_CC * PD_LDG];
    __shared__ float Ks[PD_CC * PD_LDK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int ci0 = 128 * blockIdx.y;
    const long tiles = (pixels + PO_DX_PT - 1) / PO_DX_PT;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long p0 = t * PO_DX_PT;
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][i] = 0.0f;
        for (int cc = 0; cc < PY_CO / PD_CC; ++cc) {
            __syncthreads();  // the previous chunk's MFMAs are done with Gs / Ks
            for (int e = tid; e < PO_DX_PT * (PD_CC / 4); e += 256) {
                const int pl = e >> 3, q = e & 7;
                const long p = p0 + pl;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (p < pixels) {
                    const float4 gv = reinterpret_cast<const float4 *>(g32 + p * PY_CO + PD_CC * cc)[q];
                    const float4 sv = reinterpret_cast<const float4 *>(s1 + PD_CC * cc)[q];
                    v = make_float4(sv.x * gv.x, sv.y * gv.y, sv.z * gv.z, sv.w * gv.w);
                }
                Gs[(4 * q + 0) * PD_LDG + pl] = v.x;
                Gs[(4 * q + 1) * PD_LDG + pl] = v.y;
                Gs[(4 * q + 2) * PD_LDG + pl] = v.z;
                Gs[(4 * q + 3) * PD_LDG + pl] = v.w;
            }
            for (int e = tid; e < 128 * (PD_CC / 4); e += 256) {
                const int ci = e >> 3, q = e & 7;
                const float4 v = reinterpret_cast<const float4 *>(K1 + (long)(ci0 + ci) * PY_CO + PD_CC * cc)[q];
                Ks[(4 * q + 0) * PD_LDK + ci] = v.x;
                Ks[(4 * q + 1) * PD_LDK + ci] = v.y;
                Ks[(4 * q + 2) * PD_LDK + ci] = v.z;
                Ks[(4 * q + 3) * PD_LDK + ci] = v.w;
            }
            __syncthreads();
            const float *ap = Gs + hh * PD_LDG + r;
            const float *bp = Ks + hh * PD_LDK + 32 * wave + r;
#pragma unroll 4
            for (int s = 0; s < PD_CC / 2; ++s) {
                const float b = bp[2 * s * PD_LDK];
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = mfma32(ap[2 * s * PD_LDG + 32 * j], b, acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const long p = p0 + 32 * j + (i & 3) + 8 * (i >> 2) + 4 * hh;
                if (p < pixels) dsum[p * PY_CIN + ci0 + 32 * wave + r] = acc[j][i];
            }
    }
}

// stage 1 of the resize adjoints, shaped as k_ppm_rowsum: cols[n][y][cs][c] = sum_x w(x; column j of level k) dsum[n, y, x, c],
// columns ascending, fmaf, for the 12 column slots cs = po_cbase(k) + j.  One thread per (n, row, channel quad).
__global__ __launch_bounds__(256) void k_icnet_ppm_adj_rows(const float4 *__restrict__ dsum, int N, int H, int W, int C4,
                                                            float4 *__restrict__ cols)
{
    const long total = (long)N * H * C4;
    for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long)gridDim.x * 256) {
        const int c = (int)(o % C4);
        const long ny = o / C4;
        float4 s[PO_CSLOTS];
#pragma unroll
        for (int cs = 0; cs < PO_CSLOTS; ++cs) s[cs] = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 *row = dsum + ny * W * C4 + c;
        for (int x = 0; x < W; ++x) {
            const float4 v = row[(long)x * C4];
#pragma unroll
            for (int cs = 0; cs < PO_CSLOTS; ++cs) {
                const int k = cs >= 6 ? 3 : cs >= 3 ? 2 : cs >= 1 ? 1 : 0;
                float wgt;
                const bool in = po_weight(x, W, po_bins(k), cs - po_cbase(k), &wgt);
                s[cs].x = in ? fmaf(wgt, v.x, s[cs].x) : s[cs].x;
                s[cs].y = in ? fmaf(wgt, v.y, s[cs].y) : s[cs].y;
                s[cs].z = in ? fmaf(wgt, v.z, s[cs].z) : s[cs].z;
                s[cs].w = in ? fmaf(wgt, v.w, s[cs].w) : s[cs].w;
            }
        }
#pragma unroll
        for (int cs = 0; cs < PO_CSLOTS; ++cs) cols[(ny * PO_CSLOTS + cs) * C4 + c] = s[cs];
    }
}

// stage 2, shaped as k_ppm_pool: gb[n][slot][c] = (sum_y w(y; row i of level k) cols[n][y][po_cbase(k) + j][c]) / count, rows
// ascending, fmaf; count: the pixels of bin (i, j), [floor(i H / b), ceil((i + 1) H / b)) x the same of W, as k_ppm_pool counts
// them.  A bin no pixel reads keeps its zero.  One thread per (n, slot, channel quad).
__global__ __launch_bounds__(256) void k_icnet_ppm_adj_bins(const float4 *__restrict__ cols, int N, int H, int W, int C4,
                                                            float4 *__restrict__ gb)
{
    const long total = (long)N * PO_SLOTS * C4;
    for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long)gridDim.x * 256) {
        const int c = (int)(o % C4);
        const int slot = (int)((o / C4) % PO_SLOTS);
        const long n = o / ((long)C4 * PO_SLOTS);
        const int k = slot >= 14 ? 3 : slot >= 5 ? 2 : slot >= 1 ? 1 : 0;
        const int b = po_bins(k), idx = slot - po_base(k);
        const int i = idx / b, j = idx % b;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int y = 0; y < H; ++y) {
            float wgt;
            if (!po_weight(y, H, b, i, &wgt)) continue;
            const float4 v = cols[((n * H + y) * PO_CSLOTS + po_cbase(k) + j) * C4 + c];
            s.x = fmaf(wgt, v.x, s.x);
            s.y = fmaf(wgt, v.y, s.y);
            s.z = fmaf(wgt, v.z, s.z);
            s.w = fmaf(wgt, v.w, s.w);
        }
        const int y0 = (i * H) / b, y1 = ((i + 1) * H + b - 1) / b;
        const int x0 = (j * W) / b, x1 = ((j + 1) * W + b - 1) / b;
        const float cnt = (float)((y1 - y0) * (x1 - x0));
        gb[o] = make_float4(s.x / cnt, s.y / cnt, s.z / cnt, s.w / cnt);
    }
}

// g53[n, y, x, c] = conv5_3 > 0 ? dsum + sum over the levels (1, 2, 3, 6), the bin rows i that hold y and the bin columns j that
// hold x (each ascending) of gb[n][level, i, j][c] : 0 -- the identity term first, then every bin the pixel was averaged into:
// at most 2 x 2 per level where b <= H, W (the bins overlap where b does not divide the side), all the coinciding ones where
// b is larger.  One thread per (pixel, channel quad).
__global__ __launch_bounds__(256) void k_icnet_ppm_adj_sum(const float4 *__restrict__ dsum, const float4 *__restrict__ gb,
                                                           const float4 *__restrict__ c53, int N, int H, int W, int C4,
                                                           float4 *__restrict__ g53)
{
    const long total = (long)N * H * W * C4;
    for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long)gridDim.x * 256) {
        const int c = (int)(o % C4);
        const long p = o / C4;
        const int x = (int)(p % W), y = (int)((p / W) % H);
        const long n = p / ((long)W * H);
        float4 d = dsum[o];
        const float4 *gn = gb + n * PO_SLOTS * C4 + c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int b = po_bins(k);
#pragma unroll
            for (int i = 0; i < b; ++i) {
                if (y < (i * H) / b || y >= ((i + 1) * H + b - 1) / b) continue;
#pragma unroll
                for (int j = 0; j < b; ++j) {
                    if (x < (j * W) / b || x >= ((j + 1) * W + b - 1) / b) continue;
                    const float4 v = gn[(long)(po_base(k) + i * b + j) * C4];
                    d.x += v.x;
                    d.y += v.y;
                    d.z += v.z;
                    d.w += v.w;
                }
            }
        }
        const float4 f = c53[o];
        g53[o] = make_float4(f.x > 0.0f ? d.x : 0.0f, f.y > 0.0f ? d.y : 0.0f, f.z > 0.0f ? d.z : 0.0f, f.w > 0.0f ? d.w : 0.0f);
    }
}

hipError_t launch_icnet_pool_grad(const float *a33, const float *c52, const float *c31, const float *c3, int N, int h32, int w32,
                                  int K, const float *params, const float *stats, const uint8_t *labels, const float *mask,
                                  float weight, float label_smoothing, int max_workgroups, const IcnetPoolWs &ws, double *loss,
                                  float *grad, hipStream_t s)
{
    if (N < 1 || K < 2 || K > 32 || max_workgroups < 0 || !icnet_pool_fits(h32, w32)) return hipErrorInvalidValue;
    const long pixels = (long)N * h32 * w32;
    const double pix32 = (double)pixels;
    constexpr int C4 = PO_CO / 4;
    hipError_t e;
    // ---- forward: the pack, then run_trunk's launches of the increase layer and the pyramid pooling on the weights being trained ----
    {
        ProfScope prof("k_icnet_pool_pack", 0.0, 8.0 * (PO_G + PO_CO), s);
        hipLaunchKernelGGL(k_icnet_pool_pack, dim3(icnet_cdiv(PO_G + PO_CO, 256)), dim3(256), 0, s, params, stats, ws.wt, ws.rows);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    e = launch_igemm(a33, N, h32, w32, PO_CIN, ws.wt, 1, 1, PO_CO, 1, 1, ws.rows, ws.rows + PO_CO, c52, true, false, ws.c53, s);
    if (e != hipSuccess) return e;
    if ((e = launch_ppm(ws.c53, N, h32, w32, PO_CO, ws.pooled, ws.sum, s)) != hipSuccess) return e;
    // section 39 as it stands: conv5_4_k1, both fusion blocks, the head, the loss, its seventeen gradients, g32 behind conv5_4_k1's
    // ReLU
    e = launch_icnet_pyramid_grad(ws.sum, c31, c3, N, h32, w32, K, params + PO_PYRAMID, stats + PO_STATS_OWN, labels, mask, weight,
                                  label_smoothing, max_workgroups, ws.pyramid, loss, grad + PO_PYRAMID, s);
    if (e != hipSuccess) return e;
    const float *scale = ws.pyramid.cascade.fusion.fold + FU_PART;  // 1 / sum(mask), as the fusion trainer's finish left it
    // ---- backward ----
    {
        const int G = icnet_grid(icnet_cdiv(pixels, PO_DX_PT), PO_DX_MAX_WG, max_workgroups);
        ProfScope prof("k_icnet_pool_dx", 2.0 * pix32 * PY_CIN * PY_CO,
                       4.0 * pix32 * (8.0 * PY_CO + PY_CIN) + 4.0 * (double)icnet_cdiv(pixels, PO_DX_PT) * PY_CIN * PY_CO, s);
        hipLaunchKernelGGL(k_icnet_pool_dx, dim3(G, PY_CIN / 128), dim3(256), 0, s, ws.pyramid.g32, params + PO_PYRAMID + PY_K,
                           ws.pyramid.rows, pixels, ws.dsum);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    {
        const int B = icnet_grid(icnet_cdiv((long)N * h32 * C4, 256), 65536, max_workgroups);
        ProfScope prof("k_icnet_ppm_adj_rows", 2.0 * 8.0 * pix32 * PO_CO, 4.0 * (pix32 + (double)N * h32 * PO_CSLOTS) * PO_CO, s);
        hipLaunchKernelGGL(k_icnet_ppm_adj_rows, dim3(B), dim3(256), 0, s, (const float4 *)ws.dsum, N, h32, w32, C4,
                           (float4 *)ws.cols);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    {
        const int B = icnet_grid(icnet_cdiv((long)N * PO_SLOTS * C4, 256), 65536, max_workgroups);
        ProfScope prof("k_icnet_ppm_adj_bins", 2.0 * 2.0 * (double)N * h32 * PO_CSLOTS * PO_CO,
                       4.0 * (2.0 * (double)N * h32 * PO_CSLOTS + (double)N * PO_SLOTS) * PO_CO, s);
        hipLaunchKernelGGL(k_icnet_ppm_adj_bins, dim3(B), dim3(256), 0, s, (const float4 *)ws.cols, N, h32, w32, C4,
                           (float4 *)ws.gb);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    {
        const int B = icnet_grid(icnet_cdiv(pixels * C4, 256), 65536, max_workgroups);
        ProfScope prof("k_icnet_ppm_adj_sum", 16.0 * pix32 * PO_CO, 4.0 * (3.0 * pix32 + (double)N * PO_SLOTS) * PO_CO, s);
        hipLaunchKernelGGL(k_icnet_ppm_adj_sum, dim3(B), dim3(256), 0, s, (const float4 *)ws.dsum, (const float4 *)ws.gb,
                           (const float4 *)ws.c53, N, h32, w32, C4, (float4 *)ws.g53);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return launch_icnet_wgrad_256x1024(a33, ws.g53, pixels, max_workgroups, scale, ws.rows, params + PO_K, stats, stats + PO_CO,
                                       ws.part, ws.fold, grad + PO_K, grad + PO_G, grad + PO_B, s);
}

}  // namespace ssal
