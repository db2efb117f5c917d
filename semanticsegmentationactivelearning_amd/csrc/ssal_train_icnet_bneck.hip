// ssal_train_icnet_bneck.hip -- training of ICNet's last backbone bottleneck: conv5_3's reduce layer (1 x 1, 1024 -> 256,
// batch-norm, ReLU) and its 3 x 3 (256 -> 256, dilation 4, batch-norm, ReLU) under everything the pooling trainer trains, over
// everything below conv5_2 and the two other frozen branches, gfx950.  Behind the forward path's own
// launches on the weights being trained (launch_igemm twice) and the pooling trainer's gradient (ssal_train_icnet_pool.hip,
// which leaves g53 = dL/dconv5_3 behind its ReLU, the increase layer's batch-norm row and the scale 1 / sum(mask)):
//   k_icnet_bneck_pack      the packed vector -> the two kernels in launch_igemm's layouts, their folded batch-norm rows
//   k_icnet_bneck_dx_inc    the data gradient through the increase layer on the fp32 matrix cores, the ReLU mask of
//                           conv5_3_3x3 in the epilogue: g3 = relu'(a) ((s_i g53) K_i^T)
//   k_icnet_bneck_wgrad3    the 3 x 3 weight gradient: split-K over pixel tiles, one tap and one 128 x 128 slab per workgroup
//   k_icnet_bneck_finish3   fixed-order fold of its partials, the batch-norm scale, 1 / sum(mask); dBeta
//   k_icnet_bneck_gamma3    dGamma contracted from the folded weight gradient (section 28's re-association)
//   k_icnet_bneck_dx_3x3    the data gradient through the dilated 3 x 3 as an implicit GEMM over a tile window with four pixels
//                           of halo, the ReLU mask of conv5_3_1x1_reduce in the epilogue: gr = relu'(r) (sum_tap (s_3 g3) K_3^T)
//   k_icnet_pyramid_wgrad<1024, 256>, its finish and gamma (ssal_train_icnet_pyramid.hip; the profile's k_icnet_bneck_wgrad_r, ...)
// The backward launches stand in launch_icnet_bneck_link, the block's backward below its output gradient: conv5_3's here,
// conv5_2's in ssal_train_icnet_bneck2.hip.
// g3 and gr are un-normalised and WITHOUT their layers' batch-norm scales: each finish kernel applies both once.  No
// floating-point atomics, no inline assembly, 64-bit offsets, grids strided over the tiles: two runs give the same bits.
#include "ssal_icnet.h"
#include "ssal_internal.h"
#include "ssal_mfma.h"
#include "ssal_prof.h"
#include "ssal_train_icnet_bneck.h"

namespace ssal {

bool icnet_bneck_fits(int h32, int w32) { return icnet_pool_fits(h32, w32); }

// P: reduce kernel [1024][256] | gamma | beta | 3 x 3 kernel [9][256][256] | gamma | beta; stats: mean_r | var_r | mean_3 | var_3.
// rows: icnet_bn_row's s_r | t_r | s_3 | t_3 (256 each)
__global__ __launch_bounds__(256) void k_icnet_bneck_pack(const float *__restrict__ P, const float *__restrict__ stats,
                                                          float *__restrict__ wt_r, float *__restrict__ wt_3,
                                                          float *__restrict__ rows)
{
    constexpr int K3 = 9 * BK_C * BK_C;
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o < BK_GR) {
        wt_r[igemm_wt_index(0, o >> 8, o & 255, BK_CIN / 32, BK_C)] = P[BK_KR + o];
    } else if (o < BK_GR + K3) {
        const int e = o - BK_GR;
        wt_3[igemm_wt_index(e >> 16, (e >> 8) & 255, e & 255, BK_C / 32, BK_C)] = P[BK_K3 + e];
    } else if (o < BK_GR + K3 + 2 * BK_C) {
        const int e = o - BK_GR - K3, b = e >> 8, c = e & 255;
        icnet_bn_row(P[(b ? BK_G3 : BK_GR) + c], P[(b ? BK_B3 : BK_BR) + c], stats[2 * b * BK_C + c],
                     stats[(2 * b + 1) * BK_C + c], rows + 2 * b * BK_C + c, rows + (2 * b + 1) * BK_C + c);
    }
}

// g3[p, ci] = a[p, ci] > 0 ? sum_co (s_i[co] g53[p, co]) K_i[ci, co] : 0: the data gradient of the increase layer (1 x 1,
// 256 -> 1024) behind conv5_3_3x3's ReLU.  g53 [pixels, 1024] un-normalised behind conv5_3's ReLU, K_i [256][1024], s_i [1024]
// its batch-norm scale, a = conv5_3_3x3 [pixels, 256] (the fp32 forward values) -> g3 [pixels, 256]; the unmasked sum never
// reaches memory.
// grid (G, 2): k_icnet_pool_dx's plan at the opposite channel counts.  Workgroup (b, y) owns the input channels ci = 128 y ..
// + 127 and takes the tiles b, b + G, ... of BK_DI_PT = 64 pixels (linear over [N, h32, w32]); wave w keeps D[pixel 32 j ..
// + 31][ci = 128 y + 32 w .. + 31], j = 0, 1, in two v_mfma_f32_32x32x2_f32 accumulators.  Per tile, for each of the 32 chunks of
// 32 output channels (ascending): s_i g53 of the chunk (the product rounded once, here; zeros behind the last pixel) -> LDS as
// [co][pixel], K_i's chunk -> LDS as [co][ci] (every global load a float4 of a 128-byte row piece), then 16 steps of two co each.
// One accumulator therefore adds its 1024 products in ascending co, two per instruction.
// LDS banking, under the model k_icnet_pool_dx states (32 banks, a 4-byte access served in groups of 32 consecutive lanes):
// operand reads are 32 consecutive floats per lane group; a staging store's lane group is 4 consecutive pixels x 8 quads at
// bank (4 q + i + pixel) mod 32 for the odd leading dimensions, 32 distinct banks WITHIN the group.  The two groups of a wave
// (pixels pl .. pl + 3 and pl + 4 .. pl + 7) do share banks -- (q, pl + 4) and (q + 1, pl) -- so the stores are free of
// conflicts only as far as the two groups are served in separate passes; no counter run has confirmed that.
constexpr int BD_CC = 32;    // output channels of the layer per chunk
constexpr int BD_LDG = 65;   // 64 pixels + 1
constexpr int BD_LDK = 129;  // 128 ci + 1
__global__ __launch_bounds__(256) void k_icnet_bneck_dx_inc(const float *__restrict__ g53, const float *__restrict__ Ki,
                                                            const float *__restrict__ si, const float *__restrict__ a33,
                                                            long pixels, float *__restrict__ g3)
{
    __shared__ float Gs[BD_CC * BD_LDG];
    __shared__ float Ks[BD_CC * BD_LDK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int ci0 = 128 * blockIdx.y;
    const long tiles = (pixels + BK_DI_PT - 1) / BK_DI_PT;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long p0 = t * BK_DI_PT;
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][i] = 0.0f;
        for (int cc = 0; cc < PO_CO / BD_CC; ++cc) {
            __syncthreads();  // the previous chunk's MFMAs are done with Gs / Ks
            for (int e = tid; e < BK_DI_PT * (BD_CC / 4); e += 256) {
                const int pl = e >> 3, q = e & 7;
                const long p = p0 + pl;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (p < pixels) {
                    const float4 gv = reinterpret_cast<const float4 *>(g53 + p * PO_CO + BD_CC * cc)[q];
                    const float4 sv = reinterpret_cast<const float4 *>(si + BD_CC * cc)[q];
                    v = make_float4(sv.x * gv.x, sv.y * gv.y, sv.z * gv.z, sv.w * gv.w);
                }
                Gs[(4 * q + 0) * BD_LDG + pl] = v.x;
                Gs[(4 * q + 1) * BD_LDG + pl] = v.y;
                Gs[(4 * q + 2) * BD_LDG + pl] = v.z;
                Gs[(4 * q + 3) * BD_LDG + pl] = v.w;
            }
            for (int e = tid; e < 128 * (BD_CC / 4); e += 256) {
                const int ci = e >> 3, q = e & 7;
                const float4 v = reinterpret_cast<const float4 *>(Ki + (long)(ci0 + ci) * PO_CO + BD_CC * cc)[q];
                Ks[(4 * q + 0) * BD_LDK + ci] = v.x;
                Ks[(4 * q + 1) * BD_LDK + ci] = v.y;
                Ks[(4 * q + 2) * BD_LDK + ci] = v.z;
                Ks[(4 * q + 3) * BD_LDK + ci] = v.w;
            }
            __syncthreads();
            const float *ap = Gs + hh * BD_LDG + r;
            const float *bp = Ks + hh * BD_LDK + 32 * wave + r;
#pragma unroll 4
            for (int s = 0; s < BD_CC / 2; ++s) {
                const float b = bp[2 * s * BD_LDK];
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = mfma32(ap[2 * s * BD_LDG + 32 * j], b, acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const long p = p0 + 32 * j + (i & 3) + 8 * (i >> 2) + 4 * hh;
                if (p < pixels) {
                    const long o = p * BK_C + ci0 + 32 * wave + r;
                    g3[o] = a33[o] > 0.0f ? acc[j][i] : 0.0f;
                }
            }
    }
}

// gr[n, y, x, ci] = r[n, y, x, ci] > 0 ? sum_tap sum_co (s_3[co] g3[n, y - 4 (ky - 1), x - 4 (kx - 1), co]) K_3[tap, ci, co] : 0
// (tap = 3 ky + kx; zero outside the map): the data gradient of the 3 x 3 at dilation 4 behind the reduce layer's ReLU.  g3
// [N, H, W, 256] un-normalised behind conv5_3_3x3's ReLU, K_3 [9][256][256], s_3 [256], r = conv5_3_1x1_reduce (the fp32 forward
// values) -> gr [N, H, W, 256].
// grid (G, 2): workgroup (b, y) owns the input channels ci = 128 y .. + 127 and takes the tiles b, b + G, ... of BK_T x BK_T =
// 8 x 8 pixels of one image (tiles linear over [N, ceil(H / 8), ceil(W / 8)]); wave w keeps D[pixel 32 j .. + 31][ci = 128 y +
// 32 w .. + 31], j = 0, 1 (pixel = 8 row + column of the tile).  Per tile, for each of the 8 chunks of 32 output channels
// (ascending): the chunk's window of 16 x 16 pixels -- the tile and four pixels of halo on every side -- of s_3 g3 (the product
// rounded once, here; zeros outside the map) -> LDS as [co][window row][window column]; then for each of the 9 taps (ascending)
// K_3[tap]'s chunk -> LDS as [co][ci] and 16 steps of two co each, the A operand read from the window at the tap's shift.  One
// accumulator therefore adds its 2304 products chunk by chunk, tap by tap within a chunk, co ascending within a tap.
// LDS banking: a window row holds 16 floats at a stride of B3_WROW = 24, so that the 32 pixels of an operand read (4 tile rows
// of 8) fall on banks {0..7, 24..31, 16..23, 8..15} + const; the window store's lane group holds 8 quads x 4 consecutive window
// columns at (4 q + i) B3_LDW + position, conflict-free for an odd B3_LDW; Ks as in k_icnet_bneck_dx_inc.
constexpr int B3_WIN = BK_T + 2 * BK_DIL;                   // 16
constexpr int B3_WROW = 24;
constexpr int B3_LDW = (B3_WIN - 1) * B3_WROW + B3_WIN + 1;  // 377
static_assert(B3_WIN == 16 && BK_T == 8 && (B3_LDW & 1) == 1, "the index arithmetic below is written for 8 x 8 under 16 x 16");
__global__ __launch_bounds__(256) void k_icnet_bneck_dx_3x3(const float *__restrict__ g3, const float *__restrict__ K3,
                                                            const float *__restrict__ s3, const float *__restrict__ rd, int N,
                                                            int H, int W, float *__restrict__ gr)
{
    __shared__ float Ws[BD_CC * B3_LDW];
    __shared__ float Ks[BD_CC * BD_LDK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int ci0 = 128 * blockIdx.y;
    const long tyn = (H + BK_T - 1) / BK_T, txn = (W + BK_T - 1) / BK_T;
    const long tiles = (long)N * tyn * txn;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long n = t / (tyn * txn);
        const int y0 = BK_T * (int)((t / txn) % tyn), x0 = BK_T * (int)(t % txn);
        const float *gn = g3 + n * H * W * BK_C;
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][i] = 0.0f;
        for (int cc = 0; cc < BK_C / BD_CC; ++cc) {
            __syncthreads();  // the previous chunk's MFMAs are done with Ws / Ks
            for (int e = tid; e < B3_WIN * B3_WIN * (BD_CC / 4); e += 256) {
                const int wp = e >> 3, q = e & 7, wy = wp >> 4, wx = wp & 15;
                const int y = y0 - BK_DIL + wy, x = x0 - BK_DIL + wx;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (y >= 0 && y < H && x >= 0 && x < W) {
                    const float4 gv = reinterpret_cast<const float4 *>(gn + ((long)y * W + x) * BK_C + BD_CC * cc)[q];
                    const float4 sv = reinterpret_cast<const float4 *>(s3 + BD_CC * cc)[q];
                    v = make_float4(sv.x * gv.x, sv.y * gv.y, sv.z * gv.z, sv.w * gv.w);
                }
                const int pos = wy * B3_WROW + wx;
                Ws[(4 * q + 0) * B3_LDW + pos] = v.x;
                Ws[(4 * q + 1) * B3_LDW + pos] = v.y;
                Ws[(4 * q + 2) * B3_LDW + pos] = v.z;
                Ws[(4 * q + 3) * B3_LDW + pos] = v.w;
            }
            for (int tap = 0; tap < 9; ++tap) {
                if (tap) __syncthreads();  // the previous tap's MFMAs are done with Ks
                for (int e = tid; e < 128 * (BD_CC / 4); e += 256) {
                    const int ci = e >> 3, q = e & 7;
                    const float4 v = reinterpret_cast<const float4 *>(K3 + ((long)tap * BK_C + ci0 + ci) * BK_C + BD_CC * cc)[q];
                    Ks[(4 * q + 0) * BD_LDK + ci] = v.x;
                    Ks[(4 * q + 1) * BD_LDK + ci] = v.y;
                    Ks[(4 * q + 2) * BD_LDK + ci] = v.z;
                    Ks[(4 * q + 3) * BD_LDK + ci] = v.w;
                }
                __syncthreads();
                // output pixel (py, px) of the tile reads g3 at (py - 4 (ky - 1), px - 4 (kx - 1)): window (py + 8 - 4 ky, px + 8 - 4 kx)
                const int ky = tap / 3, kx = tap - 3 * ky;
                const float *ap = Ws + hh * B3_LDW + ((r >> 3) + 2 * BK_DIL - BK_DIL * ky) * B3_WROW + (r & 7) + 2 * BK_DIL - BK_DIL * kx;
                const float *bp = Ks + hh * BD_LDK + 32 * wave + r;
#pragma unroll 4
                for (int s = 0; s < BD_CC / 2; ++s) {
                    const float b = bp[2 * s * BD_LDK];
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[j] = mfma32(ap[2 * s * B3_LDW + 4 * j * B3_WROW], b, acc[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int pl = 32 * j + (i & 3) + 8 * (i >> 2) + 4 * hh;
                const int y = y0 + (pl >> 3), x = x0 + (pl & 7);
                if (y < H && x < W) {
                    const long o = ((n * H + y) * W + x) * BK_C + ci0 + 32 * wave + r;
                    gr[o] = rd[o] > 0.0f ? acc[j][i] : 0.0f;
                }
            }
    }
}

// part[b][tap][ci][co] = sum over the pixel tiles of group b, sum_p r[p + 4 (tap - 1), ci] g3[p, co] (zero outside the map);
// part[b][9][0][co] = sum_p g3[p, co].  k_icnet_pyramid_wgrad's plan with the tap in the second grid index: grid (G, 18, 2),
// workgroup (b, y, z) owns tap y >> 1 and the slab ci = 128 (y & 1) .. + 127, co = 128 z .. + 127 and takes the tiles b, b + G,
// ... of PY_PT = 32 pixels (linear over [N, H, W]); wave w keeps D[ci = 128 (y & 1) + 32 w .. + 31][co] of its tap in four
// v_mfma_f32_32x32x2_f32 accumulators.  Per tile: r at the tap's shift and g3 -> LDS as [pixel][128 + pad] (zeros behind the
// last pixel and outside the map; every global load is a float4 of a 512-byte row piece), then 16 steps of two pixels each.  One
// accumulator so adds the products of its group's pixels in ascending order.  The y = 0 workgroups also add the rows of g3
// (threads 0 .. 127, one co each, pixels ascending): dBeta's partial.
constexpr int BW_LD = 160;  // as k_icnet_pyramid_wgrad's PW_LD
__global__ __launch_bounds__(256) void k_icnet_bneck_wgrad3(const float *__restrict__ rd, const float *__restrict__ g3, int N,
                                                            int H, int W, float *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float As[PY_PT * BW_LD];
    __shared__ __attribute__((aligned(16))) float Bs[PY_PT * BW_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int tap = blockIdx.y >> 1, ci0 = 128 * (blockIdx.y & 1), co0 = 128 * blockIdx.z;
    const int dy = BK_DIL * (tap / 3 - 1), dx = BK_DIL * (tap % 3 - 1);
    const bool ones = blockIdx.y == 0 && tid < 128;
    const long pixels = (long)N * H * W;
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
                b = reinterpret_cast<const float4 *>(g3 + p * BK_C + co0)[q];
                const int x = (int)(p % W) + dx, y = (int)((p / W) % H) + dy;
                if (y >= 0 && y < H && x >= 0 && x < W)
                    a = reinterpret_cast<const float4 *>(rd + (p + (long)dy * W + dx) * BK_C + ci0)[q];
            }
            *reinterpret_cast<float4 *>(As + pl * BW_LD + 4 * q) = a;
            *reinterpret_cast<float4 *>(Bs + pl * BW_LD + 4 * q) = b;
        }
        __syncthreads();
        const float *ap = As + hh * BW_LD + 32 * wave + r;
        const float *bp = Bs + hh * BW_LD + r;
#pragma unroll 4
        for (int s = 0; s < PY_PT / 2; ++s) {
            const float a = ap[2 * s * BW_LD];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = mfma32(a, bp[2 * s * BW_LD + 32 * j], acc[j]);
        }
        if (ones)
            for (int p = 0; p < PY_PT; ++p) gsum += Bs[p * BW_LD + tid];
    }
    float *pw = part + (long)blockIdx.x * BK_PART3;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = (i & 3) + 8 * (i >> 2) + 4 * hh;
            pw[(tap * BK_C + ci0 + 32 * wave + row) * BK_C + co0 + 32 * j + r] = acc[j][i];
        }
    if (ones) pw[9 * BK_C * BK_C + co0 + tid] = gsum;
}

// The one-layer 3 x 3 form of k_icnet_block_finish (ssal_train_icnet_common.h): raw[o] = sum over split-K groups b = 0 .. G - 1
// of part[b][o], fp32, in that order -> fold[o] ([9 * 256 + 1][256]); dK = (raw scale) s[co], dBeta = raw[9 * 256][co] scale
__global__ __launch_bounds__(256) void k_icnet_bneck_finish3(const float *__restrict__ part, int G,
                                                             const float *__restrict__ scale_p, const float *__restrict__ sl,
                                                             float *__restrict__ fold, float *__restrict__ gK,
                                                             float *__restrict__ gB)
{
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= BK_PART3) return;
    const float scale = scale_p[0];
    float acc = 0.0f;
    for (int gi = 0; gi < G; ++gi) acc += part[(long)gi * BK_PART3 + o];
    fold[o] = acc;
    const int co = o & (BK_C - 1);
    if (o < 9 * BK_C * BK_C) gK[o] = (acc * scale) * sl[co];
    else gB[co] = acc * scale;
}

// The one-layer 3 x 3 form of k_icnet_block_gamma: icnet_gamma_3x3.  One workgroup of 256 threads (co).
__global__ __launch_bounds__(256) void k_icnet_bneck_gamma3(const float *__restrict__ fold, const float *__restrict__ scale_p,
                                                            const float *__restrict__ K, const float *__restrict__ mean,
                                                            const float *__restrict__ var, float *__restrict__ gG)
{
    const int co = threadIdx.x;
    gG[co] = icnet_dgamma(icnet_gamma_3x3(K, fold, BK_C, BK_C, co), mean[co], var[co], fold[9 * BK_C * BK_C + co], scale_p[0]);
}

// The launches of one block's backward below its output gradient (ssal_train_icnet_bneck.h): conv5_3's here, conv5_2's in
// ssal_train_icnet_bneck2.hip
hipError_t launch_icnet_bneck_link(const IcnetBneckLink &L, int N, int h32, int w32, int max_workgroups, hipStream_t s)
{
    const long pixels = (long)N * h32 * w32;
    const double pix32 = (double)pixels;
    constexpr int K3 = 9 * BK_C * BK_C;
    hipError_t e;
    {
        const int G = icnet_grid(icnet_cdiv(pixels, BK_DI_PT), BK_DX_MAX_WG, max_workgroups);
        ProfScope prof(L.names[0], 2.0 * pix32 * PO_CIN * PO_CO,
                       4.0 * pix32 * (2.0 * PO_CO + 2.0 * PO_CIN) + 4.0 * (double)icnet_cdiv(pixels, BK_DI_PT) * PO_CIN * PO_CO, s);
        hipLaunchKernelGGL(k_icnet_bneck_dx_inc, dim3(G, BK_C / 128), dim3(256), 0, s, L.gout, L.Ki, L.s_i, L.a33, pixels, L.g3);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const int G3 = icnet_grid(icnet_cdiv(pixels, PY_PT), BK_W3_MAX_WG, max_workgroups);
    {
        ProfScope prof(L.names[1], 2.0 * pix32 * BK_PART3, 4.0 * pix32 * 18.0 * BK_C + 4.0 * G3 * BK_PART3, s);
        hipLaunchKernelGGL(k_icnet_bneck_wgrad3, dim3(G3, 18, BK_C / 128), dim3(256), 0, s, L.rd, L.g3, N, h32, w32, L.part3);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    {
        ProfScope prof(L.names[2], (double)G3 * BK_PART3, 4.0 * (G3 + 2.0) * BK_PART3, s);
        hipLaunchKernelGGL(k_icnet_bneck_finish3, dim3(icnet_cdiv(BK_PART3, 256)), dim3(256), 0, s, L.part3, G3, L.scale, L.s_3,
                           L.fold3, L.gK3, L.gB3);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    {
        ProfScope prof(L.names[3], 2.0 * K3, 8.0 * BK_PART3, s);
        hipLaunchKernelGGL(k_icnet_bneck_gamma3, dim3(1), dim3(256), 0, s, L.fold3, L.scale, L.K3, L.mean_3, L.var_3,
                           L.gG3);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    {
        const long tiles = (long)N * icnet_cdiv(h32, BK_T) * icnet_cdiv(w32, BK_T);
        const int G = icnet_grid(tiles, BK_DX_MAX_WG, max_workgroups);
        ProfScope prof(L.names[4], 2.0 * pix32 * K3,
                       4.0 * pix32 * 3.0 * BK_C + 4.0 * (double)tiles * (K3 + 2.0 * (B3_WIN * B3_WIN - BK_T * BK_T) * BK_C), s);
        hipLaunchKernelGGL(k_icnet_bneck_dx_3x3, dim3(G, BK_C / 128), dim3(256), 0, s, L.g3, L.K3, L.s_3, L.rd, N, h32, w32,
                           L.gr);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return launch_icnet_wgrad_1024x256(L.x, L.gr, pixels, max_workgroups, L.scale, L.s_r, L.Kr, L.mean_r, L.var_r, L.partr, L.foldr,
                                       L.gKr, L.gGr, L.gBr, s, L.names + 5);
}

hipError_t launch_icnet_bneck_grad(const float *c52, const float *c31, const float *c3, int N, int h32, int w32, int K,
                                   const float *params, const float *stats, const uint8_t *labels, const float *mask,
                                   float weight, float label_smoothing, int max_workgroups, const IcnetBneckWs &ws, double *loss,
                                   float *grad, hipStream_t s)
{
    if (N < 1 || K < 2 || K > 32 || max_workgroups < 0 || !icnet_bneck_fits(h32, w32)) return hipErrorInvalidValue;
    constexpr int K3 = 9 * BK_C * BK_C;
    const float *s_r = ws.rows, *s_3 = ws.rows + 2 * BK_C;
    hipError_t e;
    // ---- forward: the pack, then run_trunk's launches of the reduce layer and the 3 x 3 on the weights being trained ----
    {
        ProfScope prof("k_icnet_bneck_pack", 0.0, 8.0 * (BK_GR + K3 + 2 * BK_C), s);
        hipLaunchKernelGGL(k_icnet_bneck_pack, dim3(icnet_cdiv(BK_GR + K3 + 2 * BK_C, 256)), dim3(256), 0, s, params, stats, ws.wt_r,
                           ws.wt_3, ws.rows);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    e = launch_igemm(c52, N, h32, w32, BK_CIN, ws.wt_r, 1, 1, BK_C, 1, 1, s_r, s_r + BK_C, nullptr, true, false, ws.rd, s);
    if (e != hipSuccess) return e;
    e = launch_igemm(ws.rd, N, h32, w32, BK_C, ws.wt_3, 3, 3, BK_C, 1, BK_DIL, s_3, s_3 + BK_C, nullptr, true, false, ws.a33, s);
    if (e != hipSuccess) return e;
    // section 41 as it stands: the increase layer, the pyramid pooling, the pyramid head, the loss, its twenty gradients, g53 behind
    // conv5_3's ReLU
    e = launch_icnet_pool_grad(ws.a33, c52, c31, c3, N, h32, w32, K, params + BK_POOL, stats + BK_STATS_OWN, labels, mask, weight,
                               label_smoothing, max_workgroups, ws.pool, loss, grad + BK_POOL, s);
    if (e != hipSuccess) return e;
    const float *scale = ws.pool.pyramid.cascade.fusion.fold + FU_PART;  // 1 / sum(mask), as the fusion trainer's finish left it
    // ---- backward: conv5_3 as a link ----
    static const char *const names[] = {"k_icnet_bneck_dx_inc", "k_icnet_bneck_wgrad3", "k_icnet_bneck_finish3", "k_icnet_bneck_gamma3",
                                        "k_icnet_bneck_dx_3x3", "k_icnet_bneck_wgrad_r", "k_icnet_bneck_finish_r",
                                        "k_icnet_bneck_gamma_r"};
    const IcnetBneckLink L = {c52, ws.rd, ws.a33, ws.pool.g53, params + BK_POOL + PO_K, ws.pool.rows, params + BK_K3, s_3,
                              stats + 2 * BK_C, stats + 3 * BK_C, params + BK_KR, s_r, stats, stats + BK_C, scale, ws.g3, ws.gr,
                              ws.part3, ws.fold3, ws.partr, ws.foldr, grad + BK_K3, grad + BK_G3, grad + BK_B3, grad + BK_KR,
                              grad + BK_GR, grad + BK_BR, names};
    return launch_icnet_bneck_link(L, N, h32, w32, max_workgroups, s);
}

}  // namespace ssal
