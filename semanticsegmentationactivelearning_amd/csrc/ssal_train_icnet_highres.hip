// ssal_train_icnet_highres.hip -- training of ICNet's high-resolution branch (conv1_sub1, conv2_sub1, conv3_sub1) down to the
// image, with the whole cascade head, over the two frozen backbone branches, gfx950.  Behind the
// forward path's own launches on the weights being trained (launch_conv_first, launch_igemm) and the cascade trainer's
// gradient (ssal_train_icnet_cascade.hip, which leaves g = dL/dsub12_sum behind its ReLU and the scale 1 / sum(mask)):
//   k_icnet_highres_pack     the packed vector -> conv2_sub1 / conv3_sub1 in launch_igemm's layout, the three folded
//                            batch-norm rows (conv1_sub1's kernel is read where it lies: launch_conv_first takes HWIO)
//   k_icnet_highres_dproj    the data gradient through conv3_sub1_proj (128 -> 64) with F3's ReLU mask on the fp32 matrix
//                            cores: gz_3[p, ci] = F3[p, ci] > 0 ? sum_co K_b[ci, co] (s_b[co] g[p, co]) : 0
//   k_icnet_highres_dx<CO>   the data gradient through a 3 x 3 stride-2 convolution (CO -> 32) in gather form on the fp32
//                            matrix cores, the ReLU mask of the layer below applied: gz_l -> gz_{l-1}
//   k_icnet_highres_wgrad<CO>  the weight gradient of a 32 -> CO layer on the fp32 matrix cores, split-K over pixel tiles
//   k_icnet_highres_wgrad1<CIN, TX>  conv1_sub1's (27 or 36 rows x 32) on the vector ALU: it is bound by the bytes of gz_1
//                            and of the frame, and a 32 x 32 MFMA tile would be 3/32 or 4/32 full
//   k_icnet_highres_finish   fixed-order fold of the partials, the batch-norm scale, 1 / sum(mask); dBeta
//   k_icnet_highres_gamma    dGamma contracted from the folded weight gradient (section 28's re-association)
// The last two are the one-layer forms of the fusion blocks' finish and gamma; the batch-norm row fold, the relayout index, the
// gamma loop and the grid arithmetic are ssal_train_icnet_common.h's.
// Every gz is un-normalised and WITHOUT its layer's batch-norm scale: the weight gradient wants it so (s_l is applied once,
// by the finish kernel), and a data-gradient kernel forms gs_l = s_l gz_l, rounded once, while it stages its window.
// No floating-point atomics, no inline assembly, 64-bit offsets, grids strided over the tiles: two runs give the same bits.
#include "ssal_icnet.h"
#include "ssal_internal.h"
#include "ssal_mfma.h"
#include "ssal_prof.h"
#include "ssal_train_icnet_highres.h"

namespace ssal {

bool icnet_highres_fits(int n, int h32, int w32)
{
    if (n < 1 || !icnet_cascade_fits(h32, w32)) return false;
    return (double)n * h32 * w32 < 131072.0;  // n (32 h32) (32 w32) < 2^27: check_dims' limit (ssal_icnet_api.hip)
}

// P: the packed vector; o2 / o3: where conv2_sub1.kernel / conv3_sub1.kernel start; the gammas and betas follow their kernels
// (ssal_train_icnet_highres.h).  stats: mean_1 | var_1 | mean_2 | var_2 (32 each) | mean_3 | var_3 (64 each).
// rows: icnet_bn_row's s | t of each layer.
__global__ __launch_bounds__(256) void k_icnet_highres_pack(const float *__restrict__ P, IcnetHighresOff off,
                                                            const float *__restrict__ stats, float *__restrict__ wt2,
                                                            float *__restrict__ wt3, float *__restrict__ rows)
{
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o < 9 * 32 * 32) {
        const int tap = o >> 10, ci = (o >> 5) & 31, co = o & 31;
        wt2[igemm_wt_index(tap, ci, co, 1, 32)] = P[off.k2 + o];
    } else if (o < 9 * 32 * 32 + 9 * 32 * 64) {
        const int e = o - 9 * 32 * 32, tap = e >> 11, ci = (e >> 6) & 31, co = e & 63;
        wt3[igemm_wt_index(tap, ci, co, 1, 64)] = P[off.k3 + e];
    } else if (o < 9 * 32 * 32 + 9 * 32 * 64 + 128) {
        const int e = o - 9 * 32 * 32 - 9 * 32 * 64;
        int c, go, bo, mo, vo, so, w;
        if (e < 32) { c = e; go = off.g1; bo = off.b1; mo = 0; vo = 32; so = 0; w = 32; }
        else if (e < 64) { c = e - 32; go = off.g2; bo = off.b2; mo = 64; vo = 96; so = 64; w = 32; }
        else { c = e - 64; go = off.g3; bo = off.b3; mo = 128; vo = 192; so = 128; w = 64; }
        icnet_bn_row(P[go + c], P[bo + c], stats[mo + c], stats[vo + c], rows + so + c, rows + so + w + c);
    }
}

// gz3[p, ci] = F3[p, ci] > 0 ? sum_co Kb[ci, co] (sb[co] g[p, co]) : 0: a GEMM of pixels x 128 x 64.  A workgroup keeps Kb
// transposed in LDS and takes the tiles b, b + G, ... of 64 pixels; wave w owns the pixels 32 (w & 1) .. + 31 and the input
// channels 32 (w >> 1) .. + 31: one v_mfma_f32_32x32x2_f32 accumulator D[pixel][ci].  The product sb g is rounded once, when
// the tile is staged (two halves of 64 output channels); one accumulator adds its 128 products co ascending.
constexpr int DP_LD = 68;
__global__ __launch_bounds__(256) void k_icnet_highres_dproj(const float *__restrict__ g, const float *__restrict__ Kb,
                                                             const float *__restrict__ sb, const float *__restrict__ F3,
                                                             long pixels, float *__restrict__ gz3)
{
    __shared__ __attribute__((aligned(16))) float Ag[64 * DP_LD];   // [pixel][co of the half]
    __shared__ __attribute__((aligned(16))) float Bk[128 * DP_LD];  // [co][ci]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int ph = wave & 1, ch = wave >> 1;
    for (int e = tid; e < 64 * 32; e += 256) {
        const int ci = e >> 5, q = e & 31;
        const float4 v = reinterpret_cast<const float4 *>(Kb + ci * 128)[q];
        Bk[(4 * q + 0) * DP_LD + ci] = v.x;
        Bk[(4 * q + 1) * DP_LD + ci] = v.y;
        Bk[(4 * q + 2) * DP_LD + ci] = v.z;
        Bk[(4 * q + 3) * DP_LD + ci] = v.w;
    }
    const long tiles = (pixels + 63) / 64;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long p0 = t * 64;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
        for (int half = 0; half < 2; ++half) {
            __syncthreads();  // the previous half's (tile's) MFMAs are done with Ag; Bk is written
            for (int e = tid; e < 64 * 16; e += 256) {
                const int pl = e >> 4, q = e & 15;
                const long p = p0 + pl;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (p < pixels) {
                    const float4 gv = reinterpret_cast<const float4 *>(g + p * 128 + 64 * half)[q];
                    const float4 sv = reinterpret_cast<const float4 *>(sb + 64 * half)[q];
                    v = make_float4(sv.x * gv.x, sv.y * gv.y, sv.z * gv.z, sv.w * gv.w);
                }
                *reinterpret_cast<float4 *>(Ag + pl * DP_LD + 4 * q) = v;
            }
            __syncthreads();
            const float *ap = Ag + (32 * ph + r) * DP_LD + hh;
            const float *bp = Bk + (64 * half + hh) * DP_LD + 32 * ch + r;
#pragma unroll 8
            for (int s = 0; s < 32; ++s) acc = mfma32(ap[2 * s], bp[2 * s * DP_LD], acc);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long p = p0 + 32 * ph + (i & 3) + 8 * (i >> 2) + 4 * hh;
            if (p < pixels) {
                const long o = p * 64 + 32 * ch + r;
                gz3[o] = F3[o] > 0.0f ? acc[i] : 0.0f;
            }
        }
    }
}

// out[y, x, ci] = below[y, x, ci] > 0 ? sum_{kh = y, kw = x (mod 2)} sum_co K[kh, kw, ci, co] gs[(y - kh) / 2, (x - kw) / 2, co]
// : 0, gs = sc[co] gz, zero outside the map: the transposed 3 x 3 stride-2 convolution (TF SAME on even sizes: no pad before)
// in gather form.  The pixels (y, x) = (2 u + py, 2 v + px) of one parity class form a map of gz's size on which the class is
// a convolution with offsets 0 (kh = py) and -1 (kh = 2, py = 0): 4, 2, 2 and 1 taps.  A workgroup takes the tiles b, b + G,
// ... of 8 x 16 class pixels (u, v), image after image, stages the 9 x 17 window of gs behind them once (the product sc gz is
// rounded once, here) and runs the four classes one after the other; wave w owns the class pixels 32 w .. + 31 and all 32
// input channels: one v_mfma_f32_32x32x2_f32 accumulator D[pixel][ci] per class.  Per tap (kh, then kw ascending): K[tap] ->
// LDS as [co][ci], CO / 2 steps of two co each.  Every output pixel so has ONE owner that adds its at most 4 CO products in
// the order (kh, kw, co).
constexpr int HX_TH = 8, HX_TW = 16, HX_WH = HX_TH + 1, HX_WW = HX_TW + 1;
template <int CO>
__global__ __launch_bounds__(256) void k_icnet_highres_dx(const float *__restrict__ gz, const float *__restrict__ K,
                                                          const float *__restrict__ sc, const float *__restrict__ below,
                                                          int N, int Ho, int Wo, float *__restrict__ out)
{
    constexpr int LDA = CO + 4, Q = CO / 4;
    __shared__ __attribute__((aligned(16))) float win[HX_WH * HX_WW * LDA];
    __shared__ __attribute__((aligned(16))) float Wb[CO * 32];  // [co][ci]: the lane halves (co, co + 1) fall on the two bank halves
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int Hin = 2 * Ho, Win = 2 * Wo;
    const int tx = (Wo + HX_TW - 1) / HX_TW, ty = (Ho + HX_TH - 1) / HX_TH;
    const long per_image = (long)tx * ty, tiles = (long)N * per_image;
    const int pl = 32 * wave + r, ul = pl >> 4, vl = pl & 15;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long n = t / per_image;
        const int rem = (int)(t % per_image);
        const int u0 = (rem / tx) * HX_TH, v0 = (rem % tx) * HX_TW;
        __syncthreads();  // the previous tile's MFMAs are done with win
        for (int e = tid; e < HX_WH * HX_WW * Q; e += 256) {
            const int wp = e / Q, q = e % Q;
            const int i = u0 - 1 + wp / HX_WW, j = v0 - 1 + wp % HX_WW;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (i >= 0 && i < Ho && j >= 0 && j < Wo) {
                const float4 gv = reinterpret_cast<const float4 *>(gz + ((n * Ho + i) * Wo + j) * CO)[q];
                const float4 sv = reinterpret_cast<const float4 *>(sc)[q];
                v = make_float4(sv.x * gv.x, sv.y * gv.y, sv.z * gv.z, sv.w * gv.w);
            }
            *reinterpret_cast<float4 *>(win + wp * LDA + 4 * q) = v;
        }
        for (int cls = 0; cls < 4; ++cls) {
            const int py = cls >> 1, px = cls & 1;
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
            for (int kh = py; kh < 3; kh += 2)
                for (int kw = px; kw < 3; kw += 2) {
                    __syncthreads();  // the previous tap's MFMAs are done with Wb; the window is staged
                    for (int e = tid; e < 32 * Q; e += 256) {
                        const int ci = e / Q, q = e % Q;
                        const float4 v = reinterpret_cast<const float4 *>(K + ((kh * 3 + kw) * 32 + ci) * CO)[q];
                        Wb[(4 * q + 0) * 32 + ci] = v.x;
                        Wb[(4 * q + 1) * 32 + ci] = v.y;
                        Wb[(4 * q + 2) * 32 + ci] = v.z;
                        Wb[(4 * q + 3) * 32 + ci] = v.w;
                    }
                    __syncthreads();
                    // window pixel of gs[u - (kh - py) / 2, v - (kw - px) / 2] for class pixel (u, v): + 1 for the halo
                    const int du = (kh - py) >> 1, dv = (kw - px) >> 1;
                    const float *ap = win + ((ul + 1 - du) * HX_WW + vl + 1 - dv) * LDA + hh;
                    const float *bp = Wb + hh * 32 + r;
#pragma unroll 8
                    for (int s = 0; s < CO / 2; ++s) acc = mfma32(ap[2 * s], bp[2 * s * 32], acc);
                }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int p = 32 * wave + (i & 3) + 8 * (i >> 2) + 4 * hh;
                const int u = u0 + (p >> 4), v = v0 + (p & 15);
                if (u < Ho && v < Wo) {
                    const long o = ((n * Hin + 2 * u + py) * Win + 2 * v + px) * 32 + r;
                    out[o] = below[o] > 0.0f ? acc[i] : 0.0f;
                }
            }
        }
    }
}

// part[b][(kh 3 + kw) 32 + ci][co] = sum over the tiles of workgroup b, sum_p a[2 i + kh, 2 j + kw, ci] gz[p, co] (rows and
// columns Hin, Win of a read 0: TF's padding after), part[b][288][co] = sum_p gz[p, co].  grid (G, 3): workgroup (b, kh) takes
// the pixel tiles b, b + G, ... (4 x 16 pixels of gz, image after image); wave kw = 0 .. 2 keeps D[ci][co] of its tap in CO / 32
// v_mfma_f32_32x32x2_f32 accumulators, wave 3 of the kh = 0 workgroups feeds a row of ones instead (row 0 of its D: dBeta).
// Per tile: gz[tile] -> LDS (zeros outside the map), the 4 x 33 pixels of a on the tile's rows 2 i + kh -> LDS, 32 steps of
// two pixels each: lane (r = lane & 31, h = lane >> 5) feeds a[pixel 2 s + h shifted by kw][r] and gz[pixel 2 s + h][32 j + r].
constexpr int HW_TH = 4, HW_TW = 16, HW_AW = 2 * HW_TW + 1, HW_LDA = 48;  // 2 pixels = 96 floats: the lane halves on the two bank halves
template <int CO>
__global__ __launch_bounds__(256) void k_icnet_highres_wgrad(const float *__restrict__ a, const float *__restrict__ gz, int N,
                                                             int Ho, int Wo, float *__restrict__ part)
{
    constexpr int LDB = CO == 32 ? 32 : 96, Q = CO / 4, NJ = CO / 32, ROWS = 9 * 32 + 1;
    __shared__ __attribute__((aligned(16))) float As[HW_TH * HW_AW * HW_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[HW_TH * HW_TW * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int kh = blockIdx.y, Hin = 2 * Ho, Win = 2 * Wo;
    const int tx = (Wo + HW_TW - 1) / HW_TW, ty = (Ho + HW_TH - 1) / HW_TH;
    const long per_image = (long)tx * ty, tiles = (long)N * per_image;
    f32x16 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.0f;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long n = t / per_image;
        const int rem = (int)(t % per_image);
        const int i0 = (rem / tx) * HW_TH, j0 = (rem % tx) * HW_TW;
        __syncthreads();  // the previous tile's MFMAs are done with As / Bs
        for (int e = tid; e < HW_TH * HW_TW * Q; e += 256) {
            const int p = e / Q, q = e % Q;
            const int i = i0 + (p >> 4), j = j0 + (p & 15);
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (i < Ho && j < Wo) v = reinterpret_cast<const float4 *>(gz + ((n * Ho + i) * Wo + j) * CO)[q];
            *reinterpret_cast<float4 *>(Bs + p * LDB + 4 * q) = v;
        }
        for (int e = tid; e < HW_TH * HW_AW * 8; e += 256) {
            const int q = e & 7, c = (e >> 3) % HW_AW, il = (e >> 3) / HW_AW;
            const int y = 2 * (i0 + il) + kh, x = 2 * j0 + c;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (i0 + il < Ho && y < Hin && x < Win) v = reinterpret_cast<const float4 *>(a + ((n * Hin + y) * Win + x) * 32)[q];
            *reinterpret_cast<float4 *>(As + (il * HW_AW + c) * HW_LDA + 4 * q) = v;
        }
        __syncthreads();
        if (wave < 3) {
#pragma unroll 4
            for (int s = 0; s < 32; ++s) {
                const int pk = 2 * s + hh;
                const float av = As[((pk >> 4) * HW_AW + 2 * (pk & 15) + wave) * HW_LDA + r];
                const float *bp = Bs + pk * LDB + r;
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[j] = mfma32(av, bp[32 * j], acc[j]);
            }
        } else if (kh == 0) {
            const float av = r == 0 ? 1.0f : 0.0f;
#pragma unroll 4
            for (int s = 0; s < 32; ++s) {
                const float *bp = Bs + (2 * s + hh) * LDB + r;
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[j] = mfma32(av, bp[32 * j], acc[j]);
            }
        }
    }
    float *pw = part + (long)blockIdx.x * (ROWS * CO);
    if (wave < 3) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = (i & 3) + 8 * (i >> 2) + 4 * hh;
                pw[((kh * 3 + wave) * 32 + row) * CO + 32 * j + r] = acc[j][i];
            }
    } else if (kh == 0 && hh == 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) pw[(ROWS - 1) * CO + 32 * j + r] = acc[j][0];
    }
}

__device__ __forceinline__ float hr_unit(float v) { return v; }
__device__ __forceinline__ float hr_unit(uint8_t v) { return (float)v * (1.0f / 255.0f); }  // launch_conv_first's conversion

// conv1_sub1's weight gradient on the vector ALU.  part[b][(kh 3 + kw) CIN + ci][co] and part[b][9 CIN][co] = sum_p gz as
// above.  Thread (co = tid & 31, group = tid >> 5): a workgroup takes the chunks b, b + G, ... of 256 pixels of gz_1 (linear
// over [N, Ho, Wo]); group q adds the pixels 8 k + q (k = 0 .. 31) of a chunk into its 9 CIN + 1 registers, one fmaf per tap and
// input channel (the frame's value is the same for the 32 lanes of a group: one broadcast load), then the eight groups are
// added in group order through LDS.
template <int CIN, typename TX>
__global__ __launch_bounds__(256) void k_icnet_highres_wgrad1(const TX *__restrict__ x, const float *__restrict__ gz, int N,
                                                              int Ho, int Wo, float *__restrict__ part)
{
    constexpr int R = 9 * CIN + 1;
    __shared__ float red[8 * R * 32];
    const int tid = threadIdx.x, co = tid & 31, grp = tid >> 5;
    const int H = 2 * Ho, W = 2 * Wo;
    const long pixels = (long)N * Ho * Wo, chunks = (pixels + 255) / 256;
    float acc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] = 0.0f;
    for (long t = blockIdx.x; t < chunks; t += gridDim.x)
        for (int k = 0; k < 32; ++k) {
            const long p = t * 256 + 8 * k + grp;
            if (p >= pixels) continue;
            const int j = (int)(p % Wo), i = (int)((p / Wo) % Ho);
            const long n = p / ((long)Wo * Ho);
            const float gv = gz[p * 32 + co];
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int y = 2 * i + kh, xx = 2 * j + kw;
                    if (y < H && xx < W) {
                        const TX *px = x + ((n * H + y) * W + xx) * CIN;
#pragma unroll
                        for (int ci = 0; ci < CIN; ++ci)
                            acc[(kh * 3 + kw) * CIN + ci] = fmaf(hr_unit(px[ci]), gv, acc[(kh * 3 + kw) * CIN + ci]);
                    }
                }
            acc[R - 1] += gv;
        }
#pragma unroll
    for (int i = 0; i < R; ++i) red[(grp * R + i) * 32 + co] = acc[i];
    __syncthreads();
    for (int e = tid; e < R * 32; e += 256) {
        float sum = 0.0f;
        for (int q = 0; q < 8; ++q) sum += red[q * R * 32 + e];
        part[(long)blockIdx.x * (R * 32) + e] = sum;
    }
}

// The one-layer form of k_icnet_block_finish (ssal_train_icnet_common.h) at run-time widths: raw[o] = sum over split-K groups
// b = 0 .. G - 1 of part[b][o], fp32, in that order -> fold[o] ([rows + 1][CO]); dK = (raw scale) s[co] for the first `rows`
// rows, dBeta = raw[rows][co] scale; scale: the one the fusion trainer's finish took from the head kernel's lpart
__global__ __launch_bounds__(256) void k_icnet_highres_finish(const float *__restrict__ part, int G, int rows, int CO,
                                                              const float *__restrict__ scale_p, const float *__restrict__ sl,
                                                              float *__restrict__ fold, float *__restrict__ gK,
                                                              float *__restrict__ gB)
{
    const int o = blockIdx.x * 256 + threadIdx.x, total = (rows + 1) * CO;
    if (o >= total) return;
    const float scale = scale_p[0];
    float acc = 0.0f;
    for (int gi = 0; gi < G; ++gi) acc += part[(long)gi * total + o];
    fold[o] = acc;
    const int co = o % CO;
    if (o < rows * CO) gK[o] = (acc * scale) * sl[co];
    else gB[co] = acc * scale;
}

// The one-layer form of k_icnet_block_gamma: its 3 x 3 branch at run-time widths.  One workgroup of 64 threads (co).
__global__ __launch_bounds__(64) void k_icnet_highres_gamma(const float *__restrict__ fold, const float *__restrict__ scale_p,
                                                            const float *__restrict__ K, const float *__restrict__ mean,
                                                            const float *__restrict__ var, int CI, int CO,
                                                            float *__restrict__ gG)
{
    const int co = threadIdx.x;
    if (co >= CO) return;
    gG[co] = icnet_dgamma(icnet_gamma_3x3(K, fold, CI, CO, co), mean[co], var[co], fold[9 * CI * CO + co], scale_p[0]);
}

// finish + gamma of one layer whose partials lie in ws.part
static hipError_t highres_fold(int G, int CI, int CO, const float *scale, const float *sl, const float *K, const float *mean,
                               const float *var, const IcnetHighresWs &ws, float *gK, float *gG, float *gB, hipStream_t s)
{
    const int total = (9 * CI + 1) * CO;
    hipError_t e;
    {
        ProfScope prof("k_icnet_highres_finish", (double)G * total, 4.0 * (G + 2.0) * total, s);
        hipLaunchKernelGGL(k_icnet_highres_finish, dim3(icnet_cdiv(total, 256)), dim3(256), 0, s, ws.part, G, 9 * CI, CO, scale,
                           sl, ws.fold, gK, gB);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    ProfScope prof("k_icnet_highres_gamma", 2.0 * 9 * CI * CO, 8.0 * total, s);
    hipLaunchKernelGGL(k_icnet_highres_gamma, dim3(1), dim3(64), 0, s, ws.fold, scale, K, mean, var, CI, CO, gG);
    return hipGetLastError();
}

// the raw side's route (ssal_train_icnet_highres.h)
bool icnet_highres_raw_fused(int c_in, int N, int h32, int w32, int ic_front, bool mfma)
{
    if (!mfma || !(ic_front & 1) || N < 1 || h32 < 1 || w32 < 1) return false;
    const long H = 32L * h32, W = 32L * w32;
    if (H * W * c_in * 4 >= (1L << 31)) return false;
    if ((long)N * icnet_cdiv(H / 4, 8) * icnet_cdiv(W / 4, 16) >= (1L << 31)) return false;
    return front2_supported((int)H, (int)W, c_in, 1, 2);
}

// the pack, then run_trunk's launches of the branch (ssal_icnet_api.hip) on the weights being trained: ws.f3 = conv3_sub1(x).
// fused: conv1_sub1 + conv2_sub1 as one launch into ws.a2 -- ws.a1 is not written (the raw side: nobody reads it again); else
// the separate launches, which leave a_1 in ws.a1 and a_2 in ws.a2 for the backward pass
static hipError_t highres_forward(const void *x, bool x_is_u8, int c_in, int N, int h32, int w32, const float *params,
                                  const float *stats, const IcnetHighresWs &ws, bool fused, hipStream_t s)
{
    const IcnetHighresOff off = icnet_highres_offsets(c_in);
    const int H = 32 * h32, W = 32 * w32, h2 = H / 2, w2 = W / 2, h4 = H / 4, w4 = W / 4;
    const float *s1 = ws.rows, *t1 = ws.rows + 32, *s2 = ws.rows + 64, *t2 = ws.rows + 96, *s3 = ws.rows + 128,
                *t3 = ws.rows + 192;
    hipError_t e;
    {
        ProfScope prof("k_icnet_highres_pack", 0.0, 8.0 * (9 * 32 * 96 + 128), s);
        hipLaunchKernelGGL(k_icnet_highres_pack, dim3(icnet_cdiv(9 * 32 * 96 + 128, 256)), dim3(256), 0, s, params, off, stats,
                           ws.wt2, ws.wt3, ws.rows);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (fused) {
        e = launch_front2(x, x_is_u8, N, H, W, c_in, 1, params + off.k1, s1, t1, ws.wt2, s2, t2, 2, ws.a2, s);
        if (e != hipSuccess) return e;
    } else {
        if ((e = launch_conv_first(x, x_is_u8, N, H, W, c_in, 1, params + off.k1, s1, t1, ws.a1, s)) != hipSuccess) return e;
        e = launch_igemm(ws.a1, N, h2, w2, 32, ws.wt2, 3, 3, 32, 2, 1, s2, t2, nullptr, true, false, ws.a2, s);
        if (e != hipSuccess) return e;
    }
    return launch_igemm(ws.a2, N, h4, w4, 32, ws.wt3, 3, 3, 64, 2, 1, s3, t3, nullptr, true, false, ws.f3, s);
}

hipError_t launch_icnet_highres_targets(const float *c54_raw, const float *c31_raw, const void *x_raw, bool x_is_u8, int c_in,
                                        int N, int h32, int w32, int K, const float *params, const float *stats,
                                        int max_workgroups, const IcnetHighresWs &ws, const IcnetHeadSemi &semi, uint8_t *tgt,
                                        hipStream_t s)
{
    if (N < 1 || K < 2 || K > 32 || max_workgroups < 0 || (c_in != 3 && c_in != 4) || !icnet_highres_fits(N, h32, w32) ||
        !c54_raw || !c31_raw || !x_raw)
        return hipErrorInvalidValue;
    const IcnetHighresOff off = icnet_highres_offsets(c_in);
    if (semi.labelled) {  // (every image labelled: no pseudo target is read)
        const bool fused = icnet_highres_raw_fused(c_in, N, h32, w32, knobs().ic_front, mfma_family());
        const hipError_t e = highres_forward(x_raw, x_is_u8, c_in, N, h32, w32, params, stats, ws, fused, s);
        if (e != hipSuccess) return e;
    }
    return launch_icnet_cascade_targets(c54_raw, c31_raw, ws.f3, N, h32, w32, K, params + off.cascade, stats + HR_STATS_OWN,
                                        max_workgroups, ws.cascade, semi, tgt, s);
}

hipError_t launch_icnet_highres_grad(const float *c54, const float *c31, const void *x, bool x_is_u8, int c_in, int N, int h32,
                                     int w32, int K, const float *params, const float *stats, const uint8_t *labels,
                                     const float *mask, float weight, float label_smoothing, int max_workgroups,
                                     const IcnetHighresWs &ws, double *loss, float *grad, hipStream_t s, const IcnetHeadSemi *semi)
{
    if (N < 1 || K < 2 || K > 32 || max_workgroups < 0 || (c_in != 3 && c_in != 4) || !icnet_highres_fits(N, h32, w32))
        return hipErrorInvalidValue;
    const IcnetHighresOff off = icnet_highres_offsets(c_in);
    const int H = 32 * h32, W = 32 * w32, h2 = H / 2, w2 = W / 2, h4 = H / 4, w4 = W / 4, h8 = H / 8, w8 = W / 8;
    const double pix2 = (double)N * h2 * w2, pix4 = (double)N * h4 * w4, pix8 = (double)N * h8 * w8;
    const float *s1 = ws.rows, *s2 = ws.rows + 64, *s3 = ws.rows + 128;
    // ---- forward: the pack, then run_trunk's launches of the branch on the weights being trained; a_1 is kept ----
    hipError_t e = highres_forward(x, x_is_u8, c_in, N, h32, w32, params, stats, ws, false, s);
    if (e != hipSuccess) return e;
    // section 29 as it stands: both fusion blocks, the head, the loss, its fourteen gradients, g behind sub12_sum's ReLU
    e = launch_icnet_cascade_grad(c54, c31, ws.f3, N, h32, w32, K, params + off.cascade, stats + HR_STATS_OWN, labels, mask,
                                  weight, label_smoothing, max_workgroups, ws.cascade, loss, grad + off.cascade, s, semi);
    if (e != hipSuccess) return e;
    const float *scale = ws.cascade.fusion.fold + FU_PART;
    // ---- backward ----
    {
        const long tiles = icnet_cdiv((long)N * h8 * w8, 64);
        ProfScope prof("k_icnet_highres_dproj", 2.0 * pix8 * 128 * 64, 4.0 * pix8 * (128 + 64 + 64), s);
        hipLaunchKernelGGL(k_icnet_highres_dproj, dim3(icnet_grid(tiles, HR_DX_MAX_WG, max_workgroups)), dim3(256), 0, s,
                           ws.cascade.fusion.g, params + off.cascade + CA_FUSION + FU_KB, ws.cascade.fusion.rows + 256, ws.f3,
                           (long)N * h8 * w8, ws.gz3);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const long wt3 = (long)N * icnet_cdiv(h8, HW_TH) * icnet_cdiv(w8, HW_TW);
    const long wt2 = (long)N * icnet_cdiv(h4, HW_TH) * icnet_cdiv(w4, HW_TW);
    {
        const int G = icnet_grid(wt3, HR_MAX_WG, max_workgroups);
        {
            ProfScope prof("k_icnet_highres_wgrad<64>", 2.0 * pix8 * 289 * 64, 4.0 * pix8 * (3 * 64 + 3 * 4 * 32) + 4.0 * G * 289 * 64,
                           s);
            hipLaunchKernelGGL(k_icnet_highres_wgrad<64>, dim3(G, 3), dim3(256), 0, s, ws.a2, ws.gz3, N, h8, w8, ws.part);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        e = highres_fold(G, 32, 64, scale, s3, params + off.k3, stats + 128, stats + 192, ws, grad + off.k3, grad + off.g3,
                         grad + off.b3, s);
        if (e != hipSuccess) return e;
    }
    {
        const long tiles = (long)N * icnet_cdiv(h8, HX_TH) * icnet_cdiv(w8, HX_TW);
        ProfScope prof("k_icnet_highres_dx<64>", 2.0 * pix8 * 9 * 64 * 32, 4.0 * (pix8 * 64 + 2.0 * pix4 * 32), s);
        hipLaunchKernelGGL(k_icnet_highres_dx<64>, dim3(icnet_grid(tiles, HR_DX_MAX_WG, max_workgroups)), dim3(256), 0, s,
                           ws.gz3, params + off.k3, s3, ws.a2, N, h8, w8, ws.gz2);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    {
        const int G = icnet_grid(wt2, HR_MAX_WG, max_workgroups);
        {
            ProfScope prof("k_icnet_highres_wgrad<32>", 2.0 * pix4 * 289 * 32, 4.0 * pix4 * (3 * 32 + 3 * 4 * 32) + 4.0 * G * 289 * 32,
                           s);
            hipLaunchKernelGGL(k_icnet_highres_wgrad<32>, dim3(G, 3), dim3(256), 0, s, ws.a1, ws.gz2, N, h4, w4, ws.part);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        e = highres_fold(G, 32, 32, scale, s2, params + off.k2, stats + 64, stats + 96, ws, grad + off.k2, grad + off.g2,
                         grad + off.b2, s);
        if (e != hipSuccess) return e;
    }
    {
        const long tiles = (long)N * icnet_cdiv(h4, HX_TH) * icnet_cdiv(w4, HX_TW);
        ProfScope prof("k_icnet_highres_dx<32>", 2.0 * pix4 * 9 * 32 * 32, 4.0 * (pix4 * 32 + 2.0 * pix2 * 32), s);
        hipLaunchKernelGGL(k_icnet_highres_dx<32>, dim3(icnet_grid(tiles, HR_DX_MAX_WG, max_workgroups)), dim3(256), 0, s,
                           ws.gz2, params + off.k2, s2, ws.a1, N, h4, w4, ws.gz1);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const int G = icnet_grid(icnet_cdiv((long)N * h2 * w2, 256), HR_MAX_WG, max_workgroups);
    {
        ProfScope prof("k_icnet_highres_wgrad1", 2.0 * pix2 * (9 * c_in + 1) * 32,
                       4.0 * pix2 * 32 + (double)N * H * W * c_in * (x_is_u8 ? 1.0 : 4.0) + 4.0 * G * (9 * c_in + 1) * 32, s);
#define SSAL_HR_W1(C)                                                                                                         \
    case C:                                                                                                                   \
        if (x_is_u8)                                                                                                          \
            hipLaunchKernelGGL((k_icnet_highres_wgrad1<C, uint8_t>), dim3(G), dim3(256), 0, s, (const uint8_t *)x, ws.gz1, N, \
                               h2, w2, ws.part);                                                                              \
        else                                                                                                                  \
            hipLaunchKernelGGL((k_icnet_highres_wgrad1<C, float>), dim3(G), dim3(256), 0, s, (const float *)x, ws.gz1, N, h2,  \
                               w2, ws.part);                                                                                  \
        break;
        switch (c_in) {
            SSAL_HR_W1(3) SSAL_HR_W1(4)
        default:
            return hipErrorInvalidValue;
        }
#undef SSAL_HR_W1
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return highres_fold(G, c_in, 32, scale, s1, params + off.k1, stats, stats + 32, ws, grad + off.k1, grad + off.g1,
                        grad + off.b1, s);
}

}  // namespace ssal
