// ssal_predict.hip -- test-split prediction on the device (include/ssal_enet.h, "Prediction" section), gfx950.
//
// k_resize_argmax  logits [N,H,W,K] fp32 -> uint8 [N,OH,OW] (train id, or the id through a 256-entry table) or
//                  uint8 [N,OH,OW,3] (RGB through a [256][3] table): tf.image.resize_bilinear of the logits (the mapping and
//                  the lerp expression of k_resize_bilinear in ssal_kernels.hip, so the same bits under -ffp-contract=off)
//                  and the first maximum over the classes, per output pixel, in registers.  The resized logits never reach
//                  HBM and there is no workspace.  One output pixel per thread, a workgroup owns a 32 x 8 output tile (a wave
//                  = two rows of 32).  The classes run in chunks of four (16 neighbour values live, K is a run-time count:
//                  one instantiation per form, no register array, no scratch).  Three forms, chosen by the launcher:
//                  PR_STAGED (an enlargement or the identity, where the threads of a tile share their source pixels): the
//                  tile's source footprint goes into LDS first, each footprint row one contiguous run of the image read
//                  with coalesced 4-byte loads, and the four neighbours are read from there (pixel stride K words: odd K
//                  is conflict-free, lanes with the same source pixel broadcast); PR_DIRECT / PR_DIRECT16 (a reduction:
//                  nothing is shared): the four source pixels are read straight from global memory, PR_DIRECT16 with one
//                  16-byte load per neighbour and chunk, which needs K % 4 == 0 and a 16-byte aligned tensor; everything
//                  else (K = 19: a 76-byte pixel stride; views that start inside an allocation) takes the 4-byte form.
// k_label_lut      uint8 [pixels] -> uint8 [pixels] or [pixels][3] through the same tables: the tail of the path without a
//                  resize, where the label plane already comes from the fused score kernel.  Four pixels per thread (one
//                  4-byte load, one or three 4-byte stores) where both planes are 4-byte aligned, bytes otherwise.
// All offsets are 64-bit; the one limit is a one-dimensional grid (predict_fits), judged by the entry before any launch.
#include "../../include/ssal_enet.h"
#include "ssal_host.h"
#include "ssal_internal.h"
#include "ssal_prof.h"

namespace ssal {

constexpr int PR_TW = 32, PR_TH = 8;  // output tile of one 256-thread workgroup

static int64_t predict_blocks(int n, int oh, int ow)
{
    return (int64_t)n * ((oh + PR_TH - 1) / PR_TH) * ((ow + PR_TW - 1) / PR_TW);
}

bool predict_fits(int n, int oh, int ow) { return predict_blocks(n, oh, ow) <= 0x7fffffffll; }

// lut == NULL: the train id; ch == 1: lut[id]; ch == 3: lut[id][0..2]
__device__ __forceinline__ void predict_store(uint8_t *__restrict__ out, int64_t pix, int label,
                                              const uint8_t *__restrict__ lut, int ch)
{
    if (ch == 3) {
        const uint8_t *e = lut + 3 * label;
        uint8_t *o = out + 3 * pix;
        o[0] = e[0];
        o[1] = e[1];
        o[2] = e[2];
    } else {
        out[pix] = lut ? lut[label] : (uint8_t)label;
    }
}

enum : int { PR_DIRECT = 0, PR_DIRECT16 = 1, PR_STAGED = 2 };

// the source footprint of one output tile along one axis: floor(b) - floor(a) <= floor(b - a) + 1 for the first and last
// source coordinate a <= b = a + (T - 1) * scale, one more pixel for the "+ 1" neighbour and one to count both ends, so
// floor((T - 1) * scale) + 3 in exact arithmetic; one more for products that round across an integer
static int predict_extent(int t, float scale) { return (int)floorf((float)(t - 1) * scale) + 4; }

template <int FORM>
__global__ __launch_bounds__(256) void k_resize_argmax(const float *__restrict__ x, int H, int W, int K, int OH, int OW,
                                                       int BX, int BY, float hs, float ws, const uint8_t *__restrict__ lut,
                                                       int ch, uint8_t *__restrict__ out)
{
    extern __shared__ float tile[];  // PR_STAGED: the tile's source footprint [FH][FW][K]
    constexpr bool VEC = FORM == PR_DIRECT16;
    const int bx = blockIdx.x % BX, by = (blockIdx.x / BX) % BY;
    const int64_t n = blockIdx.x / BX / BY;
    const int ox = bx * PR_TW + (threadIdx.x & (PR_TW - 1)), oy = by * PR_TH + (threadIdx.x / PR_TW);
    const float *img = x + n * H * (int64_t)W * K;
    // oy * (H / OH) < H in exact arithmetic; the min keeps a product that rounds up to H (OH beyond 2^24) inside the tensor
    auto src_y = [&](int o) { return min((int)floorf((float)o * hs), H - 1); };
    auto src_x = [&](int o) { return min((int)floorf((float)o * ws), W - 1); };
    int sy0 = 0, sx0 = 0, FW = W;  // origin and row length (pixels) of what ptl .. pbr index: the image, or the footprint
    const float *base = img;
    if constexpr (FORM == PR_STAGED) {
        // rows sy0 .. sy1 and columns sx0 .. sx1 hold every neighbour of the tile (the mapping is monotonic); a footprint
        // row is FW * K contiguous floats in the image: coalesced 4-byte loads, whatever K and the alignment are
        const int oyb = min(by * PR_TH + PR_TH, OH) - 1, oxb = min(bx * PR_TW + PR_TW, OW) - 1;
        sy0 = src_y(by * PR_TH);
        sx0 = src_x(bx * PR_TW);
        const int sy1 = min(src_y(oyb) + 1, H - 1), sx1 = min(src_x(oxb) + 1, W - 1);
        FW = sx1 - sx0 + 1;
        const int row = FW * K;
        for (int r = 0; r <= sy1 - sy0; ++r) {
            const float *src = img + ((int64_t)(sy0 + r) * W + sx0) * K;
            for (int i = threadIdx.x; i < row; i += 256) tile[r * row + i] = src[i];
        }
        __syncthreads();
        base = tile;
    }
    if (ox >= OW || oy >= OH) return;
    const float fy = (float)oy * hs, fx = (float)ox * ws;
    const int y0 = src_y(oy), x0 = src_x(ox);
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float *ptl = base + ((int64_t)(y0 - sy0) * FW + (x0 - sx0)) * K, *ptr = base + ((int64_t)(y0 - sy0) * FW + (x1 - sx0)) * K;
    const float *pbl = base + ((int64_t)(y1 - sy0) * FW + (x0 - sx0)) * K, *pbr = base + ((int64_t)(y1 - sy0) * FW + (x1 - sx0)) * K;
    auto lerp = [&](float tl, float tr, float bl, float br) {
        const float top = tl + (tr - tl) * lx;
        const float bot = bl + (br - bl) * lx;
        return top + (bot - top) * ly;
    };
    float best = lerp(ptl[0], ptr[0], pbl[0], pbr[0]);
    int label = 0;
    auto take = [&](float v, int k) {
        if (v > best) {  // first maximum: the lowest class wins a tie (ssal_score.h)
            best = v;
            label = k;
        }
    };
    int k = 0;
    for (; k + 4 <= K; k += 4) {
        float4 tl, tr, bl, br;
        if constexpr (VEC) {
            tl = *reinterpret_cast<const float4 *>(ptl + k);
            tr = *reinterpret_cast<const float4 *>(ptr + k);
            bl = *reinterpret_cast<const float4 *>(pbl + k);
            br = *reinterpret_cast<const float4 *>(pbr + k);
        } else {
            tl = make_float4(ptl[k], ptl[k + 1], ptl[k + 2], ptl[k + 3]);
            tr = make_float4(ptr[k], ptr[k + 1], ptr[k + 2], ptr[k + 3]);
            bl = make_float4(pbl[k], pbl[k + 1], pbl[k + 2], pbl[k + 3]);
            br = make_float4(pbr[k], pbr[k + 1], pbr[k + 2], pbr[k + 3]);
        }
        take(lerp(tl.x, tr.x, bl.x, br.x), k);  // k == 0 compares class 0 with itself: no change
        take(lerp(tl.y, tr.y, bl.y, br.y), k + 1);
        take(lerp(tl.z, tr.z, bl.z, br.z), k + 2);
        take(lerp(tl.w, tr.w, bl.w, br.w), k + 3);
    }
    for (; k < K; ++k) take(lerp(ptl[k], ptr[k], pbl[k], pbr[k]), k);
    predict_store(out, (n * OH + oy) * (int64_t)OW + ox, label, lut, ch);
}

hipError_t launch_resize_argmax(const float *logits, int n, int h, int w, int k, int oh, int ow, const uint8_t *lut, int ch,
                                uint8_t *out, hipStream_t s)
{
    if (!predict_fits(n, oh, ow)) return hipErrorInvalidValue;
    const int BX = (ow + PR_TW - 1) / PR_TW, BY = (oh + PR_TH - 1) / PR_TH;
    const unsigned blocks = (unsigned)predict_blocks(n, oh, ow);
    const float hs = (float)h / (float)oh, ws = (float)w / (float)ow;
    const double px = (double)n * oh * ow;
    ProfScope prof("k_resize_argmax", 9.0 * px * k, 4.0 * n * h * w * k + px * (ch == 3 ? 3 : 1), s);
    // an enlargement (or the identity) reads every source pixel from several threads of a tile: stage the footprint
    // (at most 11 x 35 pixels x 32 classes = 49 280 bytes); a reduction shares nothing, its threads read for themselves
    if (hs <= 1.0f && ws <= 1.0f) {
        const size_t lds = (size_t)predict_extent(PR_TH, hs) * predict_extent(PR_TW, ws) * k * sizeof(float);
        hipLaunchKernelGGL((k_resize_argmax<PR_STAGED>), dim3(blocks), dim3(256), lds, s, logits, h, w, k, oh, ow, BX, BY, hs,
                           ws, lut, ch, out);
    } else if (k % 4 == 0 && ((uintptr_t)logits & 15) == 0) {
        // 16-byte loads need every pixel's class vector to start on a 16-byte boundary
        hipLaunchKernelGGL((k_resize_argmax<PR_DIRECT16>), dim3(blocks), dim3(256), 0, s, logits, h, w, k, oh, ow, BX, BY, hs,
                           ws, lut, ch, out);
    } else {
        hipLaunchKernelGGL((k_resize_argmax<PR_DIRECT>), dim3(blocks), dim3(256), 0, s, logits, h, w, k, oh, ow, BX, BY, hs,
                           ws, lut, ch, out);
    }
    return hipGetLastError();
}

__device__ __forceinline__ uint32_t lut4(const uint8_t *__restrict__ lut, uint32_t ids, int stride, int c)
{
    return (uint32_t)lut[(ids & 255u) * stride + c] | (uint32_t)lut[((ids >> 8) & 255u) * stride + c] << 8 |
           (uint32_t)lut[((ids >> 16) & 255u) * stride + c] << 16 | (uint32_t)lut[(ids >> 24) * stride + c] << 24;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_label_lut(const uint8_t *__restrict__ label, int64_t pixels,
                                                   const uint8_t *__restrict__ lut, int ch, uint8_t *__restrict__ out)
{
    const int64_t step = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t done = 0;
    if constexpr (VEC) {
        const int64_t quads = pixels / 4;
        for (int64_t q = t0; q < quads; q += step) {
            const uint32_t ids = reinterpret_cast<const uint32_t *>(label)[q];
            if (ch == 3) {
                // bytes 12 q .. 12 q + 11 = (r g b) of the four pixels, as three little-endian words
                const uint32_t r = lut4(lut, ids, 3, 0), g = lut4(lut, ids, 3, 1), b = lut4(lut, ids, 3, 2);
                uint32_t *o = reinterpret_cast<uint32_t *>(out) + 3 * q;
                o[0] = (r & 255u) | (g & 255u) << 8 | (b & 255u) << 16 | (r & 0xff00u) << 16;
                o[1] = ((g >> 8) & 255u) | ((b >> 8) & 255u) << 8 | (r & 0xff0000u) | (g & 0xff0000u) << 8;
                o[2] = ((b >> 16) & 255u) | (r >> 24) << 8 | (g >> 24) << 16 | (b >> 24) << 24;
            } else {
                reinterpret_cast<uint32_t *>(out)[q] = lut ? lut4(lut, ids, 1, 0) : ids;
            }
        }
        done = quads * 4;
    }
    for (int64_t p = done + t0; p < pixels; p += step) predict_store(out, p, label[p], lut, ch);
}

hipError_t launch_label_lut(const uint8_t *label, int64_t pixels, const uint8_t *lut, int ch, uint8_t *out, hipStream_t s)
{
    const bool vec = (((uintptr_t)label | (uintptr_t)out) & 3) == 0 && pixels >= 4;
    const int64_t items = vec ? pixels / 4 : pixels;
    int64_t blocks = (items + 255) / 256;
    if (blocks > 8192) blocks = 8192;  // grid-stride beyond that: 32 workgroups per CU
    ProfScope prof("k_label_lut", 0.0, (double)pixels * (1 + ch), s);
    if (vec)
        hipLaunchKernelGGL((k_label_lut<true>), dim3((unsigned)blocks), dim3(256), 0, s, label, pixels, lut, ch, out);
    else
        hipLaunchKernelGGL((k_label_lut<false>), dim3((unsigned)blocks), dim3(256), 0, s, label, pixels, lut, ch, out);
    return hipGetLastError();
}

// SSAL_OK, or SSAL_EINVAL with the message set: lut_channels in {0, 1, 3}, and a table exactly when it is not 0
static int lut_check(const uint8_t *lut_dev, int lut_channels)
{
    if (lut_channels != 0 && lut_channels != 1 && lut_channels != 3)
        return fail(SSAL_EINVAL, "lut_channels must be 0 (train ids), 1 (id table) or 3 (colour table), got %d", lut_channels);
    if (lut_channels == 0 && lut_dev) return fail(SSAL_EINVAL, "lut_channels is 0 but a table was given");
    if (lut_channels != 0 && !lut_dev) return fail(SSAL_EINVAL, "lut_channels is %d but lut_dev is NULL", lut_channels);
    return SSAL_OK;
}

}  // namespace ssal

using namespace ssal;

SSAL_API int ssal_predict_logits_nhwc(const float *logits_dev, int n, int h, int w, int classes, int oh, int ow,
                                      const uint8_t *lut_dev, int lut_channels, uint8_t *out_dev, void *stream)
{
    if (n <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0)
        return fail(SSAL_EINVAL, "bad dims n=%d h=%d w=%d oh=%d ow=%d", n, h, w, oh, ow);
    if (classes < 2 || classes > 32) return fail(SSAL_EINVAL, "classes must be in [2,32] (got %d)", classes);
    if (int rc = lut_check(lut_dev, lut_channels)) return rc;
    if (!logits_dev || !out_dev) return fail(SSAL_EINVAL, "NULL device pointer");
    if (!predict_fits(n, oh, ow))
        return fail(SSAL_EINVAL, "too many output tiles for one launch (n=%d oh=%d ow=%d): split the batch", n, oh, ow);
    HIP_TRY(launch_resize_argmax(logits_dev, n, h, w, classes, oh, ow, lut_dev, lut_channels, out_dev, (hipStream_t)stream));
    return SSAL_OK;
}

SSAL_API int ssal_label_lut(const uint8_t *label_dev, int64_t pixels, const uint8_t *lut_dev, int lut_channels,
                            uint8_t *out_dev, void *stream)
{
    if (pixels <= 0 || pixels > INT64_MAX / 4) return fail(SSAL_EINVAL, "bad pixel count %lld", (long long)pixels);
    if (int rc = lut_check(lut_dev, lut_channels)) return rc;
    if (!label_dev || !out_dev) return fail(SSAL_EINVAL, "NULL device pointer");
    HIP_TRY(launch_label_lut(label_dev, pixels, lut_dev, lut_channels, out_dev, (hipStream_t)stream));
    return SSAL_OK;
}
