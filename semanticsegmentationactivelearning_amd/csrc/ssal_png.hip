// ssal_png.hip -- batch PNG decode on the device (include/ssal_enet.h, "PNG decode" section), gfx950.
//
// k_png_decode: one wave per stream.  The wave inflates the stream's zlib payload (ssal_inflate.h, Huffman tables in LDS,
// wave-uniform decode loop, 64-lane match copies) into its workspace slot, checks the Adler-32 and the size, then
// reconstructs the filtered scanlines in place.  Concurrency comes from the number of streams in one launch: the caller
// keeps hundreds of frames in flight.
// k_png_place: one thread per output pixel of each decoded stream: crop window + optional left-right flip, image channels
// into a uint8 or float32 NHWC batch at the stream's channel offset (+ the channel-scaled image_dist), or the label plane
// through generate_mask (255 -> label 0, mask 0).
//
// The host entry points run the same inflate / unfilter source on the CPU with a single lane.
#include "../../include/ssal_enet.h"
#include "ssal_host.h"
#include "ssal_inflate.h"
#include "ssal_prof.h"

using namespace ssal;
using namespace ssal::png;

namespace {

// descriptor fields (SSAL_PNG_DESC int64 per stream)
enum {
    D_SRC_OFF, D_SRC_LEN, D_WIDTH, D_HEIGHT, D_BPP, D_WS_OFF, D_FRAME, D_ROLE, D_CH_OFF, D_NCH, D_TOP, D_LEFT, D_FLIP
};

struct Geometry {
    int64_t payload_bytes, ws_bytes;
    int frames, out_h, out_w, channels;
};

__host__ __device__ inline int64_t raw_bytes(int64_t w, int64_t h, int64_t bpp) { return h * (1 + w * bpp); }

// every field that addresses memory is checked before a byte is read or written
__host__ __device__ inline bool desc_ok(const int64_t *d, const Geometry &g)
{
    const int64_t w = d[D_WIDTH], h = d[D_HEIGHT], bpp = d[D_BPP];
    if (w < 1 || h < 1 || w > (1 << 24) || h > (1 << 24) || bpp < 1 || bpp > 4) return false;
    if (d[D_SRC_OFF] < 0 || d[D_SRC_LEN] < 0 || d[D_SRC_OFF] > g.payload_bytes - d[D_SRC_LEN]) return false;
    if (d[D_WS_OFF] < 0 || d[D_WS_OFF] > g.ws_bytes - raw_bytes(w, h, bpp)) return false;
    if (d[D_FRAME] < 0 || d[D_FRAME] >= g.frames) return false;
    if (d[D_TOP] < 0 || d[D_LEFT] < 0 || d[D_TOP] > h - g.out_h || d[D_LEFT] > w - g.out_w) return false;
    if (d[D_ROLE] == SSAL_PNG_ROLE_IMAGE) {
        if (d[D_NCH] < 1 || d[D_NCH] > bpp || d[D_CH_OFF] < 0 || d[D_CH_OFF] > g.channels - d[D_NCH]) return false;
    } else if (d[D_ROLE] != SSAL_PNG_ROLE_LABEL) {
        return false;
    }
    return true;
}

__global__ __launch_bounds__(64) void k_png_decode(const uint8_t *__restrict__ payload, const int64_t *__restrict__ desc,
                                                   int64_t n, Geometry g, uint8_t *__restrict__ ws,
                                                   int32_t *__restrict__ status)
{
    __shared__ Tables t;
    __shared__ uint8_t win[kWindow];
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    const int lane = threadIdx.x;
    const int64_t *d = desc + i * SSAL_PNG_DESC;
    int32_t st = ST_UNSUPPORTED;
    if (desc_ok(d, g)) {
        const int64_t expect = raw_bytes(d[D_WIDTH], d[D_HEIGHT], d[D_BPP]);
        uint8_t *raw = ws + d[D_WS_OFF];
        int64_t got = 0;
        st = inflate_zlib(payload + d[D_SRC_OFF], d[D_SRC_LEN], raw, expect, &got, t, win, lane, 64);
        wave_sync();  // the unfilter reads bytes other lanes stored
        if (st == ST_OK && got != expect) st = ST_SIZE;
        if (st == ST_OK) st = unfilter_image(raw, (int)d[D_HEIGHT], (int)d[D_WIDTH], (int)d[D_BPP], lane, 64);
    }
    if (lane == 0) status[i] = st;
}

__global__ __launch_bounds__(256) void k_png_place(const int64_t *__restrict__ desc, Geometry g,
                                                   const uint8_t *__restrict__ ws, const int32_t *__restrict__ status,
                                                   const float *__restrict__ scale, uint8_t *__restrict__ img_u8,
                                                   float *__restrict__ img_f32, float *__restrict__ img_dist,
                                                   uint8_t *__restrict__ label, uint8_t *__restrict__ mask)
{
    const int64_t i = blockIdx.y;
    if (status[i] != ST_OK) return;
    const int64_t *d = desc + i * SSAL_PNG_DESC;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)g.out_h * g.out_w) return;
    const int y = (int)(p / g.out_w), x = (int)(p % g.out_w);
    const int64_t bpp = d[D_BPP];
    const int64_t sx = d[D_FLIP] ? d[D_LEFT] + g.out_w - 1 - x : d[D_LEFT] + x;
    const uint8_t *src = ws + d[D_WS_OFF] + (d[D_TOP] + y) * (1 + d[D_WIDTH] * bpp) + 1 + sx * bpp;
    const int64_t frame = d[D_FRAME];
    const int64_t pix = (frame * g.out_h + y) * g.out_w + x;
    if (d[D_ROLE] == SSAL_PNG_ROLE_LABEL) {  // generate_mask: 255 -> label 0, mask 0
        const uint8_t v = src[0];
        if (label) label[pix] = v == 255 ? (uint8_t)0 : v;
        if (mask) mask[pix] = v == 255 ? (uint8_t)0 : (uint8_t)1;
        return;
    }
    const float k = 0x1.010102p-8f;  // float32(1 / 255): tf.image.convert_image_dtype
    const int nch = (int)d[D_NCH], c0 = (int)d[D_CH_OFF];
    for (int c = 0; c < nch; ++c) {
        const uint8_t v = src[c];
        const int64_t o = pix * g.channels + c0 + c;
        const float f = (float)v * k;
        if (img_u8) img_u8[o] = v;
        if (img_f32) img_f32[o] = f;
        if (img_dist) {  // clip(image * scale, 0, 1): a separate fp32 multiply (the library builds with -ffp-contract=off)
            const float s = f * scale[frame * g.channels + c0 + c];
            img_dist[o] = fminf(fmaxf(s, 0.0f), 1.0f);
        }
    }
}

}  // namespace

SSAL_API int64_t ssal_png_plan(int64_t n_streams, int64_t *desc_host)
{
    if (n_streams < 0 || (n_streams > 0 && !desc_host)) return -1;
    int64_t off = 0;
    for (int64_t i = 0; i < n_streams; ++i) {
        int64_t *d = desc_host + i * SSAL_PNG_DESC;
        const int64_t w = d[D_WIDTH], h = d[D_HEIGHT], bpp = d[D_BPP];
        if (w < 1 || h < 1 || w > (1 << 24) || h > (1 << 24) || bpp < 1 || bpp > 4) return -1;
        d[D_WS_OFF] = off;
        off += (raw_bytes(w, h, bpp) + 255) & ~(int64_t)255;
    }
    return off + 256;
}

SSAL_API int ssal_png_decode_nhwc(const uint8_t *payload_dev, int64_t payload_bytes, const int64_t *desc_dev,
                                  int64_t n_streams, int frames, int height, int width, int channels,
                                  const float *scale_dev, void *image_dev, int image_f32, float *image_dist_dev,
                                  uint8_t *label_dev, uint8_t *mask_dev, int32_t *status_dev, void *ws_dev,
                                  int64_t ws_bytes, void *stream)
{
    if (n_streams < 0 || n_streams > (1 << 20)) return fail(SSAL_EINVAL, "bad stream count %lld", (long long)n_streams);
    if (frames < 1 || height < 1 || width < 1 || channels < 1 || channels > 16)
        return fail(SSAL_EINVAL, "bad output geometry %dx%dx%dx%d", frames, height, width, channels);
    if (payload_bytes < 0 || ws_bytes < 0) return fail(SSAL_EINVAL, "negative extent");
    if (n_streams == 0) return SSAL_OK;
    if (!payload_dev || !desc_dev || !status_dev || !ws_dev) return fail(SSAL_EINVAL, "NULL device pointer");
    if (image_dist_dev && !scale_dev) return fail(SSAL_EINVAL, "image_dist needs the channel scales");
    hipStream_t s = (hipStream_t)stream;
    Geometry g{payload_bytes, ws_bytes, frames, height, width, channels};
    {
        ProfScope prof("k_png_decode", 0.0, (double)payload_bytes, s);
        hipLaunchKernelGGL(k_png_decode, dim3((unsigned)n_streams), dim3(64), 0, s, payload_dev, desc_dev, n_streams, g,
                           (uint8_t *)ws_dev, status_dev);
        HIP_TRY(hipGetLastError());
    }
    const int64_t px = (int64_t)height * width;
    ProfScope prof("k_png_place", 0.0, (double)px * n_streams * 2, s);
    hipLaunchKernelGGL(k_png_place, dim3((unsigned)((px + 255) / 256), (unsigned)n_streams), dim3(256), 0, s, desc_dev, g,
                       (const uint8_t *)ws_dev, status_dev, scale_dev, image_f32 ? nullptr : (uint8_t *)image_dev,
                       image_f32 ? (float *)image_dev : nullptr, image_dist_dev, label_dev, mask_dev);
    HIP_TRY(hipGetLastError());
    return SSAL_OK;
}

SSAL_API int ssal_inflate_host(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_cap, int64_t *out_len,
                               int32_t *status)
{
    if (in_len < 0 || out_cap < 0 || (in_len && !in) || (out_cap && !out) || !status)
        return fail(SSAL_EINVAL, "bad buffer");
    Tables t;
    std::vector<uint8_t> win(kWindow);
    *status = inflate_zlib(in, in_len, out, out_cap, out_len, t, win.data(), 0, 1);
    return SSAL_OK;
}

SSAL_API int ssal_png_unfilter_host(uint8_t *raw, int height, int width, int bpp, int32_t *status)
{
    if (!raw || !status || height < 1 || width < 1 || bpp < 1 || bpp > 4) return fail(SSAL_EINVAL, "bad image");
    *status = unfilter_image(raw, height, width, bpp, 0, 1);
    return SSAL_OK;
}
