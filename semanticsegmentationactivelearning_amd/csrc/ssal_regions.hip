// ssal_regions.hip -- region-level acquisition on the device (include/ssal_enet.h, "Region scores" section), gfx950.
//
// k_reduce_regions      tile partials of the fused score pass -> region means: one thread per region, tiles in row-major
//                       order (ssal_regions.h: tile form).  Reads n * tiles doubles (131 KB at 8 x 1024 x 2048).
// k_region_means_plane  fp32 confidence plane [n, h, w] -> region means (ssal_regions.h: plane form).  HBM-bound: the plane
//                       is read once, 16 bytes per lane where the rows are 16-byte aligned.  A workgroup of 16 waves owns
//                       one region row (rh plane rows) of 64 / G adjacent regions, G = region_lanes(rw) lanes per region:
//                       a wave reads 64 / G regions x one plane row per step (one contiguous span of the row when rw is
//                       a multiple of 4), wave v takes the rows v, v + 16, .. of a 64-row chunk, four rows in flight.
//                       The row partials of a chunk go through LDS as rows[row][region] (a wave stores, and the folding
//                       thread of a region reads, consecutive doubles: no bank conflict), and thread t < 64 / G adds the
//                       rows of region t top to bottom.  No floating-point atomics, no dependence on the grid.
//
// The stand-alone entry points, the region sibling of ssal_score_logits_nhwc and the host twin live here as well; the
// whole-network entries are next to their score entries (ssal_api.hip, ssal_icnet_api.hip).
#include "../../include/ssal_enet.h"
#include "ssal_host.h"
#include "ssal_internal.h"
#include "ssal_prof.h"
#include "ssal_regions.h"

namespace ssal {

__global__ __launch_bounds__(256) void k_reduce_regions(const double *__restrict__ partial, int N, int h, int w, int rh,
                                                        int rw, int RY, int RX, double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t per = (int64_t)RY * RX;
    if (t >= (int64_t)N * per) return;
    const int n = (int)(t / per), ry = (int)((t % per) / RX), rx = (int)(t % RX);
    const int tiles_y = region_cdiv(h, kRegionTile), tiles_x = region_cdiv(w, kRegionTile);
    out[t] = region_mean_tiles(partial + (int64_t)n * tiles_y * tiles_x, tiles_y, tiles_x, h, w, rh, rw, ry, rx);
}

hipError_t launch_reduce_regions(const double *partial, int N, int h, int w, int rh, int rw, double *out, hipStream_t s)
{
    const int RY = region_cdiv(h, rh), RX = region_cdiv(w, rw);
    const int64_t total = (int64_t)N * RY * RX;
    const int tiles = region_cdiv(h, kRegionTile) * region_cdiv(w, kRegionTile);
    ProfScope prof("k_reduce_regions", (double)N * tiles, 8.0 * N * tiles + 8.0 * total, s);
    hipLaunchKernelGGL(k_reduce_regions, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, partial, N, h, w, rh, rw,
                       RY, RX, out);
    return hipGetLastError();
}

constexpr int RP_WAVES = 16, RP_THREADS = 64 * RP_WAVES, RP_CHUNK = 64, RP_ROWS = RP_CHUNK / RP_WAVES;

// workgroups of one launch: n * RY * ceil(RX / (64 / G)) in a one-dimensional grid
static int64_t region_plane_blocks(int n, int h, int w, int rh, int rw)
{
    const int per = kRegionLanesMax / region_lanes(rw);
    return (int64_t)n * region_cdiv(h, rh) * region_cdiv(region_cdiv(w, rw), per);
}

// the kernel addresses the planes with 64-bit offsets; what it cannot take is a grid beyond 2^31 - 1 workgroups
bool region_plane_fits(int n, int h, int w, int rh, int rw) { return region_plane_blocks(n, h, w, rh, rw) <= 0x7fffffffll; }

template <bool VEC>
__global__ __launch_bounds__(RP_THREADS) void k_region_means_plane(const float *__restrict__ plane, int h, int w, int rh,
                                                                   int rw, int RY, int RX, int G, int BX,
                                                                   double *__restrict__ out)
{
    __shared__ double rows[RP_CHUNK][kRegionLanesMax];
    const int per = kRegionLanesMax / G;  // regions of one workgroup
    const int bx = blockIdx.x % BX, ry = (blockIdx.x / BX) % RY;
    const int64_t n = blockIdx.x / BX / RY;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane / G, gl = lane % G;
    const int rx = bx * per + grp;
    const bool live = rx < RX;
    const int x0 = live ? rx * rw : 0, x1 = live ? x0 + region_extent(rx, rw, w) : 0;
    const int y0 = ry * rh, ny = region_extent(ry, rh, h);
    const float *img = plane + n * h * (int64_t)w;

    // the folding thread of region t (first wave): its region and its running sum
    const int frx = bx * per + (int)threadIdx.x;
    const bool folds = (int)threadIdx.x < per && frx < RX;
    double total = 0.0;

    for (int c = 0; c < ny; c += RP_CHUNK) {
        double v[RP_ROWS];
#pragma unroll
        for (int k = 0; k < RP_ROWS; ++k) {
            const int r = c + wave + RP_WAVES * k;  // wave-uniform
            v[k] = 0.0;
            if (r < ny && live) {
                const float *row = img + (int64_t)(y0 + r) * w;
                if constexpr (VEC) {
                    const int q1 = (x1 - 1) / 4;
                    for (int q = x0 / 4 + gl; q <= q1; q += G) {  // w % 4 == 0: the whole quad lies inside the row
                        const float4 t = reinterpret_cast<const float4 *>(row)[q];
                        const float e[4] = {t.x, t.y, t.z, t.w};
                        v[k] = region_quad_add(v[k], e, q, x0, x1);
                    }
                } else {
                    v[k] = region_lane_sum(row, x0, x1, gl, G);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < RP_ROWS; ++k) {
            for (int d = 1; d < G; d *= 2) v[k] += __shfl_xor(v[k], d, 64);  // every lane of the wave takes part
            const int r = wave + RP_WAVES * k;
            if (gl == 0 && live && c + r < ny) rows[r][grp] = v[k];
        }
        __syncthreads();
        if (folds) {
            const int nr = ny - c < RP_CHUNK ? ny - c : RP_CHUNK;
            for (int r = 0; r < nr; ++r) total += rows[r][threadIdx.x];
        }
        __syncthreads();
    }
    if (folds)
        out[(n * RY + ry) * RX + frx] = total / ((double)ny * (double)region_extent(frx, rw, w));
}

hipError_t launch_region_means_plane(const float *plane, int n, int h, int w, int rh, int rw, double *out, hipStream_t s)
{
    if (!region_plane_fits(n, h, w, rh, rw)) return hipErrorInvalidValue;
    const int RY = region_cdiv(h, rh), RX = region_cdiv(w, rw), G = region_lanes(rw);
    const int BX = region_cdiv(RX, kRegionLanesMax / G);
    const unsigned blocks = (unsigned)region_plane_blocks(n, h, w, rh, rw);
    ProfScope prof("k_region_means_plane", (double)n * h * w, 4.0 * n * h * w + 8.0 * n * RY * RX, s);
    // 16-byte loads need every row to start on a 16-byte boundary
    if (w % 4 == 0 && ((uintptr_t)plane & 15) == 0)
        hipLaunchKernelGGL((k_region_means_plane<true>), dim3(blocks), dim3(RP_THREADS), 0, s, plane, h, w, rh, rw, RY, RX,
                           G, BX, out);
    else
        hipLaunchKernelGGL((k_region_means_plane<false>), dim3(blocks), dim3(RP_THREADS), 0, s, plane, h, w, rh, rw, RY, RX,
                           G, BX, out);
    return hipGetLastError();
}

int region_check(int h, int w, int rh, int rw, bool whole_tiles)
{
    if (h <= 0 || w <= 0) return fail(SSAL_EINVAL, "bad dims h=%d w=%d", h, w);
    if (rh <= 0 || rw <= 0) return fail(SSAL_EINVAL, "region size must be positive (got rh=%d rw=%d)", rh, rw);
    if (whole_tiles && (rh % kRegionTile || rw % kRegionTile))
        return fail(SSAL_EINVAL, "the fused region pass needs rh and rw to be multiples of %d (got rh=%d rw=%d): the plane "
                    "route (ssal_region_means_plane) serves other sizes", kRegionTile, rh, rw);
    return SSAL_OK;
}

}  // namespace ssal

using namespace ssal;

SSAL_API int ssal_region_grid(int h, int w, int rh, int rw, int *ry, int *rx)
{
    if (int rc = region_check(h, w, rh, rw, false)) return rc;
    if (!ry || !rx) return fail(SSAL_EINVAL, "ry / rx is NULL");
    *ry = region_cdiv(h, rh);
    *rx = region_cdiv(w, rw);
    return SSAL_OK;
}

SSAL_API int ssal_region_means_plane(const float *plane_dev, int n, int h, int w, int rh, int rw, double *region_scores_dev,
                                     void *stream)
{
    if (n <= 0) return fail(SSAL_EINVAL, "bad dims n=%d h=%d w=%d", n, h, w);
    if (int rc = region_check(h, w, rh, rw, false)) return rc;
    if (!plane_dev || !region_scores_dev) return fail(SSAL_EINVAL, "NULL device pointer");
    if (!region_plane_fits(n, h, w, rh, rw))
        return fail(SSAL_EINVAL, "too many regions for one launch (n=%d h=%d w=%d rh=%d rw=%d): split the batch", n, h, w, rh, rw);
    HIP_TRY(launch_region_means_plane(plane_dev, n, h, w, rh, rw, region_scores_dev, (hipStream_t)stream));
    return SSAL_OK;
}

SSAL_API int ssal_region_reduce_host(int form, const void *in_host, int n, int h, int w, int rh, int rw,
                                     double *region_scores_host, int64_t *counts_host)
{
    if (form != SSAL_REGION_FORM_TILES && form != SSAL_REGION_FORM_PLANE)
        return fail(SSAL_EINVAL, "form must be SSAL_REGION_FORM_TILES (0) or SSAL_REGION_FORM_PLANE (1), got %d", form);
    if (n <= 0) return fail(SSAL_EINVAL, "bad dims n=%d h=%d w=%d", n, h, w);
    if (int rc = region_check(h, w, rh, rw, form == SSAL_REGION_FORM_TILES)) return rc;
    if (!in_host || !region_scores_host) return fail(SSAL_EINVAL, "NULL host pointer");
    const int RY = region_cdiv(h, rh), RX = region_cdiv(w, rw);
    const int tiles_y = region_cdiv(h, kRegionTile), tiles_x = region_cdiv(w, kRegionTile);
    for (int i = 0; i < n; ++i)
        for (int ry = 0; ry < RY; ++ry)
            for (int rx = 0; rx < RX; ++rx) {
                double *o = region_scores_host + ((int64_t)i * RY + ry) * RX + rx;
                if (form == SSAL_REGION_FORM_TILES)
                    *o = region_mean_tiles((const double *)in_host + (int64_t)i * tiles_y * tiles_x, tiles_y, tiles_x, h, w,
                                           rh, rw, ry, rx);
                else
                    *o = region_mean_plane_host((const float *)in_host + (int64_t)i * h * w, h, w, rh, rw, ry, rx);
            }
    if (counts_host)
        for (int ry = 0; ry < RY; ++ry)
            for (int rx = 0; rx < RX; ++rx)
                counts_host[(int64_t)ry * RX + rx] = (int64_t)region_extent(ry, rh, h) * region_extent(rx, rw, w);
    return SSAL_OK;
}

// ---- region sibling of ssal_score_logits_nhwc: the plane route on materialised logits ----
SSAL_API int64_t ssal_score_regions_workspace_bytes(int n, int h, int w)
{
    if (n <= 0 || h <= 0 || w <= 0) return -1;
    // the partials of the plain op, then a confidence plane for callers that do not ask for one
    return ((int64_t)n * score_blocks(h, w) * 8 + 255) / 256 * 256 + (int64_t)n * h * w * 4 + 256;
}

SSAL_API int ssal_score_logits_regions_nhwc(const float *logits_dev, int n, int h, int w, int classes, int measure,
                                            float threshold, int rh, int rw, double *scores_dev, double *region_scores_dev,
                                            uint8_t *label_dev, uint8_t *mask_dev, float *conf_dev, void *ws_dev,
                                            int64_t ws_bytes, void *stream)
{
    if (measure < 0 || measure > 2)
        return fail(SSAL_ENOTIMPL, "Uncertainty function not implemented (measure=%d)", measure);
    if (n <= 0 || h <= 0 || w <= 0) return fail(SSAL_EINVAL, "bad dims n=%d h=%d w=%d", n, h, w);
    if (classes < 2 || classes > 32) return fail(SSAL_EINVAL, "classes must be in [2,32] (got %d)", classes);
    if (int rc = region_check(h, w, rh, rw, false)) return rc;
    if (!logits_dev || !scores_dev || !region_scores_dev || !ws_dev) return fail(SSAL_EINVAL, "NULL device pointer");
    if (!region_plane_fits(n, h, w, rh, rw))
        return fail(SSAL_EINVAL, "too many regions for one launch (n=%d h=%d w=%d rh=%d rw=%d): split the batch", n, h, w, rh, rw);
    if (ws_bytes < ssal_score_regions_workspace_bytes(n, h, w))
        return fail(SSAL_ENOMEM, "workspace too small: need %lld bytes, got %lld",
                    (long long)ssal_score_regions_workspace_bytes(n, h, w), (long long)ws_bytes);
    hipStream_t s = (hipStream_t)stream;
    Bump b(ws_dev, ws_bytes);
    double *partial = b.take<double>((int64_t)n * score_blocks(h, w));
    float *plane = conf_dev ? conf_dev : b.take<float>((int64_t)n * h * w);
    HIP_TRY(launch_score_logits(logits_dev, n, h, w, classes, measure, threshold, partial, label_dev, mask_dev, plane, s));
    HIP_TRY(launch_reduce_mean(partial, n, score_blocks(h, w), (double)h * (double)w, scores_dev, s));
    HIP_TRY(launch_region_means_plane(plane, n, h, w, rh, rw, region_scores_dev, s));
    return SSAL_OK;
}
