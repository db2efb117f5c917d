// ssal_regions.h -- region-level acquisition: the reduction core shared by the device kernels (k_reduce_regions,
// k_region_means_plane; ssal_regions.hip) and the host twin behind ssal_region_reduce_host.  Written as
// __host__ __device__ code so the CPU tests run the very source the kernels run.  gfx950 only on the device side.
//
// Terms: a region is a window of rh x rw output pixels on a grid anchored at pixel (0, 0); the grid has
// RY = ceil(h / rh) by RX = ceil(w / rw) regions, the bottom row / right column may be clipped.  The region score is the
// mean of the per-pixel confidence over the region's pixels inside the frame, accumulated in float64 in a FIXED order:
//
//   tile form  (input: one float64 sum per T x T pixel tile, row-major tiles -- what the fused score pass leaves in its
//               `partial` buffer, T = 32): rh and rw are multiples of T; a region adds its tiles in row-major tile order,
//               starting from 0.0, and divides by the clipped pixel count.
//   plane form (input: fp32 confidence plane [h, w]): row partials first, then rows top to bottom.  The row partial of
//               row y over columns [x0, x1) is folded by G "lanes", G = region_lanes(rw), a power of two <= 64 that depends
//               on rw only: the row's 4-pixel quads are counted from the frame's column 0 (quad q = columns 4q .. 4q + 3),
//               lane l owns quads q0 + l, q0 + l + G, ... (q0 = x0 / 4) and adds their in-range pixels left to right into
//               a float64 that starts at 0.0; the G lane sums are then folded by the butterfly v[l] += v[l ^ d],
//               d = 1, 2, .. G / 2.  The region sum adds the row partials top to bottom, starting from 0.0.
//
// Neither order knows the batch size, the image-group chain a frame ran on, a knob, or how a pointer is aligned (the
// 16-byte loads of the kernel fetch whole quads; the scalar path adds the same pixels to the same lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ssal {

constexpr int kRegionTile = 32;   // output pixels per side of one k_final_score workgroup (2 * FS_T)
constexpr int kRegionLanesMax = 64;

__host__ __device__ inline int region_cdiv(int a, int b) { return (a + b - 1) / b; }

// pixels of region index r (size step) inside an axis of length len
__host__ __device__ inline int region_extent(int r, int step, int len)
{
    const int64_t a = (int64_t)r * step, b = a + step;
    return (int)((b < len ? b : len) - a);
}

// lanes that fold one row of a region: the smallest power of two that holds every quad a row of rw pixels can touch
// (a row that starts inside a quad touches one more), at most 64 -- wider rows stride over the lanes
__host__ __device__ inline int region_lanes(int rw)
{
    if (rw >= 4 * kRegionLanesMax) return kRegionLanesMax;
    const int quads = (rw % 4 == 0) ? rw / 4 : (rw + 2) / 4 + 1;
    int g = 1;
    while (g < quads && g < kRegionLanesMax) g *= 2;
    return g;
}

// acc += the pixels of quad `q` (columns 4q .. 4q + 3, values v[0..3]) that lie in [x0, x1), left to right
__host__ __device__ inline double region_quad_add(double acc, const float v[4], int q, int x0, int x1)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = 4 * q + k;
        if (x >= x0 && x < x1) acc += (double)v[k];
    }
    return acc;
}

// lane `lane` of G: its share of row[x0 .. x1) (scalar loads; the kernel's 16-byte path adds the same pixels)
__host__ __device__ inline double region_lane_sum(const float *row, int x0, int x1, int lane, int G)
{
    double acc = 0.0;
    const int q1 = (x1 - 1) / 4;
    for (int q = x0 / 4 + lane; q <= q1; q += G) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = 4 * q + k;
            v[k] = (x >= x0 && x < x1) ? row[x] : 0.0f;
        }
        acc = region_quad_add(acc, v, q, x0, x1);
    }
    return acc;
}

// tile form: the sum of the tiles [ty0, ty1) x [tx0, tx1) of part[tiles_y][tiles_x], row-major
__host__ __device__ inline double region_tile_sum(const double *part, int tiles_x, int ty0, int ty1, int tx0, int tx1)
{
    double acc = 0.0;
    for (int ty = ty0; ty < ty1; ++ty)
        for (int tx = tx0; tx < tx1; ++tx) acc += part[(int64_t)ty * tiles_x + tx];
    return acc;
}

// one region of the tile form: mean over the clipped region (ry, rx); th / tw = tiles per region side
__host__ __device__ inline double region_mean_tiles(const double *part, int tiles_y, int tiles_x, int h, int w, int rh, int rw,
                                                    int ry, int rx)
{
    const int th = rh / kRegionTile, tw = rw / kRegionTile;
    const int ty1 = (ry + 1) * th < tiles_y ? (ry + 1) * th : tiles_y;
    const int tx1 = (rx + 1) * tw < tiles_x ? (rx + 1) * tw : tiles_x;
    const double count = (double)region_extent(ry, rh, h) * (double)region_extent(rx, rw, w);
    return region_tile_sum(part, tiles_x, ry * th, ty1, rx * tw, tx1) / count;
}

// host twin of the plane form (the kernel folds the lanes with wave shuffles; this walks the same butterfly)
inline double region_row_partial_host(const float *row, int x0, int x1, int G)
{
    double v[kRegionLanesMax], t[kRegionLanesMax];
    for (int l = 0; l < G; ++l) v[l] = region_lane_sum(row, x0, x1, l, G);
    for (int d = 1; d < G; d *= 2) {
        for (int l = 0; l < G; ++l) t[l] = v[l] + v[l ^ d];
        for (int l = 0; l < G; ++l) v[l] = t[l];
    }
    return v[0];
}

inline double region_mean_plane_host(const float *plane, int h, int w, int rh, int rw, int ry, int rx)
{
    const int G = region_lanes(rw);
    const int y0 = ry * rh, ny = region_extent(ry, rh, h), x0 = rx * rw, nx = region_extent(rx, rw, w);
    double acc = 0.0;
    for (int y = y0; y < y0 + ny; ++y) acc += region_row_partial_host(plane + (int64_t)y * w, x0, x0 + nx, G);
    return acc / ((double)ny * (double)nx);
}

}  // namespace ssal
