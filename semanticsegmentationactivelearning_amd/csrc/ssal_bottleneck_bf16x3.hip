// ssal_bottleneck_bf16x3.hip -- OPT-IN arithmetic mode SSAL_ARITH_BF16X3 (include/ssal_enet.h) of the regular / dilated /
// asymmetric 128-channel ENet bottleneck (enet_modules.py:526-599).  Never the default, never the bench headline.
//
// What it is.  The default kernels (ssal_bottleneck_mfma.hip) evaluate every convolution on v_mfma_f32_32x32x2_f32: exact
// fp32 fmaf chains, bit-identical to the parity oracle, and bound by the fp32 matrix rate (155 TFLOP/s measured).  Here
// every fp32 operand is split into three bf16 terms, x = x1 + x2 + x3 EXACTLY (three truncations cover the 24 significant
// bits), and a K = 16 step of a 32x32 tile is SIX v_mfma_f32_32x32x16_bf16 -- x3w1, x2w2, x1w3, x2w1, x1w2, x1w1, small terms
// first, every product exact, fp32 accumulation -- which drops only the O(2^-24) cross terms x2w3, x3w2, x3w3: the same
// accuracy class as fp32 (tests/test_split_operand_cpu.py: 7.7e-6 against 5.9e-6 max logit error versus float64), 2.7x the
// matrix rate with pre-split operands.  It is a DIFFERENT summation than the oracle's fmaf chains, so results are not
// bit-identical to the default mode; its parity gate is north_star's own tolerance (confidence <= 1e-4, identical top-k,
// pooling indices bit-identical: both pooling layers run in front of these layers and stay exact).
//
// How it is built for gfx950 (one workgroup = 4 waves = one 8 x 16 tile of ONE dilation-phase sub-image, as k_bottleneck_o4):
//   kernels   pre-split and pre-packed per layer at commit (host): [chunk][term][lane] x 16 B, one buffer_load_b128 per term
//   phase A   projection as D[co][pixel] (lane = pixel) of the 10 x 18 halo'd tile: 2 ring M-tiles (waves 0 / 1) + one centre
//             M-tile per wave; input split in registers (32 and/sub + 12 v_perm per 8 values), 32 input registers in flight
//   LDS       the projected tile P is stored ALREADY SPLIT: per halo pixel 3 terms x 32 bf16 (192 B + 16 B pad), written
//             once per pixel as packed 8-byte stores -- so the convolution's 18 K-chunks read their B operand with three
//             ds_read_b128 and no vector work at all (the round-4 probe re-split P at every tap: 9x the split work)
//   phase B   3x3 conv D[co][pixel] -> BN + PReLU -> one swap per register pair + split -> expansion D[pixel][co] (lane = output
//             channel) -> BN + residual (re-read as 128-byte rows) + PReLU -> 128-byte row stores.
// Measured forms (profiles/r05_ab_bf16x3_forms.txt): keeping the centre input in registers as the residual (block input read
// once, expansion as D[co][pixel], 16-byte stores of 4 channels per lane on a 512-byte stride; 196 VGPRs = 2 workgroups per CU)
// 116-121 us per launch; the same store shape with the residual re-read 114-123 us; THIS form 83-94 us (exact fp32: 113-120):
// what decides is the access shape of the epilogue, not the bytes.
// Roofline: the six-product arithmetic of one launch (batch 8) needs ~25 us of bf16 matrix pipe; its HBM traffic -- input
// 1.41x (halo) + residual re-read + output = ~440 MB -- 70 us at 6.3 TB/s: HBM-bound; measured 83-94 us = 4.7-5.3 TB/s.
#include "ssal_internal.h"
#include "ssal_mfma.h"
#include "ssal_bottleneck_args.h"
#include "ssal_bf16x3.h"
#include "ssal_prof.h"

namespace ssal {

namespace {
constexpr int F = 32, C = 128;
constexpr int TW = 16, TH = 8;
constexpr int PS = 208;  // bytes per P slot: 3 terms x 32 bf16 = 192 B, padded to 208 (16-byte aligned rows, 52-dword pitch)

// the activation split (split1, split_pack8) and the six-product step (mfma6): ssal_bf16x3.h, shared with ICNet's kernel
using bf16x3::Split3;
using bf16x3::pack_hi;
using bf16x3::split1;
using bf16x3::split_pack8;
using bf16x3::mfma_bf;
using bf16x3::mfma6;

// packed kernel chunk `unit` (16-byte units, bf16x3::CHUNK_UNITS per chunk): [term][lane]
__device__ __forceinline__ Split3 load_w(const rsrc_t &rs, int unit_off, int lane)
{
    Split3 s;
    const unsigned lo = (unsigned)lane * 16u;
    s.t1 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, lo, (unit_off + 0) * 16, 0));
    s.t2 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, lo, (unit_off + 64) * 16, 0));
    s.t3 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, lo, (unit_off + 128) * 16, 0));
    return s;
}

// the pre-split B operand of one K = 16 chunk from an LDS slot: term t at +64 t bytes, channels 16 c2 + 8 h .. + 7
__device__ __forceinline__ Split3 load_p(const unsigned char *slot, int c2, int h)
{
    const unsigned char *p = slot + 32 * c2 + 16 * h;
    Split3 s;
    s.t1 = *reinterpret_cast<const uint4 *>(p);
    s.t2 = *reinterpret_cast<const uint4 *>(p + 64);
    s.t3 = *reinterpret_cast<const uint4 *>(p + 128);
    return s;
}

// four consecutive channels (co0 .. co0 + 3) of one pixel -> the slot's three bf16 planes, 8 bytes each
__device__ __forceinline__ void store_split4(unsigned char *slot, int co0, float v0, float v1, float v2, float v3)
{
    unsigned a[4], b[4], c[4];
    split1(v0, a[0], b[0], c[0]);
    split1(v1, a[1], b[1], c[1]);
    split1(v2, a[2], b[2], c[2]);
    split1(v3, a[3], b[3], c[3]);
    unsigned char *p = slot + 2 * co0;
    *reinterpret_cast<uint2 *>(p) = make_uint2(pack_hi(a[0], a[1]), pack_hi(a[2], a[3]));
    *reinterpret_cast<uint2 *>(p + 64) = make_uint2(pack_hi(b[0], b[1]), pack_hi(b[2], b[3]));
    *reinterpret_cast<uint2 *>(p + 128) = make_uint2(pack_hi(c[0], c[1]), pack_hi(c[2], c[3]));
}

struct Tile {
    int n, py, px, ty0, tx0, Hp, Wp;
    bool empty;
};

__device__ __forceinline__ Tile decode(const BnkArgs &a)
{
    Tile t;
    const int d = a.dil;
    int b = blockIdx.x;
    t.empty = true;
    if (a.xcd_chunk > 0) {  // XCD-aware order: workgroup b runs on XCD b % 8; every XCD gets a contiguous run of tiles
        b = (b & 7) * a.xcd_chunk + (b >> 3);
    }
    if (b >= a.ntiles) return t;
    const int tx = b % a.tiles_x; b /= a.tiles_x;
    const int ty = b % a.tiles_y; b /= a.tiles_y;
    t.px = b % d; b /= d;
    t.py = b % d; b /= d;
    t.n = b;
    t.Hp = (a.H - t.py + d - 1) / d;
    t.Wp = (a.W - t.px + d - 1) / d;
    t.ty0 = ty * TH;
    t.tx0 = tx * TW;
    t.empty = (t.ty0 >= t.Hp) || (t.tx0 >= t.Wp);
    return t;
}

// ---- 1x1 projection 128 -> 32 of ONE M-tile as D[co][pixel]: lane (j, h) owns the pixel whose halo'd-tile slot is q
// (q < 0: no pixel), loads its channels 16 c + 8 h .. + 7 of every chunk c, and writes BN + PReLU of the result -- exact zeros outside the image: SAME padding applies to the PROJECTED
// tensor -- pre-split into P.  HWPX = pixels per halo'd row, HALO = 1 (3x3) / 2 (5x1, 1x5).
// Chunks 0..3 of the input are requested up front and chunk c + 4 when chunk c has been consumed (32 registers in flight).
template <int HWPX, int HALO>
__device__ __forceinline__ void project_tile(const BnkArgs &a, const Tile &t, const float *ximg, const rsrc_t &wrs, int q,
                                             unsigned char *P, int lane, int h)
{
    float4 X[16];
    const int d = a.dil;
    const int hr = q / HWPX, hc = q - hr * HWPX;
    const int pr = t.ty0 - HALO + hr, pc = t.tx0 - HALO + hc;
    const bool valid = (q >= 0) && (pr >= 0) && (pr < t.Hp) && (pc >= 0) && (pc < t.Wp);
    if (__ballot(valid) == 0ull) {  // wave-uniform: the whole M-tile lies outside the image
        if (q >= 0) {
#pragma unroll
            for (int g = 0; g < 12; ++g) *reinterpret_cast<uint4 *>(P + q * PS + 16 * g) = make_uint4(0u, 0u, 0u, 0u);
        }
        return;
    }
    const float *xp = valid ? ximg + ((long)(t.py + pr * d) * a.W + (t.px + pc * d)) * C : ximg;
    auto load_x = [&](int c) {
        X[2 * c] = *reinterpret_cast<const float4 *>(xp + 16 * c + 8 * h);
        X[2 * c + 1] = *reinterpret_cast<const float4 *>(xp + 16 * c + 8 * h + 4);
    };
#pragma unroll
    for (int c = 0; c < 4; ++c) load_x(c);
    f32x16 acc = {0};
    Split3 wA = load_w(wrs, bf16x3::WP_OFF, lane), wB;  // packed kernel chunks one ahead (L2)
#pragma unroll
    for (int c = 0; c < 8; c += 2) {
        wB = load_w(wrs, bf16x3::WP_OFF + (c + 1) * bf16x3::CHUNK_UNITS, lane);
        __builtin_amdgcn_sched_barrier(0);
        {
            const float v[8] = {X[2 * c].x, X[2 * c].y, X[2 * c].z, X[2 * c].w, X[2 * c + 1].x, X[2 * c + 1].y,
                                X[2 * c + 1].z, X[2 * c + 1].w};
            acc = mfma6(wA, split_pack8(v), acc);  // D[co][pixel]: A = kernel (rows co), B = activations
        }
        __builtin_amdgcn_sched_barrier(0);
        if (c < 4) { load_x(c + 4); load_x(c + 5); }
        if (c + 2 < 8) wA = load_w(wrs, bf16x3::WP_OFF + (c + 2) * bf16x3::CHUNK_UNITS, lane);
        __builtin_amdgcn_sched_barrier(0);
        {
            const float v[8] = {X[2 * c + 2].x, X[2 * c + 2].y, X[2 * c + 2].z, X[2 * c + 2].w, X[2 * c + 3].x, X[2 * c + 3].y,
                                X[2 * c + 3].z, X[2 * c + 3].w};
            acc = mfma6(wB, split_pack8(v), acc);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // reg 4g + k = co 8g + 4h + k of the lane's pixel
    const rsrc_t srs = make_rsrc(a.ps, F * 4), trs = make_rsrc(a.pt, F * 4), ars = make_rsrc(a.pa, F * 4);
    if (q >= 0) {
        unsigned char *slot = P + q * PS;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 s4 = bload4(srs, h * 16, g * 32), t4 = bload4(trs, h * 16, g * 32), a4 = bload4(ars, h * 16, g * 32);
            const float v0 = valid ? prelu1(fmaf(acc[4 * g + 0], s4.x, t4.x), a4.x) : 0.0f;
            const float v1 = valid ? prelu1(fmaf(acc[4 * g + 1], s4.y, t4.y), a4.y) : 0.0f;
            const float v2 = valid ? prelu1(fmaf(acc[4 * g + 2], s4.z, t4.z), a4.z) : 0.0f;
            const float v3 = valid ? prelu1(fmaf(acc[4 * g + 3], s4.w, t4.w), a4.w) : 0.0f;
            store_split4(slot, 8 * g + 4 * h, v0, v1, v2, v3);
        }
    }
}

// BN + PReLU of a D[co][pixel] accumulator (reg 4g + k = channel 8g + 4h + k) -> the two pre-split operand chunks of the next
// GEMM (lane (pixel j, h) holds ci = 16 c + 8 h + 0..7: the layout of an A operand with rows = pixels and of a B operand with
// columns = pixels alike)
__device__ __forceinline__ void bn_prelu_to_b(const f32x16 &acc, const rsrc_t &srs, const rsrc_t &trs, const rsrc_t &ars, int h,
                                              Split3 (&qb)[2])
{
    float qv[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 s4 = bload4(srs, h * 16, g * 32), t4 = bload4(trs, h * 16, g * 32), a4 = bload4(ars, h * 16, g * 32);
        qv[4 * g + 0] = prelu1(fmaf(acc[4 * g + 0], s4.x, t4.x), a4.x);
        qv[4 * g + 1] = prelu1(fmaf(acc[4 * g + 1], s4.y, t4.y), a4.y);
        qv[4 * g + 2] = prelu1(fmaf(acc[4 * g + 2], s4.z, t4.z), a4.z);
        qv[4 * g + 3] = prelu1(fmaf(acc[4 * g + 3], s4.w, t4.w), a4.w);
    }
    // lane (pixel j, h) needs ci = 16 c + 8 h + 0..7: groups 2c and 2c + 1 exchange halves
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
#pragma unroll
        for (int k = 0; k < 4; ++k) swap32(qv[8 * cc + k], qv[8 * cc + 4 + k]);
        const float v[8] = {qv[8 * cc + 0], qv[8 * cc + 1], qv[8 * cc + 2], qv[8 * cc + 3],
                            qv[8 * cc + 4], qv[8 * cc + 5], qv[8 * cc + 6], qv[8 * cc + 7]};
        qb[cc] = split_pack8(v);
    }
}

// 1x1 expansion as D[pixel][co] (lane = output channel, registers = the M-tile's 32 pixels): 128-byte row stores and
// row-wise residual re-reads, the access shape of the exact kernels' epilogue.  boff[i] = byte offset (inside the image, lane
// channel folded in) of pixel row i of the M-tile, out-of-range for pixels outside the image (the hardware range check drops
// their stores / answers their loads with 0).
__device__ __forceinline__ void expand_store_rows(const BnkArgs &a, const rsrc_t &wrs, int we_off, const Split3 (&qa)[2],
                                                  const rsrc_t &xrs, const rsrc_t &yrs, const unsigned (&boff)[16], int lane, int j)
{
    const rsrc_t esrs = make_rsrc(a.es, C * 4), etrs = make_rsrc(a.et, C * 4), rars = make_rsrc(a.ra, C * 4);
    float rx[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) rx[i] = bload(xrs, boff[i], 0);
    Split3 we0 = load_w(wrs, we_off, lane), we1 = load_w(wrs, we_off + bf16x3::CHUNK_UNITS, lane);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const float s1 = bload(esrs, j * 4, nt * 128), t1 = bload(etrs, j * 4, nt * 128), al = bload(rars, j * 4, nt * 128);
        f32x16 e = {0};
        e = mfma6(qa[0], we0, e);  // D[pixel][co]: A = Q (rows = pixels), B = kernel
        e = mfma6(qa[1], we1, e);
        if (nt < 3) {
            we0 = load_w(wrs, we_off + (nt * 2 + 2) * bf16x3::CHUNK_UNITS, lane);
            we1 = load_w(wrs, we_off + (nt * 2 + 3) * bf16x3::CHUNK_UNITS, lane);
        }
        float out[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) out[i] = prelu1(fmaf(e[i], s1, t1) + rx[i], al);
        if (nt < 3) {
#pragma unroll
            for (int i = 0; i < 16; ++i) rx[i] = bload(xrs, boff[i], (nt + 1) * 128);  // next N-tile's residual rows, ahead of the stores
        }
#pragma unroll
        for (int i = 0; i < 16; ++i)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, out[i]), yrs, boff[i], nt * 128, 0);
    }
}

// byte offsets (inside image n, lane channel j folded in) of the 16 pixel rows of the M-tile that starts at tile pixel tp0
// which this lane half holds in a D[pixel][co] accumulator; out of range for pixels outside the image
__device__ __forceinline__ void row_offsets(const BnkArgs &a, const Tile &t, int tp0, int h, int j, unsigned (&boff)[16])
{
    constexpr unsigned kOOB = 0x80000000u;
    const int d = a.dil;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int ti = tp0 + (i & 3) + 8 * (i >> 2) + 4 * h;
        const int pr = t.ty0 + (ti >> 4), pc = t.tx0 + (ti & 15);
        boff[i] = (pr < t.Hp && pc < t.Wp) ? (unsigned)((((t.py + pr * d) * a.W + (t.px + pc * d)) * C + j) * 4) : kOOB;
    }
}

// ---- regular / dilated 3x3 bottleneck ------------------------------------------------------------------------------------
constexpr int HWP3 = TW + 2;                   // 18
constexpr int RING3 = 2 * HWP3 + 2 * TH;       // 52 ring pixels
constexpr int PSLOTS3 = (TH + 2) * HWP3;       // 180

// 103-120 VGPRs, 37.4 KB of LDS: four workgroups per CU
__global__ __launch_bounds__(256, 4) void k_bottleneck_bf16x3(BnkArgs a, const uint4 *wpk)
{
    __shared__ __attribute__((aligned(16))) unsigned char P[PSLOTS3 * PS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const Tile t = decode(a);
    if (t.empty) return;  // whole workgroup: no barrier has been reached yet
    const float *ximg = a.x + (long)t.n * a.H * a.W * C;
    float *yimg = a.y + (long)t.n * a.H * a.W * C;
    const rsrc_t wrs = make_rsrc(wpk, bf16x3::units(9) * 16);

    auto q_ring = [&](int u) {  // halo'd-tile slot of ring pixel u: top row, bottom row, then (left, right) of rows 1..8
        const int k = u - 2 * HWP3;
        return u < HWP3 ? u
                        : (u < 2 * HWP3 ? (TH + 1) * HWP3 + (u - HWP3)
                                        : (u < RING3 ? (1 + (k >> 1)) * HWP3 + ((k & 1) ? HWP3 - 1 : 0) : -1));
    };
    if (wave < 2) project_tile<HWP3, 1>(a, t, ximg, wrs, q_ring(wave * 32 + j), P, lane, h);
    const int tp = wave * 32 + j, tr_ = tp >> 4, tc = tp & 15;  // this lane's centre pixel: tile row tr_, column tc
    project_tile<HWP3, 1>(a, t, ximg, wrs, (tr_ + 1) * HWP3 + tc + 1, P, lane, h);
    __syncthreads();

    // ---- phase B: 3x3 conv D[co][pixel], 18 K-chunks (tap, half), one chunk ahead ----
    f32x16 acc = {0};
    {
        auto fetch = [&](int q, Split3 &w, Split3 &p) {
            const int tap = q >> 1, c2 = q & 1, kh = tap / 3, kw = tap - 3 * kh;
            w = load_w(wrs, bf16x3::WC_OFF + q * bf16x3::CHUNK_UNITS, lane);
            p = load_p(P + ((tr_ + kh) * HWP3 + (tc + kw)) * PS, c2, h);
        };
        Split3 wA, wB, pA, pB;
        fetch(0, wA, pA);
#pragma unroll 1
        for (int q = 0; q < 18; q += 2) {
            fetch(q + 1, wB, pB);
            __builtin_amdgcn_sched_barrier(0);
            acc = mfma6(wA, pA, acc);
            __builtin_amdgcn_sched_barrier(0);
            if (q + 2 < 18) fetch(q + 2, wA, pA);
            __builtin_amdgcn_sched_barrier(0);
            acc = mfma6(wB, pB, acc);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    Split3 qa[2];
    bn_prelu_to_b(acc, make_rsrc(a.cs, F * 4), make_rsrc(a.ct, F * 4), make_rsrc(a.ca, F * 4), h, qa);
    unsigned boff[16];
    row_offsets(a, t, wave * 32, h, j, boff);
    const unsigned img_bytes = (unsigned)(a.H * a.W * C) * 4u;
    expand_store_rows(a, wrs, bf16x3::we_off(9), qa, make_rsrc(ximg, img_bytes), make_rsrc(yimg, img_bytes), boff, lane, j);
}

// ---- asymmetric bottleneck: (5,1) then (1,5), no BN / activation in between (enet_modules.py:553-563), dilation 1 --------
// P = the projected tile with a 2-pixel halo, 12 x 20 slots.  R = the (5,1) result for the 8 x 20 pixels the (1,5) conv
// reads, ALSO pre-split (it is the B operand of the second convolution).  R has no LDS of its own: the (5,1) pass of the
// whole tile (160 result pixels = exactly 5 M-tiles; wave 0 takes two) keeps its results in accumulator registers across a
// barrier -- behind which every read of P is over -- and then writes them over P's rows 0..7.  49.9 KB of LDS, three
// workgroups per CU (the first version: R in 20 KB of its own, the tile in two halves of 3 + 2 busy waves: 130 us).
constexpr int HWP5 = TW + 4;                   // 20
constexpr int PSLOTS5 = (TH + 4) * HWP5;       // 240

__global__ __launch_bounds__(256, 3) void k_bottleneck_asym_bf16x3(BnkArgs a, const uint4 *wpk)
{
    __shared__ __attribute__((aligned(16))) unsigned char P[PSLOTS5 * PS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const Tile t = decode(a);
    if (t.empty) return;
    const float *ximg = a.x + (long)t.n * a.H * a.W * C;
    float *yimg = a.y + (long)t.n * a.H * a.W * C;
    const rsrc_t wrs = make_rsrc(wpk, bf16x3::units(10) * 16);

    // ---- phase A: the 240 halo'd pixels = 112 ring pixels (4 M-tiles, 16 lanes idle) + 128 centre pixels (one M-tile per
    // wave).  Ring order: rows 0, 1, 10, 11 (20 each), then the 2 + 2 side pixels of rows 2..9.
    auto q_ring = [&](int u) {
        if (u < 2 * HWP5) return u;
        if (u < 4 * HWP5) return (TH + 2) * HWP5 + (u - 2 * HWP5);
        const int k = u - 4 * HWP5;  // 0 .. 31: row 2 + (k >> 2), side pixel k & 3 -> columns 0, 1, 18, 19
        return k < 32 ? (2 + (k >> 2)) * HWP5 + ((k & 3) < 2 ? (k & 3) : HWP5 - 4 + (k & 3)) : -1;
    };
    project_tile<HWP5, 2>(a, t, ximg, wrs, q_ring(wave * 32 + j), P, lane, h);
    const int tp = wave * 32 + j, tr_ = tp >> 4, tc = tp & 15;
    project_tile<HWP5, 2>(a, t, ximg, wrs, (tr_ + 2) * HWP5 + tc + 2, P, lane, h);
    __syncthreads();

    // ---- (5,1) conv, no BN / activation: result pixel u = (r, c') of the 8 x 20 grid reads P slots u + 20 kh, kh = 0..4
    auto conv51 = [&](int u) {
        f32x16 acc = {0};
        auto fetch = [&](int q, Split3 &w, Split3 &p) {
            const int kh = q >> 1, c2 = q & 1;
            w = load_w(wrs, bf16x3::WC_OFF + q * bf16x3::CHUNK_UNITS, lane);
            p = load_p(P + (u + kh * HWP5) * PS, c2, h);
        };
        Split3 wA, wB, pA, pB;
        fetch(0, wA, pA);
#pragma unroll 1
        for (int q = 0; q < 10; q += 2) {
            fetch(q + 1, wB, pB);
            __builtin_amdgcn_sched_barrier(0);
            acc = mfma6(wA, pA, acc);
            __builtin_amdgcn_sched_barrier(0);
            if (q + 2 < 10) fetch(q + 2, wA, pA);
            __builtin_amdgcn_sched_barrier(0);
            acc = mfma6(wB, pB, acc);
            __builtin_amdgcn_sched_barrier(0);
        }
        return acc;
    };
    const f32x16 r0 = conv51(wave * 32 + j);
    f32x16 r1 = {0};
    if (wave == 0) r1 = conv51(128 + j);  // the fifth M-tile (wave-uniform)
    __syncthreads();  // nobody reads the projected rows any more
    auto store_r = [&](const f32x16 &acc, int u) {
        unsigned char *slot = P + u * PS;
#pragma unroll
        for (int g = 0; g < 4; ++g) store_split4(slot, 8 * g + 4 * h, acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
    };
    store_r(r0, wave * 32 + j);
    if (wave == 0) store_r(r1, 128 + j);
    __syncthreads();  // R complete (slots 0 .. 159)

    // ---- (1,5) conv + BN + PReLU + expansion: wave w owns tile rows 2w, 2w + 1
    f32x16 acc = {0};
    {
        auto fetch = [&](int q, Split3 &w, Split3 &p) {
            const int kw = q >> 1, c2 = q & 1;
            w = load_w(wrs, bf16x3::WC_OFF + (10 + q) * bf16x3::CHUNK_UNITS, lane);
            p = load_p(P + (tr_ * HWP5 + tc + kw) * PS, c2, h);
        };
        Split3 wA, wB, pA, pB;
        fetch(0, wA, pA);
#pragma unroll 1
        for (int q = 0; q < 10; q += 2) {
            fetch(q + 1, wB, pB);
            __builtin_amdgcn_sched_barrier(0);
            acc = mfma6(wA, pA, acc);
            __builtin_amdgcn_sched_barrier(0);
            if (q + 2 < 10) fetch(q + 2, wA, pA);
            __builtin_amdgcn_sched_barrier(0);
            acc = mfma6(wB, pB, acc);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    Split3 qa[2];
    bn_prelu_to_b(acc, make_rsrc(a.cs, F * 4), make_rsrc(a.ct, F * 4), make_rsrc(a.ca, F * 4), h, qa);
    unsigned boff[16];
    row_offsets(a, t, wave * 32, h, j, boff);
    const unsigned img_bytes = (unsigned)(a.H * a.W * C) * 4u;
    expand_store_rows(a, wrs, bf16x3::we_off(10), qa, make_rsrc(ximg, img_bytes), make_rsrc(yimg, img_bytes), boff, lane, j);
}

// ---- downsample bottleneck 64 -> 128 (Bottleneck2_0; enet_modules.py:868-938) ------------------------------------------------
// 8 x 16 OUTPUT pixels per workgroup; P = the projected tile with a 1-pixel halo as in the regular kernel.  Projection =
// the 2x2 / stride-2 convolution as one GEMM over K = 4 taps x 64 channels = 16 chunks; 3x3 convolution as in the regular
// kernel; expansion as D[co][pixel] with whole-row stores through quad_transpose4.
// The residual -- max_pool_with_argmax 2x2 / s2 of the block INPUT, zero-padded from 64 to 128 channels -- is EXACT fp32
// whatever the arithmetic mode (first maximum in (dy, dx) order wins, its window code dy * 2 + dx goes to the upsample block):
// the pooling indices of a bf16x3 call are the exact path's bit for bit.  It is taken from the projection's OWN activation
// registers (a second read of the input misses L2: +80 us, measured): the chunks run channel-group-major (the four taps of 16
// channels in a row), a lane half holds the channels c with (c >> 2) & 1 == h -- exactly the ones the D[co][pixel] expansion
// hands it -- so the 32 maxima of a lane wait in registers and meet the expansion's output without leaving the lane.
constexpr int DC = 64;

template <bool POOL>
__device__ __forceinline__ void project_down(const DownArgs &a, const float *ximg, const rsrc_t &wrs, int q, int ty0, int tx0,
                                             int Ho, int Wo, unsigned char *P, int lane, int h, float (&pooled)[32],
                                             const rsrc_t &crs)
{
    float4 X[12];  // rolling window of 6 K-chunks
    const int hr = q / HWP3, hc = q - hr * HWP3;
    const int pr = ty0 - 1 + hr, pc = tx0 - 1 + hc;
    const bool valid = (q >= 0) && (pr >= 0) && (pr < Ho) && (pc >= 0) && (pc < Wo);
    if (__ballot(valid) == 0ull) {  // wave-uniform: the whole M-tile lies outside the image
        if (q >= 0) {
#pragma unroll
            for (int g = 0; g < 12; ++g) *reinterpret_cast<uint4 *>(P + q * PS + 16 * g) = make_uint4(0u, 0u, 0u, 0u);
        }
        if (POOL) {
#pragma unroll
            for (int i = 0; i < 32; ++i) pooled[i] = 0.0f;
        }
        return;
    }
    const float *xp = valid ? ximg + ((long)(2 * pr) * a.W + 2 * pc) * DC : ximg;
    const int rowf = a.W * DC;
    auto load_x = [&](int s) {  // chunk s = 4 cc + t: tap (dy, dx) = (t >> 1, t & 1); channels 16 cc + 4 h + {0..3, 8..11}
        const float *src = xp + ((s & 2) ? rowf : 0) + ((s & 1) ? DC : 0) + 16 * (s >> 2) + 4 * h;
        X[2 * (s % 6)] = *reinterpret_cast<const float4 *>(src);
        X[2 * (s % 6) + 1] = *reinterpret_cast<const float4 *>(src + 8);
    };
    float best[8];
    unsigned cw[8];  // window codes, four channels per word: cw[2 cc + (i >> 2)]
    auto consume = [&](int s, const Split3 &w, f32x16 acc) {
        const float4 u = X[2 * (s % 6)], v4 = X[2 * (s % 6) + 1];
        const float v[8] = {u.x, u.y, u.z, u.w, v4.x, v4.y, v4.z, v4.w};
        if (POOL) {
            const int t = s & 3, cc = s >> 2;
            if (t == 0) {
#pragma unroll
                for (int i = 0; i < 8; ++i) best[i] = v[i];
                cw[2 * cc] = 0u; cw[2 * cc + 1] = 0u;
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const bool gt = v[i] > best[i];  // strict '>' in (dy, dx) order: the first maximum wins
                    best[i] = gt ? v[i] : best[i];
                    const unsigned sh = 8u * (i & 3), m = 3u << sh;
                    cw[2 * cc + (i >> 2)] = gt ? ((cw[2 * cc + (i >> 2)] & ~m) | ((unsigned)t << sh)) : cw[2 * cc + (i >> 2)];
                }
            }
            if (t == 3) {
#pragma unroll
                for (int i = 0; i < 8; ++i) pooled[8 * cc + i] = best[i];
            }
        }
        return mfma6(w, split_pack8(v), acc);  // D[co][pixel]
    };
#pragma unroll
    for (int s = 0; s < 4; ++s) load_x(s);
    f32x16 acc = {0};
    Split3 wA = load_w(wrs, bf16x3::DN_WP_OFF, lane), wB;
#pragma unroll
    for (int s = 0; s < 16; s += 2) {
        wB = load_w(wrs, bf16x3::DN_WP_OFF + (s + 1) * bf16x3::CHUNK_UNITS, lane);
        __builtin_amdgcn_sched_barrier(0);
        acc = consume(s, wA, acc);
        __builtin_amdgcn_sched_barrier(0);
        if (s + 4 < 16) { load_x(s + 4); load_x(s + 5); }
        if (s + 2 < 16) wA = load_w(wrs, bf16x3::DN_WP_OFF + (s + 2) * bf16x3::CHUNK_UNITS, lane);
        __builtin_amdgcn_sched_barrier(0);
        acc = consume(s + 1, wB, acc);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (POOL) {  // codes of the lane's 32 channels: eight 4-byte stores (channels 16 cc + 4 h + 8 half .. + 3)
        const unsigned co = valid ? (unsigned)((pr * Wo + pc) * DC + 4 * h) : 0x80000000u;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            __builtin_amdgcn_raw_buffer_store_b32(cw[k], crs, co, 16 * (k >> 1) + 8 * (k & 1), 0);
    }
    const rsrc_t srs = make_rsrc(a.ps, F * 4), trs = make_rsrc(a.pt, F * 4), ars = make_rsrc(a.pa, F * 4);
    if (q >= 0) {
        unsigned char *slot = P + q * PS;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 s4 = bload4(srs, h * 16, g * 32), t4 = bload4(trs, h * 16, g * 32), a4 = bload4(ars, h * 16, g * 32);
            const float v0 = valid ? prelu1(fmaf(acc[4 * g + 0], s4.x, t4.x), a4.x) : 0.0f;
            const float v1 = valid ? prelu1(fmaf(acc[4 * g + 1], s4.y, t4.y), a4.y) : 0.0f;
            const float v2 = valid ? prelu1(fmaf(acc[4 * g + 2], s4.z, t4.z), a4.z) : 0.0f;
            const float v3 = valid ? prelu1(fmaf(acc[4 * g + 3], s4.w, t4.w), a4.w) : 0.0f;
            store_split4(slot, 8 * g + 4 * h, v0, v1, v2, v3);
        }
    }
}

__global__ __launch_bounds__(256, 3) void k_downsample_bf16x3(DownArgs a, const uint4 *wpk)
{
    __shared__ __attribute__((aligned(16))) unsigned char P[PSLOTS3 * PS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int Ho = a.H / 2, Wo = a.W / 2;
    int b = blockIdx.x;
    const int tx = b % a.tiles_x; b /= a.tiles_x;
    const int ty = b % a.tiles_y; b /= a.tiles_y;
    const int n = b;
    const int ty0 = ty * TH, tx0 = tx * TW;
    const float *ximg = a.x + (long)n * a.H * a.W * DC;
    float *yimg = a.y + (long)n * Ho * Wo * C;
    uint8_t *cimg = a.code + (long)n * Ho * Wo * DC;
    const rsrc_t wrs = make_rsrc(wpk, bf16x3::DN_UNITS * 16);
    const rsrc_t crs = make_rsrc(cimg, (unsigned)(Ho * Wo * DC));

    auto q_ring = [&](int u) {
        const int k = u - 2 * HWP3;
        return u < HWP3 ? u
                        : (u < 2 * HWP3 ? (TH + 1) * HWP3 + (u - HWP3)
                                        : (u < RING3 ? (1 + (k >> 1)) * HWP3 + ((k & 1) ? HWP3 - 1 : 0) : -1));
    };
    float pooled[32];  // this lane's pixel (wave * 32 + j): maxima of channels 16 cc + 4 h + (i & 3) + 8 (i >> 2), index 8 cc + i
    if (wave < 2) project_down<false>(a, ximg, wrs, q_ring(wave * 32 + j), ty0, tx0, Ho, Wo, P, lane, h, pooled, crs);
    const int tp = wave * 32 + j, tr_ = tp >> 4, tc = tp & 15;
    project_down<true>(a, ximg, wrs, (tr_ + 1) * HWP3 + tc + 1, ty0, tx0, Ho, Wo, P, lane, h, pooled, crs);
    __syncthreads();

    // ---- 3x3 conv D[co][pixel], 18 K-chunks ----
    f32x16 acc = {0};
    {
        auto fetch = [&](int q, Split3 &w, Split3 &p) {
            const int tap = q >> 1, c2 = q & 1, kh = tap / 3, kw = tap - 3 * kh;
            w = load_w(wrs, bf16x3::DN_WC_OFF + q * bf16x3::CHUNK_UNITS, lane);
            p = load_p(P + ((tr_ + kh) * HWP3 + (tc + kw)) * PS, c2, h);
        };
        Split3 wA, wB, pA, pB;
        fetch(0, wA, pA);
#pragma unroll 1
        for (int q = 0; q < 18; q += 2) {
            fetch(q + 1, wB, pB);
            __builtin_amdgcn_sched_barrier(0);
            acc = mfma6(wA, pA, acc);
            __builtin_amdgcn_sched_barrier(0);
            if (q + 2 < 18) fetch(q + 2, wA, pA);
            __builtin_amdgcn_sched_barrier(0);
            acc = mfma6(wB, pB, acc);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    Split3 qb[2];
    bn_prelu_to_b(acc, make_rsrc(a.cs, F * 4), make_rsrc(a.ct, F * 4), make_rsrc(a.ca, F * 4), h, qb);

    // ---- expansion 32 -> 128 as D[co][pixel] (lane = pixel, reg 4 g + k = channel 32 nt + 8 g + 4 h + k), + the pooled residual
    // on channels < 64, PReLU; the four 16-byte pieces of a lane leave as whole 128-byte rows (quad_transpose4) ----
    constexpr unsigned kOOB = 0x80000000u;
    const rsrc_t yrs = make_rsrc(yimg, (unsigned)(Ho * Wo * C) * 4u);
    const rsrc_t esrs = make_rsrc(a.es, C * 4), etrs = make_rsrc(a.et, C * 4), rars = make_rsrc(a.ra, C * 4);
    unsigned yoq[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const int ti = wave * 32 + (j & ~3) + kk;
        const int pr = ty0 + (ti >> 4), pc = tx0 + (ti & 15);
        yoq[kk] = (pr < Ho && pc < Wo) ? (unsigned)(((pr * Wo + pc) * C) * 4 + 32 * (j & 3) + 16 * h) : kOOB;
    }
    Split3 we0 = load_w(wrs, bf16x3::DN_WE_OFF, lane), we1 = load_w(wrs, bf16x3::DN_WE_OFF + bf16x3::CHUNK_UNITS, lane);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        f32x16 e = {0};
        e = mfma6(we0, qb[0], e);  // A = kernel (rows = output channels 32 nt + j), B = Q (columns = pixels)
        e = mfma6(we1, qb[1], e);
        if (nt < 3) {
            we0 = load_w(wrs, bf16x3::DN_WE_OFF + (nt * 2 + 2) * bf16x3::CHUNK_UNITS, lane);
            we1 = load_w(wrs, bf16x3::DN_WE_OFF + (nt * 2 + 3) * bf16x3::CHUNK_UNITS, lane);
        }
        float4 ov[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 s4 = bload4(esrs, h * 16, nt * 128 + g * 32), t4 = bload4(etrs, h * 16, nt * 128 + g * 32);
            const float4 a4 = bload4(rars, h * 16, nt * 128 + g * 32);
            // channel 32 nt + 8 g + 4 h + k = 16 cc + 4 h + k + 8 (g & 1) with cc = 2 nt + (g >> 1): pooled[8 cc + 4 (g & 1) + k]
            const int pi = nt < 2 ? 8 * (2 * nt + (g >> 1)) + 4 * (g & 1) : 0;
            const float r0 = nt < 2 ? pooled[pi + 0] : 0.0f, r1 = nt < 2 ? pooled[pi + 1] : 0.0f;
            const float r2 = nt < 2 ? pooled[pi + 2] : 0.0f, r3 = nt < 2 ? pooled[pi + 3] : 0.0f;  // channels >= 64: zero padding
            ov[g].x = prelu1(fmaf(e[4 * g + 0], s4.x, t4.x) + r0, a4.x);
            ov[g].y = prelu1(fmaf(e[4 * g + 1], s4.y, t4.y) + r1, a4.y);
            ov[g].z = prelu1(fmaf(e[4 * g + 2], s4.z, t4.z) + r2, a4.z);
            ov[g].w = prelu1(fmaf(e[4 * g + 3], s4.w, t4.w) + r3, a4.w);
        }
        quad_transpose4(ov[0], ov[1], ov[2], ov[3], lane);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, ov[kk]), yrs, yoq[kk], nt * 128, 0);
    }
}

// ---- upsample bottleneck 128 -> 64 (Bottleneck4_0; enet_modules.py:1217-1292) ----------------------------------------------
// 8 x 16 INPUT pixels per workgroup -> 16 x 32 output pixels.  The transposed 3x3 / s2 convolution is evaluated per output
// parity class of an input pixel from P(i, j), P(i, j-1), P(i-1, j), P(i-1, j-1) (k_upsample_mfma's slots and its stacked
// kernel: accumulator A = [ee | eo], B = [oe | oo], 16 channels each), so P carries a halo on the top / left only: 9 x 17
// slots, the 25 ring pixels are one M-tile (wave 0).  The split activations of a centre pixel feed THREE GEMMs per K-chunk --
// the projection and the two N-tiles of the 1x1 residual convolution (D[co][pixel]: the residual waits in registers in the
// layout of the expansion's output) -- so the input is read and split once.  unpool_2d is the exact kernel's gather: the
// residual lands on the output parity its window code names.  Output rows leave as whole 128-byte lines (quad_transpose4).
constexpr int CU = 64;                        // output channels
constexpr int HWPU = TW + 1;                  // 17
constexpr int RINGU = HWPU + TH;              // 25 ring pixels: the top row (17), then the left column of rows 1..8
constexpr int PSLOTSU = (TH + 1) * HWPU;      // 153

template <bool RES>
__device__ __forceinline__ void project_up(const UpArgs &a, const float *ximg, const rsrc_t &wrs, int q, int ty0, int tx0,
                                           unsigned char *P, int lane, int h, f32x16 &res0, f32x16 &res1)
{
    float4 X[12];  // rolling window of 6 K-chunks
    const int hr = q / HWPU, hc = q - hr * HWPU;
    const int pr = ty0 - 1 + hr, pc = tx0 - 1 + hc;
    const bool valid = (q >= 0) && (pr >= 0) && (pr < a.H) && (pc >= 0) && (pc < a.W);
    if (RES) { res0 = (f32x16){0}; res1 = (f32x16){0}; }
    if (__ballot(valid) == 0ull) {  // wave-uniform: the whole M-tile lies outside the image
        if (q >= 0) {
#pragma unroll
            for (int g = 0; g < 12; ++g) *reinterpret_cast<uint4 *>(P + q * PS + 16 * g) = make_uint4(0u, 0u, 0u, 0u);
        }
        return;
    }
    const float *xp = valid ? ximg + ((long)pr * a.W + pc) * C : ximg;
    auto load_x = [&](int c) {
        X[2 * (c % 6)] = *reinterpret_cast<const float4 *>(xp + 16 * c + 8 * h);
        X[2 * (c % 6) + 1] = *reinterpret_cast<const float4 *>(xp + 16 * c + 8 * h + 4);
    };
#pragma unroll
    for (int c = 0; c < 4; ++c) load_x(c);
    f32x16 acc = {0};
    Split3 wP = load_w(wrs, bf16x3::UP_WP_OFF, lane), wR0, wR1;
    if (RES) {
        wR0 = load_w(wrs, bf16x3::UP_WR_OFF, lane);
        wR1 = load_w(wrs, bf16x3::UP_WR_OFF + bf16x3::CHUNK_UNITS, lane);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float4 u = X[2 * (c % 6)], w = X[2 * (c % 6) + 1];
        const float v[8] = {u.x, u.y, u.z, u.w, w.x, w.y, w.z, w.w};
        const Split3 xs = split_pack8(v);
        __builtin_amdgcn_sched_barrier(0);
        acc = mfma6(wP, xs, acc);  // D[co][pixel]
        if (c + 1 < 8) wP = load_w(wrs, bf16x3::UP_WP_OFF + (c + 1) * bf16x3::CHUNK_UNITS, lane);  // single buffers: reloaded right after use
        if (c + 4 < 8) load_x(c + 4);
        if (RES) {
            res0 = mfma6(wR0, xs, res0);
            if (c + 1 < 8) wR0 = load_w(wrs, bf16x3::UP_WR_OFF + (2 * c + 2) * bf16x3::CHUNK_UNITS, lane);
            res1 = mfma6(wR1, xs, res1);
            if (c + 1 < 8) wR1 = load_w(wrs, bf16x3::UP_WR_OFF + (2 * c + 3) * bf16x3::CHUNK_UNITS, lane);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    const rsrc_t srs = make_rsrc(a.ps, F * 4), trs = make_rsrc(a.pt, F * 4), ars = make_rsrc(a.pa, F * 4);
    if (q >= 0) {
        unsigned char *slot = P + q * PS;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 s4 = bload4(srs, h * 16, g * 32), t4 = bload4(trs, h * 16, g * 32), a4 = bload4(ars, h * 16, g * 32);
            const float v0 = valid ? prelu1(fmaf(acc[4 * g + 0], s4.x, t4.x), a4.x) : 0.0f;
            const float v1 = valid ? prelu1(fmaf(acc[4 * g + 1], s4.y, t4.y), a4.y) : 0.0f;
            const float v2 = valid ? prelu1(fmaf(acc[4 * g + 2], s4.z, t4.z), a4.z) : 0.0f;
            const float v3 = valid ? prelu1(fmaf(acc[4 * g + 3], s4.w, t4.w), a4.w) : 0.0f;
            store_split4(slot, 8 * g + 4 * h, v0, v1, v2, v3);
        }
    }
}

// BN + PReLU of a stacked transposed-conv accumulator (reg 4g + k = row 8g + 4h + k; rows 0..15 = the first class, 16..31 =
// the second, 16 channels each: channel = row & 15) -> the pre-split K = 16 operand of each class (lane (pixel j, h): ci = 8h + i)
__device__ __forceinline__ void bn16_prelu_to_b(const f32x16 &acc, const rsrc_t &srs, const rsrc_t &trs, const rsrc_t &ars, int h,
                                                Split3 (&qb)[2])
{
    float qv[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 s4 = bload4(srs, h * 16, (g & 1) * 32), t4 = bload4(trs, h * 16, (g & 1) * 32), a4 = bload4(ars, h * 16, (g & 1) * 32);
        qv[4 * g + 0] = prelu1(fmaf(acc[4 * g + 0], s4.x, t4.x), a4.x);
        qv[4 * g + 1] = prelu1(fmaf(acc[4 * g + 1], s4.y, t4.y), a4.y);
        qv[4 * g + 2] = prelu1(fmaf(acc[4 * g + 2], s4.z, t4.z), a4.z);
        qv[4 * g + 3] = prelu1(fmaf(acc[4 * g + 3], s4.w, t4.w), a4.w);
    }
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {  // class cc: groups 2cc (channels 4h + k) and 2cc + 1 (channels 8 + 4h + k) exchange halves
#pragma unroll
        for (int k = 0; k < 4; ++k) swap32(qv[8 * cc + k], qv[8 * cc + 4 + k]);
        const float v[8] = {qv[8 * cc + 0], qv[8 * cc + 1], qv[8 * cc + 2], qv[8 * cc + 3],
                            qv[8 * cc + 4], qv[8 * cc + 5], qv[8 * cc + 6], qv[8 * cc + 7]};
        qb[cc] = split_pack8(v);
    }
}

__global__ __launch_bounds__(256, 3) void k_upsample_bf16x3(UpArgs a, const uint4 *wpk)
{
    __shared__ __attribute__((aligned(16))) unsigned char P[PSLOTSU * PS];
    __shared__ __attribute__((aligned(16))) float BNV[3 * CU];  // es | et | ra
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    int b = blockIdx.x;
    const int tx = b % a.tiles_x; b /= a.tiles_x;
    const int ty = b % a.tiles_y; b /= a.tiles_y;
    const int n = b;
    const int ty0 = ty * TH, tx0 = tx * TW;
    const float *ximg = a.x + (long)n * a.H * a.W * C;
    const uint8_t *cimg = a.code + (long)n * a.H * a.W * CU;
    float *yimg = a.y + (long)n * 4 * a.H * a.W * CU;
    const rsrc_t wrs = make_rsrc(wpk, bf16x3::UP_UNITS * 16);
    if (threadIdx.x < 3 * CU / 4) {
        const int arr = threadIdx.x / (CU / 4), k4 = threadIdx.x % (CU / 4);
        const float *src = arr == 0 ? a.es : arr == 1 ? a.et : a.ra;
        reinterpret_cast<float4 *>(BNV)[threadIdx.x] = reinterpret_cast<const float4 *>(src)[k4];
    }

    f32x16 res0, res1, d0, d1;
    if (wave == 0) {  // the ring: slot of ring pixel u = the top row, then the left column
        const int u = j;
        const int q = u < HWPU ? u : (u < RINGU ? (u - HWPU + 1) * HWPU : -1);
        project_up<false>(a, ximg, wrs, q, ty0, tx0, P, lane, h, d0, d1);
    }
    const int tp = wave * 32 + j, tr_ = tp >> 4, tc = tp & 15;  // this lane's centre pixel: tile row tr_, column tc
    project_up<true>(a, ximg, wrs, (tr_ + 1) * HWPU + tc + 1, ty0, tx0, P, lane, h, res0, res1);
    __syncthreads();

    // window codes of channels 32 nt + 8 g + 4 h .. + 3 (index 4 nt + g) of the lane's input pixel
    const int iy = ty0 + tr_, ix = tx0 + tc;
    const bool valid = iy < a.H && ix < a.W;
    unsigned codes[8];
    {
        const rsrc_t crs = make_rsrc(cimg, (unsigned)(a.H * a.W * CU));
        const unsigned co = valid ? (unsigned)((iy * a.W + ix) * CU + 4 * h) : 0x80000000u;
#pragma unroll
        for (int q = 0; q < 8; ++q) codes[q] = __builtin_amdgcn_raw_buffer_load_b32(crs, co, 8 * q, 0);
    }
    // ---- transposed conv: slots 0..3 -> A = [ee | eo], slots 4, 5 -> B = [oe | oo]; 2 K-chunks per slot ----
    f32x16 accA = {0}, accB = {0};
    {
        auto fetch = [&](int q, Split3 &w, Split3 &p) {  // chunk q = 2 slot + c2
            const int slot = q >> 1, c2 = q & 1;
            const int dr = slot < 4 ? 1 - (slot >> 1) : 1, dc = 1 - (slot & 1);
            w = load_w(wrs, bf16x3::UP_WS_OFF + q * bf16x3::CHUNK_UNITS, lane);
            p = load_p(P + ((tr_ + dr) * HWPU + (tc + dc)) * PS, c2, h);
        };
        Split3 wA, wB, pA, pB;
        fetch(0, wA, pA);
#pragma unroll
        for (int q = 0; q < 12; q += 2) {
            fetch(q + 1, wB, pB);
            __builtin_amdgcn_sched_barrier(0);
            if (q < 8) accA = mfma6(wA, pA, accA); else accB = mfma6(wA, pA, accB);
            __builtin_amdgcn_sched_barrier(0);
            if (q + 2 < 12) fetch(q + 2, wA, pA);
            __builtin_amdgcn_sched_barrier(0);
            if (q < 8) accA = mfma6(wB, pB, accA); else accB = mfma6(wB, pB, accB);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const rsrc_t csrs = make_rsrc(a.cs, 16 * 4), ctrs = make_rsrc(a.ct, 16 * 4), cars = make_rsrc(a.ca, 16 * 4);
    Split3 qcls[4];  // ee, eo, oe, oo
    {
        Split3 t2[2];
        bn16_prelu_to_b(accA, csrs, ctrs, cars, h, t2);
        qcls[0] = t2[0]; qcls[1] = t2[1];
        bn16_prelu_to_b(accB, csrs, ctrs, cars, h, t2);
        qcls[2] = t2[0]; qcls[3] = t2[1];
    }

    // ---- expansion 16 -> 64 per (class, N-tile) as D[co][pixel] + unpool-gated residual + PReLU, whole-row stores ----
    const rsrc_t yrs = make_rsrc(yimg, (unsigned)(4 * a.H * a.W * CU) * 4u);
    unsigned yoq[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const int t2 = wave * 32 + (j & ~3) + kk;
        const int iy2 = ty0 + (t2 >> 4), ix2 = tx0 + (t2 & 15);
        yoq[kk] = (iy2 < a.H && ix2 < a.W) ? (unsigned)(((2 * iy2) * (2 * a.W) + 2 * ix2) * (CU * 4) + 32 * (j & 3) + 16 * h) : 0x80000000u;
    }
    const Split3 we0 = load_w(wrs, bf16x3::UP_WE_OFF, lane), we1 = load_w(wrs, bf16x3::UP_WE_OFF + bf16x3::CHUNK_UNITS, lane);
    const float *bnl = BNV + 4 * h;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int cls = m >> 1, nt = m & 1;
        f32x16 e = {0};
        e = mfma6(nt ? we1 : we0, qcls[cls], e);
        const unsigned soff = (unsigned)((((cls >> 1) * (2 * a.W) + (cls & 1)) * CU + nt * 32) * 4);
        float4 ov[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            asm volatile("" ::: "memory");  // keep the LDS reads here (hoisted out of the class loop they would pin registers)
            const float4 s4 = *reinterpret_cast<const float4 *>(bnl + nt * 32 + 8 * g);
            const float4 t4 = *reinterpret_cast<const float4 *>(bnl + CU + nt * 32 + 8 * g);
            const float4 a4 = *reinterpret_cast<const float4 *>(bnl + 2 * CU + nt * 32 + 8 * g);
            const unsigned cd = codes[4 * nt + g];
            const f32x16 &rs = nt ? res1 : res0;
            float4 o;  // unpool_2d as a gather: the residual lands on the output parity its window code names
            o.x = prelu1(fmaf(e[4 * g + 0], s4.x, t4.x) + (((cd >> 0) & 0xFFu) == (unsigned)cls ? rs[4 * g + 0] : 0.0f), a4.x);
            o.y = prelu1(fmaf(e[4 * g + 1], s4.y, t4.y) + (((cd >> 8) & 0xFFu) == (unsigned)cls ? rs[4 * g + 1] : 0.0f), a4.y);
            o.z = prelu1(fmaf(e[4 * g + 2], s4.z, t4.z) + (((cd >> 16) & 0xFFu) == (unsigned)cls ? rs[4 * g + 2] : 0.0f), a4.z);
            o.w = prelu1(fmaf(e[4 * g + 3], s4.w, t4.w) + (((cd >> 24) & 0xFFu) == (unsigned)cls ? rs[4 * g + 3] : 0.0f), a4.w);
            ov[g] = o;
        }
        quad_transpose4(ov[0], ov[1], ov[2], ov[3], lane);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, ov[kk]), yrs, yoq[kk], soff, 0);
    }
}
}  // namespace

bool upsample_bf16x3_supported(int Cin, int Cout) { return Cin == C && Cout == CU; }

// Per-image size limits (ssal_internal.h): the output stores are k_upsample_mfma's (int byte offsets into y [2H,2W,64], the
// 0x80000000 sentinel), so the same 4 * H * W * 64 <= 2^29.  The regular block's are k_bottleneck_mfma's: H * W * 128 <= 2^29.
// The downsample's y offsets ((pixel * C) * 4 in int) would hold up to (H/2) * (W/2) * 128 <= 2^29; its launcher admits the
// H * W * 64 <= 2^29 it always has, and the layer dispatch runs larger shapes on the exact fp32 kernels.
bool upsample_bf16x3_fits(int H, int W) { return (long)4 * H * W * CU <= (1L << 29); }
bool bottleneck_bf16x3_fits(int H, int W) { return (long)H * W * C <= (1L << 29); }
bool downsample_bf16x3_fits(int H, int W) { return (long)H * W * DC <= (1L << 29); }

// x [N,H,W,128] -> y [N,2H,2W,64] with the window codes [N,H,W,64] of the matching downsample; packed = bf16x3::pack_up_layer(...)
hipError_t launch_upsample_bf16x3(const UpArgs &a0, const void *packed, hipStream_t s)
{
    UpArgs a = a0;
    if (!packed || !a.code || a.H < 1 || a.W < 1 || !upsample_bf16x3_fits(a.H, a.W)) return hipErrorInvalidValue;
    a.TH = TH;
    a.tiles_y = (a.H + TH - 1) / TH;
    a.tiles_x = (a.W + TW - 1) / TW;
    const long grid = (long)a.N * a.tiles_y * a.tiles_x;
    if (grid <= 0 || grid > 0x7fffffffL) return hipErrorInvalidValue;
    a.trace = nullptr;
    const double pix = (double)a.N * a.H * a.W;
    ProfScope prof("k_upsample_bf16x3", 2.0 * pix * (C * 32.0 + 9.0 * 32 * 16 + 4.0 * 16 * CU + C * (double)CU),
                   4.0 * (pix * C + 4.0 * pix * CU) + pix * CU, s);
    hipLaunchKernelGGL(k_upsample_bf16x3, dim3((unsigned)grid), dim3(256), 0, s, a, (const uint4 *)packed);
    return hipGetLastError();
}

bool bottleneck_bf16x3_supported(int Cin, int f) { return Cin == C && f == F; }
bool downsample_bf16x3_supported(int Cin, int Cout) { return Cin == DC && Cout == C; }

// x [N,H,W,64] -> y [N,H/2,W/2,128], code [N,H/2,W/2,64]; packed = bf16x3::pack_down_layer(...)
hipError_t launch_downsample_bf16x3(const DownArgs &a0, const void *packed, hipStream_t s)
{
    DownArgs a = a0;
    if (!packed || a.H % 2 || a.W % 2 || a.H < 2 || a.W < 2 || !downsample_bf16x3_fits(a.H, a.W)) return hipErrorInvalidValue;
    const int Ho = a.H / 2, Wo = a.W / 2;
    a.TH = TH;
    a.tiles_y = (Ho + TH - 1) / TH;
    a.tiles_x = (Wo + TW - 1) / TW;
    const long grid = (long)a.N * a.tiles_y * a.tiles_x;
    if (grid <= 0 || grid > 0x7fffffffL) return hipErrorInvalidValue;
    a.trace = nullptr;
    const double opix = (double)a.N * Ho * Wo;
    ProfScope prof("k_downsample_bf16x3", 2.0 * opix * (4.0 * DC * F + 9.0 * F * F + F * (double)C),
                   4.0 * (4.0 * opix * DC + opix * C) + opix * DC, s);
    hipLaunchKernelGGL(k_downsample_bf16x3, dim3((unsigned)grid), dim3(256), 0, s, a, (const uint4 *)packed);
    return hipGetLastError();
}

hipError_t launch_bottleneck_bf16x3(const BnkArgs &a0, const void *packed, hipStream_t s)
{
    BnkArgs a = a0;
    const bool asym = a.wc2 != nullptr;
    if (a.dil < 1 || a.dil > 64 || !packed || (asym && a.dil != 1)) return hipErrorInvalidValue;
    a.TH = TH;
    const int Hp = (a.H + a.dil - 1) / a.dil, Wp = (a.W + a.dil - 1) / a.dil;  // largest phase sub-image
    a.tiles_y = (Hp + TH - 1) / TH;
    a.tiles_x = (Wp + TW - 1) / TW;
    const long grid = (long)a.N * a.dil * a.dil * a.tiles_y * a.tiles_x;
    if (grid <= 0 || grid > 0x3fffffffL || !bottleneck_bf16x3_fits(a.H, a.W)) return hipErrorInvalidValue;
    a.ntiles = (int)grid;
    a.xcd_chunk = knobs().bnk_xcd ? (int)((grid + 7) / 8) : 0;
    const long launch_grid = a.xcd_chunk ? 8L * a.xcd_chunk : grid;
    a.trace = nullptr;
    const double pix = (double)a.N * a.H * a.W, taps = asym ? 10.0 : 9.0;
    ProfScope prof(asym ? "k_bottleneck_asym_bf16x3" : "k_bottleneck_bf16x3", 2.0 * pix * (C * F + taps * F * F + F * C),
                   4.0 * (2.0 * pix * C + C * F * 2.0 + taps * F * F), s);
    if (asym)
        hipLaunchKernelGGL(k_bottleneck_asym_bf16x3, dim3((unsigned)launch_grid), dim3(256), 0, s, a, (const uint4 *)packed);
    else
        hipLaunchKernelGGL(k_bottleneck_bf16x3, dim3((unsigned)launch_grid), dim3(256), 0, s, a, (const uint4 *)packed);
    return hipGetLastError();
}

}  // namespace ssal
