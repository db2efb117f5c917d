// ssal_bf16x3.h -- kernel packing of the opt-in SSAL_ARITH_BF16X3 mode (ssal_bottleneck_bf16x3.hip, ssal_icnet_bf16x3.hip),
// shared by the commit steps (host: ssal_api.hip, ssal_icnet_api.hip) and the kernels, and (device builds only, at the end)
// the mode's activation split and six-product step.  A layer's three kernels are pre-split into bf16 triples (w = w1 + w2 + w3
// exactly, by truncation) and laid out per K = 16 chunk in MFMA operand order: 16-byte UNITS, [chunk][term][lane], where
// operand lane (j = lane & 31, h = lane >> 5) of a v_mfma_f32_32x32x16_bf16 holds k = 8 h + i, i = 0..7, of row / column j.
//   chunks 0 .. 7                      projection   Wp[ci = 16 c + 8 h + i][co = j]
//   chunks 8 .. 8 + 2 taps - 1         convolution  Wc[tap][ci = 16 c2 + 8 h + i][co = j], chunk = 8 + 2 tap + c2
//                                      (asymmetric block: taps 0..4 = the (5,1) kernel, 5..9 = the (1,5) kernel)
//   then 8 chunks                      expansion    We[ci = 16 c + 8 h + i][co = 32 nt + j], chunk = 2 nt + c
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <string.h>

#include <vector>

namespace ssal {
namespace bf16x3 {

constexpr int CHUNK_UNITS = 192;  // 3 terms x 64 lanes
constexpr int WP_OFF = 0;
constexpr int WC_OFF = 8 * CHUNK_UNITS;
constexpr __host__ __device__ int we_off(int taps) { return WC_OFF + 2 * taps * CHUNK_UNITS; }
constexpr __host__ __device__ int units(int taps) { return we_off(taps) + 8 * CHUNK_UNITS; }

// host twin of the device split (ssal_bottleneck_bf16x3.hip: split1): three truncations, each remainder exact in fp32
inline void split_host(float x, uint32_t t[3])
{
    uint32_t u;
    memcpy(&u, &x, 4);
    const uint32_t h1 = u & 0xffff0000u;
    float f1;
    memcpy(&f1, &h1, 4);
    volatile float r1 = x - f1;  // volatile: one rounding per operation, whatever the host compiler would like to contract
    float r1f = r1;
    memcpy(&u, &r1f, 4);
    const uint32_t h2 = u & 0xffff0000u;
    float f2;
    memcpy(&f2, &h2, 4);
    volatile float r2 = r1f - f2;
    float r2f = r2;
    memcpy(&u, &r2f, 4);
    t[0] = h1 >> 16;
    t[1] = h2 >> 16;
    t[2] = u >> 16;
}

// appends one chunk: val(h, i, j) = the fp32 operand element of lane (j, h), k-slot i
template <typename Fn> void pack_chunk(std::vector<float> &out, Fn val)
{
    const size_t base = out.size();
    out.resize(base + (size_t)CHUNK_UNITS * 4);
    uint32_t *dst = reinterpret_cast<uint32_t *>(out.data() + base);
    for (int lane = 0; lane < 64; ++lane) {
        const int j = lane & 31, h = lane >> 5;
        uint32_t t[8][3];
        for (int i = 0; i < 8; ++i) split_host(val(h, i, j), t[i]);
        for (int term = 0; term < 3; ++term)
            for (int m = 0; m < 4; ++m)  // dword m = elements 2m (low half) and 2m + 1 (high half)
                dst[((size_t)term * 64 + lane) * 4 + m] = t[2 * m][term] | (t[2 * m + 1][term] << 16);
    }
}

// the whole layer: wp [128][32], wc [taps][32][32] (asymmetric: the (5,1) kernel followed by the (1,5) kernel), we [32][128];
// returned as floats (bit patterns) so that it travels in the handle's one weight arena
inline std::vector<float> pack_layer(const float *wp, const float *wc, const float *wc2, int taps, const float *we)
{
    std::vector<float> out;
    out.reserve((size_t)units(taps) * 4);
    for (int c = 0; c < 8; ++c) pack_chunk(out, [&](int h, int i, int j) { return wp[(16 * c + 8 * h + i) * 32 + j]; });
    for (int tap = 0; tap < taps; ++tap) {
        const float *w = (wc2 && tap >= 5) ? wc2 + (size_t)(tap - 5) * 32 * 32 : wc + (size_t)tap * 32 * 32;
        for (int c2 = 0; c2 < 2; ++c2) pack_chunk(out, [&](int h, int i, int j) { return w[(16 * c2 + 8 * h + i) * 32 + j]; });
    }
    for (int nt = 0; nt < 4; ++nt)
        for (int c = 0; c < 2; ++c) pack_chunk(out, [&](int h, int i, int j) { return we[(16 * c + 8 * h + i) * 128 + 32 * nt + j]; });
    return out;
}

// Downsample bottleneck 64 -> 128 (Bottleneck2_0): wp [2][2][64][32] (K = 4 taps x 64 channels = 16 chunks), wc [9][32][32],
// we [32][128] (the expansion runs as D[co][pixel] there: the chunk is the A operand, rows = output channels 32 nt + j)
constexpr int DN_WP_OFF = 0;
constexpr int DN_WC_OFF = 16 * CHUNK_UNITS;
constexpr int DN_WE_OFF = DN_WC_OFF + 18 * CHUNK_UNITS;
constexpr int DN_UNITS = DN_WE_OFF + 8 * CHUNK_UNITS;
inline std::vector<float> pack_down_layer(const float *wp, const float *wc, const float *we)
{
    std::vector<float> out;
    out.reserve((size_t)DN_UNITS * 4);
    // chunk s = 4 cc + t: tap t = dy * 2 + dx of channel group cc; k-slot (h, i) = channel 16 cc + 4 h + (i & 3) + 8 (i >> 2) -- a
    // lane half then holds the channels c with (c >> 2) & 1 == h, the ones a D[co][pixel] accumulator gives it: the pooled
    // residual of the block meets the expansion's output in the same lane (ssal_bottleneck_bf16x3.hip: project_down)
    for (int s = 0; s < 16; ++s)
        pack_chunk(out, [&](int h, int i, int j) {
            return wp[((s & 3) * 64 + 16 * (s >> 2) + 4 * h + (i & 3) + 8 * (i >> 2)) * 32 + j];
        });
    for (int tap = 0; tap < 9; ++tap)
        for (int c2 = 0; c2 < 2; ++c2)
            pack_chunk(out, [&](int h, int i, int j) { return wc[((size_t)tap * 32 + 16 * c2 + 8 * h + i) * 32 + j]; });
    for (int nt = 0; nt < 4; ++nt)
        for (int c = 0; c < 2; ++c) pack_chunk(out, [&](int h, int i, int j) { return we[(16 * c + 8 * h + i) * 128 + 32 * nt + j]; });
    return out;
}

// Upsample bottleneck 128 -> 64 (Bottleneck4_0): wp [128][32], wr (residual 1x1) [128][64], ws = the stacked transposed-conv
// kernel [6 slots][32 ci][32 rows = two output-parity classes x 16 channels] (ssal_api.hip: stack_convT), we [16][64].  Every
// chunk is an A operand (rows = output channels / stacked rows), the activations are the B operand (columns = pixels).
constexpr int UP_WP_OFF = 0;                                   // 8 chunks
constexpr int UP_WR_OFF = 8 * CHUNK_UNITS;                     // chunk 2 c + nt, c = 0..7
constexpr int UP_WS_OFF = UP_WR_OFF + 16 * CHUNK_UNITS;        // chunk 2 slot + c2
constexpr int UP_WE_OFF = UP_WS_OFF + 12 * CHUNK_UNITS;        // chunk nt (K = 16: one chunk)
constexpr int UP_UNITS = UP_WE_OFF + 2 * CHUNK_UNITS;
inline std::vector<float> pack_up_layer(const float *wp, const float *wr, const float *ws, const float *we)
{
    std::vector<float> out;
    out.reserve((size_t)UP_UNITS * 4);
    for (int c = 0; c < 8; ++c) pack_chunk(out, [&](int h, int i, int j) { return wp[(16 * c + 8 * h + i) * 32 + j]; });
    for (int c = 0; c < 8; ++c)
        for (int nt = 0; nt < 2; ++nt) pack_chunk(out, [&](int h, int i, int j) { return wr[(16 * c + 8 * h + i) * 64 + 32 * nt + j]; });
    for (int sl = 0; sl < 6; ++sl)
        for (int c2 = 0; c2 < 2; ++c2) pack_chunk(out, [&](int h, int i, int j) { return ws[((size_t)sl * 32 + 16 * c2 + 8 * h + i) * 32 + j]; });
    for (int nt = 0; nt < 2; ++nt) pack_chunk(out, [&](int h, int i, int j) { return we[(8 * h + i) * 64 + 32 * nt + j]; });
    return out;
}

// One convolution of ICNet's implicit GEMM (ssal_icnet_bf16x3.hip: k_igemm_bf16x3): kernel [KH*KW][Cin][Cout] (HWIO) ->
// [tap][Cin/16][CoutP/32] chunks, chunk (tap, c, nt) = W[tap][ci = 16 c + 8 h + i][co = 32 nt + j]; output channels are
// zero-padded to CoutP = Cout rounded up to 32 (the split of 0 is (0, 0, 0)).  1.5x the bytes of the fp32 kernel.
inline size_t igemm_units(int KH, int KW, int Cin, int Cout)
{
    return (size_t)KH * KW * (Cin / 16) * ((Cout + 31) / 32) * CHUNK_UNITS;
}
inline std::vector<float> pack_igemm(const float *w, int KH, int KW, int Cin, int Cout)
{
    std::vector<float> out;
    out.reserve(igemm_units(KH, KW, Cin, Cout) * 4);
    const int nb32 = (Cout + 31) / 32;
    for (int tap = 0; tap < KH * KW; ++tap)
        for (int c = 0; c < Cin / 16; ++c)
            for (int nt = 0; nt < nb32; ++nt)
                pack_chunk(out, [&](int h, int i, int j) {
                    const int co = 32 * nt + j;
                    return co < Cout ? w[((size_t)tap * Cin + 16 * c + 8 * h + i) * Cout + co] : 0.0f;
                });
    return out;
}

#ifdef __HIPCC__
// ---- device side: the activation split and the six-product step, shared by every kernel of the mode ----
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float acc16 __attribute__((ext_vector_type(16)));  // == ssal::f32x16 (ssal_mfma.h)

struct Split3 {
    uint4 t1, t2, t3;  // 8 values each: the leading bf16, the bf16 of the remainder, the bf16 of what remains after that
};

__device__ __forceinline__ unsigned pack_hi(unsigned lo, unsigned hi) { return __builtin_amdgcn_perm(hi, lo, 0x07060302u); }

// x = h1 + h2 + h3 exactly; h1, h2 are fp32 values with 16 zero low bits, h3 fits 8 significant bits (its low 16 bits are 0)
__device__ __forceinline__ void split1(float x, unsigned &h1, unsigned &h2, unsigned &h3)
{
    h1 = __float_as_uint(x) & 0xffff0000u;
    const float r1 = x - __uint_as_float(h1);
    h2 = __float_as_uint(r1) & 0xffff0000u;
    const float r2 = r1 - __uint_as_float(h2);
    h3 = __float_as_uint(r2);
}

__device__ __forceinline__ Split3 split_pack8(const float (&v)[8])
{
    unsigned a[8], b[8], c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) split1(v[k], a[k], b[k], c[k]);
    Split3 s;
    s.t1 = make_uint4(pack_hi(a[0], a[1]), pack_hi(a[2], a[3]), pack_hi(a[4], a[5]), pack_hi(a[6], a[7]));
    s.t2 = make_uint4(pack_hi(b[0], b[1]), pack_hi(b[2], b[3]), pack_hi(b[4], b[5]), pack_hi(b[6], b[7]));
    s.t3 = make_uint4(pack_hi(c[0], c[1]), pack_hi(c[2], c[3]), pack_hi(c[4], c[5]), pack_hi(c[6], c[7]));
    return s;
}

__device__ __forceinline__ acc16 mfma_bf(uint4 a, uint4 b, acc16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// one K = 16 step: the six leading cross products, small terms first
__device__ __forceinline__ acc16 mfma6(const Split3 &a, const Split3 &b, acc16 c)
{
    c = mfma_bf(a.t3, b.t1, c);
    c = mfma_bf(a.t2, b.t2, c);
    c = mfma_bf(a.t1, b.t3, c);
    c = mfma_bf(a.t2, b.t1, c);
    c = mfma_bf(a.t1, b.t2, c);
    c = mfma_bf(a.t1, b.t1, c);
    return c;
}
#endif  // __HIPCC__

}  // namespace bf16x3
}  // namespace ssal
