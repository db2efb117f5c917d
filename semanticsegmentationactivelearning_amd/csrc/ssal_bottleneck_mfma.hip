// ssal_bottleneck_mfma.hip -- ENet regular / dilated bottleneck (enet_modules.py:526-599) as ONE
// kernel on the gfx950 matrix cores:  1x1 proj + BN + PReLU -> 3x3 (dilated) conv + BN + PReLU ->
// 1x1 exp + BN -> + identity residual -> PReLU.  The block input is read once (plus halo) and the
// block output written once; the C/4-wide intermediates never leave the CU.
//
// Arithmetic: v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate) is bit-for-bit a k-ordered fmaf
// chain, and every GEMM below feeds its k-pairs in ascending (kh, kw, ci) order, so the result is
// bit-identical to the generic kernels and to the parity oracle.
//
// Tiling: a dilated 3x3 conv decomposes into dil x dil independent phase sub-images
// (y = py + dil*r, x = px + dil*c); a workgroup owns a TH x TW tile of ONE phase sub-image, so the
// halo is always one pixel (in phase space) whatever the dilation.
//   phase A  proj:  D[pixel][co]  = X[pixel][ci]   * Wp[ci][co]    (halo'd tile, 32-pixel M-tiles)
//            -> BN + PReLU, zero outside the image, -> LDS  P[(TH+2)*(TW+2)][32 (+2 pad)]
//   phase B  conv:  D[co][pixel]  = Wc^T[co][tap,ci] * P[tap,ci][pixel]   (9 taps x 32 ci)
//            -> BN + PReLU in registers; the accumulator tile IS the next A operand (lane = pixel)
//            exp:   D[pixel][co]  = Q[pixel][ci] * We[ci][co]      (4 N-tiles of 32)
//            -> BN, + x, PReLU, coalesced 128-B row stores.
// MFMA 32x32x2 lane maps (l = lane, r = l & 31, h = l >> 5):
//   A: lane holds A[row r][k = h]    B: lane holds B[k = h][col r]
//   D: reg i of lane holds D[row (i&3) + 8*(i>>2) + 4*h][col r]
// An instruction consumes k0 (lanes 0-31) then k1 (lanes 32-63); v_permlane32_swap pairs registers
// so that consecutive channels sit in the two lane halves (ascending-k accumulation).
#include "ssal_internal.h"
#include "ssal_mfma.h"
#include "ssal_bottleneck_args.h"
#include "ssal_prof.h"
#include <stdlib.h>
#include <type_traits>

namespace ssal {

constexpr int F = 32;         // bottleneck width
constexpr int C = 128;        // block channels
constexpr int PSTR = F + 2;   // LDS pixel stride in dwords: conflict-free ds_read_b64 / ds_write_b32
// Channel order inside an LDS pixel row: every group of 8 channels is stored as [c0 c2 c4 c6 | c1 c3 c5 c7], so the
// float2 a lane half reads at 8g + 4h (+2) holds, register by register, the (k = 2s | k = 2s + 1) pair of MFMA step s:
// no v_permlane32_swap between the LDS read and the MFMA.  (A swap costs ~13 SIMD cycles and, like every vector
// instruction, executes INSTEAD of the fp32 MFMAs, never beside them: tools/mfma_peak.py.)
__device__ __forceinline__ int kperm(int c) { return (c & ~7) | ((c & 1) << 2) | ((c & 7) >> 1); }
// the sq-th float2 (sq = 0..7) of a lane half's operand sequence inside a permuted row: steps 2sq, 2sq + 1
__device__ __forceinline__ int kperm_rd(int sq, int h) { return 8 * (sq >> 1) + 4 * h + 2 * (sq & 1); }
constexpr int PMAX = 352;     // >= (TH+2)*(TW+2) rounded up to a multiple of 32



// ---- phase A (shared by the regular and the asymmetric kernel): 1x1 projection + BN + PReLU of the
// halo'd tile into LDS; pixels outside the image are written as exact zeros (SAME padding of the
// following conv applies to the PROJECTED tensor).  HALO = 1 (3x3) or 2 (5x1 / 1x5).
// WQ: the kernel fragments come from the QUAD layout a.wq (ssal_host.h: bnk_quad_layout; round 5): element i of float4
// (q, lane) = the fragment of MFMA step 4 q + i -- one buffer_load_b128 per four steps instead of four buffer_load_b32
// (the round-5 counters show the vector-memory address unit 56 % busy in this kernel, 750 load instructions per wave)
template <int TW, int HALO, typename Args, bool WQ = false>
__device__ __forceinline__ void proj_to_lds(const Args &a, const float *ximg, float *P, int TH,
                                            int ty0, int tx0, int py, int px, int Hp, int Wp,
                                            int wave, int j, int h, int prows = PMAX)
{   // prows = rows P has room for (the last M-tile may reach beyond the halo'd tile)
    constexpr int HWP = TW + 2 * HALO;
    const int d = a.dil;
    const int npix_halo = (TH + 2 * HALO) * HWP;
    // B operand (Wp[ci][co]) for all 64 k-pair steps stays in registers for this wave's M-tiles
    // (rows 2s, 2s+1 of Wp are 64 consecutive floats: fragment s of lane l = Wp[64 s + l]).
    // The first KEEP k-pair steps stay in registers; the tail is re-fetched (L1) per M-tile into the
    // registers the first activation fragments have just vacated -- this keeps the kernel at 168 VGPRs
    // = 3 workgroups per CU.
#ifndef SSAL_KEEP
#define SSAL_KEEP 36
#endif
    constexpr int KEEP = SSAL_KEEP, UK = KEEP / 4;  // UK = float4 fragments covered by the resident part (24 .. 48 swept in round 4: profiles/r04_ab_keep_sweep.txt)
    float wpr[KEEP];
    const rsrc_t wrs = make_rsrc(WQ ? a.wq + quad::WP : a.wp, C * F * 4);
    const unsigned wlo = WQ ? (unsigned)(h * 32 + j) * 16u : (unsigned)(h * 32 + j) * 4u;
    if (WQ) {
#pragma unroll
        for (int q = 0; q < KEEP / 4; ++q) {
            const float4 w4 = bload4(wrs, wlo, q * 1024);
            wpr[4 * q] = w4.x; wpr[4 * q + 1] = w4.y; wpr[4 * q + 2] = w4.z; wpr[4 * q + 3] = w4.w;
        }
    } else {
#pragma unroll
        for (int s = 0; s < KEEP; ++s) wpr[s] = bload(wrs, wlo, s * 256);
    }
    const float bs = a.ps[j], bt = a.pt[j], ba = a.pa[j];

    const int nmt = (npix_halo + 31) / 32;
    for (int mt = wave; mt < nmt; mt += 4) {
        const int q = mt * 32 + j;
        const int hr = q / HWP, hc = q - hr * HWP;
        const int pr = ty0 - HALO + hr, pc = tx0 - HALO + hc;
        const bool valid = (q < npix_halo) && (pr >= 0) && (pr < Hp) && (pc >= 0) && (pc < Wp);
        const unsigned long long vmask = __ballot(valid);
        if (vmask == 0ull) {  // wave-uniform: M-tile entirely outside the image -> zeros
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int qi = mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (qi < prows) P[qi * PSTR + kperm(j)] = 0.0f;
            }
            continue;
        }
        const float *xp = valid ? ximg + ((long)(py + pr * d) * a.W + (px + pc * d)) * C : ximg;
        if (SSAL_ABLATE_IS(a, 6) || SSAL_ABLATE_IS(a, 7)) xp = ximg;  // timing only: every lane reads pixel 0 (cache hits)
        // all 16 activation fragments of the M-tile are requested before the first MFMA (the compiler
        // would otherwise serialise load-pair / wait / 8 MFMAs and expose the memory latency 8 times)
        float4 X[16];
#pragma unroll
        for (int u = 0; u < 16; ++u)  // lane half h takes the h-th float4 of every 8 channels
            X[u] = *reinterpret_cast<const float4 *>(xp + (2 * u + h) * 4);
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc = {0};
        auto step = [&](int u, float w0, float w1, float w2, float w3) {
            float a0 = X[u].x, a1 = X[u].y, a2 = X[u].z, a3 = X[u].w;
            swap32(a0, a1);  // a0 = ch(8u+0 | 8u+1), a1 = ch(8u+4 | 8u+5)
            swap32(a2, a3);  // a2 = ch(8u+2 | 8u+3), a3 = ch(8u+6 | 8u+7)
            acc = mfma32(a0, w0, acc);
            acc = mfma32(a2, w1, acc);
            acc = mfma32(a1, w2, acc);
            acc = mfma32(a3, w3, acc);
        };
        constexpr int U1 = (64 - KEEP) / 4;  // fragments whose registers the tail weights take over
#pragma unroll
        for (int u = 0; u < U1; ++u)  // float4 u of half h = channels 8u + 4h .. 8u + 4h + 3
            step(u, wpr[4 * u], wpr[4 * u + 1], wpr[4 * u + 2], wpr[4 * u + 3]);
        __builtin_amdgcn_sched_barrier(0);
        float wt[64 - KEEP];
        if (WQ) {
#pragma unroll
            for (int q = KEEP / 4; q < 16; ++q) {
                const float4 w4 = bload4(wrs, wlo, q * 1024);
                wt[4 * q - KEEP] = w4.x; wt[4 * q + 1 - KEEP] = w4.y; wt[4 * q + 2 - KEEP] = w4.z; wt[4 * q + 3 - KEEP] = w4.w;
            }
        } else {
#pragma unroll
            for (int s = KEEP; s < 64; ++s) wt[s - KEEP] = bload(wrs, wlo, s * 256);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = U1; u < UK; ++u)
            step(u, wpr[4 * u], wpr[4 * u + 1], wpr[4 * u + 2], wpr[4 * u + 3]);
#pragma unroll
        for (int u = UK; u < 16; ++u)
            step(u, wt[4 * (u - UK)], wt[4 * (u - UK) + 1], wt[4 * (u - UK) + 2], wt[4 * (u - UK) + 3]);
        // epilogue: rows = pixels (registers), cols = co (lanes): BN + PReLU, zero padding
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int ri = (i & 3) + 8 * (i >> 2) + 4 * h;
            const bool ok = (vmask >> ri) & 1ull;
            const float v = ok ? prelu1(fmaf(acc[i], bs, bt), ba) : 0.0f;
            if (mt * 32 + ri < prows) P[(mt * 32 + ri) * PSTR + kperm(j)] = v;
        }
    }
}

// ---- asymmetric only: R1 = conv (5,1) of P, no BN / activation (enet_modules.py:553-558), for the
// TH x (TW+4) pixels the (1,5) conv needs; D[pixel][co] = P[pixel + kh][ci] * W0[kh][ci][co] -> LDS.
// computes nmt M-tiles of the (5,1) result, pixels u0 .. u0 + 32 nmt - 1 of the row-major 8 x HWP result grid,
// into R slots 0 .. 32 nmt - 1
template <int TW>
__device__ __forceinline__ void conv5x1_to_lds(const BnkArgs &a, const float *P, float *R, int u0, int nmt,
                                               int wave, int j, int h)
{
    constexpr int HWP = TW + 4;
    const rsrc_t wrs = make_rsrc(a.wc, 5 * F * F * 4);
    const unsigned lo = (unsigned)(h * 32 + j) * 4u;
    for (int mt = wave; mt < nmt; mt += 4) {
        const int u = u0 + mt * 32 + j;
        f32x16 acc = {0};
        // one tap ahead, as in conv_tile_q: kernel fragments (L1/L2) and LDS fragments of tap kh+1 are
        // requested before the 16 MFMAs of tap kh
        float wA[16], wB[16];
        float2 pA[8], pB[8];
        auto load_tap = [&](int kh, float (&w)[16], float2 (&pv)[8]) {
#pragma unroll
            for (int k = 0; k < 16; ++k) w[k] = bload(wrs, lo, kh * (F * F * 4) + k * 256);  // W0[kh][2k + h][j]
            const float *pq = P + (u + kh * HWP) * PSTR;  // result pixel u = (r, c') reads P rows r + kh
#pragma unroll
            for (int sq = 0; sq < 8; ++sq) pv[sq] = *reinterpret_cast<const float2 *>(pq + kperm_rd(sq, h));
        };
        auto run_tap = [&](const float (&w)[16], const float2 (&pv)[8]) {
#pragma unroll
            for (int sq = 0; sq < 8; ++sq) {  // permuted rows: .x = ci(4sq | 4sq+1), .y = ci(4sq+2 | 4sq+3)
                acc = mfma32(pv[sq].x, w[2 * sq], acc);
                acc = mfma32(pv[sq].y, w[2 * sq + 1], acc);
            }
        };
        load_tap(0, wA, pA);
#pragma unroll 1
        for (int kh = 0; kh + 1 < 5; kh += 2) {
            load_tap(kh + 1, wB, pB);
            __builtin_amdgcn_sched_barrier(0);
            run_tap(wA, pA);
            __builtin_amdgcn_sched_barrier(0);
            load_tap(kh + 2, wA, pA);
            __builtin_amdgcn_sched_barrier(0);
            run_tap(wB, pB);
            __builtin_amdgcn_sched_barrier(0);
        }
        run_tap(wA, pA);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int ri = (i & 3) + 8 * (i >> 2) + 4 * h;
            R[(mt * 32 + ri) * PSTR + kperm(j)] = acc[i];
        }
    }
}

// one M-tile of the (5,1) result (pixels u0 .. u0 + 31 of the row-major 8 x HWP result grid) as an accumulator: rows =
// pixels (registers), cols = co (lanes); taps one ahead as in conv5x1_to_lds
template <int TW>
__device__ __forceinline__ f32x16 conv5x1_tile(const BnkArgs &a, const float *P, int u0, int j, int h)
{   // kernel fragments from the quad layout (taps 0..4 of a.wq's convolution part)
    constexpr int HWP = TW + 4;
    const rsrc_t wrs = make_rsrc(a.wq + quad::WC, 5 * F * F * 4);
    const unsigned lo = (unsigned)(h * 32 + j) * 16u;
    const int u = u0 + j;
    f32x16 acc = {0};
    float wA[16], wB[16];
    float2 pA[8], pB[8];
    auto load_tap = [&](int kh, float (&w)[16], float2 (&pv)[8]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // W0[kh][2 (4q + i) + h][j], i = 0..3
            const float4 w4 = bload4(wrs, lo, kh * (F * F * 4) + q * 1024);
            w[4 * q] = w4.x; w[4 * q + 1] = w4.y; w[4 * q + 2] = w4.z; w[4 * q + 3] = w4.w;
        }
        const float *pq = P + (u + kh * HWP) * PSTR;
#pragma unroll
        for (int sq = 0; sq < 8; ++sq) pv[sq] = *reinterpret_cast<const float2 *>(pq + kperm_rd(sq, h));
    };
    auto run_tap = [&](const float (&w)[16], const float2 (&pv)[8]) {
#pragma unroll
        for (int sq = 0; sq < 8; ++sq) {
            acc = mfma32(pv[sq].x, w[2 * sq], acc);
            acc = mfma32(pv[sq].y, w[2 * sq + 1], acc);
        }
    };
    load_tap(0, wA, pA);
#pragma unroll 1
    for (int kh = 0; kh + 1 < 5; kh += 2) {
        load_tap(kh + 1, wB, pB);
        __builtin_amdgcn_sched_barrier(0);
        run_tap(wA, pA);
        __builtin_amdgcn_sched_barrier(0);
        load_tap(kh + 2, wA, pA);
        __builtin_amdgcn_sched_barrier(0);
        run_tap(wB, pB);
        __builtin_amdgcn_sched_barrier(0);
    }
    run_tap(wA, pA);
    return acc;
}

// ---- KH x KW conv (F -> F) over an LDS tensor S (row stride SW pixels) for one 32-pixel M-tile,
// + BN + PReLU; returns the result as the A operand of the following expansion GEMM:
// qv[ord(s)] of lane (pixel j, half h) = Q[pixel][ci = 2s + h].
// WRAP > 0 (asymmetric block, second half): S is a ring of WRAP pixel slots, the pixel index is shifted by
// soff (< 0) and indices that become negative wrap to the end of the ring.
template <int TW, int KH, int KW, int SW, typename Args, int WRAP = 0, bool WQ = false>
__device__ __forceinline__ void conv_tile_q(const Args &a, const float *S, const float *wconv, int mt,
                                            int j, int h, float (&qv)[16], int soff = 0)
{   // WQ: wconv is the QUAD layout [tap][q][lane][4] (see proj_to_lds)
    const int t = mt * 32 + j;  // this lane's output pixel inside the tile (B operand)
    const int r = t / TW, c = t - r * TW;
    f32x16 acc = {0};
    // Software pipeline, one tap deep: while the 16 MFMAs of tap t run (~1000 cycles), the 16 weight
    // fragments (L2) and the 8 activation fragments (LDS) of tap t+1 are already in flight.  Two
    // static register buffers (A/B) alternate inside a loop over tap PAIRS; sched_barrier(0) keeps
    // the compiler from sinking the loads next to their uses.
    constexpr int NTAP = KH * KW;  // 9 or 5: odd
    float wA[16], wB[16];
    float2 pA[8], pB[8];
    const rsrc_t wrs = make_rsrc(wconv, NTAP * F * F * 4);
    const unsigned lo = WQ ? (unsigned)(h * 32 + j) * 16u : (unsigned)(h * 32 + j) * 4u;
    auto load_tap = [&](int tap, float (&w)[16], float2 (&p)[8]) {
        const int kh = tap / KW, kw = tap - KW * kh;
        if (WQ) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 w4 = bload4(wrs, lo, tap * (F * F * 4) + q * 1024);
                w[4 * q] = w4.x; w[4 * q + 1] = w4.y; w[4 * q + 2] = w4.z; w[4 * q + 3] = w4.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k)  // W[tap][ci = 2k + h][co = j]: rows 2k, 2k+1 = 64 consecutive floats
                w[k] = bload(wrs, lo, tap * (F * F * 4) + k * 256);
        }
        int slot = (r + kh) * SW + (c + kw);
        if (WRAP > 0) {
            slot += soff;
            slot = slot < 0 ? slot + WRAP : slot;
        }
        const float *pq = S + slot * PSTR;
#pragma unroll
        for (int sq = 0; sq < 8; ++sq) p[sq] = *reinterpret_cast<const float2 *>(pq + kperm_rd(sq, h));
    };
    auto run_tap = [&](const float (&w)[16], const float2 (&p)[8]) {
#pragma unroll
        for (int sq = 0; sq < 8; ++sq) {  // permuted rows: .x = ci(4sq | 4sq+1), .y = ci(4sq+2 | 4sq+3)
            acc = mfma32(w[2 * sq], p[sq].x, acc);      // W[tap][ci = 4sq + h][co = j]
            acc = mfma32(w[2 * sq + 1], p[sq].y, acc);  // W[tap][ci = 4sq + 2 + h][co = j]
        }
    };
    load_tap(0, wA, pA);
#pragma unroll 1
    for (int tp = 0; tp + 1 < NTAP; tp += 2) {
        load_tap(tp + 1, wB, pB);
        __builtin_amdgcn_sched_barrier(0);
        run_tap(wA, pA);
        __builtin_amdgcn_sched_barrier(0);
        load_tap(tp + 2, wA, pA);  // tp + 2 <= NTAP - 1 because NTAP is odd
        __builtin_amdgcn_sched_barrier(0);
        run_tap(wB, pB);
        __builtin_amdgcn_sched_barrier(0);
    }
    run_tap(wA, pA);  // the last (odd) tap
    // conv epilogue: rows = co (registers), cols = pixel (lanes); co = 8g + 4h + (0..3) per group g
    {
        const rsrc_t srs = make_rsrc(a.cs, F * 4), trs = make_rsrc(a.ct, F * 4), ars = make_rsrc(a.ca, F * 4);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 s4 = bload4(srs, h * 16, g * 32), t4 = bload4(trs, h * 16, g * 32),
                         a4 = bload4(ars, h * 16, g * 32);
            qv[4 * g + 0] = prelu1(fmaf(acc[4 * g + 0], s4.x, t4.x), a4.x);
            qv[4 * g + 1] = prelu1(fmaf(acc[4 * g + 1], s4.y, t4.y), a4.y);
            qv[4 * g + 2] = prelu1(fmaf(acc[4 * g + 2], s4.z, t4.z), a4.z);
            qv[4 * g + 3] = prelu1(fmaf(acc[4 * g + 3], s4.w, t4.w), a4.w);
        }
    }
    // the accumulator tile becomes the A operand of the expansion GEMM (lane = pixel)
#pragma unroll
    for (int u = 0; u < 8; ++u) swap32(qv[2 * u], qv[2 * u + 1]);
}

// ---- last phase of the regular / asymmetric bottleneck: conv, then 1x1 expansion + BN + identity
// residual + PReLU straight to HBM.
// QEPI = 2 (round 5, needs WQ; k_bottleneck_mfma<32>): the expansion runs as D[co][pixel] (operands swapped: the same products in
// the same k order, i.e. the same bits; lane = pixel, four consecutive channels per register group), the residual arrives as
// four 16-byte loads and the output leaves as four 16-byte stores per N-tile -- whole 128-byte rows through quad_transpose4 --
// instead of 16 + 16 four-byte accesses and three BN loads: 224 -> 116 vector-memory instructions per M-tile for +256 VALU.
// bnv = es | et | ra staged in LDS by the kernel (the per-channel constants are per REGISTER in this form).  QEPI = 1: the
// lane's own 16 bytes per store (no transpose; slower).  Measured (profiles/r05_ab_epilogue_co_major_16B.txt): the kernel alone
// -7 %, the single-chain pass +1 %, the two-chain pass +-0; the asymmetric kernel (one M-tile per wave) loses 7 % with it.
template <int TW, int KH, int KW, int SW, int WRAP = 0, bool WQ = false, int QEPI = 0>
__device__ __forceinline__ void conv_exp_store(const BnkArgs &a, const float *ximg, float *yimg,
                                               const float *S, const float *wconv, int TH, int ty0,
                                               int tx0, int py, int px, int Hp, int Wp, int wave,
                                               int j, int h, PhaseTrace &tr, int soff = 0, const float *bnv = nullptr)
{
    const int d = a.dil;
    const int nmt_out = (TH * TW) / 32;
    int trk = 3;
    if (QEPI > 0) {
        const int lane = h * 32 + j;
        const unsigned img_bytes = (unsigned)(a.H * a.W * C) * 4u;
        const rsrc_t xrs = make_rsrc(ximg, img_bytes), yrs = make_rsrc(yimg, img_bytes);
        const rsrc_t wers = make_rsrc(a.wq + quad::we(KH * KW == 9 ? 9 : 10), F * C * 4);
        const unsigned welo = (unsigned)(h * 32 + j) * 16u;
        const float *bnl = bnv + 4 * h;  // es | et | ra of channels 32 nt + 8 g + 4 h .. + 3
        for (int mt = wave; mt < nmt_out; mt += 4) {
            float qv[16];
            conv_tile_q<TW, KH, KW, SW, BnkArgs, WRAP, WQ>(a, S, wconv, mt, j, h, qv, soff);
            if (mt == wave) tr.mark(trk++);
            // own pixel (residual loads; QEPI = 1 stores) and the four pixels of the lane's quad (QEPI = 2 stores)
            unsigned xo, yoq[4];
            {
                const int ti = mt * 32 + j, rr = ti / TW, cc = ti - rr * TW, pr = ty0 + rr, pc = tx0 + cc;
                xo = (pr < Hp && pc < Wp) ? (unsigned)(((py + pr * d) * a.W + (px + pc * d)) * (C * 4) + 16 * h) : 0x80000000u;
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int ti = mt * 32 + (j & ~3) + kk, rr = ti / TW, cc = ti - rr * TW, pr = ty0 + rr, pc = tx0 + cc;
                yoq[kk] = (pr < Hp && pc < Wp) ? (unsigned)(((py + pr * d) * a.W + (px + pc * d)) * (C * 4) + 32 * (j & 3) + 16 * h) : 0x80000000u;
            }
            float weA[16], weB[16];
            float4 rxA[4], rxB[4];
            auto fetch = [&](int nt, float (&we)[16], float4 (&rx)[4]) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 w4 = bload4(wers, welo, nt * 4096 + q * 1024);
                    we[4 * q] = w4.x; we[4 * q + 1] = w4.y; we[4 * q + 2] = w4.z; we[4 * q + 3] = w4.w;
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) rx[g] = bload4(xrs, xo, nt * 128 + g * 32);  // channels 32 nt + 8 g + 4 h .. + 3
            };
            auto epi = [&](int nt, const f32x16 &e, const float4 (&rx)[4]) {
                float4 ov[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    asm volatile("" ::: "memory");  // keep the LDS reads here (hoisted they would pin registers)
                    const float4 s4 = *reinterpret_cast<const float4 *>(bnl + nt * 32 + 8 * g);
                    const float4 t4 = *reinterpret_cast<const float4 *>(bnl + C + nt * 32 + 8 * g);
                    const float4 a4 = *reinterpret_cast<const float4 *>(bnl + 2 * C + nt * 32 + 8 * g);
                    ov[g].x = prelu1(fmaf(e[4 * g + 0], s4.x, t4.x) + rx[g].x, a4.x);
                    ov[g].y = prelu1(fmaf(e[4 * g + 1], s4.y, t4.y) + rx[g].y, a4.y);
                    ov[g].z = prelu1(fmaf(e[4 * g + 2], s4.z, t4.z) + rx[g].z, a4.z);
                    ov[g].w = prelu1(fmaf(e[4 * g + 3], s4.w, t4.w) + rx[g].w, a4.w);
                }
                if (QEPI == 2) {
                    quad_transpose4(ov[0], ov[1], ov[2], ov[3], lane);
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, ov[kk]), yrs, yoq[kk], nt * 128, 0);
                } else {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, ov[g]), yrs, xo, nt * 128 + g * 32, 0);
                }
            };
            __builtin_amdgcn_sched_barrier(0);
            fetch(0, weA, rxA);
            fetch(1, weB, rxB);
            f32x16 e0 = {0}, e1 = {0};
#pragma unroll
            for (int s = 0; s < 16; ++s) e0 = mfma32(weA[s], qv[ord(s)], e0);  // D[co][pixel]: A = We^T (rows co), B = Q
#pragma unroll
            for (int s = 0; s < 16; ++s) e1 = mfma32(weB[s], qv[ord(s)], e1);
            epi(0, e0, rxA);
            __builtin_amdgcn_sched_barrier(0);
            fetch(2, weA, rxA);
            e0 = (f32x16){0};
#pragma unroll
            for (int s = 0; s < 16; ++s) e0 = mfma32(weA[s], qv[ord(s)], e0);
            epi(1, e1, rxB);
            __builtin_amdgcn_sched_barrier(0);
            fetch(3, weB, rxB);
            e1 = (f32x16){0};
#pragma unroll
            for (int s = 0; s < 16; ++s) e1 = mfma32(weB[s], qv[ord(s)], e1);
            epi(2, e0, rxA);
            __builtin_amdgcn_sched_barrier(0);
            epi(3, e1, rxB);
            if (mt == wave) tr.mark(trk++);
        }
        return;
    }
    // raw buffer resources over image n of x and y (num_records = image bytes <= 2 GiB: bottleneck_mfma_fits); kOOB is an
    // offset the range check always rejects, even after the +384 B N-tile immediates
    constexpr unsigned kOOB = 0x80000000u;
    const unsigned img_bytes = (unsigned)(a.H * a.W * C) * 4u;
    // measurement builds (timing only, results invalid): ablate 3 / 5 / 7 give the residual resource zero records (every
    // load is answered with 0 by the range check, no memory traffic), 4 / 5 / 7 the output resource (stores dropped)
    const unsigned xbytes = (SSAL_ABLATE_IS(a, 3) || SSAL_ABLATE_IS(a, 5) || SSAL_ABLATE_IS(a, 7)) ? 0u : img_bytes;
    const unsigned ybytes = (SSAL_ABLATE_IS(a, 4) || SSAL_ABLATE_IS(a, 5) || SSAL_ABLATE_IS(a, 7)) ? 0u : img_bytes;
    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(ximg), 0, xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(yimg, 0, ybytes, 0x00020000);
    const rsrc_t wers = make_rsrc(WQ ? a.wq + quad::we(KH * KW == 9 ? 9 : 10) : a.we, F * C * 4), esrs = make_rsrc(a.es, C * 4), etrs = make_rsrc(a.et, C * 4),
                 rars = make_rsrc(a.ra, C * 4);
    const unsigned welo = WQ ? (unsigned)(h * 32 + j) * 16u : (unsigned)(h * C + j) * 4u;
    for (int mt = wave; mt < nmt_out; mt += 4) {
        float qv[16];
        conv_tile_q<TW, KH, KW, SW, BnkArgs, WRAP, WQ>(a, S, wconv, mt, j, h, qv, soff);
        tr.mark(trk++);  // 3, 5: conv of this wave's 1st / 2nd M-tile done

        // BYTE offsets (inside image n) of the 16 output rows this lane-half stores, lane channel folded
        // in.  Residual loads and output stores go through raw buffer instructions (uniform resource +
        // 32-bit lane offset + immediate): no per-access address arithmetic, and rows outside the image
        // get an out-of-range offset, so the hardware range check drops their stores / returns 0 for
        // their loads -- no exec-mask branches in the epilogue.
        unsigned boff[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int ti = mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            const int rr = ti / TW, cc = ti - rr * TW;
            const int pr = ty0 + rr, pc = tx0 + cc;
            const bool ok = (pr < Hp) && (pc < Wp);
            boff[i] = ok ? (unsigned)((((py + pr * d) * a.W + (px + pc * d)) * C + j) * 4) : kOOB;
        }
        // Expansion, software-pipelined over the 4 N-tiles: the MFMA chain of N-tile nt+1 is issued
        // interleaved with the epilogue (BN + residual + PReLU + store) of N-tile nt, so the epilogue
        // executes in the shadow of 16 MFMAs (1024 cycles) instead of leaving the matrix pipe idle;
        // operands of N-tile nt+2 are requested one stage ahead.
        float weA[16], weB[16], rxA[16], rxB[16];
        float sA, tA, aA, sB, tB, aB;
        auto fetch = [&](int nt, float (&we)[16], float (&rx)[16], float &s1, float &t1, float &al) {
            if (WQ) {  // quad layout [nt][q][lane][4]
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 w4 = bload4(wers, welo, nt * 4096 + q * 1024);
                    we[4 * q] = w4.x; we[4 * q + 1] = w4.y; we[4 * q + 2] = w4.z; we[4 * q + 3] = w4.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) we[k] = bload(wers, welo, k * (2 * C * 4) + nt * 128);  // We[2k + h][nt*32 + j]
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) rx[i] = bload(xrs, boff[i], nt * 128);
            s1 = bload(esrs, j * 4, nt * 128); t1 = bload(etrs, j * 4, nt * 128); al = bload(rars, j * 4, nt * 128);
        };
        auto put = [&](int nt, int i, float v) {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), yrs, boff[i], nt * 128, 0);
        };
        __builtin_amdgcn_sched_barrier(0);
        fetch(0, weA, rxA, sA, tA, aA);
        fetch(1, weB, rxB, sB, tB, aB);
        f32x16 e0 = {0}, e1 = {0};
#pragma unroll
        for (int s = 0; s < 16; ++s) e0 = mfma32(qv[ord(s)], weA[s], e0);  // N-tile 0
        // stage 1: chain of N-tile 1  ||  epilogue of N-tile 0
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            e1 = mfma32(qv[ord(s)], weB[s], e1);
            put(0, s, prelu1(fmaf(e0[s], sA, tA) + rxA[s], aA));
        }
        __builtin_amdgcn_sched_barrier(0);
        fetch(2, weA, rxA, sA, tA, aA);
        e0 = (f32x16){0};
        // stage 2: chain of N-tile 2  ||  epilogue of N-tile 1
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            e0 = mfma32(qv[ord(s)], weA[s], e0);
            put(1, s, prelu1(fmaf(e1[s], sB, tB) + rxB[s], aB));
        }
        __builtin_amdgcn_sched_barrier(0);
        fetch(3, weB, rxB, sB, tB, aB);
        e1 = (f32x16){0};
        // stage 3: chain of N-tile 3  ||  epilogue of N-tile 2
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            e1 = mfma32(qv[ord(s)], weB[s], e1);
            put(2, s, prelu1(fmaf(e0[s], sA, tA) + rxA[s], aA));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 16; ++s) put(3, s, prelu1(fmaf(e1[s], sB, tB) + rxB[s], aB));
        tr.mark(trk++);  // 4, 6: expansion + stores issued
    }
}

struct TileId {
    int n, py, px, ty0, tx0, Hp, Wp, TH;
    bool empty;
};

template <int TW>
__device__ __forceinline__ TileId decode_tile(const BnkArgs &a)
{
    TileId t;
    const int d = a.dil;
    int b = blockIdx.x;
    if (a.xcd_chunk > 0) {  // XCD-aware order: workgroup b runs on XCD b % 8; give every XCD a contiguous run of tiles
        b = (b & 7) * a.xcd_chunk + (b >> 3);
        if (b >= a.ntiles) { t.empty = true; return t; }
    }
    t.TH = a.TH;
    const int tx = b % a.tiles_x; b /= a.tiles_x;
    const int ty = b % a.tiles_y; b /= a.tiles_y;
    t.px = b % d; b /= d;
    t.py = b % d; b /= d;
    t.n = b;
    t.Hp = (a.H - t.py + d - 1) / d;  // rows / cols of this phase sub-image
    t.Wp = (a.W - t.px + d - 1) / d;
    t.ty0 = ty * a.TH;
    t.tx0 = tx * TW;
    t.empty = (t.ty0 >= t.Hp) || (t.tx0 >= t.Wp);
    return t;
}

// regular / dilated 3x3 bottleneck: 168 VGPRs and 47 KB of LDS = three workgroups per CU
template <int TW, int QEPI = 0>
__global__ __launch_bounds__(256, 3) void k_bottleneck_mfma(BnkArgs a)
{
    __shared__ float P[PMAX * PSTR];
    __shared__ __attribute__((aligned(16))) float BNV[QEPI > 0 ? 3 * C : 4];
    if (QEPI > 0 && threadIdx.x < 3 * C / 4) {  // es | et | ra: read by every wave only after the barrier below
        const int arr = threadIdx.x / (C / 4), k4 = threadIdx.x % (C / 4);
        const float *src = arr == 0 ? a.es : arr == 1 ? a.et : a.ra;
        reinterpret_cast<float4 *>(BNV)[threadIdx.x] = reinterpret_cast<const float4 *>(src)[k4];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const TileId t = decode_tile<TW>(a);
    if (t.empty) return;  // whole workgroup: no barrier has been reached yet
    PhaseTrace tr;
    tr.mark(0);
    const float *ximg = a.x + (long)t.n * a.H * a.W * C;
    float *yimg = a.y + (long)t.n * a.H * a.W * C;
    if (!SSAL_ABLATE_IS(a, 2))
        proj_to_lds<TW, 1, BnkArgs, true>(a, ximg, P, t.TH, t.ty0, t.tx0, t.py, t.px, t.Hp, t.Wp, wave, j, h);
    tr.mark(1);
    __syncthreads();
    tr.mark(2);
    if (SSAL_ABLATE_IS(a, 1)) return;
    conv_exp_store<TW, 3, 3, TW + 2, 0, true, QEPI>(a, ximg, yimg, P, a.wq + quad::WC, t.TH, t.ty0, t.tx0, t.py, t.px, t.Hp,
                                                    t.Wp, wave, j, h, tr, 0, BNV);
#ifdef SSAL_PHASE_TRACE
    __builtin_amdgcn_s_waitcnt(0);  // mark 7 = all stores acknowledged
#endif
    tr.mark(7);
    tr.flush(a.trace, lane, wave);
}

// ---- the same block at FOUR workgroups per CU (experiment of round 4, knob bnk_o4): 8x16 tiles, <= 128 VGPRs, 40 KB of
// LDS.  What makes the registers fit: the projection kernel (16 KB) lives in LDS in B-operand order -- float4 (s4, lane) =
// Wp[2(4 s4 + i) + h][j], i = 0..3, one conflict-free ds_read_b128 per four MFMAs instead of 40 resident + 24 re-fetched
// registers -- and after the projection the same 16 KB hold the EXPANSION kernel (ds_read instead of two 16-register
// prefetch buffers fed from L1).  P needs 180 rows for a 10 x 18 halo'd tile: 24 480 + 16 384 = 40 864 of the 40 960
// bytes a quarter of the CU's LDS offers.
constexpr int O4_PROWS = 180;
__global__ __launch_bounds__(256, 4) void k_bottleneck_o4(BnkArgs a)
{
    constexpr int TW = 16, HWP = TW + 2;
    __shared__ float P[O4_PROWS * PSTR];
    __shared__ __attribute__((aligned(16))) float WL[C * F];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const TileId t = decode_tile<TW>(a);
    if (t.empty) return;
    const int d = a.dil;
    const float *ximg = a.x + (long)t.n * a.H * a.W * C;
    float *yimg = a.y + (long)t.n * a.H * a.W * C;
    PhaseTrace tr;
    tr.mark(0);
    // ---- phase A: projection of the 10 x 18 halo'd tile (6 M-tiles: waves 0, 1 take two).  The activation fragments of
    // a wave's FIRST M-tile are requested before anything else, so that their HBM round trip runs beside the kernel
    // fill and the barrier; those of its second M-tile as soon as the first one's MFMAs have consumed the registers.
    constexpr int npix_halo = 10 * HWP;
    // A tile that IS a whole phase sub-image (every tile of the dilation-16 layers at 128 x 256: sub-images of 8 x 16) has
    // its entire halo ring outside the image: the ring is exact zeros, and only the 128 centre pixels are projected --
    // 4 M-tiles, one per wave, instead of the 6 of the halo'd walk (workgroup-uniform).
    const bool whole = t.ty0 == 0 && t.tx0 == 0 && t.Hp <= 8 && t.Wp <= TW;
    const int nmt = whole ? 4 : (npix_halo + 31) / 32;
    float4 X[16];
    unsigned long long vmask = 0ull;
    auto request = [&](int mt) {  // -> vmask of the M-tile; X = its 16 fragments (not requested for an all-outside M-tile)
        const int q = mt * 32 + j;
        const int hr = whole ? (q >> 4) + 1 : q / HWP, hc = whole ? (q & 15) + 1 : q - hr * HWP;
        const int pr = t.ty0 - 1 + hr, pc = t.tx0 - 1 + hc;
        const bool valid = (whole || q < npix_halo) && (pr >= 0) && (pr < t.Hp) && (pc >= 0) && (pc < t.Wp);
        vmask = __ballot(valid);
        if (vmask == 0ull) return;
        const float *xp = valid ? ximg + ((long)(t.py + pr * d) * a.W + (t.px + pc * d)) * C : ximg;
#pragma unroll
        for (int u = 0; u < 16; ++u) X[u] = *reinterpret_cast<const float4 *>(xp + (2 * u + h) * 4);
    };
    const int mt0 = wave;
    request(mt0);
    // projection kernel -> LDS: element (k, co) of Wp[128][32] goes to float4 group (s >> 2, h, co), slot s & 3 (k = 2s + h)
#pragma unroll
    for (int it = 0; it < C * F / 256; ++it) {
        const int e = (int)threadIdx.x + 256 * it, k = e >> 5, co = e & 31, s_ = k >> 1;
        WL[(((s_ >> 2) * 64 + (k & 1) * 32 + co) << 2) + (s_ & 3)] = a.wp[e];
    }
    const float bs = a.ps[j], bt = a.pt[j], ba = a.pa[j];
    if (whole) {  // the 52 ring pixels: top row, bottom row, then (left, right) of rows 1..8
        for (int e = (int)threadIdx.x; e < 52 * F; e += 256) {
            const int u = e >> 5, k = u - 2 * HWP;
            const int q = u < HWP ? u : (u < 2 * HWP ? 9 * HWP + (u - HWP) : (1 + (k >> 1)) * HWP + ((k & 1) ? HWP - 1 : 0));
            P[q * PSTR + (e & 31)] = 0.0f;
        }
    }
    __syncthreads();
    for (int mt = mt0; mt < nmt; mt += 4) {
        if (mt != mt0) request(mt);
        const unsigned long long vm64 = vmask;
        // P row of the first pixel row (i = 0, h = 0) of the M-tile; rows of a whole-sub-image tile: see below
        if (vm64 == 0ull) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r0 = (i & 3) + 8 * (i >> 2), ri = r0 + 4 * h;
                const int qi = whole ? (2 * mt + (i >> 3) + 1) * HWP + (r0 & 15) + 4 * h + 1 : mt * 32 + ri;
                if (qi < O4_PROWS) P[qi * PSTR + kperm(j)] = 0.0f;
            }
            continue;
        }
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc = {0};
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            asm volatile("" ::: "memory");  // keep the read here: hoisted out of the M-tile loop it would pin 64 registers
            const float4 w = *reinterpret_cast<const float4 *>(WL + ((u * 64 + lane) << 2));  // steps 4u .. 4u+3
            float a0 = X[u].x, a1 = X[u].y, a2 = X[u].z, a3 = X[u].w;
            swap32(a0, a1);
            swap32(a2, a3);
            acc = mfma32(a0, w.x, acc);
            acc = mfma32(a2, w.y, acc);
            acc = mfma32(a1, w.z, acc);
            acc = mfma32(a3, w.w, acc);
        }
        const unsigned vmh = (unsigned)vm64 >> (4 * h);  // validity is per pixel: both lane halves carry the same 32 bits
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r0 = (i & 3) + 8 * (i >> 2), ri = r0 + 4 * h;
            const bool ok = (vmh >> r0) & 1u;
            const float v = ok ? prelu1(fmaf(acc[i], bs, bt), ba) : 0.0f;
            // centre pixel mt * 32 + ri of a whole-sub-image tile = tile row 2 mt + (i >> 3), column (r0 & 15) + 4 h
            const int qi = whole ? (2 * mt + (i >> 3) + 1) * HWP + (r0 & 15) + 4 * h + 1 : mt * 32 + ri;
            if (qi < O4_PROWS) P[qi * PSTR + kperm(j)] = v;
        }
    }
    // this thread's 16 elements of the expansion kernel We[32][128] (L2 hits), requested before the barrier and written
    // over WL behind it: element (ci, co) goes to float4 group (nt, s >> 2, h, j), slot s & 3 (ci = 2s + h, co = 32 nt + j)
    float wex[C * F / 256];
#pragma unroll
    for (int it = 0; it < C * F / 256; ++it) wex[it] = a.we[(int)threadIdx.x + 256 * it];
    tr.mark(1);
    __syncthreads();  // P complete, the projection kernel no longer needed
    tr.mark(2);
#pragma unroll
    for (int it = 0; it < C * F / 256; ++it) {
        const int e = (int)threadIdx.x + 256 * it, ci = e >> 7, co = e & 127, s_ = ci >> 1;
        WL[((((co >> 5) * 4 + (s_ >> 2)) * 64 + (ci & 1) * 32 + (co & 31)) << 2) + (s_ & 3)] = wex[it];
    }

    // ---- phase B: one output M-tile per wave (tile rows 2 wave, 2 wave + 1)
    const int mt = wave;
    constexpr unsigned kOOB = 0x80000000u;
    const unsigned img_bytes = (unsigned)(a.H * a.W * C) * 4u;
    const rsrc_t xrs = make_rsrc(ximg, img_bytes), yrs = make_rsrc(yimg, img_bytes);
    const rsrc_t esrs = make_rsrc(a.es, C * 4), etrs = make_rsrc(a.et, C * 4), rars = make_rsrc(a.ra, C * 4);
    unsigned boff[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int ti = mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        const int rr = ti / TW, cc = ti - rr * TW;
        const int pr = t.ty0 + rr, pc = t.tx0 + cc;
        const bool ok = (pr < t.Hp) && (pc < t.Wp);
        boff[i] = ok ? (unsigned)((((t.py + pr * d) * a.W + (t.px + pc * d)) * C + j) * 4) : kOOB;
    }
    float rxA[16], rxB[16];
    auto fetch_rx = [&](int nt, float (&rx)[16]) {
#pragma unroll
        for (int i = 0; i < 16; ++i) rx[i] = bload(xrs, boff[i], nt * 128);
    };
    fetch_rx(0, rxA);  // the first residual rows travel while the convolution runs
    float qv[16];
    conv_tile_q<TW, 3, 3, HWP, BnkArgs, 0, true>(a, P, a.wq + quad::WC, mt, j, h, qv);
    tr.mark(3);
    fetch_rx(1, rxB);
    __syncthreads();  // the expansion kernel is in WL (written by every thread before its convolution)
    float sA, tA, aA, sB, tB, aB;
    auto fetch_bn = [&](int nt, float &s1, float &t1, float &al) {
        s1 = bload(esrs, j * 4, nt * 128); t1 = bload(etrs, j * 4, nt * 128); al = bload(rars, j * 4, nt * 128);
    };
    auto chain_step = [&](int nt, int s4, f32x16 e) {  // four MFMAs: steps 4 s4 .. 4 s4 + 3 of N-tile nt
        asm volatile("" ::: "memory");
        const float4 w = *reinterpret_cast<const float4 *>(WL + (((nt * 4 + s4) * 64 + lane) << 2));
        e = mfma32(qv[ord(4 * s4 + 0)], w.x, e);
        e = mfma32(qv[ord(4 * s4 + 1)], w.y, e);
        e = mfma32(qv[ord(4 * s4 + 2)], w.z, e);
        e = mfma32(qv[ord(4 * s4 + 3)], w.w, e);
        return e;
    };
    auto put = [&](int nt, int i, float v) {
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), yrs, boff[i], nt * 128, 0);
    };
    fetch_bn(0, sA, tA, aA);
    fetch_bn(1, sB, tB, aB);
    f32x16 e0 = {0}, e1 = {0};
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) e0 = chain_step(0, s4, e0);
    // stage 1: chain of N-tile 1  ||  epilogue of N-tile 0
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        e1 = chain_step(1, s4, e1);
#pragma unroll
        for (int i = 4 * s4; i < 4 * s4 + 4; ++i) put(0, i, prelu1(fmaf(e0[i], sA, tA) + rxA[i], aA));
    }
    __builtin_amdgcn_sched_barrier(0);
    fetch_rx(2, rxA);
    fetch_bn(2, sA, tA, aA);
    e0 = (f32x16){0};
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        e0 = chain_step(2, s4, e0);
#pragma unroll
        for (int i = 4 * s4; i < 4 * s4 + 4; ++i) put(1, i, prelu1(fmaf(e1[i], sB, tB) + rxB[i], aB));
    }
    __builtin_amdgcn_sched_barrier(0);
    fetch_rx(3, rxB);
    fetch_bn(3, sB, tB, aB);
    e1 = (f32x16){0};
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        e1 = chain_step(3, s4, e1);
#pragma unroll
        for (int i = 4 * s4; i < 4 * s4 + 4; ++i) put(2, i, prelu1(fmaf(e0[i], sA, tA) + rxA[i], aA));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 16; ++i) put(3, i, prelu1(fmaf(e1[i], sB, tB) + rxB[i], aB));
    tr.mark(4);
#ifdef SSAL_PHASE_TRACE
    __builtin_amdgcn_s_waitcnt(0);
#endif
    tr.mark(7);
    tr.flush(a.trace, lane, wave);
}

// asymmetric bottleneck: (5,1) then (1,5) with no BN / activation in between (dilation 1).
// LDS: P = the projected tile with a 2-pixel halo (12 x 36 pixels), R = a ring of RROWS pixel slots of the (5,1)
// result: the tile is finished in two halves, which keeps the workgroup at 80.5 KB of LDS = two workgroups per
// CU (all 8 rows at once: 100 KB = one).  The first half computes whole M-tiles covering its 4 rows (144
// pixels -> 160 = 5 M-tiles: the 16 surplus pixels are the start of row 4 and stay where they are), the second
// half the remaining 128 pixels = exactly 4 M-tiles, written over the slots of rows 0..3: pixel p of the
// second half lives in slot (p - 160) mod 160.
constexpr int PROWS_ASYM = 432;  // (8+4)*(32+4)
constexpr int RROWS_ASYM = 160;  // 5 M-tiles of 32 >= 4*(32+4)
template <int TW>
__global__ __launch_bounds__(256, 2) void k_bottleneck_mfma_asym(BnkArgs a)
{
    __shared__ float P[PROWS_ASYM * PSTR];
    __shared__ float R[RROWS_ASYM * PSTR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const TileId t = decode_tile<TW>(a);
    if (t.empty) return;
    const float *ximg = a.x + (long)t.n * a.H * a.W * C;
    float *yimg = a.y + (long)t.n * a.H * a.W * C;
    PhaseTrace tr, tr_inner;  // tr_inner: the per-M-tile marks of conv_exp_store are not kept here
    tr.mark(0);
    proj_to_lds<TW, 2>(a, ximg, P, t.TH, t.ty0, t.tx0, t.py, t.px, t.Hp, t.Wp, wave, j, h, PROWS_ASYM);
    tr.mark(1);
    constexpr int HWP = TW + 4;
    constexpr int NMT0 = (4 * HWP + 31) / 32;        // M-tiles of the first half: 5 (TW 32) / 3 (TW 16)
    constexpr int NMT1 = (8 * HWP) / 32 - NMT0;      // the rest: 4 / 2 (8 * HWP is a multiple of 32)
    constexpr int RING = NMT0 * 32;                  // ring size in pixel slots: 160 / 96
    __syncthreads();  // P complete
    tr.mark(2);
    conv5x1_to_lds<TW>(a, P, R, 0, NMT0, wave, j, h);
    tr.mark(3);
    __syncthreads();
    tr.mark(4);
    conv_exp_store<TW, 1, 5, HWP>(a, ximg, yimg, R, a.wc2, 4, t.ty0, t.tx0, t.py, t.px, t.Hp, t.Wp, wave, j, h,
                                  tr_inner);
    tr.mark(5);
    if (t.TH > 4) {
        __syncthreads();  // rows 0..3 of R are free again
        conv5x1_to_lds<TW>(a, P, R, RING, NMT1, wave, j, h);
        __syncthreads();
        // second half: tile row 4 + r, column c' = result pixel (4 + r) * HWP + c' = slot r * HWP + c' - (RING - 4 * HWP)
        conv_exp_store<TW, 1, 5, HWP, RING>(a, ximg, yimg, R, a.wc2, 4, t.ty0 + 4, t.tx0, t.py, t.px, t.Hp, t.Wp,
                                            wave, j, h, tr_inner, -(RING - 4 * HWP));
    }
    tr.mark(6);
#ifdef SSAL_PHASE_TRACE
    __builtin_amdgcn_s_waitcnt(0);
#endif
    tr.mark(7);
    tr.flush(a.trace, lane, wave);
}

// The asymmetric block on 8 x 16 tiles at THREE workgroups per CU (round 5; knob asym_tw16).  The (5,1) result R has no LDS
// of its own: the (5,1) pass of the whole tile (8 x 20 = 160 result pixels = exactly 5 M-tiles, wave 0 takes two) keeps its
// results in accumulator registers across a barrier, behind which no wave reads the projected rows any more, and writes them
// over P's rows 0..7; the (1,5) convolution + expansion then runs one M-tile per wave.  P = 12 x 20 = 240 rows: 34.8 KB.
constexpr int PROWS_ASYM16 = 256;  // 240 halo'd pixels, rounded up to whole M-tiles
__global__ __launch_bounds__(256, 3) void k_bottleneck_mfma_asym16x(BnkArgs a)
{
    constexpr int TW = 16, HWP = TW + 4;
    __shared__ float P[PROWS_ASYM16 * PSTR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const TileId t = decode_tile<TW>(a);
    if (t.empty) return;
    const float *ximg = a.x + (long)t.n * a.H * a.W * C;
    float *yimg = a.y + (long)t.n * a.H * a.W * C;
    PhaseTrace tr;
    proj_to_lds<TW, 2, BnkArgs, true>(a, ximg, P, t.TH, t.ty0, t.tx0, t.py, t.px, t.Hp, t.Wp, wave, j, h, PROWS_ASYM16);
    __syncthreads();  // P complete
    const f32x16 r0 = conv5x1_tile<TW>(a, P, wave * 32, j, h);
    f32x16 r1 = {0};
    if (wave == 0) r1 = conv5x1_tile<TW>(a, P, 128, j, h);  // the fifth M-tile (wave-uniform)
    __syncthreads();  // nobody reads the projected rows any more
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int ri = (i & 3) + 8 * (i >> 2) + 4 * h;
        P[(wave * 32 + ri) * PSTR + kperm(j)] = r0[i];
        if (wave == 0) P[(128 + ri) * PSTR + kperm(j)] = r1[i];
    }
    __syncthreads();  // R complete: result pixel (r, c') in row r * HWP + c'
    conv_exp_store<TW, 1, 5, HWP, 0, true>(a, ximg, yimg, P, a.wq + quad::WC + 5 * F * F, 8, t.ty0, t.tx0, t.py, t.px, t.Hp, t.Wp, wave, j,
                                           h, tr);
}

// =================================================================================================
// The 128-channel blocks on EIGHT-wave workgroups (knob bnk_w8): 512 threads on the 8 x 32 tile of k_bottleneck_mfma<32>,
// two workgroups per CU = four waves per SIMD -- k_bottleneck_o4's occupancy and per-wave work (one 32-pixel M-tile per
// wave behind the projection, <= 128 VGPRs) without its 8 x 16 tiles: the projection halo stays 1.33x and the 16 KB
// kernel area is filled once per 256 pixels.  The kernel area holds the projection kernel during phase A and the
// expansion kernel behind it, as in k_bottleneck_o4; the convolution kernels stream from L1 in the quad layout.
//
// Phase A runs on 16-pixel HALF-tiles with v_mfma_f32_16x16x4_f32 (two 16-channel N halves per half-tile): the 340
// halo'd pixels are 22 half-tiles = three rounds over eight waves with 22 of the 24 slots busy, where 32-pixel M-tiles
// would take two full rounds with 11 of 16.  Like 32x32x2 the instruction is a k-ordered fmaf chain (ssal_mfma.h), so
// the projected values are the same bits.
// =================================================================================================
constexpr int W8_THREADS = 512;
constexpr long W8_MAX_ELEMS = 1L << 28;  // floats per image the eight-wave kernels take (launch_bottleneck_mfma)

// projection kernel -> LDS as 16x16x4 B operands: float4 ((u, n), lane (i, g)), element e = Wp[16 u + 4 e + g][16 n + i]
// (u = 0..7 groups of four MFMA steps, n = N half): one conflict-free ds_read_b128 per four MFMAs
__device__ __forceinline__ void w8_fill_proj(const BnkArgs &a, float *WL)
{
#pragma unroll
    for (int it = 0; it < C * F / W8_THREADS; ++it) {
        const int e = (int)threadIdx.x + W8_THREADS * it, k = e >> 5, co = e & 31;
        WL[((((k >> 4) * 2 + (co >> 4)) * 64 + (k & 3) * 16 + (co & 15)) << 2) + ((k >> 2) & 3)] = a.wp[e];
    }
}

// requests the 8 activation fragments of half-tile ht (lane (i, g): pixel 16 ht + i of the row-major halo'd tile, channels
// 16 u + 4 g .. + 3) and returns the validity of its 16 pixels (0: nothing requested, the half-tile is all padding)
template <int HWP, int HALO, int NPIX>
__device__ __forceinline__ unsigned w8_request(const BnkArgs &a, const float *ximg, const TileId &t, int ht, int lane,
                                               float4 (&X)[8])
{
    const int i = lane & 15, g = lane >> 4;
    const int q = ht * 16 + i;
    const int hr = q / HWP, hc = q - hr * HWP;
    const int pr = t.ty0 - HALO + hr, pc = t.tx0 - HALO + hc;
    const bool valid = (q < NPIX) && (pr >= 0) && (pr < t.Hp) && (pc >= 0) && (pc < t.Wp);
    const unsigned vm = (unsigned)__ballot(valid) & 0xffffu;  // validity is per pixel: every lane quarter carries the same bits
    if (vm == 0u) return 0u;
    const float *xp = valid ? ximg + ((long)(t.py + pr * a.dil) * a.W + (t.px + pc * a.dil)) * C : ximg;
#pragma unroll
    for (int u = 0; u < 8; ++u) X[u] = *reinterpret_cast<const float4 *>(xp + 16 * u + 4 * g);
    return vm;
}

// projects half-tile ht: D[pixel 4 g + r][co 16 n + i] -> BN + PReLU, exact zeros outside the image -> P rows 16 ht ..
template <int NPIX>
__device__ __forceinline__ void w8_project(const float *WL, float *P, int ht, unsigned vm, const float4 (&X)[8], int lane,
                                           const float (&bs)[2], const float (&bt)[2], const float (&ba)[2])
{
    const int i = lane & 15, g = lane >> 4;
    const int kp = kperm(i);  // kperm(16 + i) = 16 + kperm(i)
    if (vm == 0u) {  // wave-uniform
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qi = ht * 16 + 4 * g + r;
            if (qi < NPIX) { P[qi * PSTR + kp] = 0.0f; P[qi * PSTR + 16 + kp] = 0.0f; }
        }
        return;
    }
    f32x4 acc0 = {0}, acc1 = {0};
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        asm volatile("" ::: "memory");  // keep the reads here: hoisted they would pin 64 registers
        const float4 w0 = *reinterpret_cast<const float4 *>(WL + (((2 * u) * 64 + lane) << 2));
        const float4 w1 = *reinterpret_cast<const float4 *>(WL + (((2 * u + 1) * 64 + lane) << 2));
        float r0 = X[u].x, r1 = X[u].y, r2 = X[u].z, r3 = X[u].w;
        transpose4(r0, r1, r2, r3);  // reg e of quarter g: channel 16 u + 4 e + g = k index g of step 4 u + e
        acc0 = mfma16(r0, w0.x, acc0); acc1 = mfma16(r0, w1.x, acc1);
        acc0 = mfma16(r1, w0.y, acc0); acc1 = mfma16(r1, w1.y, acc1);
        acc0 = mfma16(r2, w0.z, acc0); acc1 = mfma16(r2, w1.z, acc1);
        acc0 = mfma16(r3, w0.w, acc0); acc1 = mfma16(r3, w1.w, acc1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = ht * 16 + 4 * g + r;
        const bool ok = (vm >> (4 * g + r)) & 1u;
        const float v0 = ok ? prelu1(fmaf(acc0[r], bs[0], bt[0]), ba[0]) : 0.0f;
        const float v1 = ok ? prelu1(fmaf(acc1[r], bs[1], bt[1]), ba[1]) : 0.0f;
        if (qi < NPIX) { P[qi * PSTR + kp] = v0; P[qi * PSTR + 16 + kp] = v1; }
    }
}

// phase A of both eight-wave kernels: wave w projects half-tiles w, w + 8, ...  The fragments of a wave's first half-tile are
// requested before the kernel fill and the barrier, those of half-tile r + 1 before the MFMAs of half-tile r (two buffers).
template <int HWP, int HALO, int NPIX>
__device__ __forceinline__ void w8_proj_to_lds(const BnkArgs &a, const float *ximg, const TileId &t, float *P, float *WL,
                                               int wave, int lane)
{
    constexpr int NR = ((NPIX + 15) / 16 + 7) / 8;  // rounds; a half-tile past the last one requests and writes nothing
    float4 XA[8], XB[8];
    unsigned vA = w8_request<HWP, HALO, NPIX>(a, ximg, t, wave, lane, XA), vB = 0u;
    w8_fill_proj(a, WL);
    const int i = lane & 15;
    const float bs[2] = {a.ps[i], a.ps[16 + i]}, bt[2] = {a.pt[i], a.pt[16 + i]}, ba[2] = {a.pa[i], a.pa[16 + i]};
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NR; r += 2) {
        if (r + 1 < NR) vB = w8_request<HWP, HALO, NPIX>(a, ximg, t, wave + 8 * (r + 1), lane, XB);
        __builtin_amdgcn_sched_barrier(0);
        w8_project<NPIX>(WL, P, wave + 8 * r, vA, XA, lane, bs, bt, ba);
        __builtin_amdgcn_sched_barrier(0);
        if (r + 2 < NR) vA = w8_request<HWP, HALO, NPIX>(a, ximg, t, wave + 8 * (r + 2), lane, XA);
        __builtin_amdgcn_sched_barrier(0);
        if (r + 1 < NR) w8_project<NPIX>(WL, P, wave + 8 * (r + 1), vB, XB, lane, bs, bt, ba);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// last phase of both eight-wave kernels, k_bottleneck_o4's register plan on an 8 x 32 tile: wave w convolves M-tile w (tile
// row w) of the LDS tensor S, then expansion (kernel in WL, quad layout) + BN + residual + PReLU as D[pixel][co] with
// 128-byte row stores through range-checked raw buffer instructions; the residual is re-read one N-tile ahead and every
// load of a stage is issued before that stage's stores.  SYNC: WL was written by this workgroup's threads after the last
// barrier (regular block) -- one more barrier between the convolution and the expansion.
template <int KH, int KW, int SW, bool SYNC>
__device__ __forceinline__ void w8_conv_exp_store(const BnkArgs &a, const float *ximg, float *yimg, const float *S,
                                                  const float *wconv, const float *WL, const TileId &t, int wave, int lane)
{
    constexpr int TW = 32;
    const int j = lane & 31, h = lane >> 5, d = a.dil;
    const int mt = wave;
    constexpr unsigned kOOB = 0x80000000u;
    const unsigned img_bytes = (unsigned)(a.H * a.W * C) * 4u;
    const rsrc_t xrs = make_rsrc(ximg, img_bytes), yrs = make_rsrc(yimg, img_bytes);
    const rsrc_t esrs = make_rsrc(a.es, C * 4), etrs = make_rsrc(a.et, C * 4), rars = make_rsrc(a.ra, C * 4);
    unsigned boff[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int ti = mt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        const int rr = ti / TW, cc = ti - rr * TW;
        const int pr = t.ty0 + rr, pc = t.tx0 + cc;
        const bool ok = (pr < t.Hp) && (pc < t.Wp);
        boff[i] = ok ? (unsigned)((((t.py + pr * d) * a.W + (t.px + pc * d)) * C + j) * 4) : kOOB;
    }
    float rxA[16], rxB[16];
    auto fetch_rx = [&](int nt, float (&rx)[16]) {
#pragma unroll
        for (int i = 0; i < 16; ++i) rx[i] = bload(xrs, boff[i], nt * 128);
    };
    fetch_rx(0, rxA);  // the first residual rows travel while the convolution runs
    float qv[16];
    conv_tile_q<TW, KH, KW, SW, BnkArgs, 0, true>(a, S, wconv, mt, j, h, qv);
    fetch_rx(1, rxB);
    if (SYNC) __syncthreads();  // the expansion kernel is in WL
    float sA, tA, aA, sB, tB, aB;
    auto fetch_bn = [&](int nt, float &s1, float &t1, float &al) {
        s1 = bload(esrs, j * 4, nt * 128); t1 = bload(etrs, j * 4, nt * 128); al = bload(rars, j * 4, nt * 128);
    };
    auto chain_step = [&](int nt, int s4, f32x16 e) {  // four MFMAs: steps 4 s4 .. 4 s4 + 3 of N-tile nt
        asm volatile("" ::: "memory");
        const float4 w = *reinterpret_cast<const float4 *>(WL + (((nt * 4 + s4) * 64 + lane) << 2));
        e = mfma32(qv[ord(4 * s4 + 0)], w.x, e);
        e = mfma32(qv[ord(4 * s4 + 1)], w.y, e);
        e = mfma32(qv[ord(4 * s4 + 2)], w.z, e);
        e = mfma32(qv[ord(4 * s4 + 3)], w.w, e);
        return e;
    };
    auto put = [&](int nt, int i, float v) {
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), yrs, boff[i], nt * 128, 0);
    };
    fetch_bn(0, sA, tA, aA);
    fetch_bn(1, sB, tB, aB);
    f32x16 e0 = {0}, e1 = {0};
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) e0 = chain_step(0, s4, e0);
    // stage 1: chain of N-tile 1  ||  epilogue of N-tile 0
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        e1 = chain_step(1, s4, e1);
#pragma unroll
        for (int i = 4 * s4; i < 4 * s4 + 4; ++i) put(0, i, prelu1(fmaf(e0[i], sA, tA) + rxA[i], aA));
    }
    __builtin_amdgcn_sched_barrier(0);
    fetch_rx(2, rxA);
    fetch_bn(2, sA, tA, aA);
    e0 = (f32x16){0};
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        e0 = chain_step(2, s4, e0);
#pragma unroll
        for (int i = 4 * s4; i < 4 * s4 + 4; ++i) put(1, i, prelu1(fmaf(e1[i], sB, tB) + rxB[i], aB));
    }
    __builtin_amdgcn_sched_barrier(0);
    fetch_rx(3, rxB);
    fetch_bn(3, sB, tB, aB);
    e1 = (f32x16){0};
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
        e1 = chain_step(3, s4, e1);
#pragma unroll
        for (int i = 4 * s4; i < 4 * s4 + 4; ++i) put(2, i, prelu1(fmaf(e0[i], sA, tA) + rxA[i], aA));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 16; ++i) put(3, i, prelu1(fmaf(e1[i], sB, tB) + rxB[i], aB));
}

// regular / dilated 3x3 block: P = 10 x 34 rows (46.2 KB) + 16 KB kernel area = 62.6 KB, two workgroups per CU
constexpr int W8_PROWS = 10 * 34;
__global__ __launch_bounds__(W8_THREADS, 2) void k_bottleneck_w8(BnkArgs a)
{
    constexpr int TW = 32, HWP = TW + 2;
    __shared__ float P[W8_PROWS * PSTR];
    __shared__ __attribute__((aligned(16))) float WL[C * F];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const TileId t = decode_tile<TW>(a);
    if (t.empty) return;  // whole workgroup: no barrier has been reached yet
    const float *ximg = a.x + (long)t.n * a.H * a.W * C;
    float *yimg = a.y + (long)t.n * a.H * a.W * C;
    w8_proj_to_lds<HWP, 1, W8_PROWS>(a, ximg, t, P, WL, wave, lane);
    // the expansion kernel is already in the order phase B reads it (quad layout): two float4 per thread, requested before
    // the barrier and written over the projection kernel behind it
    const float4 *weq = reinterpret_cast<const float4 *>(a.wq + quad::we(9));
    const float4 wex0 = weq[threadIdx.x], wex1 = weq[threadIdx.x + W8_THREADS];
    __syncthreads();  // P complete, the projection kernel no longer needed
    reinterpret_cast<float4 *>(WL)[threadIdx.x] = wex0;
    reinterpret_cast<float4 *>(WL)[threadIdx.x + W8_THREADS] = wex1;
    w8_conv_exp_store<3, 3, HWP, true>(a, ximg, yimg, P, a.wq + quad::WC, WL, t, wave, lane);
}

// one quarter of a (5,1) M-tile on 16x16x4: result pixels u0 .. u0 + 15 of the row-major 8 x 36 grid, channels 16 n ..
// + 15, taps and channels in ascending order; reg r of lane (i, g) = D[pixel u0 + 4 g + r][co 16 n + i]
__device__ __forceinline__ f32x4 w8_conv5x1_quarter(const BnkArgs &a, const float *P, int u0, int n, int lane)
{
    constexpr int HWP = 36;
    const int i = lane & 15, g = lane >> 4;
    const rsrc_t wrs = make_rsrc(a.wc, 5 * F * F * 4);
    const unsigned lo = (unsigned)(g * F + 16 * n + i) * 4u;  // W0[kh][ci = 4 s + g][co = 16 n + i]
    const int pos = ((g & 1) << 2) + (g >> 1);  // place of channel 8 G + g inside a permuted row; channel 8 G + 4 + g: + 2
    f32x4 acc = {0};
#pragma unroll
    for (int kh = 0; kh < 5; ++kh) {
        const float *pq = P + (u0 + i + kh * HWP) * PSTR + pos;
#pragma unroll
        for (int s = 0; s < 8; ++s)
            acc = mfma16(pq[8 * (s >> 1) + 2 * (s & 1)], bload(wrs, lo, kh * (F * F * 4) + s * (4 * F * 4)), acc);
    }
    return acc;
}

// asymmetric block: P = 12 x 36 projected rows (58.8 KB) + 16 KB kernel area = 75.1 KB, two workgroups per CU.  The (5,1)
// pass over the 8 x 36 region is nine M-tiles: wave w takes M-tile w, and the ninth is split into four 16-pixel x 16-channel
// quarters for waves 0..3.  As in k_bottleneck_mfma_asym16x the results wait in accumulators behind a barrier and are
// written over P's rows 0..287; then (1,5) + expansion, one M-tile per wave.
constexpr int W8_PROWS_ASYM = 12 * 36;
__global__ __launch_bounds__(W8_THREADS, 2) void k_bottleneck_asym_w8(BnkArgs a)
{
    constexpr int TW = 32, HWP = TW + 4;
    __shared__ float P[W8_PROWS_ASYM * PSTR];
    __shared__ __attribute__((aligned(16))) float WL[C * F];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const TileId t = decode_tile<TW>(a);
    if (t.empty) return;
    const float *ximg = a.x + (long)t.n * a.H * a.W * C;
    float *yimg = a.y + (long)t.n * a.H * a.W * C;
    w8_proj_to_lds<HWP, 2, W8_PROWS_ASYM>(a, ximg, t, P, WL, wave, lane);
    const float4 *weq = reinterpret_cast<const float4 *>(a.wq + quad::we(10));
    const float4 wex0 = weq[threadIdx.x], wex1 = weq[threadIdx.x + W8_THREADS];
    __syncthreads();  // P complete, the projection kernel no longer needed
    reinterpret_cast<float4 *>(WL)[threadIdx.x] = wex0;
    reinterpret_cast<float4 *>(WL)[threadIdx.x + W8_THREADS] = wex1;
    const f32x16 r0 = conv5x1_tile<TW>(a, P, wave * 32, j, h);
    f32x4 r1 = {0};
    if (wave < 4) r1 = w8_conv5x1_quarter(a, P, 256 + 16 * (wave >> 1), wave & 1, lane);  // wave-uniform
    __syncthreads();  // nobody reads the projected rows any more
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int ri = (i & 3) + 8 * (i >> 2) + 4 * h;
        P[(wave * 32 + ri) * PSTR + kperm(j)] = r0[i];
    }
    if (wave < 4) {
        const int i16 = lane & 15, g = lane >> 4;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            P[(256 + 16 * (wave >> 1) + 4 * g + r) * PSTR + 16 * (wave & 1) + kperm(i16)] = r1[r];
    }
    __syncthreads();  // R complete (result pixel (r, c') in row r * HWP + c'), and the expansion kernel is in WL
    w8_conv_exp_store<1, 5, HWP, false>(a, ximg, yimg, P, a.wq + quad::WC + 5 * F * F, WL, t, wave, lane);
}

// =================================================================================================
// Downsample bottleneck, C = 64 -> 128 (Bottleneck2_0; enet_modules.py:868-938) in one launch:
//   main:     2x2/s2 proj (64 -> 32) + BN + PReLU -> 3x3 conv (32 -> 32) + BN + PReLU -> 1x1 exp
//             (32 -> 128) + BN
//   residual: max_pool_with_argmax 2x2/s2 of the block input, zero-padded to 128 channels; the first
//             maximum in (dy,dx) order wins; its window code dy*2+dx is saved for the upsample block
//   out = PReLU(main + residual)                                   [N,H,W,64] -> [N,H/2,W/2,128]
// The strided projection is a GEMM with K = (dy,dx,ci) = 4 x 64 over the 2x2 input patch of every
// (halo'd) output pixel.
// =================================================================================================

constexpr int CDN = 64;  // input channels of the downsample block

// Structure (same recipe as k_bottleneck16): the tile's CENTRE output pixels are projected with the
// (wave, M-tile, lane) mapping phase B uses, so the 2x2 input patches the projection loads are exactly the
// pooling windows of the residual: the first-max pooling and its window codes are evaluated on the fly
// while the four taps stream through (codes stored at once, 32 pooled values per lane and M-tile kept in
// registers) -- the block input is read once.  The expansion is evaluated as D[co][pixel] (lane = pixel,
// 4 consecutive channels per register group): float4 stores, residual of N-tiles 0/1 straight from the
// pooled registers.  Expansion kernel and BN vectors live in LDS, the projection kernel streams from L1
// through a window of WIN k-pair steps; activation fragments are double-buffered per tap.
template <int TW>
__global__ __launch_bounds__(256, 2) void k_downsample_mfma(DownArgs a)
{
    constexpr int TH = 8, HW2 = TW + 2;
    constexpr int MPW = (TH * TW) / 32 / 4;  // centre M-tiles per wave: 2 (TW 32) or 1 (TW 16)
    constexpr int RING = 2 * HW2 + 2 * TH;   // 84 / 52
    constexpr int NRMT = (RING + 31) / 32;   // ring M-tiles: wave w < NRMT projects ring tile w
    constexpr int QDUMP = PMAX - 1;          // spare P row for M-tile pixels beyond the ring
    __shared__ float P[PMAX * PSTR];
    __shared__ float WE[F * C];              // expansion kernel [ci][co]
    __shared__ float BNV[3 * C];             // es | et | ra
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int Ho = a.H / 2, Wo = a.W / 2;
    int b = blockIdx.x;
    const int tx = b % a.tiles_x; b /= a.tiles_x;
    const int ty = b % a.tiles_y; b /= a.tiles_y;
    const int n = b;
    const int ty0 = ty * TH, tx0 = tx * TW;
    const float *ximg = a.x + (long)n * a.H * a.W * CDN;
    float *yimg = a.y + (long)n * Ho * Wo * C;
    uint8_t *cimg = a.code + (long)n * Ho * Wo * CDN;
    PhaseTrace tr;
    tr.mark(0);

    for (int i = threadIdx.x; i < F * C / 4; i += 256)
        reinterpret_cast<float4 *>(WE)[i] = reinterpret_cast<const float4 *>(a.we)[i];
    if (threadIdx.x < 3 * C / 4) {
        const int arr = threadIdx.x / (C / 4), k4 = threadIdx.x % (C / 4);
        const float *src = arr == 0 ? a.es : arr == 1 ? a.et : a.ra;
        reinterpret_cast<float4 *>(BNV)[threadIdx.x] = reinterpret_cast<const float4 *>(src)[k4];
    }

    // ---- phase A: 2x2/s2 projection (K = 4 taps x 64 ci) -----------------------------------------------
    constexpr int WIN = 8;                   // k-pair steps per weight window; 32 steps per tap
    const rsrc_t wrs = make_rsrc(a.wp, 4 * CDN * F * 4);
    const unsigned wlo = (unsigned)lane * 4u;  // fragment s of lane l = Wp[64 s + l]  (rows 2s, 2s+1)
    const float bs = a.ps[j], bt = a.pt[j], ba = a.pa[j];
    auto q_ring = [&](int u) {  // halo'd-tile index of ring pixel u (branch-free)
        const int k = u - 2 * HW2;
        const int side = (1 + (k >> 1)) * HW2 + ((k & 1) ? HW2 - 1 : 0);
        const int q = u < HW2 ? u : (u < 2 * HW2 ? (TH + 1) * HW2 + (u - HW2) : side);
        return u < RING ? q : QDUMP;
    };
    auto load_tap = [&](const float *xp, int tap, float4 (&v)[8]) {  // lane half h: channels 8m + 4h .. +3
        const float *xt = xp + ((tap >> 1) * a.W + (tap & 1)) * CDN + 4 * h;
#pragma unroll
        for (int m = 0; m < 8; ++m) v[m] = *reinterpret_cast<const float4 *>(xt + 8 * m);
    };
    // one M-tile: 4 taps x 32 k-pair steps; POOL: track the first maximum of the window and its code
    auto project = [&](const float *xp, unsigned vmask, auto qf, bool pool, float4 (&best)[8], unsigned (&code)[8]) {
        f32x16 acc = {0};
        float4 va[8], vb[8];
        float wa[WIN], wb[WIN];
        auto fetch_w = [&](int s0, float (&w)[WIN]) {
#pragma unroll
            for (int s = 0; s < WIN; ++s) w[s] = bload(wrs, wlo, (s0 + s) * 256);
        };
        auto steps = [&](const float4 (&v)[8], int m0, const float (&w)[WIN]) {  // WIN / 4 fragments
#pragma unroll
            for (int u = 0; u < WIN / 4; ++u) {
                float a0 = v[m0 + u].x, a1 = v[m0 + u].y, a2 = v[m0 + u].z, a3 = v[m0 + u].w;
                swap32(a0, a1);
                swap32(a2, a3);
                acc = mfma32(a0, w[4 * u + 0], acc);
                acc = mfma32(a2, w[4 * u + 1], acc);
                acc = mfma32(a1, w[4 * u + 2], acc);
                acc = mfma32(a3, w[4 * u + 3], acc);
            }
        };
        auto pool_tap = [&](const float4 (&v)[8], int tap) {  // strict '>' in (dy,dx) order: first maximum wins
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                if (tap == 0) { best[m] = v[m]; code[m] = 0u; continue; }
                const unsigned cd = (unsigned)tap;
                if (v[m].x > best[m].x) { best[m].x = v[m].x; code[m] = (code[m] & 0xFFFFFF00u) | cd; }
                if (v[m].y > best[m].y) { best[m].y = v[m].y; code[m] = (code[m] & 0xFFFF00FFu) | (cd << 8); }
                if (v[m].z > best[m].z) { best[m].z = v[m].z; code[m] = (code[m] & 0xFF00FFFFu) | (cd << 16); }
                if (v[m].w > best[m].w) { best[m].w = v[m].w; code[m] = (code[m] & 0x00FFFFFFu) | (cd << 24); }
                // pin the code update here: left free, LLVM sinks it to the store after the M-tile and keeps
                // the 96 compare masks of an M-tile alive in (spilled) SGPR pairs instead
                asm volatile("" : "+v"(code[m]));
            }
        };
        auto run_tap = [&](const float4 (&v)[8], int tap) {  // 32 steps = 4 windows; the window after next is in flight
            fetch_w(tap * 32 + WIN, wb);
            __builtin_amdgcn_sched_barrier(0);
            steps(v, 0, wa);
            __builtin_amdgcn_sched_barrier(0);
            fetch_w(tap * 32 + 2 * WIN, wa);
            __builtin_amdgcn_sched_barrier(0);
            steps(v, 2, wb);
            __builtin_amdgcn_sched_barrier(0);
            fetch_w(tap * 32 + 3 * WIN, wb);
            __builtin_amdgcn_sched_barrier(0);
            steps(v, 4, wa);
            __builtin_amdgcn_sched_barrier(0);
            if (tap < 3) fetch_w(tap * 32 + 4 * WIN, wa);
            __builtin_amdgcn_sched_barrier(0);
            steps(v, 6, wb);
            __builtin_amdgcn_sched_barrier(0);
            if (pool) pool_tap(v, tap);
        };
        load_tap(xp, 0, va);
        fetch_w(0, wa);
        load_tap(xp, 1, vb);
        run_tap(va, 0);
        load_tap(xp, 2, va);
        run_tap(vb, 1);
        load_tap(xp, 3, vb);
        run_tap(va, 2);
        run_tap(vb, 3);
#pragma unroll
        for (int i = 0; i < 16; ++i) {  // rows = pixels (registers), cols = co (lanes)
            const int ri = (i & 3) + 8 * (i >> 2) + 4 * h;
            const bool ok = (vmask >> ri) & 1u;
            P[qf(ri) * PSTR + kperm(j)] = ok ? prelu1(fmaf(acc[i], bs, bt), ba) : 0.0f;  // exact zero outside the image
        }
    };

    float4 pooled[MPW][8];  // max-pooled input, channels 8m + 4h .. +3 of the lane's centre pixel
    long opixk[MPW];        // output pixel index of the lane's centre pixel, -1 outside the image
    if (wave < NRMT) {      // wave-uniform: this wave's ring tile
        const int u = wave * 32 + j;
        const int q = q_ring(u);
        const int pr = ty0 - 1 + q / HW2, pc = tx0 - 1 + q % HW2;
        const bool rvalid = (u < RING) && pr >= 0 && pr < Ho && pc >= 0 && pc < Wo;
        const float *xp = rvalid ? ximg + ((long)(2 * pr) * a.W + 2 * pc) * CDN : ximg;
        float4 dummy_best[8];
        unsigned dummy_code[8];
        project(xp, (unsigned)__ballot(rvalid), [&](int ri) { return q_ring(wave * 32 + ri); }, false, dummy_best,
                dummy_code);
    }
    tr.mark(1);  // ring tile projected
#pragma unroll
    for (int k = 0; k < MPW; ++k) {
        const int mt = wave + 4 * k;
        const int tt = mt * 32 + j;
        const int oy = ty0 + tt / TW, ox = tx0 + tt % TW;
        const bool valid = oy < Ho && ox < Wo;
        opixk[k] = valid ? (long)oy * Wo + ox : -1;
        const float *xp = valid ? ximg + ((long)(2 * oy) * a.W + 2 * ox) * CDN : ximg;
        unsigned code[8];
        project(xp, (unsigned)__ballot(valid),
                [&](int ri) { const int t2 = mt * 32 + ri; return (t2 / TW + 1) * HW2 + (t2 % TW) + 1; }, true,
                pooled[k], code);
        if (valid) {  // window codes dy*2+dx of channels 8m + 4h .. +3: 4 bytes per store
#pragma unroll
            for (int m = 0; m < 8; ++m)
                *reinterpret_cast<unsigned *>(cimg + opixk[k] * CDN + 8 * m + 4 * h) = code[m];
        }
    }
    tr.mark(2);  // centre tiles projected and pooled
    __syncthreads();
    tr.mark(3);

    // ---- phase B: 3x3 conv -> expansion D[co][pixel] -> + pooled residual (registers) -> float4 stores ----
    const float *wel = WE + h * C + j;  // We[2s + h][nt*32 + j] = wel[2s*C + nt*32]
    const float *bnl = BNV + 4 * h;     // vectors of channels nt*32 + 8g + 4h .. +3
    const rsrc_t yrs = make_rsrc(yimg, (unsigned)(Ho * Wo * C) * 4u);  // downsample_mfma_fits: Ho * Wo * C <= 2^29
#pragma unroll
    for (int k = 0; k < MPW; ++k) {
        const int mt = wave + 4 * k;
        float qv[16];
        conv_tile_q<TW, 3, 3, HW2>(a, P, a.wc, mt, j, h, qv);
        if (k == 0) tr.mark(4);  // first conv done
        // Output stores.  The accumulator hands every lane (= pixel) four 16-byte pieces (g = 0..3) of its own 128-byte row
        // of N-tile nt; stored as they stand, one instruction touches 32 rows with 32 bytes each.  quad_transpose4 moves
        // piece g = q of pixel 4Q + kk into register kk of lane q of the quad: store kk of a quad (both lane halves) then
        // carries one WHOLE 128-byte row -- the store shape of a row-major epilogue (profiles/r05_ab_quad_transposed_stores.txt).
        unsigned yoq[4];  // byte offsets (inside the image) of this lane's piece (32 q + 16 h) in the rows of pixels 4Q + kk
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int t2 = mt * 32 + (j & ~3) + kk;
            const int oy2 = ty0 + t2 / TW, ox2 = tx0 + t2 % TW;
            yoq[kk] = (oy2 < Ho && ox2 < Wo) ? (unsigned)((oy2 * Wo + ox2) * (C * 4) + 32 * (j & 3) + 16 * h) : 0x80000000u;
        }
        float4 ov[4];
        auto chain = [&](int nt, int s, f32x16 e) { return mfma32(wel[2 * s * C + nt * 32], qv[ord(s)], e); };
        auto epilogue = [&](int nt, int g, const f32x16 &e) {
            const float4 s4 = *reinterpret_cast<const float4 *>(bnl + nt * 32 + 8 * g);
            const float4 t4 = *reinterpret_cast<const float4 *>(bnl + C + nt * 32 + 8 * g);
            const float4 a4 = *reinterpret_cast<const float4 *>(bnl + 2 * C + nt * 32 + 8 * g);
            const float4 x4 = nt < 2 ? pooled[k][(4 * nt + g) & 7] : make_float4(0.f, 0.f, 0.f, 0.f);  // channels >= 64: zero padding
            float4 o;
            o.x = prelu1(fmaf(e[4 * g + 0], s4.x, t4.x) + x4.x, a4.x);
            o.y = prelu1(fmaf(e[4 * g + 1], s4.y, t4.y) + x4.y, a4.y);
            o.z = prelu1(fmaf(e[4 * g + 2], s4.z, t4.z) + x4.z, a4.z);
            o.w = prelu1(fmaf(e[4 * g + 3], s4.w, t4.w) + x4.w, a4.w);
            ov[g] = o;
            if (g == 3) {
                quad_transpose4(ov[0], ov[1], ov[2], ov[3], lane);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, ov[kk]), yrs, yoq[kk], nt * 128, 0);
            }
        };
        f32x16 e0 = {0}, e1 = {0};
#pragma unroll
        for (int s = 0; s < 16; ++s) e0 = chain(0, s, e0);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int s = 4 * g; s < 4 * g + 4; ++s) e1 = chain(1, s, e1);
            epilogue(0, g, e0);
        }
        e0 = (f32x16){0};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int s = 4 * g; s < 4 * g + 4; ++s) e0 = chain(2, s, e0);
            epilogue(1, g, e1);
        }
        e1 = (f32x16){0};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int s = 4 * g; s < 4 * g + 4; ++s) e1 = chain(3, s, e1);
            epilogue(2, g, e0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) epilogue(3, g, e1);
        if (k == 0) tr.mark(5);  // first M-tile stored (issued)
    }
    tr.mark(6);
#ifdef SSAL_PHASE_TRACE
    __builtin_amdgcn_s_waitcnt(0);
#endif
    tr.mark(7);
    tr.flush(a.trace, lane, wave);
}

// =================================================================================================
// Upsample bottleneck, C = 128 -> 64 (Bottleneck4_0; enet_modules.py:1217-1292) in one launch:
//   main:     1x1 proj (128 -> 32) + BN + PReLU  ->  conv2d_transpose 3x3/s2 (32 -> 16) + BN + PReLU
//             -> 1x1 exp (16 -> 64) + BN
//   residual: 1x1 conv (128 -> 64, no BN) -> unpool_2d with the saved 2x2 window codes (gather form)
//   out = PReLU(main + residual)                                       [N,H,W,128] -> [N,2H,2W,64]
// The transposed conv is evaluated per OUTPUT PARITY class of an input pixel (i,j):
//   ee out(2i,2j)     = P(i,j)W00 + P(i,j-1)W02 + P(i-1,j)W20 + P(i-1,j-1)W22
//   eo out(2i,2j+1)   = P(i,j)W01 + P(i-1,j)W21
//   oe out(2i+1,2j)   = P(i,j)W10 + P(i,j-1)W12
//   oo out(2i+1,2j+1) = P(i,j)W11                    (taps in (kh,kw) ascending = oracle order)
// With only 16 output channels two classes share one 32-row MFMA: accumulator A carries
// [ee | eo], accumulator B carries [oe | oo]; the commit step stacks the kernels accordingly
// (ws[slot][ci][row], zero rows where a class has no tap: adding an exact zero keeps the chain).
// =================================================================================================

constexpr int CUP = 64;  // output channels of the upsample block

// Structure (the k_bottleneck16 recipe): the tile's CENTRE pixels are projected with the (wave, M-tile,
// lane) mapping phase B uses, and the SAME swapped activation fragment feeds three accumulators per
// k-pair step -- the projection D[pixel][co] and the two N-tiles of the 1x1 residual conv, evaluated as
// D[co][pixel] -- so the block input is read once and the residual waits in registers in exactly the
// layout of the (flipped) expansion output: lane = pixel, 4 consecutive channels per register group,
// hence packed window codes (one 32-bit load per group) and float4 stores.  Kernel fragments stream from
// L1 through rolling windows; the transposed conv is pipelined one slot ahead like conv_tile_q.
template <int TW>
__global__ __launch_bounds__(256, 2) void k_upsample_mfma(UpArgs a)
{
    constexpr int TH = 8, HW2 = TW + 2;
    constexpr int MPW = (TH * TW) / 32 / 4;  // centre M-tiles per wave: 2 (TW 32) or 1 (TW 16)
    constexpr int RING = 2 * HW2 + 2 * TH;   // 84 / 52
    constexpr int NRMT = (RING + 31) / 32;   // ring M-tiles: wave w < NRMT projects ring tile w
    constexpr int QDUMP = PMAX - 1;          // spare P row for M-tile pixels beyond the ring
    __shared__ float P[PMAX * PSTR];
    __shared__ float BNV[3 * CUP + 3 * 16];  // es | et | ra (64 each), then cs | ct | ca (16 each)
    __shared__ float WEL[16 * CUP];          // expansion kernel [ci 16][co 64]: A operand of the flipped expansion
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    reinterpret_cast<float4 *>(WEL)[threadIdx.x] = reinterpret_cast<const float4 *>(a.we)[threadIdx.x];  // 256 x float4
    int b = blockIdx.x;
    const int tx = b % a.tiles_x; b /= a.tiles_x;
    const int ty = b % a.tiles_y; b /= a.tiles_y;
    const int n = b;
    const int ty0 = ty * TH, tx0 = tx * TW;
    const float *ximg = a.x + (long)n * a.H * a.W * C;
    const uint8_t *cimg = a.code + (long)n * a.H * a.W * CUP;
    float *yimg = a.y + (long)n * 4 * a.H * a.W * CUP;
    PhaseTrace tr;
    tr.mark(0);

    if (threadIdx.x < 3 * CUP / 4) {
        const int arr = threadIdx.x / (CUP / 4), k4 = threadIdx.x % (CUP / 4);
        const float *src = arr == 0 ? a.es : arr == 1 ? a.et : a.ra;
        reinterpret_cast<float4 *>(BNV)[threadIdx.x] = reinterpret_cast<const float4 *>(src)[k4];
    } else if (threadIdx.x < 3 * CUP / 4 + 12) {
        const int q = threadIdx.x - 3 * CUP / 4, arr = q / 4, k4 = q % 4;
        const float *src = arr == 0 ? a.cs : arr == 1 ? a.ct : a.ca;
        reinterpret_cast<float4 *>(BNV + 3 * CUP)[q] = reinterpret_cast<const float4 *>(src)[k4];
    }

    // ---- phase A -------------------------------------------------------------------------------------
    constexpr int WIN = 4;
    const rsrc_t wprs = make_rsrc(a.wp, C * F * 4), wrrs = make_rsrc(a.wr, C * CUP * 4);
    const unsigned wplo = (unsigned)lane * 4u;            // Wp fragment s of lane l = Wp[64 s + l]
    const unsigned wrlo = (unsigned)(h * CUP + j) * 4u;   // Wr[2s + h][nt*32 + j] = + s*512 + nt*128 bytes
    const float bs = a.ps[j], bt = a.pt[j], ba = a.pa[j];
    auto q_ring = [&](int u) {  // halo'd-tile index of ring pixel u (branch-free)
        const int k = u - 2 * HW2;
        const int side = (1 + (k >> 1)) * HW2 + ((k & 1) ? HW2 - 1 : 0);
        const int q = u < HW2 ? u : (u < 2 * HW2 ? (TH + 1) * HW2 + (u - HW2) : side);
        return u < RING ? q : QDUMP;
    };
    // one M-tile; RES (compile time): also accumulate the 1x1 residual conv of the same pixels
    auto project = [&](const float *xp, unsigned vmask, auto qf, auto RES, f32x16 &res0, f32x16 &res1) {
        constexpr bool with_res = decltype(RES)::value;
        float4 X[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) X[u] = *reinterpret_cast<const float4 *>(xp + (2 * u + h) * 4);
        f32x16 acc = {0};
        float pa_[WIN], pb_[WIN], r0a[WIN], r0b[WIN], r1a[WIN], r1b[WIN];
        auto fetch_w = [&](int s0, float (&wp_)[WIN], float (&w0)[WIN], float (&w1)[WIN]) {
#pragma unroll
            for (int s = 0; s < WIN; ++s) {
                wp_[s] = bload(wprs, wplo, (s0 + s) * 256);
                if (with_res) {
                    w0[s] = bload(wrrs, wrlo, (s0 + s) * 512);
                    w1[s] = bload(wrrs, wrlo, (s0 + s) * 512 + 128);
                }
            }
        };
        auto steps = [&](int s0, const float (&wp_)[WIN], const float (&w0)[WIN], const float (&w1)[WIN]) {
#pragma unroll
            for (int v = 0; v < WIN / 4; ++v) {
                const int u = s0 / 4 + v;
                float a0 = X[u].x, a1 = X[u].y, a2 = X[u].z, a3 = X[u].w;
                swap32(a0, a1);  // a0 = ch(8u+0 | 8u+1), a1 = ch(8u+4 | 8u+5)
                swap32(a2, a3);  // a2 = ch(8u+2 | 8u+3), a3 = ch(8u+6 | 8u+7)
                const float xs[4] = {a0, a2, a1, a3};  // ascending k-pair order
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc = mfma32(xs[q], wp_[4 * v + q], acc);
                    if (with_res) {
                        res0 = mfma32(w0[4 * v + q], xs[q], res0);
                        res1 = mfma32(w1[4 * v + q], xs[q], res1);
                    }
                }
            }
        };
        fetch_w(0, pa_, r0a, r1a);
#pragma unroll
        for (int s0 = 0; s0 < 64; s0 += 2 * WIN) {
            fetch_w(s0 + WIN, pb_, r0b, r1b);
            __builtin_amdgcn_sched_barrier(0);
            steps(s0, pa_, r0a, r1a);
            __builtin_amdgcn_sched_barrier(0);
            if (s0 + 2 * WIN < 64) fetch_w(s0 + 2 * WIN, pa_, r0a, r1a);
            __builtin_amdgcn_sched_barrier(0);
            steps(s0 + WIN, pb_, r0b, r1b);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {  // rows = pixels (registers), cols = co (lanes)
            const int ri = (i & 3) + 8 * (i >> 2) + 4 * h;
            const bool ok = (vmask >> ri) & 1u;
            P[qf(ri) * PSTR + kperm(j)] = ok ? prelu1(fmaf(acc[i], bs, bt), ba) : 0.0f;  // exact zero outside the image
        }
    };

    f32x16 res[MPW][2];    // residual 1x1 conv of the lane's centre pixel: reg 4g + c = channel nt*32 + 8g + 4h + c
    long ipixk[MPW];         // input pixel index of the lane's centre pixel, -1 outside the image
    if (wave < NRMT) {       // wave-uniform: this wave's ring tile
        const int u = wave * 32 + j;
        const int q = q_ring(u);
        const int pr = ty0 - 1 + q / HW2, pc = tx0 - 1 + q % HW2;
        const bool rvalid = (u < RING) && pr >= 0 && pr < a.H && pc >= 0 && pc < a.W;
        const float *xp = rvalid ? ximg + ((long)pr * a.W + pc) * C : ximg;
        f32x16 d0 = {0}, d1 = {0};
        project(xp, (unsigned)__ballot(rvalid), [&](int ri) { return q_ring(wave * 32 + ri); }, std::false_type(), d0, d1);
    }
    tr.mark(1);  // ring tile projected
#pragma unroll
    for (int k = 0; k < MPW; ++k) {
        const int mt = wave + 4 * k;
        const int tt = mt * 32 + j;
        const int iy = ty0 + tt / TW, ix = tx0 + tt % TW;
        const bool valid = iy < a.H && ix < a.W;
        ipixk[k] = valid ? (long)iy * a.W + ix : -1;
        const float *xp = valid ? ximg + ipixk[k] * C : ximg;
        res[k][0] = (f32x16){0};
        res[k][1] = (f32x16){0};
        project(xp, (unsigned)__ballot(valid),
                [&](int ri) { const int t2 = mt * 32 + ri; return (t2 / TW + 1) * HW2 + (t2 % TW) + 1; },
                std::true_type(), res[k][0], res[k][1]);
    }
    const float *wel = WEL + h * CUP + j;  // We[2s + h][nt*32 + j] = wel[2s*CUP + nt*32]: lane (r = j, k = h)
    tr.mark(2);  // centre tiles projected (+ residual conv)
    __syncthreads();
    tr.mark(3);

    // ---- phase B: transposed conv (2 stacked accumulators) -> expansion per parity class -> unpool-gated
    // residual -> float4 stores ----------------------------------------------------------------------------
    const rsrc_t wsrs = make_rsrc(a.ws, 6 * F * 32 * 4);
    const rsrc_t yrs = make_rsrc(yimg, (unsigned)(4 * a.H * a.W * CUP) * 4u);  // upsample_mfma_fits: 4 * H * W * 64 <= 2^29
    const float *bnl = BNV + 4 * h;
#pragma unroll
    for (int k = 0; k < MPW; ++k) {
        const int mt = wave + 4 * k;
        const int t = mt * 32 + j;
        const int r = t / TW, c = t - r * TW;
        // window codes of channels nt*32 + 8g + 4h .. +3 (index 4 nt + g), one byte each; requested here (needed
        // only by the epilogues below), ahead of this M-tile's stores
        unsigned codes[8];
        {
            const uint8_t *cp = cimg + (ipixk[k] >= 0 ? ipixk[k] : 0) * CUP + 4 * h;
#pragma unroll
            for (int q = 0; q < 8; ++q) codes[q] = *reinterpret_cast<const unsigned *>(cp + 8 * q);  // nt*32 + 8g = 8 (4nt + g)
        }
        f32x16 accA = {0}, accB = {0};
        {
            float wA[16], wB[16];
            float2 pA[8], pB[8];
            auto load_slot = [&](int slot, float (&w)[16], float2 (&pv)[8]) {
                const int dr = slot < 4 ? 1 - (slot >> 1) : 1, dc = 1 - (slot & 1);
#pragma unroll
                for (int q = 0; q < 16; ++q) w[q] = bload(wsrs, wplo, (slot * 16 + q) * 256);  // ws[slot][2q + h][j]
                const float *pq = P + ((r + dr) * HW2 + (c + dc)) * PSTR;
#pragma unroll
                for (int sq = 0; sq < 8; ++sq) pv[sq] = *reinterpret_cast<const float2 *>(pq + kperm_rd(sq, h));
            };
            auto run_slot = [&](f32x16 &acc, const float (&w)[16], const float2 (&pv)[8]) {
#pragma unroll
                for (int sq = 0; sq < 8; ++sq) {  // permuted rows: no re-pairing
                    acc = mfma32(w[2 * sq], pv[sq].x, acc);
                    acc = mfma32(w[2 * sq + 1], pv[sq].y, acc);
                }
            };
            // slots 0..3 = P(i,j), P(i,j-1), P(i-1,j), P(i-1,j-1) -> [ee|eo];  4, 5 = P(i,j), P(i,j-1) -> [oe|oo]
            load_slot(0, wA, pA);
            load_slot(1, wB, pB);
            __builtin_amdgcn_sched_barrier(0);
            run_slot(accA, wA, pA);
            __builtin_amdgcn_sched_barrier(0);
            load_slot(2, wA, pA);
            __builtin_amdgcn_sched_barrier(0);
            run_slot(accA, wB, pB);
            __builtin_amdgcn_sched_barrier(0);
            load_slot(3, wB, pB);
            __builtin_amdgcn_sched_barrier(0);
            run_slot(accA, wA, pA);
            __builtin_amdgcn_sched_barrier(0);
            load_slot(4, wA, pA);
            __builtin_amdgcn_sched_barrier(0);
            run_slot(accA, wB, pB);
            __builtin_amdgcn_sched_barrier(0);
            load_slot(5, wB, pB);
            __builtin_amdgcn_sched_barrier(0);
            run_slot(accB, wA, pA);
            __builtin_amdgcn_sched_barrier(0);
            run_slot(accB, wB, pB);
        }
        if (k == 0) tr.mark(4);  // first transposed conv done
        // BN + PReLU; reg i: class = i >> 3, channel = (i&3) + 8*((i>>2)&1) + 4h
        float qa[16], qb[16];
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {  // register group gq: channels 8*(gq&1) + 4h .. +3
            const float4 sc = *reinterpret_cast<const float4 *>(bnl + 3 * CUP + 8 * (gq & 1));
            const float4 sh = *reinterpret_cast<const float4 *>(bnl + 3 * CUP + 16 + 8 * (gq & 1));
            const float4 al = *reinterpret_cast<const float4 *>(bnl + 3 * CUP + 32 + 8 * (gq & 1));
            const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w}, alv[4] = {al.x, al.y, al.z, al.w};
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                qa[4 * gq + cc] = prelu1(fmaf(accA[4 * gq + cc], scv[cc], shv[cc]), alv[cc]);
                qb[4 * gq + cc] = prelu1(fmaf(accB[4 * gq + cc], scv[cc], shv[cc]), alv[cc]);
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            swap32(qa[2 * u], qa[2 * u + 1]);
            swap32(qb[2 * u], qb[2 * u + 1]);
        }
        // expansion per (parity class, N-tile): D[co][pixel]; the chain of combination m+1 is issued
        // interleaved with the epilogue of combination m
        // quad-transposed stores (see k_downsample_mfma): byte offsets of this lane's piece (32 q + 16 h) in the output rows
        // that belong to the INPUT pixels 4Q + kk of its quad (class (0, 0); the class / N-tile displacement is wave-uniform)
        unsigned yoq[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int t2 = mt * 32 + (j & ~3) + kk;
            const int iy2 = ty0 + t2 / TW, ix2 = tx0 + t2 % TW;
            yoq[kk] = (iy2 < a.H && ix2 < a.W) ? (unsigned)(((2 * iy2) * (2 * a.W) + 2 * ix2) * (CUP * 4) + 32 * (j & 3) + 16 * h) : 0x80000000u;
        }
        auto chain = [&](int m, f32x16 e) {  // m = cls * 2 + nt
            const int cls = m >> 1, nt = m & 1;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const float qv = cls < 2 ? qa[(cls & 1) * 8 + ord(s)] : qb[(cls & 1) * 8 + ord(s)];
                e = mfma32(wel[2 * s * CUP + nt * 32], qv, e);
            }
            return e;
        };
        auto epilogue = [&](int m, const f32x16 &e) {
            const int cls = m >> 1, nt = m & 1;
            const unsigned soff = (unsigned)((((cls >> 1) * (2 * a.W) + (cls & 1)) * CUP + nt * 32) * 4);
            float4 ov[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                // keep the three LDS vector reads here: hoisted out of the class loop (they do not depend on
                // cls) they would pin 96 registers and push the residual into scratch
                asm volatile("" ::: "memory");
                const float4 s4 = *reinterpret_cast<const float4 *>(bnl + nt * 32 + 8 * g);
                const float4 t4 = *reinterpret_cast<const float4 *>(bnl + CUP + nt * 32 + 8 * g);
                const float4 a4 = *reinterpret_cast<const float4 *>(bnl + 2 * CUP + nt * 32 + 8 * g);
                const unsigned cd = codes[4 * nt + g];
                const f32x16 &rs = res[k][nt];
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
        };
        f32x16 e0 = chain(0, (f32x16){0}), e1;
#pragma unroll
        for (int m = 0; m < 8; m += 2) {
            e1 = chain(m + 1, (f32x16){0});
            epilogue(m, e0);
            if (m + 2 < 8) e0 = chain(m + 2, (f32x16){0});
            epilogue(m + 1, e1);
        }
        if (k == 0) tr.mark(5);  // first M-tile stored (issued)
    }
    tr.mark(6);
#ifdef SSAL_PHASE_TRACE
    __builtin_amdgcn_s_waitcnt(0);
#endif
    tr.mark(7);
    tr.flush(a.trace, lane, wave);
}

// one probe for the hardware assumptions this file rests on (tests only): out[0..63] / out[64..127]
// = the two registers after swap32 of (lane, 100 + lane)
__global__ void k_probe_swap(float *out)
{
    float a = (float)threadIdx.x, b = 100.0f + (float)threadIdx.x;
    swap32(a, b);
    out[threadIdx.x] = a;
    out[64 + threadIdx.x] = b;
    float c = (float)threadIdx.x, e = 100.0f + (float)threadIdx.x;
    swap16(c, e);
    out[128 + threadIdx.x] = c;
    out[192 + threadIdx.x] = e;
}

Knobs &knobs()
{
    static Knobs k = [] {
        Knobs q;
        q.bnk_tw = 0;
        q.bnk_o4 = 2;
        q.bnk_w8 = BNK_W8_DEFAULT;
        q.bnk_xcd = 1;
        q.asym_tw16 = ASYM_TW16_DEFAULT;
        q.bnk_qepi = BNK_QEPI_DEFAULT;
        q.img_groups = 2;
        q.img_span = 4;
        q.fuse_ends = 3;
        q.img_lag = 0;
        q.ig_div = 0;
        q.ic_front = IC_FRONT_DEFAULT;
        q.ic_dual = IC_DUAL_DEFAULT;
        q.ig_sb = IG_SB_DEFAULT;
        q.ic_groups = IC_GROUPS_DEFAULT;
        q.conf_reps = CONF_REPS_DEFAULT;
#ifdef SSAL_MEASURE  // measurement builds only: the product library reads no environment
        auto env = [](const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; };
        q.bnk_tw = env("SSAL_BNK_TW", 0);
        q.bnk_xcd = env("SSAL_BNK_XCD", 1);
        q.ablate = env("SSAL_ABLATE", 0);
        q.bnk_split = env("SSAL_BNK_SPLIT", 0);
        q.img_groups = env("SSAL_IMG_GROUPS", 2);
        q.fuse_ends = env("SSAL_FUSE_ENDS", 3);
#endif
        return q;
    }();
    return k;
}

unsigned long long *g_trace_buf = nullptr;
long g_trace_bytes = 0;

hipError_t launch_probe_swap(float *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_probe_swap, dim3(1), dim3(64), 0, s, out);
    return hipGetLastError();
}

// 16x16x4 family (ssal_bottleneck_mfma16.hip)
bool bottleneck_mfma16_supported(int Cin, int f);
bool bottleneck16_fits(int Cin, int H, int W);
hipError_t launch_bottleneck_mfma16(const BnkArgs &a, int Cin, hipStream_t s);
bool downsample_mfma16_supported(int Cin, int Cout);
bool downsample16_fits(int H, int W);
hipError_t launch_downsample_mfma16(const DownArgs &a, hipStream_t s);
bool upsample_mfma16_supported(int Cin, int Cout);
bool upsample16_fits(int H, int W);
hipError_t launch_upsample_mfma16(const UpArgs &a, hipStream_t s);

// Per-image size limits (ssal_internal.h).  The 32x32x2 kernels of this file address the residual / output of ONE image
// through raw buffer resources: byte offsets are evaluated in int ((pixel * C + c) * 4 and the like), num_records is the
// image's byte count, and a row outside the image gets the offset 0x80000000, which the range check must reject -- so the
// image may hold at most 2^31 bytes (2^29 floats).  Past that the sentinel lands inside the buffer (a ragged tile's idle
// lanes overwrite a valid pixel), and past 2^32 bytes num_records wraps.
//   k_bottleneck_mfma* / k_bottleneck_o4 (128 ch): x and y [H,W,128]           H * W * 128 <= 2^29
//   k_downsample_mfma (64 -> 128): y [H/2,W/2,128] (x, codes: 64-bit offsets)   (H/2) * (W/2) * 128 <= 2^29 (kept as H * W * 128 < 2^31)
//   k_upsample_mfma (128 -> 64): y [2H,2W,64] (x, codes: 64-bit offsets)        4 * H * W * 64 <= 2^29
bool bottleneck_mfma_fits(int Cin, int H, int W)
{
    return Cin == C ? (long)H * W * C <= (1L << 29) : bottleneck16_fits(Cin, H, W);
}

bool downsample_mfma_fits(int Cin, int H, int W)
{
    return Cin == CDN ? (long)H * W * C < (1L << 31) : downsample16_fits(H, W);
}

bool upsample_mfma_fits(int Cin, int H, int W)
{
    return Cin == C ? (long)4 * H * W * CUP <= (1L << 29) : upsample16_fits(H, W);
}

bool downsample_mfma_supported(int Cin, int Cout)
{
    return (Cin == CDN && Cout == C) || downsample_mfma16_supported(Cin, Cout);
}

hipError_t launch_downsample_mfma(const float *x, float *y, uint8_t *code, int N, int H, int W,
                                  int Cin, const float *wp, const float *ps, const float *pt, const float *pa,
                                  const float *wc, const float *cs, const float *ct, const float *ca,
                                  const float *we, const float *es, const float *et, const float *ra,
                                  hipStream_t s)
{
    if (H % 2 || W % 2 || !downsample_mfma_fits(Cin, H, W)) return hipErrorInvalidValue;
    DownArgs a;
    a.x = x; a.y = y; a.code = code;
    a.trace = nullptr;
    a.wp = wp; a.ps = ps; a.pt = pt; a.pa = pa;
    a.wc = wc; a.cs = cs; a.ct = ct; a.ca = ca;
    a.we = we; a.es = es; a.et = et; a.ra = ra;
    a.N = N; a.H = H; a.W = W;
    if (Cin != CDN) return launch_downsample_mfma16(a, s);
    a.TH = 8;
    const int Ho = H / 2, Wo = W / 2;
    const bool wide = Wo > 16;
    const int TW = wide ? 32 : 16;
    a.tiles_y = (Ho + a.TH - 1) / a.TH;
    a.tiles_x = (Wo + TW - 1) / TW;
    const long grid = (long)N * a.tiles_y * a.tiles_x;
    if (grid <= 0 || grid > 0x7fffffffL) return hipErrorInvalidValue;
    a.trace = (g_trace_buf && grid * 4 * 16 * 8 <= g_trace_bytes) ? g_trace_buf : nullptr;
    const double opix = (double)N * Ho * Wo;
    ProfScope prof("k_downsample_mfma", 2.0 * opix * (4.0 * CDN * F + 9.0 * F * F + F * (double)C),
                   4.0 * (4.0 * opix * CDN + opix * C) + opix * CDN, s);
    if (wide)
        hipLaunchKernelGGL(k_downsample_mfma<32>, dim3((unsigned)grid), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(k_downsample_mfma<16>, dim3((unsigned)grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

bool upsample_mfma_supported(int Cin, int Cout)
{
    return (Cin == C && Cout == CUP) || upsample_mfma16_supported(Cin, Cout);
}

hipError_t launch_upsample_mfma(const float *x, float *y, const uint8_t *code, int N, int H, int W,
                                int Cin, const float *wp, const float *ps, const float *pt, const float *pa,
                                const float *ws, const float *cs, const float *ct, const float *ca,
                                const float *we, const float *es, const float *et, const float *wr,
                                const float *ra, hipStream_t s)
{
    if (!upsample_mfma_fits(Cin, H, W)) return hipErrorInvalidValue;
    UpArgs a;
    a.x = x; a.y = y; a.code = code;
    a.trace = nullptr;
    a.wp = wp; a.ps = ps; a.pt = pt; a.pa = pa;
    a.ws = ws; a.cs = cs; a.ct = ct; a.ca = ca;
    a.we = we; a.es = es; a.et = et; a.wr = wr; a.ra = ra;
    a.N = N; a.H = H; a.W = W; a.dil = 1;
    if (Cin != C) return launch_upsample_mfma16(a, s);
    a.TH = 8;
    const bool wide = W > 16;
    const int TW = wide ? 32 : 16;
    a.tiles_y = (H + a.TH - 1) / a.TH;
    a.tiles_x = (W + TW - 1) / TW;
    const long grid = (long)N * a.tiles_y * a.tiles_x;
    if (grid <= 0 || grid > 0x7fffffffL) return hipErrorInvalidValue;
    a.trace = (g_trace_buf && grid * 4 * 16 * 8 <= g_trace_bytes) ? g_trace_buf : nullptr;
    const double pix = (double)N * H * W;
    ProfScope prof("k_upsample_mfma",
                   2.0 * pix * (C * 32.0 + 9.0 * 32 * 16 + 4.0 * 16 * CUP + C * (double)CUP),
                   4.0 * (pix * C + 4.0 * pix * CUP) + pix * CUP, s);
    if (wide)
        hipLaunchKernelGGL(k_upsample_mfma<32>, dim3((unsigned)grid), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(k_upsample_mfma<16>, dim3((unsigned)grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

bool bottleneck_mfma_supported(int Cin, int f, bool asym)
{
    return (Cin == C && f == F) || (!asym && bottleneck_mfma16_supported(Cin, f));
}

hipError_t launch_bottleneck_mfma(const float *x, float *y, int N, int H, int W, int Cin, int dil,
                                  const float *wp, const float *ps, const float *pt, const float *pa,
                                  const float *wc, const float *wc2, const float *cs, const float *ct,
                                  const float *ca, const float *we, const float *es, const float *et,
                                  const float *ra, hipStream_t s, const float *wq)
{
    if (dil < 1 || dil > 64 || !bottleneck_mfma_fits(Cin, H, W)) return hipErrorInvalidValue;
    const bool asym = wc2 != nullptr;
    if (Cin == C && !wq && (!asym || knobs().asym_tw16)) return hipErrorInvalidValue;  // these kernels read the quad layout
    if (asym && (dil != 1 || Cin != C)) return hipErrorInvalidValue;
    BnkArgs a;
    a.x = x; a.y = y;
    a.wp = wp; a.ps = ps; a.pt = pt; a.pa = pa;
    a.wc = wc; a.wc2 = wc2; a.cs = cs; a.ct = ct; a.ca = ca;
    a.we = we; a.es = es; a.et = et; a.ra = ra;
    a.wq = wq;
    a.N = N; a.H = H; a.W = W; a.dil = dil;
    const Knobs &kn = knobs();
#ifdef SSAL_MEASURE
    a.ablate = kn.ablate;
#endif
    a.trace = nullptr;
    if (Cin != C) return launch_bottleneck_mfma16(a, Cin, s);
#ifdef SSAL_MEASURE
    if (kn.bnk_split && !asym) return launch_bottleneck_split(a, s);  // bf16x3 probe: results differ in the last bits
#endif
    a.TH = 8;
    const int Hp = (H + dil - 1) / dil, Wp = (W + dil - 1) / dil;  // largest phase sub-image
    // 8x16 tiles at four workgroups per CU (k_bottleneck_o4): bnk_o4 = 1 everywhere (experiment), 2 = only where the phase
    // sub-image is at most 16 pixels wide, i.e. where 8x16 tiles are used anyway (the dilation-16 layers at 128 x 256)
    const bool o4 = !asym && Cin == C && (kn.bnk_o4 == 1 || (kn.bnk_o4 == 2 && Wp <= 16));
    // eight-wave workgroups on 8x32 tiles (bnk_w8: 1 = the regular block at dilations 1..8, 2 (default) = also the asymmetric
    // one) wherever the 8x32 kernels of the four-wave family would run; every other shape keeps the four-wave kernels
    // Images above W8_MAX_ELEMS (half the 2^29-element guard of this family) keep the four-wave kernels: the eight-wave kernels
    // were measured at the ranking shape only, and inside this limit every byte offset they form stays below 2^30.
    const bool w8_shape = Wp > 16 && kn.bnk_tw != 16 && wq != nullptr && (long)H * W * C <= W8_MAX_ELEMS;
    const bool w8 = !asym && !o4 && dil <= 8 && kn.bnk_w8 >= 1 && w8_shape;
    const bool asym_w8 = asym && kn.bnk_w8 >= 2 && w8_shape;
    const bool asym16x = asym && kn.asym_tw16 != 0 && !asym_w8;  // 8 x 16 tiles, three workgroups per CU, R written over P
    const bool wide = (Wp > 16 && kn.bnk_tw != 16 && !o4 && !asym16x) || w8 || asym_w8;
    const int TW = wide ? 32 : 16;
    a.tiles_y = (Hp + a.TH - 1) / a.TH;
    a.tiles_x = (Wp + TW - 1) / TW;
    const long grid = (long)N * dil * dil * a.tiles_y * a.tiles_x;
    if (grid <= 0 || grid > 0x7fffffffL) return hipErrorInvalidValue;
    a.ntiles = (int)grid;
    a.xcd_chunk = kn.bnk_xcd ? (int)((grid + 7) / 8) : 0;
    const long launch_grid = kn.bnk_xcd ? 8L * a.xcd_chunk : grid;
    if (g_trace_buf && launch_grid * 4 * 16 * 8 <= g_trace_bytes) a.trace = g_trace_buf;
    const double pix = (double)N * H * W;
    const double f = Cin / 4.0;
    const double taps = asym ? 10.0 : 9.0;
    // one profile row per kernel symbol, as rocprofv3 lists them
    ProfScope prof(asym_w8 ? "k_bottleneck_asym_w8" : w8 ? "k_bottleneck_w8" : asym16x ? "k_bottleneck_mfma_asym16x" : asym ? (wide ? "k_bottleneck_mfma_asym<32>" : "k_bottleneck_mfma_asym<16>")
                        : o4 ? "k_bottleneck_o4" : (wide ? "k_bottleneck_mfma<32>" : "k_bottleneck_mfma<16>"),
                   2.0 * pix * (Cin * f + taps * f * f + f * Cin),
                   4.0 * (2.0 * pix * Cin + Cin * f * 2.0 + taps * f * f), s);
    if (w8 || asym_w8) a.trace = nullptr;  // the trace buffer is laid out for four waves per workgroup
    if (asym_w8) {
        hipLaunchKernelGGL(k_bottleneck_asym_w8, dim3((unsigned)launch_grid), dim3(W8_THREADS), 0, s, a);
    } else if (w8) {
        hipLaunchKernelGGL(k_bottleneck_w8, dim3((unsigned)launch_grid), dim3(W8_THREADS), 0, s, a);
    } else if (asym16x) {
        hipLaunchKernelGGL(k_bottleneck_mfma_asym16x, dim3((unsigned)launch_grid), dim3(256), 0, s, a);
    } else if (asym) {
        if (wide)
            hipLaunchKernelGGL(k_bottleneck_mfma_asym<32>, dim3((unsigned)launch_grid), dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL(k_bottleneck_mfma_asym<16>, dim3((unsigned)launch_grid), dim3(256), 0, s, a);
    } else if (o4) {
        hipLaunchKernelGGL(k_bottleneck_o4, dim3((unsigned)launch_grid), dim3(256), 0, s, a);
    } else {
        if (wide && kn.bnk_qepi == 1)
            hipLaunchKernelGGL((k_bottleneck_mfma<32, 1>), dim3((unsigned)launch_grid), dim3(256), 0, s, a);
        else if (wide && kn.bnk_qepi >= 2)
            hipLaunchKernelGGL((k_bottleneck_mfma<32, 2>), dim3((unsigned)launch_grid), dim3(256), 0, s, a);
        else if (wide)
            hipLaunchKernelGGL(k_bottleneck_mfma<32>, dim3((unsigned)launch_grid), dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL(k_bottleneck_mfma<16>, dim3((unsigned)launch_grid), dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace ssal
