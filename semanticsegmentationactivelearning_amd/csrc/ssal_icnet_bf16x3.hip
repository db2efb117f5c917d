// ssal_icnet_bf16x3.hip -- OPT-IN arithmetic mode SSAL_ARITH_BF16X3 (include/ssal_enet.h) of ICNet's implicit-GEMM
// convolution: k_igemm_bf16x3<NT>, the plain form of k_igemm (ssal_icnet_kernels.hip: UP2 = 0, no DUAL) in the six-product
// split-operand arithmetic of ssal_bottleneck_bf16x3.hip.  Never the default.  gfx950 (MI355X / CDNA4) only.
//
//   D[pixel][cout] = sum over (kh, kw) ascending, 32-channel chunks ascending, two K = 16 steps per chunk, of the six
//   v_mfma_f32_32x32x16_bf16 products x3w1, x2w2, x1w3, x2w1, x1w2, x1w1 (x = activation term, w = kernel term; small terms
//   first), fp32 accumulation in the MFMA accumulator; the epilogue is k_igemm's to the letter.
//
// Everything that is not arithmetic is k_igemm's: tile = 128 pixels x 32 NT output channels, wave w owns pixel rows
// [32 w, 32 w + 32) and all NT column tiles, raw buffer resources with 32-bit offsets, IG_OOB for SAME padding and for rows
// past M (the hardware answers zeros; the split of 0 is (0, 0, 0), so padding stays an exact zero), the xcd_chunk tile remap.
//
// Operands.
//   A  the activation chunk (128 pixels x 32 channels) goes global -> registers -> LDS as fp32, rows padded to 36 floats, in
//      natural channel order.  Lane (r, h) of wave w reads channels 16 s + 8 h .. + 7 of row 32 w + r for step s (two
//      ds_read_b128, conflict-free on the 36-float pitch) and splits them IN REGISTERS (split_pack8).  Wave w is the only
//      reader of its 32 rows and lane (r, h) the only reader of those eight channels, so every A element is split exactly
//      once per workgroup -- the same count as a split in front of the LDS write, which would cost 192 B instead of 128 B
//      of LDS per pixel row and chunk (DESIGN.md section 35 has the numbers of both).
//   B  the kernel is pre-split at commit (bf16x3::pack_igemm): [tap][Cin/16][CoutP/32] chunks of CHUNK_UNITS 16-byte units
//      in MFMA operand order [term][lane].  A workgroup stages the 2 NT chunks of a 32-channel step as they are (6 KB x NT),
//      and every wave reads its fragments with three ds_read_b128 per column tile and step: lane l reads unit l of a term,
//      consecutive lanes consecutive 16 bytes.
// LDS: two buffers at NT = 1 / 2 (48 / 60 KB: three / two workgroups per CU), ONE at NT = 4 (42 KB, two barriers per chunk,
// three workgroups per CU instead of one with two buffers).
#include "ssal_bf16x3.h"
#include "ssal_icnet.h"
#include "ssal_internal.h"
#include "ssal_mfma.h"

namespace ssal {

namespace {

constexpr int BX_BM = 128, BX_LDK = 36;
constexpr unsigned BX_OOB = 0xFFFFFFFFu;  // k_igemm's IG_OOB: a byte offset no tensor reaches
constexpr int BX_CHUNK_BYTES = bf16x3::CHUNK_UNITS * 16;

}  // namespace

template <int NT>
__global__ __launch_bounds__(256, NT == 2 ? 2 : 3) void k_igemm_bf16x3(IgemmArgs a, const uint4 *wpk)
{
    constexpr int BM = BX_BM, LDK = BX_LDK;
    constexpr int NBUF = NT >= 4 ? 1 : 2;
    constexpr int A_BYTES = BM * LDK * 4;                 // 18432
    constexpr int B_UNITS = 2 * NT * bf16x3::CHUNK_UNITS;  // 16-byte units of one 32-channel step: [s][nt][term][lane]
    constexpr int BUF_BYTES = A_BYTES + B_UNITS * 16;
    constexpr int NBL = (B_UNITS + 255) / 256;            // kernel units a thread stages per chunk
    __shared__ __attribute__((aligned(16))) unsigned char smem[NBUF * BUF_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;

    int tile = blockIdx.x;
    if (a.xcd_chunk) {
        tile = (int)(blockIdx.x & 7) * a.xcd_chunk + (int)(blockIdx.x >> 3);
        if (tile >= a.ntiles) return;  // whole workgroup, before any barrier
    }
    const int tn = tile % a.tiles_n, tm = tile / a.tiles_n;
    const int m0 = tm * BM;
    const int n0 = tn * 32 * NT;
    const int M = (int)a.M;
    const int nb32 = a.CoutP >> 5;

    const rsrc_t xrs = make_rsrc(a.x, (unsigned)((long)a.N * a.H * a.W * a.Cin * 4));
    const rsrc_t wrs = make_rsrc(wpk, (unsigned)((long)a.KH * a.KW * (a.Cin >> 4) * nb32 * BX_CHUNK_BYTES));

    // ---- per-thread A rows (tid >> 3) + 32 i, channel quad tid & 7: k_igemm's plain loader ----
    const int col4 = tid & 7;
    int iyb[4], ixb[4];
    unsigned nbase[4];
    bool mv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + (tid >> 3) + 32 * i;
        mv[i] = m < M;
        const unsigned mm = mv[i] ? (unsigned)m : 0u;
        const unsigned t = mm / (unsigned)a.Wo;
        const int ox = (int)(mm - t * (unsigned)a.Wo);
        const unsigned n = t / (unsigned)a.Ho;
        const int oy = (int)(t - n * (unsigned)a.Ho);
        iyb[i] = oy * a.stride - a.pad_t;
        ixb[i] = ox * a.stride - a.pad_l;
        nbase[i] = (unsigned)n * (unsigned)(a.H * a.W * a.Cin * 4) + 16u * col4;
    }
    const int cpt = a.Cin >> 5;
    const int nchunks = a.KH * a.KW * cpt;
    const unsigned rowb = (unsigned)(a.W * a.Cin * 4), pixb = (unsigned)(a.Cin * 4);

    // kernel units of this thread: unit u = tid + 256 j of the staged image is unit (u % (192 NT)) of K = 16 step u / (192 NT);
    // in memory the two steps of a chunk lie nb32 chunks apart, the NT column tiles of one step side by side
    unsigned boff[NBL];
#pragma unroll
    for (int j = 0; j < NBL; ++j) {
        const int u = tid + 256 * j;
        const int s = u / (NT * bf16x3::CHUNK_UNITS), rem = u - s * (NT * bf16x3::CHUNK_UNITS);
        boff[j] = u < B_UNITS ? (unsigned)(s * nb32 * bf16x3::CHUNK_UNITS + rem) * 16u : BX_OOB;
    }
    unsigned ld_wofs = (unsigned)(tn * NT) * (unsigned)BX_CHUNK_BYTES;  // wave-uniform byte offset of the next chunk's kernel units

    unsigned aoff[4];
    float4 rq[4];
    uint4 rb[NBL];
    int ld_cc = 0, ld_kh = 0, ld_kw = 0;
    auto tap_offsets = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int iy = iyb[i] + ld_kh * a.dil, ix = ixb[i] + ld_kw * a.dil;
            const bool ok = mv[i] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            aoff[i] = ok ? nbase[i] + (unsigned)iy * rowb + (unsigned)ix * pixb : BX_OOB;
        }
    };
    auto gload = [&]() {
        if (ld_cc == 0) tap_offsets();  // wave-uniform
        const unsigned cofs = 128u * (unsigned)ld_cc;
#pragma unroll
        for (int q = 0; q < 4; ++q) rq[q] = bload4(xrs, aoff[q], cofs);
#pragma unroll
        for (int j = 0; j < NBL; ++j)
            rb[j] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(wrs, boff[j], ld_wofs, 0));
        ld_wofs += 2u * (unsigned)nb32 * (unsigned)BX_CHUNK_BYTES;
        if (++ld_cc == cpt) {
            ld_cc = 0;
            if (++ld_kw == a.KW) { ld_kw = 0; ++ld_kh; }
        }
    };
    auto lds_write = [&](int buf) {
        unsigned char *base = smem + buf * BUF_BYTES;
        float *As = reinterpret_cast<float *>(base);
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<float4 *>(As + ((tid >> 3) + 32 * i) * LDK + 4 * col4) = rq[i];
        uint4 *Bs = reinterpret_cast<uint4 *>(base + A_BYTES);
#pragma unroll
        for (int j = 0; j < NBL; ++j)
            if (tid + 256 * j < B_UNITS) Bs[tid + 256 * j] = rb[j];
    };

    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[nt][i] = 0.0f;
    gload();
    lds_write(0);
    __syncthreads();
    for (int t = 0; t < nchunks; ++t) {
        const bool more = t + 1 < nchunks;
        const int buf = NBUF == 1 ? 0 : t & 1;
        const float *As = reinterpret_cast<const float *>(smem + buf * BUF_BYTES) + (32 * wave + r) * LDK + 8 * h;
        const uint4 *Bs = reinterpret_cast<const uint4 *>(smem + buf * BUF_BYTES + A_BYTES) + lane;
        if (more) gload();  // the loads of chunk t + 1 are in flight across the matrix section
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const float4 lo = *reinterpret_cast<const float4 *>(As + 16 * s);
            const float4 hi = *reinterpret_cast<const float4 *>(As + 16 * s + 4);
            const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            const bf16x3::Split3 xa = bf16x3::split_pack8(v);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const uint4 *bp = Bs + (s * NT + nt) * bf16x3::CHUNK_UNITS;
                bf16x3::Split3 wb;
                wb.t1 = bp[0];
                wb.t2 = bp[64];
                wb.t3 = bp[128];
                acc[nt] = bf16x3::mfma6(xa, wb, acc[nt]);
            }
        }
        if (NBUF == 1) __syncthreads();  // every wave has read its last fragment of chunk t
        if (more) lds_write(NBUF == 1 ? 0 : (t + 1) & 1);
        __syncthreads();
    }

    // ---- epilogue: k_igemm's -- folded batch-norm, shortcut add, ReLU, store ----
    const unsigned ybytes = (unsigned)(a.M * a.Cout * 4);
    const rsrc_t yrs = make_rsrc(a.y, ybytes);
    const rsrc_t rrs = make_rsrc(a.res ? a.res : a.y, ybytes);
    unsigned moff[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int m = m0 + 32 * wave + (i & 3) + 8 * (i >> 2) + 4 * h;
        moff[i] = m < M ? (unsigned)m * (unsigned)(a.Cout * 4) : BX_OOB;
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = n0 + 32 * nt + r;
        const float sc = a.scale[co], sh = a.shift[co];
        const bool cok = co < a.Cout;
        float rv[16];
        if (a.res) {  // wave-uniform
#pragma unroll
            for (int i = 0; i < 16; ++i) rv[i] = bload(rrs, (cok && moff[i] != BX_OOB) ? moff[i] + 4u * co : BX_OOB, 0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            float v = fmaf(acc[nt][i], sc, sh);
            if (a.res) v = v + rv[i];
            if (a.relu) v = v > 0.0f ? v : 0.0f;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), yrs,
                                                  (cok && moff[i] != BX_OOB) ? moff[i] + 4u * co : BX_OOB, 0, 0);
        }
    }
}

// a = launch_igemm's arguments with the tile counts for this NT filled in; packed = bf16x3::pack_igemm of the kernel
hipError_t launch_igemm_bf16x3(const IgemmArgs &a, int NT, const void *packed, int grid, hipStream_t s)
{
    if (!packed || a.up2 || a.x2) return hipErrorInvalidValue;
    // the packed kernel is addressed with 32-bit byte offsets like every other tensor of the launch
    if ((long)a.KH * a.KW * (a.Cin >> 4) * (a.CoutP >> 5) * BX_CHUNK_BYTES >= (1L << 32) - 16384) return hipErrorInvalidValue;
    const uint4 *w = reinterpret_cast<const uint4 *>(packed);
    if (NT == 4) hipLaunchKernelGGL((k_igemm_bf16x3<4>), dim3(grid), dim3(256), 0, s, a, w);
    else if (NT == 2) hipLaunchKernelGGL((k_igemm_bf16x3<2>), dim3(grid), dim3(256), 0, s, a, w);
    else if (NT == 1) hipLaunchKernelGGL((k_igemm_bf16x3<1>), dim3(grid), dim3(256), 0, s, a, w);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace ssal
