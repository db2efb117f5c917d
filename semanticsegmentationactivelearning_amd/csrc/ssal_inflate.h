// ssal_inflate.h -- zlib / DEFLATE inflate (RFC 1950 / 1951) and PNG scanline unfilter (PNG spec section 9), written
// once as __host__ __device__ code: the GPU decoder (ssal_png.hip) runs it with one wave per stream, the host entry points
// (ssal_inflate_host / ssal_png_unfilter_host) run the identical source with a single lane, so the CPU tests exercise the
// exact code the device runs -- malformed streams included.
//
// Lane model: every lane of the wave keeps the same decoder state (bit buffer, positions, symbols), so the decode loop is
// wave-uniform.  Only the bulk work is split across the lanes: filling the Huffman lookup tables, match copies, stored-block
// copies, the Adler-32 sums and the byte-parallel filter types.  `lane` / `nl` are (threadIdx.x, 64) on the device and
// (0, 1) on the host.
//
// Safety: every read of the input is bounds-checked against [0, in_len) and every write of the output against
// [0, out_cap), whatever the bytes hold; a violation ends the stream with a status word (Status below).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SSAL_HD __host__ __device__
#else
#define SSAL_HD
#endif

namespace ssal {
namespace png {

// per-stream status word (include/ssal_enet.h SSAL_PNG_*)
enum Status : int32_t {
    ST_OK = 0,
    ST_TRUNCATED = 1,     // the input ended before the final block / the Adler-32 trailer
    ST_BAD_CODES = 2,     // invalid block type, stored-length check, code-length set or symbol
    ST_BAD_DISTANCE = 3,  // a match reaches before the start of the output
    ST_SIZE = 4,          // the output would exceed its extent, or its size differs from the expected one
    ST_ADLER = 5,         // Adler-32 trailer mismatch
    ST_BAD_FILTER = 6,    // PNG filter type byte > 4
    ST_UNSUPPORTED = 7,   // zlib header: CM != 8, CINFO > 7, FDICT = 1, bad FCHECK; or a descriptor out of range
};

constexpr int kLitBits = 10, kDistBits = 9;  // first-level lookup widths; longer codes take the canonical slow path
constexpr int kMaxBits = 15;
constexpr int kWindow = 32768;  // DEFLATE history: the match sources are read from this ring, never from the output

// lookup entry: (length << 9) | symbol; length 0 = "code longer than the table width" -> canonical decode
struct Tables {
    uint16_t lfast[1 << kLitBits];
    uint16_t dfast[1 << kDistBits];
    int16_t lcount[kMaxBits + 1], dcount[kMaxBits + 1];
    int16_t lsym[288], dsym[32];
    uint8_t lens[320];
    int16_t ccount[kMaxBits + 1], csym[19];  // code-length code
};

SSAL_HD inline void wave_sync()
{
#if defined(__HIP_DEVICE_COMPILE__)
    // stores of one lane are read by other lanes of the same wave: order them for the compiler and the memory pipeline
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
}

SSAL_HD inline uint32_t wave_sum(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
#endif
    return v;
}

// bounds-checked little-endian bit reader over [in, in + len).  Aligned 32-bit words are loaded one refill AHEAD of their
// use (`ahead`), so the load latency hides behind the symbols decoded in between; unaligned heads and the tail go bytewise.
struct Bits {
    const uint8_t *in;
    int64_t len, pos;  // pos: next byte not yet loaded (into buf or ahead)
    uint64_t buf;
    int cnt;
    uint32_t ahead;
    int ahead_ok;

    SSAL_HD static bool aligned(const uint8_t *p) { return ((uintptr_t)p & 3u) == 0u; }
    SSAL_HD void prefetch()
    {
        ahead_ok = 0;
        if (pos + 4 <= len && aligned(in + pos)) {
            ahead = *(const uint32_t *)(in + pos);
            pos += 4;
            ahead_ok = 1;
        }
    }
    SSAL_HD void refill()
    {
        for (;;) {
            if (ahead_ok) {
                if (cnt > 32) return;
                buf |= (uint64_t)ahead << cnt;
                cnt += 32;
            } else {
                if (cnt > 56 || pos >= len) return;
                buf |= (uint64_t)in[pos] << cnt;
                ++pos;
                cnt += 8;
            }
            prefetch();
        }
    }
    // n <= 32 bits; false if the input is exhausted
    SSAL_HD bool need(int n)
    {
        if (cnt < n) refill();
        return cnt >= n;
    }
    SSAL_HD uint32_t take(int n)
    {
        const uint32_t v = (uint32_t)(buf & ((1ull << n) - 1ull));
        buf >>= n;
        cnt -= n;
        return v;
    }
    // byte position of the next unread whole byte (after dropping to a byte boundary); forgets what is buffered
    SSAL_HD int64_t byte_pos_reset()
    {
        const int64_t p = pos - (ahead_ok ? 4 : 0) - (cnt >> 3);
        buf = 0ull;
        cnt = 0;
        ahead_ok = 0;
        return p;
    }
    SSAL_HD void seek(int64_t p)
    {
        pos = p;
        buf = 0ull;
        cnt = 0;
        prefetch();
    }
};

// canonical Huffman code (puff.c style counts + symbols) and its first-level lookup table.
// Returns 0 complete, > 0 incomplete, < 0 over-subscribed.
SSAL_HD inline int build_code(const uint8_t *lens, int n, int16_t *count, int16_t *sym, uint16_t *fast, int fbits, int lane,
                              int nl)
{
    int16_t c[kMaxBits + 1];
    for (int l = 0; l <= kMaxBits; ++l) c[l] = 0;
    for (int s = 0; s < n; ++s) c[lens[s]]++;
    int left = 1;
    for (int l = 1; l <= kMaxBits; ++l) {
        left <<= 1;
        left -= c[l];
        if (left < 0) return left;
    }
    int16_t offs[kMaxBits + 1];
    offs[1] = 0;
    for (int l = 1; l < kMaxBits; ++l) offs[l + 1] = offs[l] + c[l];
    if (lane == 0) {
        for (int l = 0; l <= kMaxBits; ++l) count[l] = c[l];
        for (int s = 0; s < n; ++s)
            if (lens[s]) sym[offs[lens[s]]++] = (int16_t)s;
    }
    if (fast) {
        const int size = 1 << fbits;
        for (int i = lane; i < size; i += nl) fast[i] = 0;
        wave_sync();
        // canonical codes of the lengths <= fbits, bit-reversed (DEFLATE sends Huffman codes MSB first)
        int code = 0;
        int next[kMaxBits + 1];
        next[0] = 0;
        for (int l = 1; l <= kMaxBits; ++l) {
            code = (code + (l > 1 ? c[l - 1] : 0)) << 1;
            next[l] = code;
        }
        for (int s = 0; s < n; ++s) {
            const int l = lens[s];
            if (l == 0) continue;
            const int cd = next[l]++;
            if (l > fbits) continue;
            int rev = 0;
            for (int b = 0; b < l; ++b) rev |= ((cd >> b) & 1) << (l - 1 - b);
            const uint16_t e = (uint16_t)((l << 9) | s);
            for (int k = rev + (lane << l); k < size; k += nl << l) fast[k] = e;
        }
    }
    wave_sync();
    return left;
}

// decode one symbol; -1 truncated, -2 invalid code
SSAL_HD inline int decode_sym(Bits &br, const uint16_t *fast, int fbits, const int16_t *count, const int16_t *sym)
{
    if (br.cnt < kMaxBits) br.refill();
    const uint16_t e = fast ? fast[br.buf & ((1u << fbits) - 1u)] : 0;
    if (e >> 9) {
        const int l = e >> 9;
        if (l > br.cnt) return -1;
        br.buf >>= l;
        br.cnt -= l;
        return e & 511;
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= kMaxBits; ++l) {
        if (l > br.cnt) return -1;
        code |= (int)((br.buf >> (l - 1)) & 1u);
        const int cnt = count[l];
        if (code - cnt < first) {
            br.buf >>= l;
            br.cnt -= l;
            return sym[index + (code - first)];
        }
        index += cnt;
        first += cnt;
        first <<= 1;
        code <<= 1;
    }
    return -2;
}

SSAL_HD inline void length_base(int i, int &base, int &extra)  // i = symbol - 257, 0..28
{
    if (i < 8) { base = 3 + i; extra = 0; }
    else if (i == 28) { base = 258; extra = 0; }
    else { extra = (i - 4) >> 2; base = ((4 + ((i - 4) & 3)) << extra) + 3; }
}

SSAL_HD inline void dist_base(int i, int &base, int &extra)  // i = 0..29
{
    if (i < 4) { base = 1 + i; extra = 0; }
    else { extra = (i - 2) >> 1; base = ((2 + (i & 1)) << extra) + 1; }
}

// inflate one zlib stream (2-byte header, DEFLATE blocks, Adler-32) from in[0, in_len) into out[0, out_cap).
// *out_len receives the number of bytes produced.  Every lane returns the same status.  win: kWindow bytes of history
// ring (LDS on the device): every byte goes to out AND to the ring, and match copies read the ring only, so the output is
// written with plain stores that nothing waits for.
SSAL_HD inline int32_t inflate_zlib(const uint8_t *in, int64_t in_len, uint8_t *out, int64_t out_cap, int64_t *out_len,
                                    Tables &t, uint8_t *win, int lane, int nl)
{
    Bits br{in, in_len, 0, 0ull, 0, 0u, 0};
    br.prefetch();
    int64_t o = 0;
    if (out_len) *out_len = 0;
    if (!br.need(16)) return ST_TRUNCATED;
    const uint32_t cmf = br.take(8), flg = br.take(8);
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) return ST_UNSUPPORTED;

    int last = 0;
    while (!last) {
        if (!br.need(3)) return ST_TRUNCATED;
        last = (int)br.take(1);
        const int type = (int)br.take(2);
        if (type == 0) {  // stored: to a byte boundary, LEN, NLEN, LEN raw bytes
            br.take(br.cnt & 7);
            if (!br.need(32)) return ST_TRUNCATED;
            const uint32_t len = br.take(16), nlen = br.take(16);
            if (len != (~nlen & 0xffffu)) return ST_BAD_CODES;
            // the bytes still buffered come first, then the input itself
            const int64_t start = br.byte_pos_reset();
            if (start + (int64_t)len > in_len) return ST_TRUNCATED;
            if (o + (int64_t)len > out_cap) return ST_SIZE;
            for (int64_t i = lane; i < (int64_t)len; i += nl) {
                const uint8_t v = in[start + i];
                out[o + i] = v;
                win[(o + i) & (kWindow - 1)] = v;
            }
            o += len;
            br.seek(start + len);
            wave_sync();
            continue;
        }
        if (type == 3) return ST_BAD_CODES;
        if (type == 1) {  // fixed codes
            if (lane == 0) {
                for (int s = 0; s < 144; ++s) t.lens[s] = 8;
                for (int s = 144; s < 256; ++s) t.lens[s] = 9;
                for (int s = 256; s < 280; ++s) t.lens[s] = 7;
                for (int s = 280; s < 288; ++s) t.lens[s] = 8;
                for (int s = 0; s < 30; ++s) t.lens[288 + s] = 5;
            }
            wave_sync();
            build_code(t.lens, 288, t.lcount, t.lsym, t.lfast, kLitBits, lane, nl);
            build_code(t.lens + 288, 30, t.dcount, t.dsym, t.dfast, kDistBits, lane, nl);
        } else {  // dynamic codes
            if (!br.need(14)) return ST_TRUNCATED;
            const int nlen = (int)br.take(5) + 257, ndist = (int)br.take(5) + 1, ncode = (int)br.take(4) + 4;
            if (nlen > 286 || ndist > 30) return ST_BAD_CODES;
            const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            uint8_t cl[19];
            for (int i = 0; i < 19; ++i) cl[i] = 0;
            for (int i = 0; i < ncode; ++i) {
                if (!br.need(3)) return ST_TRUNCATED;
                cl[order[i]] = (uint8_t)br.take(3);
            }
            if (build_code(cl, 19, t.ccount, t.csym, nullptr, 0, lane, nl) != 0) return ST_BAD_CODES;
            int idx = 0;
            uint8_t prev = 0;
            while (idx < nlen + ndist) {
                int s = decode_sym(br, nullptr, 0, t.ccount, t.csym);
                if (s == -1) return ST_TRUNCATED;
                if (s < 0) return ST_BAD_CODES;
                int rep = 1;
                uint8_t v = (uint8_t)s;
                if (s >= 16) {
                    if (s == 16) {
                        if (idx == 0) return ST_BAD_CODES;
                        if (!br.need(2)) return ST_TRUNCATED;
                        v = prev;
                        rep = 3 + (int)br.take(2);
                    } else if (s == 17) {
                        if (!br.need(3)) return ST_TRUNCATED;
                        v = 0;
                        rep = 3 + (int)br.take(3);
                    } else {
                        if (!br.need(7)) return ST_TRUNCATED;
                        v = 0;
                        rep = 11 + (int)br.take(7);
                    }
                }
                if (idx + rep > nlen + ndist) return ST_BAD_CODES;
                if (lane == 0)
                    for (int r = 0; r < rep; ++r) t.lens[idx + r] = v;
                idx += rep;
                prev = v;
            }
            wave_sync();
            if (t.lens[256] == 0) return ST_BAD_CODES;  // no end-of-block code
            int err = build_code(t.lens, nlen, t.lcount, t.lsym, t.lfast, kLitBits, lane, nl);
            if (err < 0 || (err > 0 && nlen != t.lcount[0] + t.lcount[1])) return ST_BAD_CODES;
            err = build_code(t.lens + nlen, ndist, t.dcount, t.dsym, t.dfast, kDistBits, lane, nl);
            if (err < 0 || (err > 0 && ndist != t.dcount[0] + t.dcount[1])) return ST_BAD_CODES;
        }
        // decode loop: literals by lane 0, match copies by every lane
        for (;;) {
            const int s = decode_sym(br, t.lfast, kLitBits, t.lcount, t.lsym);
            if (s < 0) return s == -1 ? ST_TRUNCATED : ST_BAD_CODES;
            if (s < 256) {
                if (o >= out_cap) return ST_SIZE;
                if (lane == 0) {
                    out[o] = (uint8_t)s;
                    win[o & (kWindow - 1)] = (uint8_t)s;
                }
                ++o;
                continue;
            }
            if (s == 256) break;
            if (s > 285) return ST_BAD_CODES;
            int base, extra;
            length_base(s - 257, base, extra);
            if (!br.need(extra)) return ST_TRUNCATED;
            const int len = base + (int)br.take(extra);
            const int ds = decode_sym(br, t.dfast, kDistBits, t.dcount, t.dsym);
            if (ds < 0) return ds == -1 ? ST_TRUNCATED : ST_BAD_CODES;
            if (ds > 29) return ST_BAD_CODES;
            dist_base(ds, base, extra);
            if (!br.need(extra)) return ST_TRUNCATED;
            const int dist = base + (int)br.take(extra);
            if ((int64_t)dist > o) return ST_BAD_DISTANCE;
            if (o + len > out_cap) return ST_SIZE;
            wave_sync();
            // sources lie in [o - dist, o): an overlapping copy (dist < len) repeats with period dist.  A ring slot written
            // here is never a source of the same copy (that would need dist > kWindow).
            const int64_t s0 = o - dist;
            for (int i = lane; i < len; i += nl) {
                const uint8_t v = win[(s0 + (dist >= len ? i : i % dist)) & (kWindow - 1)];
                out[o + i] = v;
                win[(o + i) & (kWindow - 1)] = v;
            }
            o += len;
            wave_sync();
        }
    }
    // Adler-32 trailer (big-endian) at the next byte boundary
    br.take(br.cnt & 7);
    if (!br.need(32)) return ST_TRUNCATED;
    uint32_t want = 0;
    for (int i = 0; i < 4; ++i) want = (want << 8) | br.take(8);
    if (out_len) *out_len = o;
    wave_sync();
    // A = 1 + sum d_i, B = n + sum (n - i) d_i  (mod 65521); each lane sums the bytes i = lane (mod nl)
    const uint32_t MOD = 65521u;
    uint64_t a = 0, b = 0;
    uint32_t w = (uint32_t)((o - lane) % MOD);  // (o - i) mod 65521, stepped down by nl
    const uint32_t step = (uint32_t)nl % MOD;
    int k = 0;
    for (int64_t i = lane; i < o; i += nl) {
        const uint32_t d = out[i];
        a += d;
        b += (uint64_t)w * d;
        w = w >= step ? w - step : w + MOD - step;
        if (++k == 4096) { a %= MOD; b %= MOD; k = 0; }
    }
    uint32_t A = wave_sum((uint32_t)(a % MOD)) % MOD;
    uint32_t B = wave_sum((uint32_t)(b % MOD)) % MOD;
    A = (A + 1u) % MOD;
    B = (uint32_t)((B + (uint64_t)(o % MOD)) % MOD);
    if (((B << 16) | A) != want) return ST_ADLER;
    return ST_OK;
}

SSAL_HD inline int paeth(int a, int b, int c)
{
    const int p = a + b - c;
    int pa = p - a, pb = p - b, pc = p - c;
    pa = pa < 0 ? -pa : pa;
    pb = pb < 0 ? -pb : pb;
    pc = pc < 0 ? -pc : pc;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// one filtered scanline -> reconstructed bytes, in place.  cur / prev are distinct rows (prev == nullptr on row 0).
SSAL_HD inline void unfilter_row(int f, uint8_t *__restrict__ cur, const uint8_t *__restrict__ prev, int n, int bpp,
                                 int lane, int nl)
{
    if (f == 0) return;
    if (f == 2) {
        if (prev)
            for (int i = lane; i < n; i += nl) cur[i] = (uint8_t)(cur[i] + prev[i]);
        return;
    }
    // Sub / Average / Paeth: serial along the row, one lane per byte of a pixel.  The row is walked in chunks of 16
    // pixels: the chunk's loads are issued together, the dependent chain then runs in registers.
    constexpr int CH = 16;
    for (int c = lane; c < bpp; c += nl) {
        int left = 0, ul = 0;
        int i = c;
        for (; i + (CH - 1) * bpp < n; i += CH * bpp) {
            int cv[CH], pv[CH];
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                cv[k] = cur[i + k * bpp];
                pv[k] = prev ? prev[i + k * bpp] : 0;
            }
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                const int up = pv[k];
                const int p = f == 1 ? left : (f == 3 ? (left + up) >> 1 : paeth(left, up, ul));
                left = (cv[k] + p) & 255;
                cv[k] = left;
                ul = up;
            }
#pragma unroll
            for (int k = 0; k < CH; ++k) cur[i + k * bpp] = (uint8_t)cv[k];
        }
        for (; i < n; i += bpp) {
            const int up = prev ? prev[i] : 0;
            const int p = f == 1 ? left : (f == 3 ? (left + up) >> 1 : paeth(left, up, ul));
            left = (cur[i] + p) & 255;
            cur[i] = (uint8_t)left;
            ul = up;
        }
    }
}

// PNG unfilter of a whole non-interlaced 8-bit image, in place: raw holds height rows of (1 filter byte + width * bpp).
SSAL_HD inline int32_t unfilter_image(uint8_t *raw, int height, int width, int bpp, int lane, int nl)
{
    const int64_t stride = 1 + (int64_t)width * bpp;
    for (int y = 0; y < height; ++y) {
        uint8_t *row = raw + y * stride;
        const int f = row[0];
        if (f > 4) return ST_BAD_FILTER;
        unfilter_row(f, row + 1, y ? row + 1 - stride : nullptr, (int)(stride - 1), bpp, lane, nl);
        wave_sync();
    }
    return ST_OK;
}

}  // namespace png
}  // namespace ssal
