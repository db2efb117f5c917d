"""PNG / zlib corpus shared by tests/test_png_cpu.py and tests/test_gpu_png.py: PNGs written with a chosen filter type
per row, PNGs re-chunked into many IDAT chunks, zlib streams with flushes, long matches and far distances."""
import io
import struct
import zlib

import numpy as np
from PIL import Image


def chunk(ctype, body):
    return struct.pack(">I", len(body)) + ctype + body + struct.pack(">I", zlib.crc32(body, zlib.crc32(ctype)) & 0xffffffff)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(img, filters):
    """uint8 [h, w, c] -> filtered scanlines (filter byte + bytes) with filters[y] applied to row y"""
    h, w, c = img.shape
    rows = img.reshape(h, w * c).astype(np.int32)
    out = bytearray()
    for y in range(h):
        cur = rows[y]
        prev = rows[y - 1] if y else np.zeros_like(cur)
        left = np.concatenate([np.zeros(c, np.int32), cur[:-c]])
        ul = np.concatenate([np.zeros(c, np.int32), prev[:-c]])
        f = int(filters[y % len(filters)])
        pred = [np.zeros_like(cur), left, prev, (left + prev) >> 1, _paeth(left, prev, ul)][f]
        out.append(f)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def write_png(img, color_type, filters=(0,), level=6, strategy=zlib.Z_DEFAULT_STRATEGY, idat_size=None, palette=None,
              interlace=0, depth=8):
    """a PNG of uint8 [h, w, c] written by hand: chosen filter per row, zlib level / strategy, IDAT chunk size"""
    h, w = img.shape[:2]
    img = img.reshape(h, w, -1)
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    data = co.compress(filter_rows(img, filters)) + co.flush()
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, interlace))
    if color_type == 3:
        pal = palette if palette is not None else bytes(range(256)) * 3
        out += chunk(b"PLTE", pal[:768])
    step = idat_size or len(data)
    for i in range(0, len(data), step):
        out += chunk(b"IDAT", data[i:i + step])
    return out + chunk(b"IEND", b"")


def rechunk(png_bytes, idat_size):
    """the same PNG with its IDAT data split into chunks of idat_size bytes"""
    pos, head, idat, tail = 8, [], b"", []
    while pos < len(png_bytes):
        n, t = struct.unpack_from(">I4s", png_bytes, pos)
        body = png_bytes[pos + 8:pos + 8 + n]
        pos += 12 + n
        if t == b"IDAT":
            idat += body
        elif idat:
            tail.append(chunk(t, body))
        else:
            head.append(chunk(t, body))
    mid = [chunk(b"IDAT", idat[i:i + idat_size]) for i in range(0, len(idat), idat_size)]
    return png_bytes[:8] + b"".join(head + mid + tail)


def pillow_png(arr, mode=None, **kw):
    b = io.BytesIO()
    im = Image.fromarray(arr, mode=mode)
    if mode == "P":
        im.putpalette(list(range(256)) * 3)  # a full palette: Pillow writes bit depth 8
    im.save(b, format="PNG", **kw)
    return b.getvalue()


def pillow_decode(data):
    a = np.asarray(Image.open(io.BytesIO(data)))
    return a[:, :, None] if a.ndim == 2 else a


def photo(h, w, c, seed):
    """smooth gradients + noise + flat areas: every filter type and both literals and matches show up"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = (x * 3 + y * 5)[..., None] + np.arange(c)[None, None, :] * 40
    img = base + rng.integers(-6, 7, size=(h, w, c))
    img[h // 3:h // 2, :] = 77
    return (img % 256).astype(np.uint8)


def png_corpus():
    """[(name, png bytes)]: colour types 0/2/3/6, widths 1, 3, 2047, 2048, all filters and mixes, IDAT splits"""
    out = []
    for ct, c in ((0, 1), (2, 3), (3, 1), (6, 4)):
        for w in (1, 3, 2047, 2048):
            h = 3 if w >= 2047 else 9
            img = photo(h, w, c, seed=w * 10 + ct)
            for filters in ((0,), (1,), (2,), (3,), (4,), (0, 1, 2, 3, 4), (4, 2, 3, 1, 0)):
                out.append(("ct%d_w%d_f%s" % (ct, w, "".join(map(str, filters))), write_png(img, ct, filters)))
    img = photo(40, 37, 3, seed=5)
    for lvl in (0, 1, 6, 9):
        for strat in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE):
            out.append(("rgb_l%d_s%d" % (lvl, strat), write_png(img, 2, (0, 1, 2, 3, 4), level=lvl, strategy=strat)))
    p = pillow_png(photo(33, 50, 3, seed=9))
    out.append(("pillow_rgb", p))
    out.append(("idat_1byte", rechunk(p, 1)))
    out.append(("idat_7byte", rechunk(p, 7)))
    out.append(("pillow_gray", pillow_png(photo(21, 30, 1, seed=3)[:, :, 0])))
    out.append(("pillow_P", pillow_png(photo(21, 30, 1, seed=4)[:, :, 0], mode="P")))
    out.append(("pillow_rgba", pillow_png(photo(17, 19, 4, seed=6))))
    return out


def zlib_corpus():
    """[(name, raw, zlib stream)]"""
    rng = np.random.default_rng(1)
    text = (rng.integers(0, 6, size=60000).astype(np.uint8) + 97).tobytes()
    far = rng.bytes(32768)
    cases = {
        "text": text,
        "zeros": bytes(100000),                      # distance-1 runs, length-258 matches
        "far": far + far[:300] + rng.bytes(100) + far[:5000],  # distance 32768 matches
        "noise": rng.bytes(70000),
        "mixed": text[:20000] + bytes(5000) + rng.bytes(9000) + text[:20000],
        "empty": b"",
    }
    out = []
    for name, raw in cases.items():
        for lvl in (0, 1, 6, 9):
            for strat in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE):
                out.append(("%s_l%d_s%d" % (name, lvl, strat), raw, _compress(raw, lvl, strat)))
        # sync / full flushes inside the stream (empty stored blocks)
        co = zlib.compressobj(6)
        z = b""
        for i in range(0, len(raw), 7001):
            z += co.compress(raw[i:i + 7001]) + co.flush(zlib.Z_SYNC_FLUSH if (i // 7001) % 2 else zlib.Z_FULL_FLUSH)
        out.append(("%s_flush" % name, raw, z + co.flush()))
    return out


def _compress(raw, lvl, strat):
    co = zlib.compressobj(lvl, zlib.DEFLATED, 15, 9, strat)
    return co.compress(raw) + co.flush()
