"""PNG container parsing for the GPU decode path (``InputStage(decode="gpu")``).

``parse(data)`` walks the chunks of one encoded image on the host -- signature, IHDR, the IDAT payload split over any
number of chunks -- and checks the zlib header.  It returns a ``PngStream`` whose ``payload`` pieces, concatenated, are
the zlib stream the device inflates (``include/ssal_enet.h``, PNG decode), or ``None`` when the image needs the Pillow
path: not a PNG (JPEG, ...), bit depth other than 8, interlaced, colour type 4 (gray + alpha), a zlib preset dictionary
or a method other than deflate, or a container this parser does not accept.  ``None`` is a per-image decision: the
caller decodes that image with Pillow, which also raises what it raises for a corrupt file.

``inflate_host`` / ``unfilter_host`` run the library's inflate and unfilter source on the CPU (tests, debugging).
"""
import ctypes
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 6: 4}  # colour type -> bytes per pixel at bit depth 8 (palette: the index)

# per-stream status words (include/ssal_enet.h SSAL_PNG_*)
STATUS = {0: "ok", 1: "truncated", 2: "bad code lengths", 3: "distance before start of output", 4: "size mismatch",
          5: "bad Adler-32", 6: "bad filter type", 7: "unsupported"}
OK = 0


class PngStream:
    """one PNG image ready for the device: ``payload`` is a list of memoryviews (the IDAT data, in order) of total
    length ``nbytes``; ``width`` x ``height`` x ``channels`` uint8 once decoded"""
    __slots__ = ("payload", "nbytes", "width", "height", "channels", "color_type")

    def __init__(self, payload, nbytes, width, height, channels, color_type):
        self.payload, self.nbytes = payload, nbytes
        self.width, self.height, self.channels, self.color_type = width, height, channels, color_type

    def raw_bytes(self):
        return self.height * (1 + self.width * self.channels)

    def joined(self):
        return b"".join(self.payload)


def parse(data, check_crc=True):
    """-> PngStream, or None (decode this image with Pillow)"""
    mv = memoryview(data)
    n = len(mv)
    if n < 8 or bytes(mv[:8]) != SIGNATURE:
        return None
    pos = 8
    ihdr = None
    pieces, total = [], 0
    seen_idat_end = False
    while True:
        if pos + 8 > n:
            return None  # no IEND: let Pillow decide what a truncated file is
        length, ctype = struct.unpack_from(">I4s", mv, pos)
        start, end = pos + 8, pos + 8 + length
        if end + 4 > n:
            return None
        body = mv[start:end]
        if check_crc and (zlib.crc32(body, zlib.crc32(ctype)) & 0xffffffff) != struct.unpack_from(">I", mv, end)[0]:
            return None
        pos = end + 4
        if ihdr is None:
            if ctype != b"IHDR" or length != 13:
                return None
            ihdr = struct.unpack(">IIBBBBB", body)
            continue
        if ctype == b"IDAT":
            if seen_idat_end:
                return None  # IDAT chunks must be consecutive
            pieces.append(body)
            total += length
        else:
            if pieces:
                seen_idat_end = True
            if ctype == b"IEND":
                break
    width, height, depth, color, method, filt, interlace = ihdr
    if depth != 8 or color not in CHANNELS or method != 0 or filt != 0 or interlace != 0:
        return None
    if width < 1 or height < 1 or total < 2:
        return None
    head = b""
    for p in pieces:  # the two zlib header bytes may straddle 1-byte IDAT chunks
        head += bytes(p[:2 - len(head)])
        if len(head) == 2:
            break
    cmf, flg = head[0], head[1]
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31 != 0 or (flg & 0x20):
        return None
    return PngStream(pieces, total, width, height, CHANNELS[color], color)


def inflate_host(stream, out_cap):
    """(status, bytes) of the library's inflate run on the host over one zlib stream, into a buffer of out_cap bytes"""
    from .._lib import lib, check
    src = np.frombuffer(bytes(stream), dtype=np.uint8)
    out = np.zeros(max(int(out_cap), 1), dtype=np.uint8)
    got, st = ctypes.c_int64(0), ctypes.c_int32(-1)
    check(lib().ssal_inflate_host(src.ctypes.data_as(ctypes.c_void_p), len(src), out.ctypes.data_as(ctypes.c_void_p),
                                  int(out_cap), ctypes.byref(got), ctypes.byref(st)))
    return st.value, out[:got.value].tobytes()


def unfilter_host(raw, height, width, channels):
    """(status, uint8 [height, width, channels]) of the library's unfilter run on the host over the inflated scanlines"""
    from .._lib import lib, check
    buf = np.frombuffer(bytes(raw), dtype=np.uint8).copy()
    if len(buf) != height * (1 + width * channels):
        raise ValueError("raw scanlines have %d bytes, expected %d" % (len(buf), height * (1 + width * channels)))
    st = ctypes.c_int32(-1)
    check(lib().ssal_png_unfilter_host(buf.ctypes.data_as(ctypes.c_void_p), height, width, channels, ctypes.byref(st)))
    img = buf.reshape(height, 1 + width * channels)[:, 1:].reshape(height, width, channels)
    return st.value, img


def decode_host(data):
    """whole PNG through the host build of the device decoder: uint8 [h, w, c] (the palette index for colour type 3),
    or None when ``parse`` sends the image to Pillow; raises ValueError with the status of a stream that fails"""
    s = parse(data)
    if s is None:
        return None
    st, raw = inflate_host(s.joined(), s.raw_bytes())
    if st == OK and len(raw) != s.raw_bytes():
        st = 4
    if st == OK:
        st, img = unfilter_host(raw, s.height, s.width, s.channels)
        if st == OK:
            return img
    raise ValueError("PNG decode failed: %s" % STATUS.get(st, st))
