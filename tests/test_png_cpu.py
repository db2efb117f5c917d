"""CPU tests of the PNG decode path (include/ssal_enet.h "PNG decode"): the host build of the SAME inflate / unfilter
source the GPU runs (ssal_inflate.h) against zlib and Pillow, its status words on malformed streams, the chunk parser's
fallback classification, and the InputStage option."""
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from png_corpus import chunk, png_corpus, pillow_decode, pillow_png, photo, rechunk, write_png, zlib_corpus
from semanticsegmentationactivelearning_amd.tensortools import InputStage, png

TRUNCATED, BAD_CODES, BAD_DISTANCE, SIZE, ADLER, BAD_FILTER, UNSUPPORTED = range(1, 8)


@pytest.mark.parametrize("name,raw,z", zlib_corpus(), ids=[c[0] for c in zlib_corpus()])
def test_inflate_matches_zlib(name, raw, z):
    assert zlib.decompress(z) == raw
    st, out = png.inflate_host(z, len(raw))
    assert st == png.OK, png.STATUS[st]
    assert out == raw


@pytest.mark.parametrize("name,data", png_corpus(), ids=[c[0] for c in png_corpus()])
def test_png_decode_matches_pillow(name, data):
    got = png.decode_host(data)
    assert got is not None
    want = pillow_decode(data)
    assert got.shape == want.shape and np.array_equal(got, want)


# ---- malformed streams: the right status, never outside the extents ----------------------------------------------------
class _BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value, n):  # LSB first
        self.bits += [(value >> i) & 1 for i in range(n)]

    def code(self, code, n):  # Huffman codes go MSB first
        self.bits += [(code >> (n - 1 - i)) & 1 for i in range(n)]

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def _zlib(deflate, raw=b""):
    return b"\x78\x9c" + deflate + struct.pack(">I", zlib.adler32(raw))


def test_truncated_at_every_block_boundary_and_byte():
    raw = (b"abcabcabd" * 3000) + bytes(range(256)) * 40
    co = zlib.compressobj(6)
    z = b""
    cuts = []
    for i in range(0, len(raw), 4000):
        z += co.compress(raw[i:i + 4000]) + co.flush(zlib.Z_FULL_FLUSH)
        cuts.append(len(z))
    z += co.flush()
    assert zlib.decompress(z) == raw
    for cut in cuts[:-1] + list(range(0, 300)) + list(range(len(z) - 12, len(z))):
        st, out = png.inflate_host(z[:cut], len(raw))
        assert st == TRUNCATED, (cut, png.STATUS[st])
        assert len(out) <= len(raw)


def test_bad_adler_and_size():
    raw = photo(20, 20, 3, 0).tobytes()
    z = bytearray(zlib.compress(raw, 6))
    z[-1] ^= 1
    assert png.inflate_host(bytes(z), len(raw))[0] == ADLER
    good = zlib.compress(raw, 6)
    assert png.inflate_host(good, len(raw) - 1)[0] == SIZE  # over-long output for its extent
    assert png.inflate_host(zlib.compress(b"x" * 5000, 9), 4999)[0] == SIZE  # ... in a match copy


def test_distance_before_start():
    w = _BitWriter()
    w.put(1, 1), w.put(1, 2)  # final, fixed codes
    w.code(0x30 + ord("a"), 8)  # literal 'a'
    w.code(0b0000001, 7)  # length 3
    w.code(1, 5)  # distance 2 > 1 byte produced
    w.code(0, 7)  # end of block
    assert png.inflate_host(_zlib(w.bytes(), b"aaaa"), 100)[0] == BAD_DISTANCE
    w = _BitWriter()
    w.put(1, 1), w.put(1, 2)
    w.code(0x30 + ord("a"), 8)
    w.code(0b0000001, 7)
    w.code(0, 5)  # distance 1: fine
    w.code(0, 7)
    assert png.inflate_host(_zlib(w.bytes(), b"aaaa"), 4) == (png.OK, b"aaaa")


def test_invalid_code_length_sets():
    # dynamic block: 19 code-length codes of length 1 -> over-subscribed
    w = _BitWriter()
    w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(0, 5), w.put(15, 4)
    for _ in range(19):
        w.put(1, 3)
    assert png.inflate_host(_zlib(w.bytes()), 100)[0] == BAD_CODES
    # block type 3
    w = _BitWriter()
    w.put(1, 1), w.put(3, 2)
    assert png.inflate_host(_zlib(w.bytes()), 100)[0] == BAD_CODES
    # stored block with NLEN != ~LEN
    assert png.inflate_host(b"\x78\x01" + b"\x01\x05\x00\x00\x00" + b"hello" + b"\0\0\0\0", 100)[0] == BAD_CODES
    # HLIT > 286
    w = _BitWriter()
    w.put(1, 1), w.put(2, 2), w.put(30, 5), w.put(0, 5), w.put(0, 4)
    w.put(0, 64)
    assert png.inflate_host(_zlib(w.bytes()), 100)[0] == BAD_CODES
    # a random-bytes body: every outcome is a status, none is a crash or an overrun
    rng = np.random.default_rng(0)
    for _ in range(300):
        body = rng.bytes(int(rng.integers(1, 200)))
        st, out = png.inflate_host(b"\x78\x9c" + body, 64)
        assert st in png.STATUS and len(out) <= 64


def test_unsupported_zlib_headers():
    raw = b"hello world" * 10
    z = zlib.compress(raw)
    fdict = bytes([0x78, 0xBB]) + z[2:]  # FDICT set, FCHECK still valid
    assert (0x78 * 256 + 0xBB) % 31 == 0
    assert png.inflate_host(fdict, len(raw))[0] == UNSUPPORTED
    assert png.inflate_host(bytes([0x77, z[1]]) + z[2:], len(raw))[0] == UNSUPPORTED  # CM != 8
    assert png.inflate_host(bytes([0x78, 0x9d]) + z[2:], len(raw))[0] == UNSUPPORTED  # FCHECK


def test_bad_filter_type():
    raw = bytes([0]) + bytes(12) + bytes([5]) + bytes(12)  # row 1 has filter type 5
    st, _ = png.unfilter_host(raw, 2, 4, 3)
    assert st == BAD_FILTER


# ---- chunk parser ----------------------------------------------------------------------------------------------------
def _jpeg():
    b = io.BytesIO()
    Image.fromarray(photo(16, 16, 3, 1)).save(b, format="JPEG")
    return b.getvalue()


def test_parser_classifies_fallbacks():
    rgb = photo(10, 12, 3, 2)
    assert png.parse(pillow_png(rgb)) is not None
    assert png.parse(rechunk(pillow_png(rgb), 1)) is not None
    assert png.parse(_jpeg()) is None
    assert png.parse(pillow_png(np.arange(120, dtype=np.uint16).reshape(10, 12) * 500)) is None  # 16-bit
    assert png.parse(pillow_png(photo(10, 16, 1, 2)[:, :, 0] > 128)) is None  # 1-bit
    assert png.parse(pillow_png(photo(10, 12, 2, 2), mode="LA")) is None  # colour type 4
    assert png.parse(write_png(rgb, 2, interlace=1)) is None  # interlaced
    assert png.parse(write_png(rgb, 2, depth=4)) is None
    # zlib preset dictionary / method != deflate in the IDAT stream
    good = write_png(rgb, 2)
    s = png.parse(good)
    z = s.joined()
    for head in (bytes([0x78, 0xBB]), bytes([0x77, 0x9c])):
        bad = good[:good.index(b"IDAT") - 4] + chunk(b"IDAT", head + z[2:]) + chunk(b"IEND", b"")
        assert png.parse(bad) is None
    # container damage: bad CRC, missing IEND, not a PNG
    broken = bytearray(good)
    broken[good.index(b"IDAT") + 10] ^= 0xFF
    assert png.parse(bytes(broken)) is None
    assert png.parse(good[:-12]) is None
    assert png.parse(b"") is None
    assert s.width == 12 and s.height == 10 and s.channels == 3 and s.nbytes == len(z)


def test_parser_channels_per_colour_type():
    assert png.parse(pillow_png(photo(4, 5, 1, 0)[:, :, 0])).channels == 1
    assert png.parse(pillow_png(photo(4, 5, 1, 0)[:, :, 0], mode="P")).color_type == 3
    assert png.parse(pillow_png(photo(4, 5, 4, 0))).channels == 4


def test_input_stage_decode_option():
    assert InputStage([8, 8]).decode == "cpu"
    st = InputStage([8, 8], decode="gpu", decode_ahead=16)
    assert st.decode == "gpu" and st.decode_ahead == 16 and st.decode_stats == {"gpu": 0, "fallback": 0}
    with pytest.raises(ValueError):
        InputStage([8, 8], decode="tpu")
    with pytest.raises(ValueError):
        InputStage([8, 8], decode="gpu", decode_ahead=0)
