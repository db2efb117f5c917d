"""The guarded-allocation harness (tests/guarded_alloc.py) has teeth: the same code the GPU tests run, on CPU tensors
with the device filter set to "cpu".  Every planted stray byte must be reported with its side and offset, every clean
use must pass, and the patch must be gone afterwards."""
import numpy as np
import pytest
import torch

from guarded_alloc import G, PATTERNS, PATTERN_IDS, GuardedAlloc, GuardViolation, guarded_alloc, pattern_values, same_bits  # noqa: F401

ORIG_EMPTY, ORIG_EMPTY_LIKE = torch.empty, torch.empty_like


def _slab_of(g, t):
    return g._find(t).slab


@pytest.mark.parametrize("pattern", PATTERNS, ids=PATTERN_IDS)
@pytest.mark.parametrize("shape,dtype", [((2, 3, 5), torch.float32), ((7,), torch.uint8), ((3, 1, 2), torch.float64),
                                         ((4, 4), torch.int64), ((5,), torch.int32), ((), torch.float32)])
def test_interior_is_the_tensor_the_unpatched_call_gives(guarded_alloc, pattern, shape, dtype):
    want = ORIG_EMPTY(shape, dtype=dtype, device="cpu")
    g = guarded_alloc("cpu", pattern)
    for t in (torch.empty(shape, dtype=dtype, device="cpu"), torch.empty(*shape, dtype=dtype) if shape else None):
        if t is None:
            continue
        assert t.dtype == want.dtype and t.shape == want.shape and t.device == want.device and t.is_contiguous()
        assert t.stride() == want.stride()
        slab = _slab_of(g, t)
        nbytes = want.numel() * want.element_size()
        assert slab.dtype == torch.uint8 and slab.numel() == G + nbytes + G
        assert t.untyped_storage().data_ptr() == slab.untyped_storage().data_ptr()
        assert t.storage_offset() * t.element_size() == G and t.data_ptr() == slab.data_ptr() + G  # a view at offset G
        assert t.data_ptr() % 256 == slab.data_ptr() % 256                                        # alignment kept
        assert bool((slab == pattern).all())                                                      # guards AND interior
        assert g.is_guarded(t) and g.is_guarded(t.reshape(-1)[1:] if t.numel() > 1 else t)
    assert g.count == (2 if shape else 1) and g.live == g.count
    g.check()


def test_default_dtype_and_device_follow_torch(guarded_alloc):
    g = guarded_alloc("cpu", 0x7F)
    t = torch.empty(3, 2)
    assert t.dtype == torch.get_default_dtype() and t.device.type == "cpu" and g.is_guarded(t)
    t = torch.empty(size=(3, 2), dtype=torch.uint8)
    assert t.shape == (3, 2) and g.is_guarded(t)
    t = torch.empty(torch.Size([2, 2]), dtype=torch.float64)
    assert t.shape == (2, 2) and g.is_guarded(t)
    t = torch.empty([2, 5], dtype=torch.float32, requires_grad=True)
    assert t.requires_grad and g.is_guarded(t)
    g.check()


def test_empty_like_is_covered(guarded_alloc):
    g = guarded_alloc("cpu", 0xFE)
    src = ORIG_EMPTY((3, 5, 2), dtype=torch.float32)
    t = torch.empty_like(src)
    assert t.shape == src.shape and t.dtype == src.dtype and t.is_contiguous() and g.is_guarded(t) and g.count == 1
    assert bool((t.view(torch.uint8) == 0xFE).all())
    u = torch.empty_like(src, dtype=torch.int64)
    assert u.dtype == torch.int64 and u.shape == src.shape and g.is_guarded(u) and int(u[0, 0, 0]) == pattern_values(0xFE)["int64"]
    v = torch.empty_like(src.transpose(0, 2))  # a strided source: the interior is contiguous, shape kept
    assert v.shape == (2, 5, 3) and v.is_contiguous() and g.is_guarded(v)
    assert not g.is_guarded(src) and g.count == 3
    g.check()


@pytest.mark.parametrize("shape,dtype,nbytes", [((0,), torch.float32, 0), ((3, 0, 2), torch.float64, 0), ((0,), torch.uint8, 0),
                                                ((1,), torch.uint8, 1), ((3,), torch.uint8, 3), ((5, 7), torch.uint8, 35),
                                                ((4097,), torch.uint8, 4097)])
def test_zero_size_and_byte_counts_that_are_no_multiple_of_four(guarded_alloc, shape, dtype, nbytes):
    g = guarded_alloc("cpu", 0xFF)
    t = torch.empty(shape, dtype=dtype, device="cpu")
    assert t.shape == shape and t.dtype == dtype and t.numel() * t.element_size() == nbytes
    slab = _slab_of(g, t)
    assert slab.numel() == 2 * G + nbytes  # zero elements: a slab of the two guards only
    t.zero_()                              # a clean use: writes the whole interior and nothing else
    g.check()
    slab[G + nbytes] = 0                   # the first byte past the interior, at any alignment
    with pytest.raises(GuardViolation) as e:
        g.check()
    (v,) = e.value.violations
    assert v["side"] == "rear" and v["first_offset"] == 0 == v["last_offset"] and v["nbytes"] == nbytes


def test_a_clean_use_passes_and_refill_restores_the_poison(guarded_alloc):
    g = guarded_alloc("cpu", 0x7F)
    ws = torch.empty(1000, dtype=torch.uint8, device="cpu")
    out = torch.empty((4, 6), dtype=torch.float32, device="cpu")
    x = g.guarded_from_numpy(np.arange(24, dtype=np.float32).reshape(4, 6))
    y = g.guarded_clone(torch.arange(5, dtype=torch.int64))
    assert g.count == 2 and g.live == 4  # inputs are guarded and checked, but are not allocations of the code under test
    assert x.dtype == torch.float32 and x.shape == (4, 6) and g.is_guarded(x) and g.is_guarded(y)
    assert np.array_equal(x.numpy(), np.arange(24, dtype=np.float32).reshape(4, 6)) and y.tolist() == [0, 1, 2, 3, 4]
    assert bool((_slab_of(g, x)[:G] == 0x7F).all()) and bool((_slab_of(g, x)[G + 96:] == 0x7F).all())
    out.copy_(x * 2)
    ws[:].fill_(3)
    ws[-1] = 9  # the last interior byte
    out[-1, -1] = 1.0
    g.check()
    g.refill(ws)
    assert bool((ws == 0x7F).all())
    g.refill(out[1:])  # any view of the interior names it
    assert float(out[0, 0]) == pattern_values(0x7F)["float32"]
    with pytest.raises(ValueError):
        g.refill(ORIG_EMPTY(3))
    g.check()
    g.release()
    assert g.live == 0 and not g.is_guarded(ws)
    g.check()


@pytest.mark.parametrize("pattern", PATTERNS, ids=PATTERN_IDS)
@pytest.mark.parametrize("where,side,offset", [("end", "rear", 0), ("end+G-1", "rear", G - 1), ("-1", "front", -1),
                                               ("-G", "front", -G)])
def test_one_stray_byte_is_reported_with_side_and_offset(guarded_alloc, pattern, where, side, offset):
    g = guarded_alloc("cpu", pattern)
    clean = torch.empty((16,), dtype=torch.float64, device="cpu")
    t = torch.empty((3, 7), dtype=torch.float32, device="cpu")  # 84 bytes: the call site is the line this test names
    nbytes = 84
    slab = _slab_of(g, t)
    pos = {"end": G + nbytes, "end+G-1": G + nbytes + G - 1, "-1": G - 1, "-G": 0}[where]
    g.check()
    slab[pos] = 0x11
    with pytest.raises(GuardViolation) as e:
        g.check()
    (v,) = e.value.violations  # the clean neighbour is not reported
    assert v["side"] == side and v["first_offset"] == offset and v["last_offset"] == offset and v["count"] == 1
    assert v["first_value"] == 0x11 == v["last_value"]
    assert v["shape"] == (3, 7) and v["dtype"] == torch.float32 and v["index"] == 1 and v["kind"] == "empty"
    assert "test_guarded_alloc_cpu.py" in v["site"] and "test_one_stray_byte_is_reported_with_side_and_offset" in v["site"]
    msg = str(e.value)
    assert side + " guard" in msg and "shape=(3, 7)" in msg and "torch.float32" in msg and "0x11" in msg and v["site"] in msg
    assert g.is_guarded(clean)


def test_a_run_of_stray_bytes_reports_first_and_last(guarded_alloc):
    g = guarded_alloc("cpu", 0xFF)
    t = torch.empty((10,), dtype=torch.float32, device="cpu")
    x = g.guarded_from_numpy(np.zeros(3, dtype=np.uint8))
    slab = _slab_of(g, t)
    slab[G + 40 + 4:G + 40 + 20] = torch.arange(1, 17, dtype=torch.uint8)   # a float4 store one element past the end
    _slab_of(g, x)[G - 8:G] = 5                                            # and two floats before an input
    with pytest.raises(GuardViolation) as e:
        g.check()
    a, b = e.value.violations
    assert (a["side"], a["first_offset"], a["last_offset"], a["count"], a["first_value"], a["last_value"]) == ("rear", 4, 19, 16, 1, 16)
    assert (b["side"], b["first_offset"], b["last_offset"], b["count"], b["kind"]) == ("front", -8, -1, 8, "input")


@pytest.mark.parametrize("pattern", PATTERNS, ids=PATTERN_IDS)
def test_a_stray_byte_of_the_patterns_own_value_is_the_blind_spot(guarded_alloc, pattern):
    """why the GPU tests run three patterns: a stray store of byte b is invisible under pattern b, and only there"""
    seen = []
    for p in PATTERNS:
        g = guarded_alloc("cpu", p)
        t = torch.empty((8,), dtype=torch.uint8, device="cpu")
        _slab_of(g, t)[G + 8] = pattern
        try:
            g.check()
            seen.append(False)
        except GuardViolation as e:
            assert e.violations[0]["first_value"] == pattern
            seen.append(True)
    assert seen == [p != pattern for p in PATTERNS]


def test_patch_is_removed_on_exit_also_after_an_exception():
    assert torch.empty is ORIG_EMPTY and torch.empty_like is ORIG_EMPTY_LIKE
    with GuardedAlloc("cpu", 0xFF) as g:
        assert torch.empty is not ORIG_EMPTY and torch.empty_like is not ORIG_EMPTY_LIKE
        assert g.is_guarded(torch.empty(3))
        with pytest.raises(RuntimeError):
            GuardedAlloc("cpu", 0x7F).__enter__()  # one at a time
    assert torch.empty is ORIG_EMPTY and torch.empty_like is ORIG_EMPTY_LIKE
    with pytest.raises(KeyError):
        with GuardedAlloc("cpu", 0xFF) as g:
            torch.empty(3)
            raise KeyError("boom")
    assert torch.empty is ORIG_EMPTY and torch.empty_like is ORIG_EMPTY_LIKE
    assert g.live == 0 and not g.is_guarded(torch.empty(3))
    with pytest.raises(ValueError):
        GuardedAlloc("cpu", 0x1FF)
    with pytest.raises(ValueError):
        GuardedAlloc("cpu", 0xFF, guard=100)


def test_allocations_for_other_devices_pass_through(guarded_alloc):
    g = guarded_alloc("cuda", 0xFF)  # a GPU is selected: CPU tensors are not ours (and no GPU is touched by that)
    a = torch.empty((4, 4), dtype=torch.float32)
    b = torch.empty((4, 4), dtype=torch.float32, device="cpu")
    c = torch.empty_like(a)
    m = torch.empty((2, 2), device="meta")
    assert not g.is_guarded(a) and not g.is_guarded(b) and not g.is_guarded(c) and m.device.type == "meta"
    assert a.untyped_storage().nbytes() == 64 and g.count == 0 and g.live == 0
    g = guarded_alloc("cpu", 0xFF)
    m = torch.empty((2, 2), device="meta")
    assert m.device.type == "meta" and g.count == 0
    o = ORIG_EMPTY(4)
    r = torch.empty(4, out=o)  # out=: the caller's own memory
    assert r.data_ptr() == o.data_ptr() and g.count == 0
    cl = torch.empty((1, 3, 4, 4), memory_format=torch.channels_last)
    assert cl.is_contiguous(memory_format=torch.channels_last) and g.count == 0


@pytest.mark.parametrize("pattern,f32,f64,u8,i64", [
    (0xFF, np.nan, np.nan, 255, -1),
    (0x7F, 3.39e38, 1.4e306, 127, 0x7F7F7F7F7F7F7F7F),
    (0xFE, -1.69e38, -5.4e303, 254, -0x0101010101010102),
])
def test_every_pattern_decodes_to_the_documented_values(guarded_alloc, pattern, f32, f64, u8, i64):
    g = guarded_alloc("cpu", pattern)
    got = {"float32": torch.empty(3, dtype=torch.float32)[1].item(), "float64": torch.empty(3, dtype=torch.float64)[2].item(),
           "uint8": torch.empty(3, dtype=torch.uint8)[0].item(), "int64": torch.empty(3, dtype=torch.int64)[1].item()}
    pv = pattern_values(pattern)
    for k in got:
        assert same_bits(np.asarray(got[k], dtype=k), np.asarray(pv[k], dtype=k)), k
    if np.isnan(f32):
        assert np.isnan(got["float32"]) and np.isnan(got["float64"])
    else:
        assert np.isfinite(got["float32"]) and np.isfinite(got["float64"])
        assert abs(got["float32"] / f32 - 1) < 5e-3 and abs(got["float64"] / f64 - 1) < 5e-2
        assert np.sign(got["float32"]) == np.sign(f32) == np.sign(got["float64"])
    assert got["uint8"] == u8 and got["int64"] == i64
    g.check()


def test_same_bits_compares_nan_payloads_and_refuses_shape_or_dtype_changes():
    a = np.array([np.nan, 1.0, -0.0], dtype=np.float32)
    assert same_bits(a, a.copy()) and same_bits(torch.from_numpy(a), a)
    assert not same_bits(a, np.array([np.nan, 1.0, 0.0], dtype=np.float32))  # -0.0 != +0.0 in bits
    assert not same_bits(a, a.astype(np.float64)) and not same_bits(a, a.reshape(3, 1))
