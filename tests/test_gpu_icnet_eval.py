"""ICNet's fused validation pass on the MI355X: ``ICNet.evaluate`` (ssal_icnet_evaluate_nhwc: conv6_interp + argmax +
confusion matrix inside one up-sampling kernel, k_upeval) against the composed route it replaces
(``ICNet._evaluate_composed``: the label plane of ``score`` + ``tensortools.metrics.confusion_mat``).  Every comparison
is exact: the counts are integers and the argmax is the label plane's.

Sizes.  The kernel's tile is 256 consecutive 1/4-resolution pixels of one image (one thread per 4 x 4 block of output
pixels).  64 x 128 frames (the size of tests/golden/icnet_c3k19_64x128.npz) give a 16 x 32 map = exactly two tiles per
image, with interior pixels and all four borders of the 4x interpolation.  ICNet's size guard wants H and W divisible by 32
(``ssal_icnet_eval_workspace_bytes`` returns -1 below that), so 32 x 32 is the smallest frame: its 8 x 8 map fills a quarter
of one tile; 96 x 160 (24 x 40 = 960 = 3.75 tiles) has whole tiles followed by a partial one."""
import ctypes

import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _lib
from semanticsegmentationactivelearning_amd import synthetic as syn

pytestmark = pytest.mark.gpu

TILE = 256          # 1/4-resolution pixels per workgroup (UPEVAL_TILE, csrc/ssal_icnet_eval.hip)
H, W, N = 64, 128, 2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    _lib.lib()
    yield
    torch.cuda.synchronize()


def _net(k, seed=0):
    net = ssal.ICNet(k)
    net.build((None, None, None, 3))
    syn.randomize_icnet(net, seed=seed)
    return net


@pytest.fixture(scope="module")
def nets():
    return {k: _net(k, seed=k) for k in (2, 19, 32)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _targets(n, h, w, k, seed):
    """labels random in [0, K) with a band of 255 (ignored); mask random 0 / 1, the LAST image's all zero"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, k, size=(n, h, w), dtype=np.uint8)
    lab[:, h // 4:h // 4 + 5, :] = 255
    mask = (rng.random((n, h, w)) < 0.8).astype(np.uint8)
    mask[n - 1] = 0
    return lab, mask


def _counted(lab, mask, k):
    """pixels a confusion matrix of weights 0 / 1 must hold: mask 1 and label < K"""
    m = np.ones_like(lab) if mask is None else mask
    return int(((m != 0) & (lab < k)).sum())


@pytest.mark.parametrize("k", [2, 19, 32])
def test_evaluate_equals_the_composed_route(nets, k):
    net = nets[k]
    x = syn.synth_frames_device(3, N, H, W, 3)
    lab, mask = _targets(N, H, W, k, seed=10 + k)
    lab_d, mask_d = dev(lab), dev(mask)
    # with mask
    got, want = net.evaluate(x, lab_d, mask_d), net._evaluate_composed(x, lab_d, mask_d)
    assert got.dtype == torch.int64 and tuple(got.shape) == (k, k)
    assert torch.equal(got, want)
    assert int(got.sum()) == _counted(lab, mask, k) > 0
    # without mask (weight 1; the 255 band is dropped by its key)
    got1, want1 = net.evaluate(x, lab_d), net._evaluate_composed(x, lab_d)
    assert torch.equal(got1, want1)
    assert int(got1.sum()) == _counted(lab, None, k)
    # added into a pre-filled matrix
    start = np.random.default_rng(k).integers(0, 1 << 40, size=(k, k)).astype(np.int64)
    acc = dev(start)
    assert net.evaluate(x, lab_d, mask_d, confusion=acc) is acc
    assert torch.equal(acc, dev(start) + want)
    # mask values are weights (the reference's bincount), not flags
    heavy = dev(mask * np.uint8(7))
    assert torch.equal(net.evaluate(x, lab_d, heavy), 7 * want)
    assert torch.equal(net.evaluate(x, lab_d, heavy), net._evaluate_composed(x, lab_d, heavy))


@pytest.mark.parametrize("k,tied", [(2, (0, 1)), (3, (0, 2)), (19, (3, 7))])
def test_exact_ties_take_the_label_planes_class(k, tied):
    """conv6_cls kernel and bias zero for two classes: their logits are exactly equal (0) at every output pixel, so
    wherever they are the maximum the prediction is decided by the tie rule alone (first maximum)"""
    net = _net(k, seed=40 + k)
    kern, bias = net.conv6_cls.kernel.numpy().copy(), net.conv6_cls.bias.numpy().copy()
    kern[..., list(tied)] = 0.0
    bias[list(tied)] = 0.0
    net.conv6_cls.kernel.assign(kern)
    net.conv6_cls.bias.assign(bias)
    x = syn.synth_frames_device(5, N, H, W, 3)
    _, extra = net.score(x, measure="confidence", return_label=True)
    pred = extra["label"].cpu().numpy()
    assert not (pred == tied[1]).any(), "the fixture's second tied class can never be the first maximum"
    if k <= 3:
        assert (pred == tied[0]).any(), "the fixture must have pixels the tie decides"
    lab, mask = _targets(N, H, W, k, seed=50 + k)
    lab[0, H // 2:] = tied[1]  # rows of the matrix that a wrong tie rule would move to the diagonal
    got = net.evaluate(x, dev(lab), dev(mask))
    assert torch.equal(got, net._evaluate_composed(x, dev(lab), dev(mask)))
    assert int(got[:, tied[1]].sum()) == 0


def test_uint8_frames_count_as_their_fp32_twin(nets):
    net = nets[19]
    xu = syn.synth_frames_device(7, N, H, W, 3, dtype=torch.uint8)
    xf = syn.synth_frames_device(7, N, H, W, 3)  # the same frames as fp32 x * (1/255)
    assert torch.equal(xf, xu.to(torch.float32) * float(np.float32(1.0 / 255.0)))
    lab, mask = _targets(N, H, W, 19, seed=70)
    got_u, got_f = net.evaluate(xu, dev(lab), dev(mask)), net.evaluate(xf, dev(lab), dev(mask))
    assert torch.equal(got_u, got_f)
    assert torch.equal(got_u, net._evaluate_composed(xu, dev(lab), dev(mask)))


def test_batch_independence(nets):
    net = nets[19]
    x = syn.synth_frames_device(9, N, H, W, 3)
    lab, mask = _targets(N, H, W, 19, seed=90)
    mask[N - 1] = mask[0]  # both images count
    lab_d, mask_d = dev(lab), dev(mask)
    whole = net.evaluate(x, lab_d, mask_d)
    parts = net.evaluate(x[:1], lab_d[:1], mask_d[:1]) + net.evaluate(x[1:], lab_d[1:], mask_d[1:])
    assert torch.equal(whole, parts)
    # two image-group chains: both tail launches add into the same replicas
    assert _lib.get_knobs()["ic_groups"] == 1
    try:
        _lib.set_knob("ic_groups", 2)
        assert torch.equal(net.evaluate(x, lab_d, mask_d), whole)
    finally:
        _lib.set_knob("ic_groups", 1)


@pytest.mark.parametrize("n,h,w", [(1, 32, 32), (2, 96, 160)])
def test_partial_tiles_count_only_pixels_of_the_image(nets, n, h, w):
    net = nets[19]
    L = _lib.lib()
    x = syn.synth_frames_device(11, n, h, w, 3)
    handle = net._sync_handle()
    # the size guard: 32 x 32 is the smallest frame the pass accepts, and neither map is a whole number of tiles
    assert L.ssal_icnet_eval_workspace_bytes(handle, 1, 16, 16) == -1
    assert L.ssal_icnet_eval_workspace_bytes(handle, 1, 32, 32) > L.ssal_icnet_workspace_bytes(handle, 1, 32, 32) > 0
    assert ((h // 4) * (w // 4)) % TILE != 0
    lab, mask = _targets(n, h, w, 19, seed=h)
    mask[n - 1] = 1
    for m in (mask, None):
        got = net.evaluate(x, dev(lab), None if m is None else dev(m))
        assert int(got.sum()) == _counted(lab, m, 19)
        assert torch.equal(got, net._evaluate_composed(x, dev(lab), None if m is None else dev(m)))


def test_error_paths(nets):
    net = nets[19]
    L = _lib.lib()
    x = syn.synth_frames_device(13, N, H, W, 3)
    lab, mask = _targets(N, H, W, 19, seed=130)
    lab_d, mask_d = dev(lab), dev(mask)
    with pytest.raises(ValueError, match="labels must have shape"):
        net.evaluate(x, lab_d[:, :-1], mask_d)
    with pytest.raises(ValueError, match="mask must have shape"):
        net.evaluate(x, lab_d, mask_d[:1])
    with pytest.raises(ValueError, match="confusion must be"):  # a matrix of another class count
        net.evaluate(x, lab_d, mask_d, confusion=torch.zeros((6, 6), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="confusion must be"):
        net.evaluate(x, lab_d, mask_d, confusion=torch.zeros((19, 19), dtype=torch.int32, device="cuda"))
    # the raw entry
    handle = net._sync_handle()
    need = L.ssal_icnet_eval_workspace_bytes(handle, N, H, W)
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    conf = torch.zeros((19, 19), dtype=torch.int64, device="cuda")

    def call(n=N, h=H, w=W, labels=lab_d, ws_bytes=need, xin=x):
        return L.ssal_icnet_evaluate_nhwc(handle, _lib.dev_ptr(xin), 0, n, h, w, _lib.dev_ptr(labels), _lib.dev_ptr(mask_d),
                                          _lib.dev_ptr(conf), _lib.dev_ptr(ws), ws_bytes, _lib.stream_ptr())

    assert call(ws_bytes=need - 1) == _lib.SSAL_ENOMEM
    assert call(ws_bytes=L.ssal_icnet_workspace_bytes(handle, N, H, W)) == _lib.SSAL_ENOMEM  # the score call's size
    assert call(labels=None) == _lib.SSAL_EINVAL
    assert call(xin=None) == _lib.SSAL_EINVAL
    assert call(h=H + 8) == _lib.SSAL_EINVAL
    assert call(n=0) == _lib.SSAL_EINVAL
    assert L.ssal_icnet_evaluate_nhwc(None, _lib.dev_ptr(x), 0, N, H, W, _lib.dev_ptr(lab_d), None, _lib.dev_ptr(conf),
                                      _lib.dev_ptr(ws), need, _lib.stream_ptr()) == _lib.SSAL_EINVAL
    odd = torch.zeros((N * H * W + 4,), dtype=torch.uint8, device="cuda")[1:1 + N * H * W]  # not 4-byte aligned
    assert call(labels=odd) == _lib.SSAL_EINVAL
    torch.cuda.synchronize()
    assert int(conf.sum()) == 0, "a refused call must not have counted anything"
    assert call() == _lib.SSAL_OK
    assert torch.equal(conf, net._evaluate_composed(x, lab_d, mask_d))
    # a handle that was never committed
    h2 = ctypes.c_void_p()
    assert L.ssal_icnet_create(3, 19, ctypes.byref(h2)) == _lib.SSAL_OK
    try:
        assert L.ssal_icnet_eval_workspace_bytes(h2, N, H, W) == -1
        assert L.ssal_icnet_evaluate_nhwc(h2, _lib.dev_ptr(x), 0, N, H, W, _lib.dev_ptr(lab_d), None, _lib.dev_ptr(conf),
                                          _lib.dev_ptr(ws), need, _lib.stream_ptr()) == _lib.SSAL_ESTATE
    finally:
        L.ssal_icnet_destroy(h2)


def test_active_learning_evaluate_goes_through_the_fused_entry(nets, monkeypatch):
    """the loop's validation pass (with its all_reduce_confusion) counts through ICNet.evaluate, never the label plane"""
    from semanticsegmentationactivelearning_amd import active_learning as al
    from semanticsegmentationactivelearning_amd.tensortools import metrics as M
    net = nets[19]
    batches, want = [], torch.zeros((19, 19), dtype=torch.int64, device="cuda")
    for i in range(2):
        x = syn.synth_frames_device(20 + 2 * i, N, H, W, 3, dtype=torch.uint8)
        lab, mask = _targets(N, H, W, 19, seed=200 + i)
        mask[N - 1] = 1
        batches.append((x, dev(lab), dev(mask)))
        net._evaluate_composed(x, dev(lab), dev(mask), confusion=want)

    def no_plane(*a, **kw):
        raise AssertionError("the validation pass wrote a label plane")

    monkeypatch.setattr(net, "score", no_plane)
    got = al.evaluate(net, iter(batches), 19, prefetch=0)
    ref = M.create_metrics(want)
    assert set(got) == set(ref)
    for key in ref:
        np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(ref[key]), err_msg=key)
