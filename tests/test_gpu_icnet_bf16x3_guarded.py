"""The three entry points of ICNet's opt-in bf16x3 mode on poisoned workspaces and guarded outputs (tests/guarded_alloc.py;
DESIGN.md "Poisoned workspaces"): ssal_icnet_forward_nhwc_arith, ssal_icnet_score_nhwc_arith and ssal_conv_bn_act_arith under the
three byte patterns -- nothing outside an output's interior is written, nothing is read from the workspace before it is
written (the results do not depend on the pattern), and the results are those of a clean run."""
import numpy as np
import pytest
import torch

import semanticsegmentationactivelearning_amd as ssal
from helpers import frames
from semanticsegmentationactivelearning_amd import _lib, synthetic as syn
from semanticsegmentationactivelearning_amd.models.util import conv_ops as cops
from test_gpu_guarded import guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    _lib.lib()
    yield
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def icnet19():
    net = ssal.ICNet(19)
    net.build((None, None, None, 3))
    syn.randomize_icnet(net, seed=0)
    return net


def test_forward_arith_guarded(icnet19):
    x = frames([3, 4], 64, 96, 3)

    def body(put):
        put.fresh()
        return {"logits": icnet19(put(x), arithmetic="bf16x3")}

    got = guarded(body, nets=(icnet19,), clean=True, tag="icnet forward bf16x3")
    assert got["logits"].shape == (2, 64, 96, 19) and np.isfinite(got["logits"]).all()


@pytest.mark.parametrize("u8", [False, True], ids=["float", "u8"])
def test_score_arith_guarded(icnet19, u8):
    x = frames([5, 6, 7], 32, 64, 3)
    if u8:
        x = np.clip(np.rint(x * 255), 0, 255).astype(np.uint8)

    def body(put):
        put.fresh()
        s, e = icnet19.score(put(x), "margin", return_label=True, return_mask=True, return_confidence=True, arithmetic="bf16x3")
        return {"scores": s, "label": e["label"], "mask": e["mask"], "confidence": e["confidence"]}

    got = guarded(body, nets=(icnet19,), clean=True, tag="icnet score bf16x3")
    assert got["scores"].shape == (3,) and np.isfinite(got["scores"]).all()


@pytest.mark.parametrize("n,h,w,cin,cout,k,stride,dil,res", [
    (1, 9, 15, 64, 19, 3, 1, 2, True),     # a 7-row tail and 13 dead columns: the stores the predicates must drop
    (2, 5, 7, 96, 160, 1, 2, 1, False),    # five column tiles, stride 2 on an odd map
])
def test_conv_bn_act_arith_guarded(n, h, w, cin, cout, k, stride, dil, res):
    rng = np.random.default_rng(n + h + cin + cout)
    x = rng.normal(size=(n, h, w, cin)).astype(np.float32)
    kern = (rng.normal(size=(k, k, cin, cout)) / np.sqrt(k * k * cin)).astype(np.float32)
    bias = rng.normal(size=cout).astype(np.float32)
    r = rng.normal(size=(n, -(-h // stride), -(-w // stride), cout)).astype(np.float32) if res else None

    def body(put):
        return {"y": cops.conv_bn_act(put(x), kern, stride, dil, bias=bias, residual=None if r is None else put(r), relu=True,
                                      arithmetic="bf16x3")}

    got = guarded(body, clean=True, tag="conv_bn_act bf16x3")
    assert got["y"].shape == (n, -(-h // stride), -(-w // stride), cout)
