"""numpy restatement of the fused prediction kernel (``ssal_predict_logits_nhwc``): the C oracle's ``resize_bilinear``
(TF-1.13 legacy mapping, fp32 lerp without contraction), the first maximum over the classes, an optional table.  Shared by
tests/test_predict_cpu.py and tests/test_gpu_predict.py."""
import numpy as np

from oracle import icnet_oracle as ico

SIZES = [(3, 4), (5, 7), (10, 14), (11, 13), (1, 1), (1, 9), (23, 37)]  # the sizes the GPU test resizes [2,5,7,K] to
SEED, IN_SHAPE, ORACLE_K = 1234, (2, 5, 7), (2, 4, 19, 32)              # the CPU-oracle case of the GPU test
MARGIN, SURE_SHARE = 1e-4, 0.99  # the rule of test_gpu_parity.py::test_inference_path_labels_embedding_and_png


def id_table():
    """256-entry id table, distinct values for the 32 possible train ids"""
    return ((np.arange(256) * 7 + 3) % 251).astype(np.uint8)


def colour_table():
    """[256, 3] colour table, distinct rows for the 32 possible train ids"""
    i = np.arange(256)
    return np.stack([(i * 5 + 1) % 256, (i * 11 + 2) % 256, 255 - i], axis=1).astype(np.uint8)


def logits(k, seed=SEED, shape=IN_SHAPE):
    return np.random.default_rng(seed + k).standard_normal(shape + (k,)).astype(np.float32)


def resized(x, size):
    return ico.resize_bilinear(x, int(size[0]), int(size[1]))


def predict(x, size, lut=None):
    """uint8 [N,OH,OW] or, through a [256,3] table, [N,OH,OW,3]; np.argmax takes the first maximum"""
    label = resized(x, size).argmax(-1).astype(np.uint8)
    return label if lut is None else np.asarray(lut, np.uint8)[label]


def sure_pixels(x, size, margin=MARGIN):
    """(labels, mask of the pixels whose top-two margin of the oracle's resized logits exceeds ``margin``)"""
    r = resized(x, size)
    srt = np.sort(r, -1)
    return r.argmax(-1).astype(np.uint8), (srt[..., -1] - srt[..., -2]) > margin


def predict_literal(x, size):
    """the mapping as include/ssal_enet.h states it, one output pixel at a time in np.float32 scalars"""
    f = np.float32
    n, h, w, k = x.shape
    oh, ow = size
    hs, ws = f(h) / f(oh), f(w) / f(ow)
    out = np.zeros((n, oh, ow), np.uint8)
    for i in range(n):
        for oy in range(oh):
            fy = f(oy) * hs
            y0 = int(np.floor(fy)); y1 = min(y0 + 1, h - 1); ly = f(fy - f(y0))
            for ox in range(ow):
                fx = f(ox) * ws
                x0 = int(np.floor(fx)); x1 = min(x0 + 1, w - 1); lx = f(fx - f(x0))
                best, lab = None, 0
                for c in range(k):
                    tl, tr, bl, br = x[i, y0, x0, c], x[i, y0, x1, c], x[i, y1, x0, c], x[i, y1, x1, c]
                    top = f(tl + f(f(tr - tl) * lx))
                    bot = f(bl + f(f(br - bl) * lx))
                    v = f(top + f(f(bot - top) * ly))
                    if best is None or v > best:
                        best, lab = v, c
                out[i, oy, ox] = lab
    return out
