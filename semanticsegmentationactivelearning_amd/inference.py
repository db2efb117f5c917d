"""Test-split inference: host-side mirror of the reference's ``inference.py:61-153`` on the MI355X path.

logits = net(image, training=False) -> optional ``tf.image.resize_bilinear(logits, size)`` (the
reference resizes the LOGITS, :96-99; TF-1.13 legacy mapping) -> argmax (first maximum) -> reverse
embedding trainId -> dataset id (:101-106) or colour map (:107-109) -> PNG (:110-119).
Dataset tables (``embedding_reversed``, ``colormap``) are passed in by the caller (the reference's
``datasets`` package is out of scope).

Two routes give the same bytes: the composed one (``predict_labels`` + ``reverse_embedding`` / ``colorize``: one
stand-alone operator per step, the logits in HBM between them) and the fused one (``predict``: resize, argmax and table in
one kernel, or the fused score kernel's label plane where there is no resize).
"""
import os

import numpy as np

from . import _lib
from . import active_learning as al


def resize_bilinear(x, size):
    """tf.image.resize_bilinear(x, size) with TF-1.13 defaults (align_corners=False, src = dst*in/out)."""
    torch = _lib.require_gpu()
    x = _lib.as_device_f32(x)
    n, h, w, c = x.shape
    oh, ow = int(size[0]), int(size[1])
    y = torch.empty((n, oh, ow, c), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().ssal_resize_bilinear(_lib.dev_ptr(x), n, h, w, c, oh, ow, _lib.dev_ptr(y),
                                                   _lib.stream_ptr()))
    return y


def predict_labels(net, images, size=None):
    """uint8 train-id map [N,H',W'] on the GPU (reference :95-99: argmax of the (resized) logits)"""
    logits = net(images, training=False)
    if size is not None:
        logits = resize_bilinear(logits, size)
    _, extra = al.score_logits(logits, "confidence", return_label=True)
    return extra["label"]


def reverse_embedding(pred, embedding_reversed):
    """trainId -> dataset id through a 256-entry table (reference :101-106, tf.gather_nd)"""
    torch = _lib.require_gpu()
    lut = torch.as_tensor(np.asarray(embedding_reversed, dtype=np.uint8), device=pred.device)
    return lut[pred.long()]


def colorize(pred, colormap):
    """trainId -> RGB through a [256,3] table (reference :107-109)"""
    torch = _lib.require_gpu()
    lut = torch.as_tensor(np.asarray(colormap, dtype=np.uint8), device=pred.device)
    return lut[pred.long()]


def _table(values, classes, channels, name):
    """a dataset table as the kernels take it: uint8 [256] (channels 1) or [256, 3], zero-padded on the host"""
    t = np.asarray(values, dtype=np.uint8)
    if t.ndim != (1 if channels == 1 else 2) or (channels == 3 and t.shape[1] != 3) or t.shape[0] > 256:
        raise ValueError("%s must be a table of at most 256 %s (got shape %s)"
                         % (name, "ids" if channels == 1 else "RGB rows", t.shape))
    if t.shape[0] < classes:
        raise ValueError("%s has %d entries, fewer than the network's %d classes" % (name, t.shape[0], classes))
    full = np.zeros((256,) + t.shape[1:], np.uint8)
    full[:t.shape[0]] = t
    return full


def predict(net, images, size=None, embedding_reversed=None, colormap=None, arithmetic="f32"):
    """What ``run_inference`` writes for one batch, on the GPU: uint8 [N,OH,OW] (train ids, or dataset ids through
    ``embedding_reversed``) or [N,OH,OW,3] (``colormap``).  With ``size`` the logits are resized, reduced to their first
    maximum and mapped in one kernel (``ssal_predict_logits_nhwc``; the resized logits never reach HBM); without it the label
    plane comes from the network's fused score kernel (no logits in HBM at all) and ``ssal_label_lut`` applies the table.
    The bytes are those of ``predict_labels`` + ``reverse_embedding`` / ``colorize``.  ``arithmetic``: as ``ENet.__call__`` / ``ICNet.__call__``."""
    if embedding_reversed is not None and colormap is not None:
        raise ValueError("give embedding_reversed or colormap, not both")
    _lib.arithmetic_code(arithmetic)
    channels = 3 if colormap is not None else 1 if embedding_reversed is not None else 0
    table = None
    if channels:
        table = _table(colormap if channels == 3 else embedding_reversed, net.classes, channels,
                       "colormap" if channels == 3 else "embedding_reversed")
    torch = _lib.require_gpu()
    L = _lib.lib()
    if size is None:
        _, extra = net.score(images, "confidence", return_label=True, arithmetic=arithmetic)
        label = extra["label"]
        if not channels:
            return label
        src, (n, oh, ow) = label, label.shape
    else:
        src = net(images, training=False, arithmetic=arithmetic)
        n, h, w, k = src.shape
        oh, ow = int(size[0]), int(size[1])
    lut = torch.from_numpy(table).to(src.device) if channels else None
    out = torch.empty((n, oh, ow, 3) if channels == 3 else (n, oh, ow), dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        if size is None:
            _lib.check(L.ssal_label_lut(_lib.dev_ptr(src), n * oh * ow, _lib.dev_ptr(lut), channels, _lib.dev_ptr(out),
                                        _lib.stream_ptr()))
        else:
            _lib.check(L.ssal_predict_logits_nhwc(_lib.dev_ptr(src), n, h, w, k, oh, ow, _lib.dev_ptr(lut), channels,
                                                  _lib.dev_ptr(out), _lib.stream_ptr()))
    return out


def write_png(path, array):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(array)).save(path, format="PNG")


def run_inference(net, batches, output_dir, embedding_reversed=None, colormap=None, size=None, fused=False):
    """``batches`` yields (images NHWC float32, file ids); writes ``<output_dir>/<id>.png`` per example
    (reference :110-147) and returns the list of written paths.  ``fused=True`` takes ``predict`` (a colour map wins over
    an id table, as on the composed route) and downloads each batch into one page-locked buffer kept across batches."""
    os.makedirs(output_dir, exist_ok=True)
    written = []
    pinned = None
    for images, ids in batches:
        if fused:
            dev_out = predict(net, images, size, None if colormap is not None else embedding_reversed, colormap)
            if pinned is None or pinned.numel() < dev_out.numel():
                pinned = _lib.require_gpu().empty(dev_out.numel(), dtype=dev_out.dtype).pin_memory()
            host = pinned[:dev_out.numel()].view(dev_out.shape)
            host.copy_(dev_out)  # synchronous: the PNG writer below reads the buffer, the next batch overwrites it
            out = host.numpy()
        else:
            pred = predict_labels(net, images, size)
            if colormap is not None:
                out = colorize(pred, colormap)
            elif embedding_reversed is not None:
                out = reverse_embedding(pred, embedding_reversed)
            else:
                out = pred
            out = out.cpu().numpy()
        for k, fid in enumerate(ids):
            fid = fid.decode() if isinstance(fid, bytes) else str(fid)
            path = os.path.join(output_dir.rstrip("/"), fid + ".png")
            write_png(path, out[k])
            written.append(path)
    return written


def region_boxes(selected, region, size):
    """Pixel boxes of selected regions for the annotation tool: ``selected`` [k, 3] rows ``(example id, ry, rx)`` as
    ``active_learning.select_regions`` / ``rank_regions`` return them, ``region`` an int or ``(rh, rw)``, ``size`` the
    frame's ``(h, w)``.  Returns int64 [k, 4] rows ``(y0, x0, y1, x1)`` (end-exclusive), clipped to the frame; a region
    outside the frame's grid raises ValueError."""
    rh, rw = _lib.region_size(region)
    h, w = int(size[0]), int(size[1])
    if rh <= 0 or rw <= 0 or h <= 0 or w <= 0:
        raise ValueError("region and size must be positive (got region=%r size=%r)" % (region, size))
    sel = np.asarray(selected, dtype=np.int64).reshape(-1, 3)
    y0, x0 = sel[:, 1] * rh, sel[:, 2] * rw
    if len(sel) and (sel[:, 1:].min() < 0 or y0.max() >= h or x0.max() >= w):
        raise ValueError("a selected region lies outside the %d x %d grid of a %d x %d frame" % (-(-h // rh), -(-w // rw), h, w))
    return np.stack([y0, x0, np.minimum(y0 + rh, h), np.minimum(x0 + rw, w)], axis=1).astype(np.int64).reshape(-1, 4)
