"""Mirror of the reference's ``tensortools/metrics.py``: the masked confusion matrix of a validation / test pass and
the metrics derived from it.

``confusion_mat`` (reference :226-257) counts on the device through the HIP op ``ssal_confusion_matrix``; the fused
form, where the network's argmax never leaves the Final kernel, is ``models.ENet.evaluate``.  ``create_metrics``
(reference ``Metrics._create_metrics``, :155-224) is a K x K computation and runs on the host in float64.  ``Metrics``
keeps the reference's accumulate / reset semantics (:8-27, :65-78) without a TensorFlow graph.
"""
import numpy as np

from .. import _lib


def confusion_mat(labels, predictions, num_classes, weights=None, out=None):
    """``bincount(num_classes * labels + predictions, weights, minlength = maxlength = K * K)`` as an int64 [K, K]
    device tensor (row = label, column = prediction).  ``labels`` / ``predictions`` / ``weights``: uint8-valued tensors
    of one shape (any layout; flattened).  A pixel adds its weight (the mask value); keys >= K * K (label 255, any
    label >= K) are dropped.  ``out``: an int64 [K, K] device tensor to ADD into (the reference's ``assign_add``);
    a new zeroed one otherwise."""
    torch = _lib.require_gpu()
    k = int(num_classes)
    if not 2 <= k <= 32:
        raise ValueError("num_classes must be in [2, 32] (got %d)" % k)
    pred = _as_u8(predictions, None, "predictions")
    dev = pred.device
    lab = _as_u8(labels, dev, "labels")
    wts = _as_u8(weights, dev, "weights") if weights is not None else None
    if lab.numel() != pred.numel() or (wts is not None and wts.numel() != pred.numel()):
        raise ValueError("labels, predictions and weights must have the same number of elements")
    if out is None:
        out = torch.zeros((k, k), dtype=torch.int64, device=dev)
    elif out.dtype != torch.int64 or tuple(out.shape) != (k, k) or out.device != dev or not out.is_contiguous():
        raise ValueError("out must be a contiguous int64 [%d, %d] tensor on %s" % (k, k, dev))
    L = _lib.lib()
    with torch.cuda.device(dev):
        ws = torch.empty(int(L.ssal_confusion_workspace_bytes(k)), dtype=torch.uint8, device=dev)
        _lib.check(L.ssal_confusion_matrix(_lib.dev_ptr(pred), _lib.dev_ptr(lab), _lib.dev_ptr(wts), pred.numel(), k,
                                           _lib.dev_ptr(out), _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr()))
    return out


def _as_u8(x, device, name):
    """a contiguous uint8 device tensor of ``x`` (values outside [0, 255] are not representable: the reference's labels
    and masks are uint8 planes)"""
    torch = _lib.require_gpu()
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.dtype != torch.uint8:
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            t = t.to(torch.uint8)
        else:
            if t.numel() and (int(t.min()) < 0 or int(t.max()) > 255):
                raise ValueError("%s must hold values in [0, 255]" % name)
            t = t.to(torch.uint8)
    if device is None:
        device = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return t.to(device).contiguous()


def create_metrics(confusion):
    """Reference ``Metrics._create_metrics`` (:155-224) on an int [K, K] confusion matrix (numpy or tensor), in float64
    numpy.  Keeps the reference's conventions: denominators ``max(., 1)`` for precision / recall / IoU, ``MeanIoU``
    averaged over ALL K classes (absent ones count 0), accuracies divided by the total count (NaN for an empty
    matrix, as TensorFlow's truediv gives)."""
    if hasattr(confusion, "detach"):
        confusion = confusion.detach().cpu().numpy()
    cm = np.asarray(confusion, dtype=np.int64)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1]:
        raise ValueError("confusion must be a square matrix (got shape %s)" % (cm.shape,))
    samples_tot = cm.sum()
    tp = np.diag(cm).copy()
    off = cm - np.diag(tp)
    fp = off.sum(axis=0)
    fn = off.sum(axis=1)
    tp_fp = tp + fp
    tp_fp_fn = tp_fp + fn
    tn = samples_tot - tp_fp_fn
    with np.errstate(divide="ignore", invalid="ignore"):
        tot = np.float64(samples_tot)
        class_accuracy = (tp + tn) / tot
        pix_accuracy = np.float64(tp.sum()) / tot
    class_miou = tp / np.maximum(tp_fp_fn, 1).astype(np.float64)
    return {
        "TruePositive": tp,
        "TrueNegative": tn,
        "FalsePositive": fp,
        "FalseNegative": fn,
        "ClassAccuracy": class_accuracy,
        "ClassPrecission": tp / np.maximum(tp_fp, 1).astype(np.float64),
        "ClassRecall": tp / np.maximum(tp + fn, 1).astype(np.float64),
        "ClassMeanIoU": class_miou,
        "PixelAccuracy": pix_accuracy,
        "MeanIoU": class_miou.mean(),
        "ConfusionMat": cm,
    }


class Metrics:
    """Reference ``tensortools.metrics.Metrics`` (:4-27): an int64 K x K confusion accumulator.
    ``update(predictions, labels, mask)`` counts one batch on the device (the reference's update op), ``add(confusion)``
    adds a matrix counted elsewhere (``ENet.evaluate``'s fused result), ``reset()`` zeroes the accumulator (the
    reference's ``reset_metrics``).  ``metrics`` derives from the accumulated matrix, ``batch_metrics`` from the last
    update / add.  The accumulator lives on the device of the first matrix added (no GPU is needed for ``add``)."""

    def __init__(self, num_classes):
        self.nclasses = int(num_classes)
        self._confusion = None
        self._batch = None

    def update(self, predictions, labels, mask=None):
        """count one batch on the device; returns its confusion matrix"""
        return self.add(confusion_mat(labels, predictions, self.nclasses, weights=mask))

    def add(self, confusion):
        """accumulate an integer [K, K] confusion matrix (tensor or array); returns it as int64"""
        import torch
        c = confusion if isinstance(confusion, torch.Tensor) else torch.as_tensor(np.asarray(confusion))
        if tuple(c.shape) != (self.nclasses, self.nclasses):
            raise ValueError("confusion must be [%d, %d] (got %s)" % (self.nclasses, self.nclasses, tuple(c.shape)))
        if c.dtype.is_floating_point:
            raise ValueError("confusion must hold integer counts")
        if self._confusion is None:
            self._confusion = torch.zeros((self.nclasses, self.nclasses), dtype=torch.int64, device=c.device)
        c = c.to(device=self._confusion.device, dtype=torch.int64)
        self._confusion += c
        self._batch = c
        return c

    def reset(self):
        """zero the accumulator (and forget the last batch)"""
        self._confusion = None
        self._batch = None

    @property
    def confusion(self):
        """the accumulated int64 [K, K] matrix as numpy (zeros before the first update)"""
        if self._confusion is None:
            return np.zeros((self.nclasses, self.nclasses), dtype=np.int64)
        return self._confusion.cpu().numpy()

    @property
    def metrics(self):
        return create_metrics(self.confusion)

    @property
    def batch_metrics(self):
        if self._batch is None:
            return create_metrics(np.zeros((self.nclasses, self.nclasses), dtype=np.int64))
        return create_metrics(self._batch)
