"""Pool scoring and ranking: host-side mirror of the scoring slice of the reference's
``active_learning.py`` (EPSILON :39-40, score ops :229-269, ``rank_confidence`` :682-715,
its caller :776-784).

The per-pixel work (ENet forward, softmax, entropy / margin / confidence, float64 mean) runs in the
HIP kernels behind ``models.ENet.score``; this module keeps the host control flow of the
reference: scatter batch results by example index into a float32 vector, filter the unlabelled
examples, ``np.argpartition`` the ``selection_size`` lowest.  The MI355X addition is pool
sharding: every rank (one process per GPU) scores a strided shard of the pool and ONE RCCL
all-gather of ``(index, score)`` pairs over xGMI per ranking pass rebuilds the full vector on every
rank -- the reference itself is single-process.
"""
import numpy as np

from . import _lib

# Lowest representable (normal) float32 -- reference active_learning.py:39-40
EPSILON = np.finfo(np.float32).tiny

MEASURES = tuple(_lib.MEASURES)  # ("entropy", "margin", "confidence")


class ScoringConfig:
    """The JSON keys the scoring path reads (conf/default_params.json:2,32-35,53-59)."""

    def __init__(self, measure="entropy", selection_size=50, threshold=0.95, batch_size=8,
                 height=None, width=None):
        if measure not in _lib.MEASURES:
            raise NotImplementedError("Uncertainty function not implemented.")
        self.measure = measure
        self.selection_size = int(selection_size)
        self.threshold = float(threshold)
        self.batch_size = int(batch_size)
        self.height = height
        self.width = width

    @classmethod
    def from_params(cls, params):
        al = params["active_learning"]
        net_in = params.get("network", {}).get("input", {})
        return cls(measure=al["measure"], selection_size=al["selection_size"],
                   threshold=al["threshold"], batch_size=params["batch_size"],
                   height=net_in.get("height"), width=net_in.get("width"))


def score_logits(logits, measure="entropy", threshold=0.0, return_label=False, return_mask=False,
                 return_confidence=False, region=None):
    """softmax -> {entropy, margin, confidence} -> float64 mean over (H, W) on materialised logits
    (reference :239-263): ``pseudo_mean_confidence`` [N] float64, plus optionally ``pseudo_label``
    (uint8 argmax, :234-236), ``pseudo_mask`` (conf < threshold -> 0 else 1, :265-269) and the
    per-pixel ``pseudo_confidence``.  Raises NotImplementedError for an unknown measure (:259-260).

    ``region`` (an int or ``(rh, rw)``, any size >= 1) adds the region scores [N, RY, RX] float64 as the second return
    value: ``(scores, region_scores[, maps])`` (``ssal_score_logits_regions_nhwc``; the per-image scores keep their bits)."""
    if measure not in _lib.MEASURES:
        raise NotImplementedError("Uncertainty function not implemented.")
    torch = _lib.require_gpu()
    x = _lib.as_device_f32(logits)
    if x.dim() != 4:
        raise ValueError("logits must be [N,H,W,classes]")
    n, h, w, k = x.shape
    L = _lib.lib()
    if region is not None:
        rh, rw = _lib.region_size(region)
        ry, rx = _lib.region_grid(h, w, (rh, rw))
        with torch.cuda.device(x.device):
            ws = torch.empty(int(L.ssal_score_regions_workspace_bytes(n, h, w)), dtype=torch.uint8, device=x.device)
            scores = torch.empty((n,), dtype=torch.float64, device=x.device)
            regions = torch.empty((n, ry, rx), dtype=torch.float64, device=x.device)
            label = torch.empty((n, h, w), dtype=torch.uint8, device=x.device) if return_label else None
            mask = torch.empty((n, h, w), dtype=torch.uint8, device=x.device) if return_mask else None
            conf = torch.empty((n, h, w), dtype=torch.float32, device=x.device) if return_confidence else None
            _lib.check(L.ssal_score_logits_regions_nhwc(
                _lib.dev_ptr(x), n, h, w, k, _lib.MEASURES[measure], float(threshold), rh, rw,
                _lib.dev_ptr(scores), _lib.dev_ptr(regions), _lib.dev_ptr(label), _lib.dev_ptr(mask), _lib.dev_ptr(conf),
                _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr()))
        if return_label or return_mask or return_confidence:
            return scores, regions, {"label": label, "mask": mask, "confidence": conf}
        return scores, regions
    with torch.cuda.device(x.device):
        nbytes = L.ssal_score_workspace_bytes(n, h, w)
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=x.device)
        scores = torch.empty((n,), dtype=torch.float64, device=x.device)
        label = torch.empty((n, h, w), dtype=torch.uint8, device=x.device) if return_label else None
        mask = torch.empty((n, h, w), dtype=torch.uint8, device=x.device) if return_mask else None
        conf = torch.empty((n, h, w), dtype=torch.float32, device=x.device) if return_confidence else None
        _lib.check(L.ssal_score_logits_nhwc(
            _lib.dev_ptr(x), n, h, w, k, _lib.MEASURES[measure], float(threshold),
            _lib.dev_ptr(scores), _lib.dev_ptr(label), _lib.dev_ptr(mask), _lib.dev_ptr(conf),
            _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr()))
    if return_label or return_mask or return_confidence:
        return scores, {"label": label, "mask": mask, "confidence": conf}
    return scores


def select_lowest(unlabelled_confidence, selection_size):
    """``np.argpartition(conf, k)[:k]`` -- the k lowest-confidence positions as an unordered set
    (reference :707-712).  The reference raises when ``selection_size == len(unlabelled)`` (kth out
    of bounds, a known defect); here that case returns every position."""
    conf = np.asarray(unlabelled_confidence)
    k = int(np.minimum(len(conf), selection_size))
    if k <= 0:
        return np.zeros((0,), dtype=np.int64)
    if k >= len(conf):
        return np.arange(len(conf), dtype=np.int64)
    return np.argpartition(conf, k)[:k].astype(np.int64)


def shard_positions(num_examples, rank, world_size):
    """Strided shard of pool positions for one rank; every rank gets the same count after padding
    with -1 sentinels (2975 = 8*371 + 7 -> 372 per rank)."""
    per = (num_examples + world_size - 1) // world_size
    pos = np.arange(rank, num_examples, world_size, dtype=np.int64)
    pad = np.full((per - len(pos),), -1, dtype=np.int64)
    return np.concatenate([pos, pad])


def all_gather_scores(local_index, local_score, group=None):
    """ONE all-gather (RCCL over xGMI for GPU tensors, gloo for CPU tensors) of each rank's
    ``(index int64, score float64)`` shard; returns the concatenation (sentinel index -1 kept)."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return local_index, local_score
    return _gather_pairs(local_index, local_score, group)


def _gather_pairs(local_index, local_score, group=None):
    """the collective itself (also what the single-rank RCCL smoke test drives): pack the index next to the score in a
    float64 pair -> [per, 2], one ``all_gather_into_tensor``.  ``local_score`` may carry trailing dimensions (the region
    pass: [per, RY, RX]); a row is then the index followed by the flattened scores -> [per, 1 + RY * RX], still one
    collective, and the scores come back in their shape."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    tail = tuple(local_score.shape[1:])
    packed = torch.cat([local_index.to(torch.float64).reshape(-1, 1),
                        local_score.to(torch.float64).reshape(local_index.numel(), -1)], dim=1).contiguous()
    home = packed.device
    if packed.is_cuda and dist.get_backend(group) == "gloo":
        packed = packed.cpu()  # rehearsals of the multi-rank path on one GPU run over gloo: collectives on CPU tensors
    gathered = torch.empty((world * packed.shape[0], packed.shape[1]), dtype=torch.float64, device=packed.device)
    dist.all_gather_into_tensor(gathered, packed, group=group)
    gathered = gathered.to(home)
    return gathered[:, 0].to(torch.int64), gathered[:, 1:].reshape((gathered.shape[0],) + tail)


def prefetch_to_device(batches, depth=2):
    """Host batches -> device batches, copied ``depth`` batches ahead on a side HIP stream, so that the
    host-to-device copy of batch i+1 overlaps the kernels of batch i (the reference gets
    the same effect from ``tf.data`` prefetching, ``tensortools/input.py:195``).  ``batches`` yields
    ``(images, example_indices)`` with images as numpy / CPU-torch arrays (uint8 frames or float32) or tensors
    already on the GPU (passed through)."""
    import collections
    torch = _lib.require_gpu()
    copy_stream = torch.cuda.Stream()
    queue = collections.deque()

    def stage(item):
        images, indices = item
        if isinstance(images, torch.Tensor) and images.is_cuda:
            return images, indices, None, None
        host = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
        host = host.contiguous()
        # The copy runs on the side stream, i.e. NOT behind the kernels of the batches already enqueued on the
        # compute stream.  Pinned sources are copied asynchronously; pageable ones block the host for the copy
        # (the runtime stages them through its own pinned buffers) while the GPU keeps computing.  Pinning
        # per batch here would cost more than it saves (page-locking 50-200 MB takes milliseconds).
        with torch.cuda.stream(copy_stream):
            dev = host.cuda(non_blocking=True)
            done = torch.cuda.Event()
            done.record(copy_stream)
        # page-locked ring slot of a tensortools.input.InputStage (found by the address of the batch's memory, so
        # sliced / re-wrapped batches resolve too): the stage does not rewrite it before `done`
        from .tensortools import input as _input
        _input.copy_issued(host, done)
        return dev, indices, done, host  # the host buffer must outlive the copy

    def release(entry):
        dev, indices, done, _pinned = entry
        if done is not None:
            cur = torch.cuda.current_stream()
            cur.wait_event(done)
            dev.record_stream(cur)  # allocated on the copy stream, consumed on this one
        return dev, indices

    for item in batches:
        queue.append(stage(item))
        if len(queue) > depth:
            yield release(queue.popleft())
    while queue:
        yield release(queue.popleft())


def pad_to_length(index, score, length):
    """Local (collective-free) padding of one rank's ``(index, score)`` shard to ``length`` entries with the
    ``(-1, +inf)`` sentinel.  ``shard_positions`` gives every rank ``ceil(num_examples / world)`` positions, so
    a rank that scored its whole shard pads to exactly that length without asking the others.  ``score`` may carry
    trailing dimensions (region scores [len, RY, RX]); the sentinel rows are +inf throughout."""
    import torch
    pad = int(length) - index.numel()
    if pad < 0:
        raise ValueError("shard has %d entries, more than the per-rank length %d" % (index.numel(), length))
    if pad > 0:
        index = torch.cat([index, torch.full((pad,), -1, dtype=torch.int64, device=index.device)])
        score = torch.cat([score, torch.full((pad,) + tuple(score.shape[1:]), float("inf"), dtype=torch.float64,
                                             device=score.device)])
    return index, score


def _check_arithmetic(net_call, arithmetic):
    """ValueError, before any GPU work, for an unknown mode or a non-default one the model's call does not take in these
    loops (ICNet: ``evaluate`` / ``score_regions`` take no ``arithmetic`` argument, and ``ICNet.score``'s opt-in mode is offered
    on direct calls and ``inference.predict`` only -- ``ICNet.loop_arithmetics``)"""
    import inspect
    _lib.arithmetic_code(arithmetic)
    offered = getattr(net_call.__self__, "loop_arithmetics", None)
    if arithmetic != "f32" and ("arithmetic" not in inspect.signature(net_call).parameters
                                or (offered is not None and arithmetic not in offered)):
        raise ValueError("arithmetic=%r: %s has no such mode (only 'f32')" % (arithmetic, type(net_call.__self__).__name__))


def rank_confidence(net, batches, num_examples, unlabelled, selection_size, measure="entropy",
                    group=None, prefetch=0, ragged=False, arithmetic="f32"):
    """Mirror of ``rank_confidence()`` (reference :682-715).

    ``batches`` yields ``(images NHWC float32 or uint8, example_indices)``; on a multi-GPU job each rank
    passes only its own shard (``shard_positions``).  ``prefetch`` > 0 copies host batches that many batches
    ahead on a side stream (``prefetch_to_device``).  Returns ``(low_conf_examples, unlabelled_confidence)``:
    the ids (into the full example list) of the ``selection_size`` least confident unlabelled examples and
    the float32 confidence of every unlabelled example (the reference feeds it to a histogram summary,
    :781-784).

    ``arithmetic`` is handed to ``net.score`` ("f32": exact fp32, the default; "bf16x3": ENet's opt-in split-operand mode).

    Collectives per ranking pass: exactly ONE all-gather of ``(index, score)`` pairs.  Shards handed out by
    ``shard_positions`` hold at most ``ceil(num_examples / world)`` examples, so each rank pads locally to that
    length (+ one flag entry).  A rank whose shard is longer raises ``ValueError`` -- on EVERY rank, after the
    collective, so nobody is left blocking in it.  ``ragged=True`` is for callers that split the pool some other way
    (shard lengths unknown to the other ranks): it costs one extra all-reduce(MAX) to agree on the length."""
    _check_arithmetic(net.score, arithmetic)
    torch = _lib.require_gpu()
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        _lib.warn_if_few_hw_queues()  # caller + 2 chains + prefetch copy + RCCL = 5 streams (once per process)
    idx_chunks, score_chunks = [], []
    if prefetch > 0:
        batches = prefetch_to_device(batches, depth=prefetch)
    for images, indices in batches:
        # [n] float64 on device, stream-ordered; arithmetic: "f32" (the reference's, default) or ENet's opt-in "bf16x3"
        s = net.score(images, measure=measure) if arithmetic == "f32" else net.score(images, measure=measure, arithmetic=arithmetic)
        score_chunks.append(s)
        idx_chunks.append(torch.as_tensor(np.asarray(indices, dtype=np.int64), device=s.device))
    if score_chunks:
        local_score = torch.cat(score_chunks)
        local_index = torch.cat(idx_chunks)
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
        local_score = torch.zeros((0,), dtype=torch.float64, device=dev)
        local_index = torch.zeros((0,), dtype=torch.int64, device=dev)
    return merge_and_rank(local_index, local_score, num_examples, unlabelled, selection_size, group, ragged)


def evaluate(net, batches, num_classes, group=None, prefetch=2, arithmetic="f32"):
    """The validation / test pass of the reference loop (active_learning.py:277-282 ``val_net`` + ``val_pred``, the
    ``Metrics`` update :390-427, read back at :616-630 and :655-680): ``batches`` yields ``(image, label, mask, ...)``
    as ``InputStage``'s evaluation path produces them (centre crop, ``generate_mask``); extra items are ignored.  Each
    batch is counted on the device by ``net.evaluate`` (ENet: fused into the Final kernel; ICNet: into the up-sampling
    kernel) into one int64 K x K accumulator; host batches are copied ``prefetch`` batches ahead on a side stream
    (``prefetch_to_device``).  With a process group (every rank evaluates its own shard) the K x K matrices are summed
    with exactly ONE all-reduce.  Returns ``tensortools.metrics.create_metrics`` of the total (``MeanIoU`` decides the
    reference's early stopping)."""
    from .tensortools import metrics as _metrics
    _check_arithmetic(net.evaluate, arithmetic)
    torch = _lib.require_gpu()
    k = int(num_classes)
    confusion = torch.zeros((k, k), dtype=torch.int64, device=torch.device("cuda", torch.cuda.current_device()))
    items = ((b[0], tuple(b[1:3])) for b in batches)  # (images, (label, mask)): prefetch copies the images only
    if prefetch > 0:
        items = prefetch_to_device(items, depth=prefetch)
    for images, (label, mask) in items:
        if arithmetic == "f32":
            net.evaluate(images, label, mask, confusion=confusion)
        else:
            net.evaluate(images, label, mask, confusion=confusion, arithmetic=arithmetic)
    return _metrics.create_metrics(all_reduce_confusion(confusion, group))


def all_reduce_confusion(confusion, group=None):
    """ONE all-reduce(SUM) of an int64 K x K confusion matrix over the process group (RCCL for GPU tensors; gloo runs
    it on a CPU copy); the matrix itself when no group of more than one rank is up.  Integer sums: every rank ends with
    the same matrix bit for bit."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return confusion
    home = confusion.device
    t = confusion.contiguous()
    if t.is_cuda and dist.get_backend(group) == "gloo":
        t = t.cpu()
    elif t.data_ptr() == confusion.data_ptr():
        t = t.clone()
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t.to(home)


def merge_and_rank(local_index, local_score, num_examples, unlabelled, selection_size, group=None, ragged=False):
    """the collective + host tail of a ranking pass (shared by ``rank_confidence`` and ``bench.py``)"""
    all_index, all_score = _merge_shards(local_index, local_score, num_examples, group, ragged)
    return finish_ranking(all_index, all_score, num_examples, unlabelled, selection_size)


def _merge_shards(local_index, local_score, num_examples, group=None, ragged=False):
    """the collective of a ranking pass: every rank's ``(index, score)`` rows on every rank, as numpy (sentinel rows
    kept).  ``local_score`` is [len] (image scores) or [len, RY, RX] (region scores)."""
    import torch.distributed as dist
    world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
    overflow = False
    if world > 1:
        if ragged:
            local_index, local_score = _pad_to_common_length(local_index, local_score, group)
        else:
            # precondition: len(shard) <= ceil(num_examples / world) (what shard_positions hands out).  A rank that
            # violates it must not raise BEFORE the collective (the others would block in the all-gather until the
            # backend times out): it contributes an all-sentinel shard of the agreed length whose extra last entry
            # carries the flag (index -1, score -inf; +inf = fine), and EVERY rank raises after the collective.
            per = (num_examples + world - 1) // world
            overflow = local_index.numel() > per
            if overflow:
                local_index, local_score = local_index[:0], local_score[:0]
            local_index, local_score = pad_to_length(local_index, local_score, per + 1)
            if overflow:
                local_score = local_score.clone()
                local_score[-1] = float("-inf")
    all_index, all_score = all_gather_scores(local_index, local_score, group)
    all_index, all_score = all_index.cpu().numpy(), all_score.cpu().numpy()
    if world > 1 and not ragged:
        bad = np.nonzero((all_index < 0) & np.isneginf(all_score.reshape(len(all_index), -1)[:, 0]))[0]
        if len(bad):
            raise ValueError("rank(s) %s handed merge_and_rank a shard longer than ceil(num_examples / world) = %d "
                             "entries; split the pool with shard_positions() or pass ragged=True"
                             % (sorted(set((bad // (per + 1)).tolist())), per))
    return all_index, all_score


def _pad_to_common_length(index, score, group):
    """Ragged callers only: all_gather_into_tensor needs equal shard lengths, and nobody knows the longest
    one, so agree on it with one all-reduce(MAX), then pad with the (-1, +inf) sentinel."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return index, score
    on_cpu = index.is_cuda and dist.get_backend(group) == "gloo"
    n = torch.tensor([index.numel()], dtype=torch.int64, device="cpu" if on_cpu else index.device)
    dist.all_reduce(n, op=dist.ReduceOp.MAX, group=group)
    return pad_to_length(index, score, int(n.item()))


def finish_ranking(all_index, all_score, num_examples, unlabelled, selection_size):
    """Host tail of rank_confidence (reference :685,700,705-715): scatter into a float32 vector by
    example index (the float64 -> float32 rounding happens here, like ``confidence[batch_indices] =
    batch_confidence``), filter the unlabelled subset, pick the lowest ``selection_size``."""
    confidence = np.zeros(num_examples, dtype=np.float32)
    valid = all_index >= 0
    confidence[all_index[valid]] = all_score[valid]
    unlabelled = np.asarray(unlabelled, dtype=np.int64)
    unlabelled_confidence = confidence[unlabelled]
    example_indices = select_lowest(unlabelled_confidence, selection_size)
    low_conf_examples = unlabelled[example_indices]
    return low_conf_examples, unlabelled_confidence


# ---- region-level acquisition ------------------------------------------------------------------------------------------
def select_regions(region_confidence, examples, selection_size, max_per_image=None, annotated=None):
    """The ``selection_size`` least confident regions of a pool (host, numpy).

    ``region_confidence`` [E, RY, RX] float32 (rounded from the float64 region scores the way ``finish_ranking`` rounds
    image scores); ``examples`` [E] the example id of every row; ``annotated`` an optional bool array of the same shape:
    those regions are never selected.  Regions are taken in the TOTAL order (score ascending, example id, ry, rx), so every
    tie has one answer and every rank picks the same rows; with ``max_per_image = m`` the walk skips the regions of an
    example that already has ``m`` selected.  Returns int64 [k, 3] rows ``(example id, ry, rx)`` in selection order,
    ``k = min(selection_size, candidates)``."""
    conf = np.asarray(region_confidence, dtype=np.float32)
    if conf.ndim != 3:
        raise ValueError("region_confidence must be [E, RY, RX] (got shape %s)" % (conf.shape,))
    e = conf.shape[0]
    examples = np.asarray(examples, dtype=np.int64).reshape(-1)
    if len(examples) != e:
        raise ValueError("examples has %d entries for %d rows of region_confidence" % (len(examples), e))
    if max_per_image is not None and int(max_per_image) < 1:
        raise ValueError("max_per_image must be >= 1 or None (got %r)" % (max_per_image,))
    free = np.ones(conf.shape, dtype=bool)
    if annotated is not None:
        annotated = np.asarray(annotated, dtype=bool)
        if annotated.shape != conf.shape:
            raise ValueError("annotated must have shape %s (got %s)" % (conf.shape, annotated.shape))
        free = ~annotated
    row, yy, xx = np.nonzero(free)
    order = np.lexsort((xx, yy, examples[row], conf[row, yy, xx]))  # lexsort: the LAST key is the primary one
    row, yy, xx = row[order], yy[order], xx[order]
    want = max(0, int(selection_size))
    if max_per_image is None:
        keep = np.arange(min(want, len(row)))
    else:
        # position of every candidate among the candidates of its own example id, in walk order: a capped walk takes a
        # candidate iff fewer than m of its example's candidates came before it
        ex = examples[row]
        by_ex = np.argsort(ex, kind="stable")
        sorted_ex = ex[by_ex]
        first = np.searchsorted(sorted_ex, sorted_ex, side="left")
        before = np.empty(len(row), dtype=np.int64)
        before[by_ex] = np.arange(len(row)) - first
        keep = np.nonzero(before < int(max_per_image))[0][:want]
    return np.stack([examples[row[keep]], yy[keep], xx[keep]], axis=1).astype(np.int64).reshape(-1, 3)


def finish_region_ranking(all_index, all_region_score, num_examples, unlabelled, selection_size, max_per_image=None,
                          annotated=None):
    """Host tail of ``rank_regions``, the region twin of ``finish_ranking``: scatter the gathered rows into a float32
    [num_examples, RY, RX] array by example index (the float64 -> float32 rounding happens here), keep the unlabelled
    examples, ``select_regions``.  ``annotated`` is aligned with ``unlabelled``: [len(unlabelled), RY, RX]."""
    all_region_score = np.asarray(all_region_score)
    confidence = np.zeros((num_examples,) + all_region_score.shape[1:], dtype=np.float32)
    valid = all_index >= 0
    confidence[all_index[valid]] = all_region_score[valid]
    unlabelled = np.asarray(unlabelled, dtype=np.int64)
    region_confidence = confidence[unlabelled]
    selected = select_regions(region_confidence, unlabelled, selection_size, max_per_image, annotated)
    return selected, region_confidence


def merge_and_rank_regions(local_index, local_region_score, num_examples, unlabelled, selection_size, max_per_image=None,
                           annotated=None, group=None, ragged=False):
    """the collective + host tail of a region ranking pass: ``merge_and_rank`` with ``(index, RY * RX scores)`` rows --
    the same ONE all-gather, the same behaviour on a too-long shard"""
    all_index, all_score = _merge_shards(local_index, local_region_score, num_examples, group, ragged)
    return finish_region_ranking(all_index, all_score, num_examples, unlabelled, selection_size, max_per_image, annotated)


def rank_regions(net, batches, num_examples, unlabelled, selection_size, region=(128, 128), measure="entropy",
                 max_per_image=None, annotated=None, group=None, prefetch=0, ragged=False, arithmetic="f32"):
    """The region twin of ``rank_confidence``: which WINDOWS of the pool's frames is the network least sure about.

    ``batches``, ``num_examples``, ``unlabelled``, ``group``, ``prefetch``, ``ragged`` and ``arithmetic`` as in
    ``rank_confidence`` (the same strided shards, the same ``prefetch_to_device``); every batch goes through
    ``net.score_regions(images, region, measure)``.  ``annotated`` (optional bool [len(unlabelled), RY, RX]) marks regions
    that already have labels; ``max_per_image`` caps the regions taken from one frame (``select_regions``).  Returns
    ``(selected [k, 3] int64 rows (example id, ry, rx) in selection order, region_confidence [len(unlabelled), RY, RX]
    float32)``.

    Collectives per pass: exactly ONE all-gather, of ``(index, RY * RX scores)`` rows; a rank whose shard is longer than
    ``ceil(num_examples / world)`` makes EVERY rank raise ``ValueError`` after the collective (``ragged=True``: one extra
    all-reduce(MAX) instead).  Every frame of the pool must have the same size (one region grid), and every rank scores at
    least one batch (the grid comes from the frames) unless ``annotated`` states it."""
    _check_arithmetic(net.score_regions, arithmetic)
    torch = _lib.require_gpu()
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        _lib.warn_if_few_hw_queues()  # caller + 2 chains + prefetch copy + RCCL = 5 streams (once per process)
    rh, rw = _lib.region_size(region)
    idx_chunks, score_chunks = [], []
    if prefetch > 0:
        batches = prefetch_to_device(batches, depth=prefetch)
    for images, indices in batches:
        if arithmetic == "f32":
            _, r = net.score_regions(images, region=(rh, rw), measure=measure)
        else:
            _, r = net.score_regions(images, region=(rh, rw), measure=measure, arithmetic=arithmetic)
        if score_chunks and tuple(r.shape[1:]) != tuple(score_chunks[0].shape[1:]):
            raise ValueError("every frame of a region ranking pass must have the same size: region grid %s after %s"
                             % (tuple(r.shape[1:]), tuple(score_chunks[0].shape[1:])))
        score_chunks.append(r)  # [n, RY, RX] float64 on device, stream-ordered
        idx_chunks.append(torch.as_tensor(np.asarray(indices, dtype=np.int64), device=r.device))
    if score_chunks:
        local_score = torch.cat(score_chunks)
        local_index = torch.cat(idx_chunks)
    else:
        if annotated is None:
            raise ValueError("rank_regions got no batch on this rank and no `annotated` array to take the region grid from")
        dev = torch.device("cuda", torch.cuda.current_device())
        local_score = torch.zeros((0,) + tuple(np.shape(annotated)[1:]), dtype=torch.float64, device=dev)
        local_index = torch.zeros((0,), dtype=torch.int64, device=dev)
    return merge_and_rank_regions(local_index, local_score, num_examples, unlabelled, selection_size, max_per_image,
                                  annotated, group, ragged)


def training_targets(labelled, labels, mask, pseudo_label, pseudo_mask):
    """The training batch's targets (active_learning.py:272-275): per image, the annotation where the example is
    labelled and the pseudo annotation (``score(return_label=True, return_mask=True)``) where it is not --
    ``tf.where(train_labelled, train_label, pseudo_label)`` and the same for the mask.

    ``labelled`` [N] bool; ``labels`` / ``mask`` / ``pseudo_label`` / ``pseudo_mask`` [N, H, W] (numpy arrays or torch
    tensors, all of one kind).  The pseudo planes are cast to the dtype of the annotation, as the reference builds them
    (:265-269).  Returns ``(label, mask)``."""
    try:
        import torch
        is_torch = isinstance(labels, torch.Tensor)
    except ImportError:  # pragma: no cover
        is_torch = False
    if is_torch:
        sel = torch.as_tensor(labelled, dtype=torch.bool, device=labels.device)
        if sel.dim() != 1 or sel.shape[0] != labels.shape[0]:
            raise ValueError("labelled must be a [N] vector (N = %d)" % labels.shape[0])
        for name, t in (("mask", mask), ("pseudo_label", pseudo_label), ("pseudo_mask", pseudo_mask)):
            if tuple(t.shape) != tuple(labels.shape):
                raise ValueError("%s must have shape %s (got %s)" % (name, tuple(labels.shape), tuple(t.shape)))
        sel = sel.view((-1,) + (1,) * (labels.dim() - 1))
        return (torch.where(sel, labels, pseudo_label.to(device=labels.device, dtype=labels.dtype)),
                torch.where(sel, mask, pseudo_mask.to(device=mask.device, dtype=mask.dtype)))
    labels, mask = np.asarray(labels), np.asarray(mask)
    sel = np.asarray(labelled, dtype=bool)
    if sel.ndim != 1 or sel.shape[0] != labels.shape[0]:
        raise ValueError("labelled must be a [N] vector (N = %d)" % labels.shape[0])
    for name, t in (("mask", mask), ("pseudo_label", pseudo_label), ("pseudo_mask", pseudo_mask)):
        if np.shape(t) != labels.shape:
            raise ValueError("%s must have shape %s (got %s)" % (name, labels.shape, np.shape(t)))
    sel = sel.reshape((-1,) + (1,) * (labels.ndim - 1))
    return (np.where(sel, labels, np.asarray(pseudo_label).astype(labels.dtype)),
            np.where(sel, mask, np.asarray(pseudo_mask).astype(mask.dtype)))
