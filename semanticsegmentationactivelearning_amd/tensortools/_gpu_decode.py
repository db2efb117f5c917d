"""``InputStage(decode="gpu")``: the batch loop of the GPU PNG decode path.

Per example a worker reads the record, parses its PNG chunks (``png.parse``) and draws the crop / flip / channel scales
from the example's seed exactly as ``InputStage.default_decoder`` does.  The main thread packs a launch of up to
``decode_ahead`` frames -- descriptors, channel scales and compressed payloads -- into one buffer of the page-locked
ring, copies it to the device on a side stream and launches the decoder there (``ssal_png_decode_nhwc``), which writes
the batch planes directly.  Two launches are kept in flight: while the batches of one are consumed, the next one is
parsed, copied and inflated.  Examples the device does not take, and streams whose device status is not ok, are decoded
by the Pillow path (``default_decoder``) and copied into their frame.
"""
import collections
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import png, tfrecord
from .. import _lib

_DESC = 16  # SSAL_PNG_DESC
_ROLE_IMAGE, _ROLE_LABEL = 0, 1
_RING = 3  # page-locked payload buffers: two launches in flight + the one being packed


def _named(err, filename):
    """the exception Pillow (or the decoder) raised, re-raised with the record's name"""
    try:
        return type(err)("%s: %s" % (filename, err))
    except Exception:
        return err


class _Item:
    __slots__ = ("filename", "seed", "example", "streams", "top", "left", "flip", "scale", "out", "has_label", "arrays")


def _fallback(stage, item, augment):
    try:
        return stage.default_decoder(item.example, augment=augment, rng=np.random.default_rng(item.seed))
    except Exception as e:
        raise _named(e, item.filename) from e


def _prepare(stage, filename, augment, seed):
    """worker: read + parse one record; -> _Item with .streams (GPU) or .arrays (decoded by the Pillow path)"""
    it = _Item()
    it.filename, it.seed, it.streams, it.arrays = filename, seed, None, None
    from .input import DEFAULT_FORMAT
    rec = tfrecord.read_tfrecord(filename)
    fmt = dict(DEFAULT_FORMAT)
    for m in stage.modalities:
        fmt["%s/data" % m] = b""
    example = tfrecord.parse_single_example(rec, fmt)
    it.example = example
    plan = _plan(stage, example, augment, seed)
    if plan is None:
        it.arrays = _fallback(stage, it, augment)
        return it
    it.streams, it.top, it.left, it.flip, it.scale, it.out, it.has_label = plan
    return it


def _plan(stage, example, augment, seed):
    """(streams, top, left, flip, scale, (ch, cw, channels), has_label), or None -> Pillow path"""
    img = png.parse(example["image/data"])
    if img is None:
        return None
    h, w = img.height, img.width
    nch = min(3, img.channels)
    streams = [(img, _ROLE_IMAGE, 0, nch)]
    channels = nch
    for m in stage.modalities:
        data = example.get("%s/data" % m, b"")
        s = png.parse(data) if data else None
        if s is None or s.height != h or s.width != w:
            return None  # (a missing modality raises on the Pillow path)
        streams.append((s, _ROLE_IMAGE, channels, s.channels))
        channels += s.channels
    has_label = bool(example["label"])
    if has_label:
        lab = png.parse(example["label"])
        if lab is None or lab.height != h or lab.width != w:
            return None
        streams.append((lab, _ROLE_LABEL, 0, 1))
    else:
        hh = example["height"] if example["height"] > 0 else h
        ww = example["width"] if example["width"] > 0 else w
        if (hh, ww) != (h, w):
            return None
    ch, cw = stage.shape[0], stage.shape[1]
    if ch is None or cw is None:
        ch, cw = h, w
    if h < ch or w < cw:
        return None  # the Pillow path raises the error
    scale = None
    if augment:  # the draws of default_decoder, in its order
        rng = np.random.default_rng(seed)
        top = int(rng.integers(0, h - ch + 1))
        left = int(rng.integers(0, w - cw + 1))
        flip = bool(rng.random() < 0.5)
        scale = rng.uniform(0.8, 1.4, size=channels).astype(np.float32)
    else:
        top, left, flip = h // 2 - ch // 2, w // 2 - cw // 2, False
    return streams, top, left, flip, scale, (ch, cw, channels), has_label


class _Launch:
    """one decoder launch: device planes of ``len(items)`` frames + the event that ends its work"""
    __slots__ = ("items", "planes", "status", "status_host", "done", "keep")


def _launch(stage, items, augment, side):
    import torch
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    first = next((it for it in items if it.streams is not None), None)
    if first is not None:
        ch, cw, channels = first.out
    else:
        a = items[0].arrays[0]
        ch, cw, channels = a.shape
    for it in items:
        shape = it.out if it.streams is not None else it.arrays[0].shape
        if tuple(shape) != (ch, cw, channels):
            raise ValueError("all frames of a batch need the same shape: %s vs %s (%s)"
                             % ((ch, cw, channels), tuple(shape), it.filename))
    F = len(items)
    descs, pieces = [], []
    off = 0
    for f, it in enumerate(items):
        if it.streams is None:
            continue
        for s, role, c0, nc in it.streams:
            descs.append([off, s.nbytes, s.width, s.height, s.channels, 0, f, role, c0, nc, it.top, it.left,
                          int(it.flip), 0, 0, 0])
            pieces.append((off, s.payload))
            off += (s.nbytes + 15) & ~15
    n = len(descs)
    desc = np.asarray(descs, dtype=np.int64).reshape(n, _DESC)
    ws_bytes = int(L.ssal_png_plan(n, desc.ctypes.data_as(ctypes.c_void_p)))
    if ws_bytes < 0:
        raise ValueError("bad PNG geometry in this batch")
    scale = np.ones((F, channels), dtype=np.float32)
    if augment:
        for f, it in enumerate(items):
            if it.streams is not None:
                scale[f] = it.scale
    # one page-locked buffer: descriptors | scales | payloads (256-B aligned sections)
    d_bytes = desc.nbytes
    s_off = (d_bytes + 255) & ~255
    p_off = (s_off + scale.nbytes + 255) & ~255
    total = p_off + off
    host = stage._pin_slot(total, torch.uint8, ring=_RING)[:total]
    hv = host.numpy()
    hv[:d_bytes] = desc.view(np.uint8).reshape(-1)
    hv[s_off:s_off + scale.nbytes] = scale.view(np.uint8).reshape(-1)
    for o, parts in pieces:
        o += p_off
        for p in parts:
            k = len(p)
            hv[o:o + k] = np.frombuffer(p, dtype=np.uint8)
            o += k

    lc = _Launch()
    lc.items = items
    img_dtype = torch.uint8 if stage.image_dtype == np.uint8 else torch.float32
    cur = torch.cuda.current_stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        buf = host.to(dev, non_blocking=True)
        copied = torch.cuda.Event()
        copied.record(side)
        from .input import copy_issued
        copy_issued(host, copied)  # the ring slot is not rewritten before the copy has read it
        image = torch.empty((F, ch, cw, channels), dtype=img_dtype, device=dev)
        dist = torch.empty((F, ch, cw, channels), dtype=torch.float32, device=dev) if augment else None
        label = torch.zeros((F, ch, cw), dtype=torch.uint8, device=dev)  # a record without label: 255 -> 0, mask 0
        mask = torch.zeros((F, ch, cw), dtype=torch.uint8, device=dev)
        status = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
        ws = torch.empty((max(ws_bytes, 1),), dtype=torch.uint8, device=dev)
        vp = ctypes.c_void_p
        _lib.check(L.ssal_png_decode_nhwc(
            vp(buf.data_ptr() + p_off), off, vp(buf.data_ptr()), n, F, ch, cw, channels, vp(buf.data_ptr() + s_off),
            vp(image.data_ptr()), int(img_dtype == torch.float32), vp(dist.data_ptr()) if dist is not None else None,
            vp(label.data_ptr()), vp(mask.data_ptr()), vp(status.data_ptr()), vp(ws.data_ptr()), ws_bytes,
            vp(side.cuda_stream)))
        status_host = torch.empty((max(n, 1),), dtype=torch.int32, pin_memory=True)
        status_host.copy_(status, non_blocking=True)
        done = torch.cuda.Event()
        done.record(side)
    lc.planes = (image, dist, label, mask)
    lc.status, lc.status_host, lc.done = status, status_host, done
    lc.keep = (buf, ws, desc)  # freed when the launch is finished (their memory is stream-ordered on `side`)
    return lc


def _finish(stage, lc, augment):
    """wait for a launch, decode its failed / unsupported examples with Pillow, hand the planes to the current stream"""
    import torch
    lc.done.synchronize()
    st = lc.status_host.numpy()
    image, dist, label, mask = lc.planes
    cur = torch.cuda.current_stream()
    for t in lc.planes:
        if t is not None:
            t.record_stream(cur)
    k = 0
    for f, it in enumerate(lc.items):
        arrays = it.arrays
        if it.streams is not None:
            ok = all(int(st[k + j]) == png.OK for j in range(len(it.streams)))
            k += len(it.streams)
            if ok:
                stage.decode_stats["gpu"] += 1
                continue
            arrays = _fallback(stage, it, augment)
        stage.decode_stats["fallback"] += 1
        outs = (image, dist, label, mask) if augment else (image, label, mask)
        for t, a in zip(outs, arrays):
            t[f].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    lc.keep = None


def batches(stage, files, aux, batch_size, augment, seeds):
    torch = _lib.require_gpu()
    group = max(batch_size, (stage.decode_ahead // batch_size) * batch_size)
    side = torch.cuda.Stream()
    with ThreadPoolExecutor(stage._workers) as pool:
        futures = collections.deque()
        pos = 0

        def submit_until(limit):
            nonlocal pos
            while pos < len(files) and len(futures) < limit:
                futures.append(pool.submit(_prepare, stage, files[pos], augment, int(seeds[pos])))
                pos += 1

        launches = collections.deque()
        start = 0

        def launch_next():
            nonlocal start
            if start >= len(files):
                return
            submit_until(2 * group)
            n = min(group, len(files) - start)
            items = [futures.popleft().result() for _ in range(n)]
            submit_until(2 * group)
            launches.append((start, _launch(stage, items, augment, side)))
            start += n

        launch_next()
        while launches:
            launch_next()  # the next launch is in flight while this one's batches are consumed
            g0, lc = launches.popleft()
            _finish(stage, lc, augment)
            planes = [p for p in lc.planes if p is not None]
            F = len(lc.items)
            for b in range(0, F, batch_size):
                n = min(batch_size, F - b)
                yield tuple(p[b:b + n] for p in planes) + tuple(a[g0 + b:g0 + b + n] for a in aux)
