"""ENet model: host-side mirror of the reference's ``models.ENet`` (models/enet/enet.py:6-407).

``ENet(classes, ...)(inputs_NHWC_f32, training=False) -> logits [N,H,W,classes]`` keeps the
reference operator API (constructor kwargs, sub-layer attribute names, weight names/layouts,
``.layers[i].variables[j]``, ``.Final.kernel``, ``.endpoint_outputs``).  The forward pass runs the
hand-written HIP kernels of libssal_hip.so through the C ABI on the current HIP stream; tensors
are torch tensors resident on the MI355X.  ``score()`` is the fused pool-scoring entry
(forward + softmax + acquisition measure + fp64 per-image mean; logits never reach HBM).
"""
import ctypes

from ... import _lib
from . import enet_modules as mod


class ENet(_lib.DeviceState):
    """https://arxiv.org/pdf/1606.02147.pdf"""

    def __init__(self, classes,
                 kernel_initializer=None,
                 alpha_initializer=None,
                 weight_regularization=None,
                 regularization_scaling=False,
                 drop_rates=[0.01, 0.1, 0.1, 0.1, 0.1],
                 name="ENet"):
        if len(drop_rates) != 5:
            raise ValueError("Illegal argument value @drop_rates, length must be 5.")
        self.classes = classes
        self.name = name
        self.built = False
        kernel_initializer = kernel_initializer or mod.glorot_uniform()
        alpha_initializer = alpha_initializer or mod.constant(0.25)
        kw = dict(kernel_initializer=kernel_initializer, alpha_initializer=alpha_initializer,
                  kernel_regularizer=weight_regularization,
                  regularization_scaling=regularization_scaling)

        # reference models/enet/enet.py:35-247
        self.Initial = mod.Initial(16, name="Initial", **kw)
        # Stage 1
        self.Bottleneck1_0 = mod.BottleneckDownsample(64, name="Bottleneck1_0", drop_rate=drop_rates[0], **kw)
        for i in range(1, 5):
            setattr(self, "Bottleneck1_%d" % i,
                    mod.Bottleneck(64, name="Bottleneck1_%d" % i, drop_rate=drop_rates[0], **kw))
        # Stage 2 / 3
        self.Bottleneck2_0 = mod.BottleneckDownsample(128, name="Bottleneck2_0", drop_rate=drop_rates[1], **kw)
        variants = {1: {}, 2: dict(dilation_rate=(2, 2)), 3: dict(asymmetric=True, kernel_size=(5, 5)),
                    4: dict(dilation_rate=(4, 4)), 5: {}, 6: dict(dilation_rate=(8, 8)),
                    7: dict(asymmetric=True, kernel_size=(5, 5)), 8: dict(dilation_rate=(16, 16))}
        for stage, rate in ((2, drop_rates[1]), (3, drop_rates[2])):
            for i in range(1, 9):
                nm = "Bottleneck%d_%d" % (stage, i)
                setattr(self, nm, mod.Bottleneck(128, name=nm, drop_rate=rate, **variants[i], **kw))
        # Stage 4
        self.Bottleneck4_0 = mod.BottleneckUpsample(64, name="Bottleneck4_0", drop_rate=drop_rates[3], **kw)
        self.Bottleneck4_1 = mod.Bottleneck(64, name="Bottleneck4_1", drop_rate=drop_rates[3], **kw)
        self.Bottleneck4_2 = mod.Bottleneck(64, name="Bottleneck4_2", drop_rate=drop_rates[3], **kw)
        # Stage 5
        self.Bottleneck5_0 = mod.BottleneckUpsample(16, name="Bottleneck5_0", drop_rate=drop_rates[4], **kw)
        self.Bottleneck5_1 = mod.Bottleneck(16, name="Bottleneck5_1", drop_rate=drop_rates[4], **kw)
        # Final UpConv
        self.Final = mod.Final(self.classes, kernel_initializer=kernel_initializer,
                               kernel_regularizer=weight_regularization,
                               regularization_scaling=regularization_scaling)

        self._layer_names = (["Initial", "Bottleneck1_0"] + ["Bottleneck1_%d" % i for i in range(1, 5)]
                             + ["Bottleneck2_0"] + ["Bottleneck2_%d" % i for i in range(1, 9)]
                             + ["Bottleneck3_%d" % i for i in range(1, 9)]
                             + ["Bottleneck4_0", "Bottleneck4_1", "Bottleneck4_2",
                                "Bottleneck5_0", "Bottleneck5_1", "Final"])
        for nm in self._layer_names:
            getattr(self, nm)._owner = self
        self._c_in = None
        self._init_device_state()  # per-device handles, per-(device, stream) workspaces (_lib.DeviceState)
        self._endpoints = []
        self.outputs = []

    # ---- keras-like surface ----------------------------------------------------------------
    @property
    def layers(self):
        return [getattr(self, nm) for nm in self._layer_names]

    @property
    def variables(self):
        return [v for l in self.layers for v in l.variables]

    weights = variables

    def assign_named(self, named, strict=False):
        """Name-keyed weight copy: ``named`` maps variable names to arrays.  Names are matched on
        ``<Layer>/<weight path>`` -- a leading model scope (``ENet/``) and a trailing ``:0`` as in
        ``{v.name: sess.run(v) for v in tf_net.variables}`` are ignored.  Unknown names raise KeyError;
        with ``strict`` every variable of the model must be present.  Returns the number assigned."""
        mine = {v.name: v for v in self.variables}
        seen = set()
        for name, value in named.items():
            key = name[:-2] if name.endswith(":0") else name
            while key not in mine and "/" in key:
                key = key.split("/", 1)[1]
            if key not in mine:
                raise KeyError("no variable of %s matches '%s'" % (self.name, name))
            mine[key].assign(value)
            seen.add(key)
        if strict and len(seen) != len(mine):
            raise KeyError("missing variables: %s" % sorted(set(mine) - seen)[:5])
        return len(seen)

    def build(self, input_shape):
        """Create all weights for an NHWC input shape (reference build :249-309 + lazy layer builds)."""
        if self.built:
            return
        c = int(input_shape[-1])
        self._c_in = c
        for nm in self._layer_names:
            layer = getattr(self, nm)
            layer.build((None, None, None, c))
            c = layer.output_shape(1, 8, 8)[-1]
        self.built = True

    @property
    def endpoint_outputs(self):
        """[[final, bottleneck5_1, bottleneck4_2, bottleneck3_8]] of the most recent call (the reference
        keeps one entry per graph build, :311-318; eager calls would pile up device memory).  The three
        intermediate tensors are views into the device workspace and are overwritten by the next call."""
        return list(self._endpoints)

    # ---- device handle ---------------------------------------------------------------------
    def _create_handle(self, L):
        h = ctypes.c_void_p()
        _lib.check(L.ssal_enet_create(self._c_in, self.classes, ctypes.byref(h)))
        return h

    def _push_tensors(self, L, handle):
        for nm in self._layer_names:
            for attr, var in getattr(self, nm).abi_tensors().items():
                arr = var.numpy()
                _lib.check(L.ssal_enet_set_tensor(
                    handle, ("%s.%s" % (nm, attr)).encode(),
                    arr.ctypes.data_as(ctypes.c_void_p), arr.size))
        _lib.check(L.ssal_enet_commit(handle, _lib.stream_ptr()))

    def _destroy_handle(self, L, handle):
        L.ssal_enet_destroy(handle)

    def __del__(self):
        self._release_device_state()

    def _prepare(self, inputs, training):
        if training:
            raise NotImplementedError(
                "training=True (spatial dropout + batch statistics) is outside the MI355X "
                "scoring path; call with training=False")
        x = _lib.as_device_image(inputs)  # float32 in [0,1] (the reference's tensor) or the uint8 decoded frame
        if x.dim() != 4:
            raise ValueError("inputs must be NHWC rank-4 (got shape %s)" % (tuple(x.shape),))
        if not self.built:
            self.build(tuple(x.shape))
        if x.shape[-1] != self._c_in:
            raise ValueError("model was built for %d input channels, got %d" % (self._c_in, x.shape[-1]))
        return x

    # ---- forward: ENet.call (reference :320-407) -------------------------------------------
    def __call__(self, inputs, training, arithmetic="f32"):
        """``arithmetic``: "f32" (default; exact fp32, bit-identical to the parity oracle -- the reference's arithmetic) or
        the OPT-IN "bf16x3" (include/ssal_enet.h SSAL_ARITH_BF16X3: split-operand bf16 MFMAs in the 128-channel
        bottlenecks; logits within ~1e-5, pooling indices bit-identical, not bit-identical logits)."""
        arith = _lib.arithmetic_code(arithmetic)
        if training:
            raise NotImplementedError(
                "training=True (spatial dropout + batch statistics) is outside the MI355X "
                "scoring path; call with training=False")
        torch = _lib.require_gpu()
        x = self._prepare(inputs, training)
        n, h, w, _ = x.shape
        L = _lib.lib()
        with torch.cuda.device(x.device):
            handle = self._sync_handle()
            nbytes = L.ssal_enet_workspace_bytes(handle, n, h, w)
            if nbytes < 0:
                raise ValueError("bad input dims %s" % (tuple(x.shape),))
            ws = self._workspace(nbytes, x.device)
            logits = torch.empty((n, h, w, self.classes), dtype=torch.float32, device=x.device)
            if arith:
                _lib.check(L.ssal_enet_forward_nhwc_arith(handle, _lib.dev_ptr(x), int(x.dtype == torch.uint8), n, h, w, arith,
                                                          _lib.dev_ptr(logits), _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr()))
            else:
                fwd = L.ssal_enet_forward_nhwc_u8 if x.dtype == torch.uint8 else L.ssal_enet_forward_nhwc
                _lib.check(fwd(handle, _lib.dev_ptr(x), n, h, w, _lib.dev_ptr(logits),
                               _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr()))
            self._note_call(ws, (n, h, w), "forward")
            self._record_endpoints(handle, logits, ws, n, h, w)
        # The reference appends one symbolic tensor per graph build (enet.py:405); this implementation is
        # eager, so retaining every call's logits would grow device memory without bound (1.27 GB per batch
        # of 8 at 1024x2048x19): only the most recent call is kept.
        self.outputs = [logits]
        return logits

    call = __call__

    def _record_endpoints(self, handle, final, ws, n, h, w):
        torch = _lib.require_gpu()
        offs = (ctypes.c_int64 * 3)()
        _lib.check(_lib.lib().ssal_enet_endpoint_offsets(handle, n, h, w, offs))
        shapes = [(n, h // 2, w // 2, 16), (n, h // 4, w // 4, 64), (n, h // 8, w // 8, 128)]
        views = []
        for off, shp in zip(offs, shapes):
            cnt = shp[0] * shp[1] * shp[2] * shp[3]
            views.append(ws[off:off + 4 * cnt].view(torch.float32).view(shp))
        # the views alias one workspace that the next call overwrites: only the latest entry is meaningful
        self._endpoints = [[final] + views]

    def pooling_argmax(self):
        """(argmax1 [n,h/4,w/4,16], argmax2 [n,h/8,w/8,64]) int64 of the most recent ``__call__`` / ``score``:
        the indices ``ENet.call`` passes from the downsampling to the upsampling blocks (reference
        enet.py:331,338,359,364), in the reference's per-image form ``(y*W + x)*C + c``."""
        torch = _lib.require_gpu()
        if self._last_dims is None:
            raise RuntimeError("no forward pass has run yet")
        n, h, w = self._last_dims
        ws = self._ws
        out = []
        with torch.cuda.device(ws.device):
            for which, (div, c) in ((1, (4, 16)), (2, (8, 64))):
                a = torch.empty((n, h // div, w // div, c), dtype=torch.int64, device=ws.device)
                _lib.check(_lib.lib().ssal_enet_export_argmax(self._handle, _lib.dev_ptr(ws), ws.numel(), n, h, w,
                                                              which, _lib.dev_ptr(a), _lib.stream_ptr()))
                out.append(a)
        return tuple(out)

    # ---- fused pool scoring (active_learning.py:229-263) -----------------------------------
    def score(self, inputs, measure="entropy", threshold=0.0, return_label=False,
              return_mask=False, return_confidence=False, out=None, arithmetic="f32"):
        """forward(training=False) + softmax + acquisition measure + float64 per-image mean.

        Returns scores [N] float64 (device tensor); optionally a dict with the per-pixel
        pseudo label (uint8), pseudo mask (uint8, conf >= threshold) and confidence (fp32).
        ``arithmetic="bf16x3"`` is the opt-in split-operand mode (see ``__call__``): per-pixel confidences within
        north_star's 1e-4 of the exact path, per-image scores within 1e-6, the same top-k on the bench pool
        (tests/test_gpu_bf16x3.py); the default "f32" is the reference's arithmetic."""
        if measure not in _lib.MEASURES:
            raise NotImplementedError("Uncertainty function not implemented.")
        arith = _lib.arithmetic_code(arithmetic)
        torch = _lib.require_gpu()
        x = self._prepare(inputs, False)
        n, h, w, _ = x.shape
        L = _lib.lib()
        with torch.cuda.device(x.device):
            handle = self._sync_handle()
            nbytes = L.ssal_enet_workspace_bytes(handle, n, h, w)
            if nbytes < 0:
                raise ValueError("bad input dims %s" % (tuple(x.shape),))
            ws = self._workspace(nbytes, x.device)
            scores = out if out is not None else torch.empty((n,), dtype=torch.float64, device=x.device)
            label = torch.empty((n, h, w), dtype=torch.uint8, device=x.device) if return_label else None
            mask = torch.empty((n, h, w), dtype=torch.uint8, device=x.device) if return_mask else None
            conf = torch.empty((n, h, w), dtype=torch.float32, device=x.device) if return_confidence else None
            if arith:
                _lib.check(L.ssal_enet_score_nhwc_arith(
                    handle, _lib.dev_ptr(x), int(x.dtype == torch.uint8), n, h, w, _lib.MEASURES[measure], float(threshold),
                    arith, _lib.dev_ptr(scores, torch.float64, "scores"), _lib.dev_ptr(label), _lib.dev_ptr(mask),
                    _lib.dev_ptr(conf), _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr()))
            else:
                score = L.ssal_enet_score_nhwc_u8 if x.dtype == torch.uint8 else L.ssal_enet_score_nhwc
                _lib.check(score(
                    handle, _lib.dev_ptr(x), n, h, w, _lib.MEASURES[measure], float(threshold),
                    _lib.dev_ptr(scores, torch.float64, "scores"), _lib.dev_ptr(label), _lib.dev_ptr(mask),
                    _lib.dev_ptr(conf), _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr()))
            self._note_call(ws, (n, h, w), "score")
        if return_label or return_mask or return_confidence:
            return scores, {"label": label, "mask": mask, "confidence": conf}
        return scores

    # ---- region-level acquisition: per-image scores + per-region scores in one pass -------------------------------------
    def score_regions(self, inputs, region=(128, 128), measure="entropy", threshold=0.0, return_label=False,
                      return_mask=False, return_confidence=False, arithmetic="f32"):
        """``score`` plus the mean confidence of every ``region`` (an int or ``(rh, rw)`` output pixels; grid anchored at
        pixel (0, 0), bottom / right regions clipped by the frame).

        Returns ``(scores [N] float64, region_scores [N, RY, RX] float64)`` on the device, plus the dict of per-pixel maps
        when one was requested.  ``scores`` has the bits ``score`` gives.  A region size that is a multiple of 32 in both
        directions takes the fused route: the Final kernel's 32 x 32 tile sums, which the pass computes anyway, are folded
        into regions by one small launch (``ssal_enet_score_regions_nhwc_arith``; nothing per-pixel reaches HBM unless a
        map was requested).  Any other size goes through the per-pixel confidence plane and ``ssal_region_means_plane``."""
        if measure not in _lib.MEASURES:
            raise NotImplementedError("Uncertainty function not implemented.")
        arith = _lib.arithmetic_code(arithmetic)
        rh, rw = _lib.region_size(region)
        want_maps = return_label or return_mask or return_confidence
        if rh <= 0 or rw <= 0 or (rh % _lib.REGION_TILE == 0 and rw % _lib.REGION_TILE == 0):
            torch = _lib.require_gpu()
            x = self._prepare(inputs, False)
            n, h, w, _ = x.shape
            ry, rx = _lib.region_grid(h, w, (rh, rw))  # ValueError for a size <= 0
            L = _lib.lib()
            with torch.cuda.device(x.device):
                handle = self._sync_handle()
                nbytes = L.ssal_enet_workspace_bytes(handle, n, h, w)
                if nbytes < 0:
                    raise ValueError("bad input dims %s" % (tuple(x.shape),))
                ws = self._workspace(nbytes, x.device)
                scores = torch.empty((n,), dtype=torch.float64, device=x.device)
                regions = torch.empty((n, ry, rx), dtype=torch.float64, device=x.device)
                label = torch.empty((n, h, w), dtype=torch.uint8, device=x.device) if return_label else None
                mask = torch.empty((n, h, w), dtype=torch.uint8, device=x.device) if return_mask else None
                conf = torch.empty((n, h, w), dtype=torch.float32, device=x.device) if return_confidence else None
                _lib.check(L.ssal_enet_score_regions_nhwc_arith(
                    handle, _lib.dev_ptr(x), int(x.dtype == torch.uint8), n, h, w, _lib.MEASURES[measure], float(threshold),
                    arith, rh, rw, _lib.dev_ptr(scores), _lib.dev_ptr(regions), _lib.dev_ptr(label), _lib.dev_ptr(mask),
                    _lib.dev_ptr(conf), _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr()))
                self._note_call(ws, (n, h, w), "score")
            maps = {"label": label, "mask": mask, "confidence": conf}
        else:
            scores, maps = self.score(inputs, measure=measure, threshold=threshold, return_label=return_label,
                                      return_mask=return_mask, return_confidence=True, arithmetic=arithmetic)
            regions = _lib.region_means_plane(maps["confidence"], (rh, rw))
            if not return_confidence:
                maps["confidence"] = None
        return (scores, regions, maps) if want_maps else (scores, regions)

    # ---- fused validation pass (active_learning.py:277-282 + tensortools.metrics.Metrics :390-427) ----------------------
    def evaluate(self, inputs, labels, mask=None, confusion=None, arithmetic="f32"):
        """forward(training=False) + argmax + masked confusion matrix in one pass: the logits and the predicted labels
        never reach HBM (the Final kernel counts them, ``ssal_enet_evaluate_nhwc_arith``).

        ``inputs`` as ``score`` accepts (float32 or decoded uint8 NHWC); ``labels`` / ``mask`` [N, H, W] uint8-valued
        (``mask`` None = weight 1; a mask value is the pixel's weight, as in the reference's bincount).  Returns an
        int64 [K, K] device tensor (row = label, column = prediction); with ``confusion`` given (int64 [K, K] on the
        input's device) the batch is ADDED into it and it is returned.  Keys >= K * K (label 255) are dropped."""
        from ...tensortools import metrics as _metrics
        arith = _lib.arithmetic_code(arithmetic)
        torch = _lib.require_gpu()
        x = self._prepare(inputs, False)
        n, h, w, _ = x.shape
        lab = _metrics._as_u8(labels, x.device, "labels")
        msk = _metrics._as_u8(mask, x.device, "mask") if mask is not None else None
        for name, t in (("labels", lab), ("mask", msk)):
            if t is not None and tuple(t.shape) != (n, h, w):
                raise ValueError("%s must have shape %s (got %s)" % (name, (n, h, w), tuple(t.shape)))
        k = self.classes
        if confusion is None:
            confusion = torch.zeros((k, k), dtype=torch.int64, device=x.device)
        elif (confusion.dtype != torch.int64 or tuple(confusion.shape) != (k, k) or confusion.device != x.device
              or not confusion.is_contiguous()):
            raise ValueError("confusion must be a contiguous int64 [%d, %d] tensor on %s" % (k, k, x.device))
        L = _lib.lib()
        with torch.cuda.device(x.device):
            handle = self._sync_handle()
            nbytes = L.ssal_enet_eval_workspace_bytes(handle, n, h, w)
            if nbytes < 0:
                raise ValueError("bad input dims %s" % (tuple(x.shape),))
            ws = self._workspace(nbytes, x.device)
            _lib.check(L.ssal_enet_evaluate_nhwc_arith(
                handle, _lib.dev_ptr(x), int(x.dtype == torch.uint8), n, h, w, arith, _lib.dev_ptr(lab), _lib.dev_ptr(msk),
                _lib.dev_ptr(confusion), _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr()))
            self._note_call(ws, (n, h, w), "score")
        return confusion

    # ---- single layer (Layer.__call__) -----------------------------------------------------
    def _run_layer(self, layer, x, argmax_in, want_argmax, arithmetic="f32"):
        torch = _lib.require_gpu()
        if not self.built:
            raise RuntimeError("build the model (call it once, or .build(input_shape)) before "
                               "running single layers")
        n, h, w, _ = x.shape
        L = _lib.lib()
        with torch.cuda.device(x.device):
            handle = self._sync_handle()
            name = layer.name.encode()
            nbytes = L.ssal_enet_layer_workspace_bytes(handle, name, n, h, w)
            ws = self._workspace(max(nbytes, 1024), x.device)
            self._note_call(ws, None, "layer")  # the single-layer call re-carves the workspace
            y = torch.empty(layer.output_shape(n, h, w), dtype=torch.float32, device=x.device)
            amax_out = None
            if want_argmax:
                amax_out = torch.empty((n, h // 2, w // 2, x.shape[-1]), dtype=torch.int64, device=x.device)
            amax_in = None
            if argmax_in is not None:
                amax_in = argmax_in if isinstance(argmax_in, torch.Tensor) else torch.as_tensor(argmax_in)
                amax_in = amax_in.to(device=x.device, dtype=torch.int64).contiguous()
                if tuple(amax_in.shape) != (n, h, w, layer.output_channels):
                    raise ValueError("unpool_argmax must have shape %s (got %s)"
                                     % ((n, h, w, layer.output_channels), tuple(amax_in.shape)))
            _lib.check(L.ssal_enet_run_layer_arith(handle, name, _lib.dev_ptr(x), n, h, w, _lib.arithmetic_code(arithmetic),
                                                   _lib.dev_ptr(y), _lib.dev_ptr(amax_out), _lib.dev_ptr(amax_in),
                                                   _lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr()))
        return (y, amax_out) if want_argmax else y
