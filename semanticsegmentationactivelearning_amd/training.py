"""Training of ENet's output layer on the MI355X: the reference's ``-r/--reinitialize-output-layer`` case
(active_learning.py:905-909, 461-462) followed by its ``train_op`` (:283-326) restricted to ``Final.kernel``.

``FinalLayerTrainer(net, ...)`` keeps the Adam state of ``net.Final.kernel`` on the device.  One ``step`` runs the frozen
trunk (``training=False``: moving averages, no dropout), then ONE fused kernel that recomputes the Final logits, the
masked softmax cross entropy and dL/dlogit and contracts them with the Bottleneck5_1 features into dL/dW (the logits never
reach HBM), then the Keras ``l1_l2`` regulariser gradient and TF-1.13 ``ApplyAdam``.  The one deliberate difference from the
reference: its ``train_op`` trains every layer with batch statistics; here the trunk is frozen and evaluated in inference
mode.

The semi-supervised step of the reference (active_learning.py:226-275, 339-342) is the same kernel with the targets built
inside it: ``labelled`` marks, per image, whether the caller's annotation or the image's own pseudo annotation (argmax and
``confidence >= threshold`` of the logits the kernel already holds) is trained on, ``confusion`` collects the training-pass
confusion matrix and ``return_pseudo_pixels`` the count of pixels the threshold lets through.
"""
import collections
import inspect

import numpy as np

from . import _icnet_depths as _depths
from . import _lib
from .models.enet import enet_modules as _mod


class FinalLayerTrainer:
    """Adam on ``net.Final.kernel`` [3, 3, K, 16] of an ``ENet``; hyper-parameters as in the reference's JSON
    (``from_params``).  ``loginverse_scaling`` is the loss' ``weight`` (ENet class weighting when > 1)."""

    def __init__(self, net, learning_rate, beta1=0.9, beta2=0.999, epsilon=1e-8, l1=0.0, l2=0.0, loginverse_scaling=0.0,
                 label_smoothing=0.0, learning_rate_decay=0.0, decay_steps=None, measure="entropy", threshold=0.0):
        self._check_model(net)
        if not (2 <= int(net.classes) <= 32):
            raise ValueError("classes must be in [2, 32] (got %d)" % net.classes)
        if learning_rate_decay > 0.0 and not decay_steps:
            raise ValueError("learning_rate_decay > 0 needs decay_steps (the reference uses the batches per epoch)")
        self.net = net
        self.learning_rate = float(learning_rate)
        self.beta1, self.beta2, self.epsilon = float(beta1), float(beta2), float(epsilon)
        self.l1, self.l2 = float(l1), float(l2)
        self.weight = float(loginverse_scaling)
        self.label_smoothing = float(label_smoothing)
        self.learning_rate_decay = float(learning_rate_decay)
        self.decay_steps = decay_steps
        if measure not in _lib.MEASURES:
            raise NotImplementedError("Uncertainty function not implemented.")
        self.measure, self.threshold = measure, float(threshold)  # defaults of the pseudo annotation's keywords
        self._dev = None  # device tensors: w, m, v, grad, loss
        self._t = 0
        self._reset_beta_powers()  # AdamOptimizer's beta powers (fp32)
        self._m0 = self._v0 = None  # host copies of Adam's slots waiting for the device

    @staticmethod
    def _check_model(net):
        """the model class the training kernels are written for (``ICNetHeadTrainer``: ICNet)"""
        from .models.enet.enet import ENet
        if not isinstance(net, ENet):
            raise NotImplementedError("output-layer training is implemented for ENet only (got %s)" % type(net).__name__)

    @classmethod
    def from_params(cls, net, params, decay_steps=None):
        """The reference's JSON layout (conf/*.json): ``hyperparams.learning_rate``, ``.learning_rate_decay``,
        ``.optimizer.kwargs`` (beta1, beta2, epsilon), ``.weight_reg.{L1, L2}``, ``.softmax.{loginverse_scaling,
        label_smoothing, multiscale}``.  ``params`` may be the whole file or its ``hyperparams`` section; the whole file also
        gives ``active_learning.{measure, threshold}``, the defaults of the pseudo annotation."""
        hp = params.get("hyperparams", params)
        sm = hp.get("softmax", {})
        if sm.get("multiscale", False):
            raise NotImplementedError("softmax.multiscale: the auxiliary heads are not trained here")
        opt = hp.get("optimizer", {})
        if opt.get("type", "Adam") != "Adam":
            raise NotImplementedError("optimizer %r: only Adam is implemented" % opt.get("type"))
        kw = dict(opt.get("kwargs", {}))
        reg = hp.get("weight_reg", {})
        al = params.get("active_learning", {}) if "hyperparams" in params else {}
        return cls(net, learning_rate=hp["learning_rate"], beta1=kw.get("beta1", 0.9), beta2=kw.get("beta2", 0.999),
                   epsilon=kw.get("epsilon", 1e-8), l1=reg.get("L1", 0.0) or 0.0, l2=reg.get("L2", 0.0) or 0.0,
                   loginverse_scaling=sm.get("loginverse_scaling", 0.0) or 0.0,
                   label_smoothing=sm.get("label_smoothing", 0.0) or 0.0,
                   learning_rate_decay=hp.get("learning_rate_decay", 0.0) or 0.0, decay_steps=decay_steps,
                   measure=al.get("measure", "entropy"), threshold=al.get("threshold", 0.0))

    # ---- state -----------------------------------------------------------------------------------------------------
    def _kernel_var(self):
        if not self.net.built:
            raise RuntimeError("build the model (call it once, or .build(input_shape)) before training")
        return self.net.Final.kernel

    def reinitialize(self, seed=None):
        """``sess.run(train_net.Final.kernel.initializer)`` (active_learning.py:461-462): glorot-uniform, the layer's default
        initializer, drawn from ``seed``.  The optimizer state is reset too."""
        var = self._kernel_var()
        var.assign(_mod.glorot_uniform(seed)(var.shape))
        self.load_state({"m": self._state_view(self._zero_state()), "v": self._state_view(self._zero_state()), "t": 0})

    # the hooks the shared state and Adam code stands on (LastBlockTrainer: the packed block)
    def _host_weights(self):
        """the trained weights of the host model as one float32 array"""
        return np.array(self._kernel_var().numpy(), dtype=np.float32)

    def _zero_state(self):
        return np.zeros(self._kernel_var().shape, np.float32)

    def _version_key(self):
        return self._kernel_var().version

    def _state_view(self, a):
        """one of Adam's slots as ``state`` presents it"""
        return a.copy()

    def _trained_tail(self):
        """how many of ``net.variables``, counted from the end, the training kernels take as an argument"""
        return 1

    def _adam_ranges(self):
        """(lo, hi, regularised) ranges of the flattened weights Adam runs on"""
        return ((0, int(np.prod(self._kernel_var().shape)), True),)

    def _write_back(self, host):
        self.net.Final.kernel.assign(host)

    def _advance_beta_powers(self):
        self._b1p = np.float32(self._b1p * np.float32(self.beta1))
        self._b2p = np.float32(self._b2p * np.float32(self.beta2))

    def _reset_beta_powers(self):
        """the beta powers as AdamOptimizer holds them before step ``t`` + 1 (fp32 products)"""
        self._b1p = self._b2p = np.float32(1.0)
        for _ in range(self._t + 1):
            self._advance_beta_powers()

    @property
    def state(self):
        """``{"m", "v"}`` float32 host copies of Adam's slots and ``"t"`` (steps taken)"""
        if self._dev is None:
            m = self._m0 if self._m0 is not None else self._zero_state()
            v = self._v0 if self._v0 is not None else self._zero_state()
        else:
            m, v = self._dev["m"].cpu().numpy(), self._dev["v"].cpu().numpy()
        return {"m": self._state_view(m), "v": self._state_view(v), "t": self._t}

    def _set_state(self, m, v, t):
        self._t = int(t)
        self._reset_beta_powers()
        self._m0, self._v0 = m, v
        self._dev = None

    def load_state(self, state):
        shape = self._kernel_var().shape
        m = np.ascontiguousarray(state["m"], dtype=np.float32)
        v = np.ascontiguousarray(state["v"], dtype=np.float32)
        if m.shape != shape or v.shape != shape:
            raise ValueError("m / v must have shape %s" % (shape,))
        self._set_state(m, v, state["t"])

    def current_learning_rate(self):
        """tf.train.inverse_time_decay(lr, global_step, decay_steps, decay_rate) (not staircase), fp32 as TF computes it;
        global_step = the number of steps taken so far"""
        lr = np.float32(self.learning_rate)
        if self.learning_rate_decay > 0.0:
            p = np.float32(np.float32(self._t) / np.float32(self.decay_steps))
            lr = np.float32(lr / np.float32(np.float32(1.0) + np.float32(self.learning_rate_decay) * p))
        return lr

    def _device_state(self, device):
        torch = _lib.require_gpu()
        ver = self._version_key()
        if self._dev is None or self._dev["w"].device != device or self._dev["version"] != ver:
            m = self._m0 if self._m0 is not None else (self._dev["m"].cpu().numpy() if self._dev else self._zero_state())
            v = self._v0 if self._v0 is not None else (self._dev["v"].cpu().numpy() if self._dev else self._zero_state())
            w = torch.from_numpy(self._host_weights()).to(device)
            self._dev = {"w": w, "m": torch.from_numpy(np.array(m)).to(device), "v": torch.from_numpy(np.array(v)).to(device),
                         "grad": torch.empty_like(w), "version": ver}
            self._m0 = self._v0 = None
        return self._dev

    def _trunk_handle(self):
        """the net's handle for the current device: reused while every variable BELOW the trained tail is unchanged (the
        training entries take the trained weights as an argument), so the whole weight set (1.5 MB) is pushed and committed
        again only when a TRUNK variable changed.  The handle's pushed-versions record keeps the old versions, so the next
        score / evaluate / call pushes the new weights once."""
        torch = _lib.require_gpu()
        net = self.net
        ent = net._handles.get(torch.cuda.current_device())
        tail = self._trained_tail()
        if ent is not None and ent[1] is not None:
            if tuple(v.version for v in net.variables)[:-tail] == ent[1][:-tail]:
                return ent[0]
        return net._sync_handle()

    def _apply(self, dev, grad):
        lr = self.current_learning_rate()
        L = _lib.lib()
        w, m, v, g = (t.view(-1) for t in (dev["w"], dev["m"], dev["v"], grad))
        for lo, hi, reg in self._adam_ranges():
            _lib.check(L.ssal_adam_apply(_lib.dev_ptr(w[lo:hi]), _lib.dev_ptr(m[lo:hi]), _lib.dev_ptr(v[lo:hi]),
                                         _lib.dev_ptr(g[lo:hi]), hi - lo, float(lr), self.beta1, self.beta2, self.epsilon,
                                         float(self._b1p), float(self._b2p), self.l1 if reg else 0.0,
                                         self.l2 if reg else 0.0, _lib.stream_ptr()))
        self._t += 1
        self._advance_beta_powers()
        # the host variables are the model's weights of record: score / evaluate / __call__ push them on their next call
        # (synchronises the stream: 11 KB for the output layer, 12.5 KB for the last block at K = 19)
        self._write_back(dev["w"].cpu().numpy())
        dev["version"] = self._version_key()

    # ---- arguments ---------------------------------------------------------------------------------------------------
    def _targets(self, labels, mask, shape, device):
        torch = _lib.require_gpu()
        lab = labels if isinstance(labels, torch.Tensor) else torch.as_tensor(np.asarray(labels))
        mk = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(np.asarray(mask))
        if tuple(lab.shape) != shape:
            raise ValueError("labels must have shape %s (got %s)" % (shape, tuple(lab.shape)))
        if tuple(mk.shape) != shape:
            raise ValueError("mask must have shape %s (got %s)" % (shape, tuple(mk.shape)))
        lab = lab.to(device=device, dtype=torch.uint8).contiguous()
        mk = mk.to(device=device, dtype=torch.float32).contiguous()
        return lab, mk

    _semi_keywords = True  # False: every semi-supervised keyword is refused (LastBlockTrainer, LastStageTrainer)

    @staticmethod
    def _no_semi(**kw):
        for name, value in kw.items():
            if value is not None and value is not False:
                raise NotImplementedError("%s: the semi-supervised step is implemented for the output layer only "
                                          "(FinalLayerTrainer)" % name)

    def _semi_call(self, batch, labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels, **raw):
        """the semi-supervised keywords of a call, before anything else is looked at: refused by the classes that do not take
        them, else ``_semi``'s verdict for the batch ``batch`` leads"""
        if not self._semi_keywords:
            self._no_semi(labelled=labelled, measure=measure, threshold=threshold, confusion=confusion,
                          return_pseudo_pixels=return_pseudo_pixels, **raw)
            return None
        n = int(np.shape(batch)[0]) if len(np.shape(batch)) else 0
        return self._semi(n, labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels)

    def _semi(self, n, labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels):
        """the semi-supervised keywords, judged on the host before any device work: None when the call is today's plain
        one (no ``labelled``, no ``confusion``, no pseudo-pixel request), else ``(labelled uint8 [n] host array or torch
        tensor, or None; measure code; threshold)``"""
        measure = self.measure if measure is None else measure
        if measure not in _lib.MEASURES:
            raise NotImplementedError("Uncertainty function not implemented.")
        threshold = self.threshold if threshold is None else float(threshold)
        if labelled is not None:
            if tuple(np.shape(labelled)) != (n,):
                raise ValueError("labelled must be a [N] vector (N = %d; got shape %s)" % (n, tuple(np.shape(labelled))))
        if confusion is not None:
            k = int(self.net.classes)
            if tuple(np.shape(confusion)) != (k, k) or "int64" not in str(getattr(confusion, "dtype", "")):
                raise ValueError("confusion must be an int64 [%d, %d] device tensor" % (k, k))
        if labels is None or mask is None:
            host = None if labelled is None else (labelled.cpu().numpy() if hasattr(labelled, "cpu") else np.asarray(labelled))
            if host is None or host.astype(bool).any():
                raise ValueError("labels / mask may be None only when labelled marks no image as labelled")
        if labelled is None and confusion is None and not return_pseudo_pixels:
            return None
        return labelled, _lib.MEASURES[measure], threshold

    def _semi_device(self, semi, n, device, labels, mask, shape):
        """device forms of the targets: labelled uint8 [n] (or None), label / mask planes (None only in a semi call that
        gives none); a plain call (``semi`` None) needs both planes"""
        if semi is None:
            return (None,) + self._targets(labels, mask, shape, device)
        torch = _lib.require_gpu()
        labelled = semi[0]
        if labelled is not None:
            t = labelled if isinstance(labelled, torch.Tensor) else torch.as_tensor(np.asarray(labelled))
            labelled = (t != 0).to(device=device, dtype=torch.uint8).contiguous()
        lab = mk = None
        if labels is not None and mask is not None:
            lab, mk = self._targets(labels, mask, shape, device)
        return labelled, lab, mk

    @staticmethod
    def _semi_c_args(semi, labelled_dev, confusion, pseudo_pixels):
        """what a semi entry takes beyond its plain sibling: (the arguments after the mask, those after the gradient)"""
        if semi is None:
            return (), ()
        torch = _lib.require_gpu()
        return ((_lib.dev_ptr(labelled_dev), semi[1], semi[2]),
                (_lib.dev_ptr(confusion, torch.int64, "confusion"), _lib.dev_ptr(pseudo_pixels)))

    # ---- the two C calls: (plain stem, semi stem) of the entries, + "_workspace_bytes" / "_nhwc" ------------------------------
    _C_FEATURES = ("ssal_final_grad", "ssal_final_grad_semi")
    _C_IMAGES = ("ssal_enet_train_final", "ssal_enet_train_final_semi")
    _CHANNELS, _UP = 16, 2  # of the feature map the features entry takes; output pixels per feature pixel and axis
    _LIMIT = ("kernel's", "kernel's")  # the wording of a plain / a semi call's "beyond the limit" error

    def _features_workspace_bytes(self, query, n, h, w, k, semi, with_raw):
        """the features entry's workspace query (here the raw features are the caller's: no ``with_raw``)"""
        return query(n, h, w, k)

    def _grad_call(self, x, x_raw, labels, mask, params_dev, semi, confusion, return_pseudo_pixels, extra=()):
        """(loss [1] float64, gradient shaped like ``params_dev``, pseudo pixels or None) through the features entry: the plain
        one, or with ``semi`` the semi-supervised one.  ``x`` / ``x_raw``: the entry's leading device tensors (features[, pooling
        indices]) of the training / the undistorted frames (``x_raw`` all None: no raw side); ``extra``: the arguments
        between the loss' knobs and the outputs"""
        torch = _lib.require_gpu()
        f = x[0]
        if f.dim() != 4 or f.shape[-1] != self._CHANNELS:
            raise ValueError("features must be [N,h,w,%d] (got %s)" % (self._CHANNELS, tuple(f.shape)))
        n, h, w, _ = f.shape
        k = int(self.net.classes)
        lbd, lab, mk = self._semi_device(semi, n, f.device, labels, mask, (n, self._UP * h, self._UP * w))
        L = _lib.lib()
        stem = self._C_FEATURES[semi is not None]
        with torch.cuda.device(f.device):
            nbytes = self._features_workspace_bytes(getattr(L, stem + "_workspace_bytes"), n, h, w, k, semi is not None,
                                                    int(x_raw[0] is not None))
            if nbytes < 0:
                raise ValueError("feature map %dx%d is beyond the gradient %s limit" % (h, w, self._LIMIT[semi is not None]))
            ws = torch.empty(int(nbytes), dtype=torch.uint8, device=f.device)
            loss = torch.empty((1,), dtype=torch.float64, device=f.device)
            grad = torch.empty_like(params_dev)
            pp = torch.empty((n,), dtype=torch.int64, device=f.device) if return_pseudo_pixels else None
            after_mask, after_grad = self._semi_c_args(semi, lbd, confusion, pp)
            inputs = tuple(x) + (tuple(x_raw) if semi is not None else ())
            _lib.check(getattr(L, stem + "_nhwc")(
                *(tuple(_lib.dev_ptr(t) for t in inputs) + (n, h, w, k, _lib.dev_ptr(params_dev), _lib.dev_ptr(lab),
                  _lib.dev_ptr(mk)) + after_mask + (self.weight, self.label_smoothing) + tuple(extra)
                  + (_lib.dev_ptr(loss), _lib.dev_ptr(grad)) + after_grad + (_lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr()))))
        return loss, grad, pp

    def _images_call(self, images, images_raw, labels, mask, semi, confusion, return_pseudo_pixels, extra=(), weights=None):
        """the images entry (the plain one, or with ``semi`` the semi-supervised one): the frozen trunk and the training
        kernels on the weights of the device state (``weights``: on that packed device vector instead), the gradient into
        the device state's ``grad``.  No update.  -> (loss [1], pseudo pixels or None, device state)"""
        torch = _lib.require_gpu()
        net = self.net
        x = net._prepare(images, False)
        n, h, w, _ = x.shape
        L = _lib.lib()
        lbd, lab, mk = self._semi_device(semi, n, x.device, labels, mask, (n, h, w))
        xr = None
        if semi is not None and images_raw is not None and images_raw is not images:
            xr = net._prepare(images_raw, False)
            if tuple(xr.shape) != tuple(x.shape) or xr.dtype != x.dtype or xr.device != x.device:
                raise ValueError("images_raw must have the shape and dtype of images %s %s (got %s %s)"
                                 % (tuple(x.shape), x.dtype, tuple(xr.shape), xr.dtype))
        stem = self._C_IMAGES[semi is not None]
        with torch.cuda.device(x.device):
            dev = self._device_state(x.device)
            handle = self._trunk_handle()
            raw = () if semi is None else (xr,)
            nbytes = getattr(L, stem + "_workspace_bytes")(handle, n, h, w, *(int(t is not None) for t in raw))
            if nbytes < 0:
                raise ValueError("bad input dims %s" % (tuple(x.shape),))
            ws = net._workspace(nbytes, x.device)
            loss = torch.empty((1,), dtype=torch.float64, device=x.device)
            pp = torch.empty((n,), dtype=torch.int64, device=x.device) if return_pseudo_pixels else None
            after_mask, after_grad = self._semi_c_args(semi, lbd, confusion, pp)
            _lib.check(getattr(L, stem + "_nhwc")(
                *((handle, _lib.dev_ptr(x)) + tuple(_lib.dev_ptr(t) for t in raw) + (int(x.dtype == torch.uint8), n, h, w,
                  _lib.dev_ptr(lab), _lib.dev_ptr(mk)) + after_mask + (_lib.dev_ptr(dev["w"] if weights is None else weights),
                  self.weight,
                  self.label_smoothing) + tuple(extra) + (_lib.dev_ptr(loss), _lib.dev_ptr(dev["grad"])) + after_grad
                  + (_lib.dev_ptr(ws), ws.numel(), _lib.stream_ptr()))))
            net._note_call(ws, (n, h, w), "train")
        return loss, pp, dev

    def _step_images(self, images, images_raw, labels, mask, semi, confusion, return_pseudo_pixels, extra=()):
        """one Adam step through the images entry: ``_images_call``, then Adam.  -> loss before the step[, pseudo pixels]"""
        torch = _lib.require_gpu()
        loss, pp, dev = self._images_call(images, images_raw, labels, mask, semi, confusion, return_pseudo_pixels, extra)
        with torch.cuda.device(dev["w"].device):
            self._apply(dev, dev["grad"])
        return (loss[0], pp) if return_pseudo_pixels else loss[0]

    # ---- gradients and steps -------------------------------------------------------------------------------------------
    def gradient_features(self, features, labels, mask, kernel=None, labelled=None, measure=None, threshold=None,
                          features_raw=None, confusion=None, return_pseudo_pixels=False):
        """(loss float64 [1], dL/dW [3, 3, K, 16] fp32) on the device for Bottleneck5_1 features [N, h, w, 16] and
        labels / mask [N, 2h, 2w]; ``kernel`` defaults to ``net.Final.kernel``.  No update.

        The semi-supervised step (active_learning.py:226-275, 339-342): ``labelled`` [N] (bool / uint8, numpy or torch) marks
        the images trained on ``labels`` / ``mask``; the others are trained on their own pseudo annotation -- the argmax of
        their Final logits under ``kernel`` and ``confidence >= threshold`` for ``measure`` (defaults: the trainer's, i.e.
        "entropy" / 0.0 or ``from_params``' ``active_learning`` section) -- whose label / mask planes are never read
        (``labels`` / ``mask`` may be None when no image is labelled).  ``features_raw`` [N, h, w, 16]: the features of the
        undistorted frames, which the pseudo annotation is then computed from.  ``confusion`` (int64 [K, K] device tensor)
        is added the training-pass confusion matrix of the targets trained on against the argmax of the training logits;
        ``return_pseudo_pixels`` appends the int64 [N] count of pseudo-mask-1 pixels per image to the result."""
        semi = self._semi_call(features, labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels)
        x = _lib.as_device_f32(features)
        if x.dim() != 4 or x.shape[-1] != 16:
            raise ValueError("features must be [N,h,w,16] (got %s)" % (tuple(x.shape),))
        k = self.net.classes
        kern = _lib.as_device_f32(self._kernel_var().numpy() if kernel is None else kernel).to(x.device)
        if tuple(kern.shape) != (3, 3, k, 16):
            raise ValueError("kernel must be [3,3,%d,16] (got %s)" % (k, tuple(kern.shape)))
        xr = None
        if semi is not None and features_raw is not None and features_raw is not features:
            xr = _lib.as_device_f32(features_raw).to(x.device)
            if tuple(xr.shape) != tuple(x.shape):
                raise ValueError("features_raw must have the shape of features %s (got %s)" % (tuple(x.shape), tuple(xr.shape)))
        loss, grad, pp = self._grad_call((x,), (xr,), labels, mask, kern, semi, confusion, return_pseudo_pixels)
        return (loss, grad, pp) if return_pseudo_pixels else (loss, grad)

    def step_features(self, features, labels, mask, labelled=None, measure=None, threshold=None, features_raw=None,
                      confusion=None, return_pseudo_pixels=False):
        """one Adam step from cached Bottleneck5_1 features (``ENet.endpoint_outputs[0][1]``); returns the loss (float64
        device scalar) of the kernel BEFORE the step, as ``sess.run([loss, train_op])`` does.  The keywords are those of
        ``gradient_features``; with ``return_pseudo_pixels`` the result is ``(loss, pseudo_pixels)``."""
        self._semi_call(features, labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels)
        x = _lib.as_device_f32(features)
        dev = self._device_state(x.device)
        out = self.gradient_features(x, labels, mask, kernel=dev["w"], labelled=labelled, measure=measure,
                                     threshold=threshold, features_raw=features_raw, confusion=confusion,
                                     return_pseudo_pixels=return_pseudo_pixels)
        self._apply(dev, out[1])
        return (out[0][0], out[2]) if return_pseudo_pixels else out[0][0]

    def step(self, images, labels, mask, labelled=None, measure=None, threshold=None, images_raw=None, confusion=None,
             return_pseudo_pixels=False):
        """one Adam step from images [N, H, W, C] (fp32 or decoded uint8) and labels / mask [N, H, W]: the frozen trunk
        up to Bottleneck5_1, the fused gradient kernel, Adam.  Returns the loss (float64 device scalar) before the step.

        ``labelled`` / ``measure`` / ``threshold`` / ``confusion`` / ``return_pseudo_pixels`` as in ``gradient_features``
        (the result is then ``(loss, pseudo_pixels)``); ``images_raw``: the undistorted frames (``InputStage``'s ``image``
        next to its ``image_dist``), same shape and dtype as ``images`` -- the trunk runs on them too and the pseudo
        annotation comes from their logits, as the reference's ``pseudo_logits`` do (active_learning.py:231)."""
        semi = self._semi_call(images, labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels)
        return self._step_images(images, images_raw, labels, mask, semi, confusion, return_pseudo_pixels)


# ---- the packed block of the ENet trainers (DESIGN.md sections 17-22) ------------------------------------------------------
# The trained blocks travel as one float array, one part per block (include/ssal_enet.h, "Last-block training" .. "Decoder
# training").  A kind of block is described once: ``layout`` (layer attribute, float offset from the part's start, regularised)
# of its trained variables, ``stats`` (attribute, offset) of its moving statistics, ``floats`` of the part.  A trainer class
# states its parts, in packed order, as ``_PARTS``: ((layer name, kind), ...).
_Kind = collections.namedtuple("_Kind", "layout stats floats")
_LAST_BLOCK = _Kind(  # Bottleneck5_1's block; Final.kernel closes this part: 144 K more floats at _FINAL_OFFSET
    (("proj_kernel", 0, True), ("proj_gamma", 64, False), ("proj_beta", 68, False), ("proj_alpha", 72, True),
     ("conv_kernel", 76, True), ("conv_gamma", 220, False), ("conv_beta", 224, False), ("conv_alpha", 228, True),
     ("exp_kernel", 232, True), ("exp_gamma", 296, False), ("exp_beta", 312, False), ("residual_alpha", 328, True)),
    (("proj_mean", 344), ("proj_variance", 348), ("conv_mean", 352), ("conv_variance", 356), ("exp_mean", 360),
     ("exp_variance", 376)), 400)
_FINAL_OFFSET = _LAST_BLOCK.floats
_UPSAMPLE16 = _Kind(  # the 64 -> 16 upsampling block (Bottleneck5_0)
    (("proj_kernel", 0, True), ("proj_gamma", 1024, False), ("proj_beta", 1040, False), ("proj_alpha", 1056, True),
     ("conv_kernel", 1072, True), ("conv_gamma", 2224, False), ("conv_beta", 2232, False), ("conv_alpha", 2240, True),
     ("exp_kernel", 2248, True), ("exp_gamma", 2376, False), ("exp_beta", 2392, False), ("res_kernel", 2408, True),
     ("residual_alpha", 3432, True)),
    (("proj_mean", 3448), ("proj_variance", 3464), ("conv_mean", 3480), ("conv_variance", 3488), ("exp_mean", 3496),
     ("exp_variance", 3512)), 3536)
_REGULAR64 = _Kind(  # a regular 64 -> 16 -> 16 -> 64 bottleneck (Bottleneck4_2, Bottleneck4_1)
    (("proj_kernel", 0, True), ("proj_gamma", 1024, False), ("proj_beta", 1040, False), ("proj_alpha", 1056, True),
     ("conv_kernel", 1072, True), ("conv_gamma", 3376, False), ("conv_beta", 3392, False), ("conv_alpha", 3408, True),
     ("exp_kernel", 3424, True), ("exp_gamma", 4448, False), ("exp_beta", 4512, False), ("residual_alpha", 4576, True)),
    (("proj_mean", 4640), ("proj_variance", 4656), ("conv_mean", 4672), ("conv_variance", 4688), ("exp_mean", 4704),
     ("exp_variance", 4768)), 4840)
_UPSAMPLE64 = _Kind(  # the 128 -> 32 -> 16 -> 64 upsampling block (Bottleneck4_0): _UPSAMPLE16's order with its sizes
    (("proj_kernel", 0, True), ("proj_gamma", 4096, False), ("proj_beta", 4128, False), ("proj_alpha", 4160, True),
     ("conv_kernel", 4192, True), ("conv_gamma", 8800, False), ("conv_beta", 8816, False), ("conv_alpha", 8832, True),
     ("exp_kernel", 8848, True), ("exp_gamma", 9872, False), ("exp_beta", 9936, False), ("res_kernel", 10000, True),
     ("residual_alpha", 18192, True)),
    (("proj_mean", 18256), ("proj_variance", 18288), ("conv_mean", 18320), ("conv_variance", 18336), ("exp_mean", 18352),
     ("exp_variance", 18416)), 18488)


def _merged(ranges):
    """(lo, hi, regularised) ranges with adjacent ones joined where they touch and carry the same flag: one Adam launch each"""
    out = []
    for lo, hi, reg in ranges:
        if out and out[-1][1] == lo and out[-1][2] == reg:
            out[-1] = (out[-1][0], hi, reg)
        else:
            out.append((lo, hi, reg))
    return out


# ---- the last block: Bottleneck5_1 + Final ---------------------------------------------------------


class LastBlockTrainer(FinalLayerTrainer):
    """Adam on the 13 variables of ENet's last block: ``Final.kernel`` and ``Bottleneck5_1``'s ``proj_kernel``,
    ``proj_gamma``, ``proj_beta``, ``proj_alpha``, ``conv_kernel``, ``conv_gamma``, ``conv_beta``, ``conv_alpha``,
    ``exp_kernel``, ``exp_gamma``, ``exp_beta`` and ``residual_alpha``: the first backward pass through a bottleneck.

    The one deliberate difference from the reference carries over from ``FinalLayerTrainer``: its ``train_op`` trains every
    layer with batch statistics and dropout.  Here everything below Bottleneck5_1 is frozen and runs with
    ``training=False``, and Bottleneck5_1 itself is trained in INFERENCE mode: its moving means and variances are constants
    (the ``*_mean`` / ``*_variance`` variables are never written), there is no spatial dropout, and batch-norm is the affine
    map ``y = gamma (x - mean) / sqrt(var + 1e-3) + beta`` with ``gamma`` and ``beta`` trainable.

    Regulariser: the Keras ``l1_l2`` gradient goes to exactly the variables the reference attaches ``kernel_regularizer``
    to: ``proj_kernel`` (enet_modules.py:366-373), ``proj_alpha`` (:375-382), ``conv_kernel`` (:433-440), ``conv_alpha``
    (:442-449), ``exp_kernel`` (:477-484), ``residual_alpha`` (:516-523) and ``Final.kernel`` (the ``Final`` layer's only
    weight).  The batch-norm ``gamma`` / ``beta`` (:398-411, :463-474, :500-513) carry none and get the plain Adam update.
    ``weight_reg.glorot_scaling`` (``regularization_scaling``, :350-362) is not implemented.

    PReLU is ``relu(x) - alpha relu(-x)`` (extra_ops.py:9-26); at an input of exactly 0 both derivatives are 0, as
    TensorFlow's ``ReluGrad`` gives them.

    ``state`` / ``load_state``: ``{"m": {name: array}, "v": {name: array}, "t": steps}`` keyed by variable name
    (``"Final.kernel"``, ``"Bottleneck5_1.proj_kernel"``, ...)."""

    _semi_keywords = False  # SemiSupervisedBlockTrainer accepts them
    _C_FEATURES = ("ssal_train_block_grad", "ssal_train_block_grad_semi")
    _C_IMAGES = ("ssal_enet_train_block", "ssal_enet_train_block_semi")
    _LIMIT = ("kernel's", "kernels'")

    @classmethod
    def from_params(cls, net, params, decay_steps=None):
        hp = params.get("hyperparams", params)
        if (hp.get("weight_reg", {}) or {}).get("glorot_scaling", False):
            raise NotImplementedError("weight_reg.glorot_scaling: the per-kernel regulariser scaling is not implemented")
        return super().from_params(net, params, decay_steps=decay_steps)

    # ---- the packed block ------------------------------------------------------------------------------------------------
    _PARTS = (("Bottleneck5_1", _LAST_BLOCK),)  # lowest block last: everything below it is frozen

    def _parts(self):
        """[(the layer, its name, its kind, the float offset of its part)] in packed order"""
        out, start = [], 0
        for name, kind in self._PARTS:
            out.append((getattr(self.net, name), name, kind, start))
            start += kind.floats + (0 if start else 144 * int(self.net.classes))  # (Final.kernel closes the first part)
        return out

    @staticmethod
    def _part_named(blk, name, kind, start):
        return [("%s.%s" % (name, a), getattr(blk, a), start + off, reg) for a, off, reg in kind.layout]

    def _named(self):
        """[(name, Variable, float offset, regularised)] of the trained variables: Final.kernel, then part by part"""
        if not self.net.built:
            raise RuntimeError("build the model (call it once, or .build(input_shape)) before training")
        return sum((self._part_named(*p) for p in self._parts()), [("Final.kernel", self.net.Final.kernel, _FINAL_OFFSET, True)])

    @property
    def variable_names(self):
        return [n for n, _, _, _ in self._named()]

    def _floats(self):
        return 144 * int(self.net.classes) + sum(kind.floats for _, kind in self._PARTS)

    def _pack(self, arrays=None):
        """the packed block from the host variables (``arrays`` None; the statistics included) or from a name -> array
        mapping (statistics and padding 0)"""
        out = np.zeros(self._floats(), np.float32)
        for name, var, off, _ in self._named():
            a = var.numpy() if arrays is None else np.ascontiguousarray(arrays[name], dtype=np.float32)
            if a.shape != var.shape:
                raise ValueError("%s must have shape %s (got %s)" % (name, var.shape, a.shape))
            out[off:off + a.size] = a.reshape(-1)
        if arrays is None:
            for blk, _, kind, start in self._parts():
                for a, off in kind.stats:
                    v = getattr(blk, a).numpy()
                    out[start + off:start + off + v.size] = v
        return out

    def _unpack(self, packed):
        return {name: np.array(packed[off:off + int(np.prod(var.shape))]).reshape(var.shape)
                for name, var, off, _ in self._named()}

    def _versions(self):
        return tuple(v.version for v in self._trained_variables())

    def _trained_variables(self):
        """every variable of the trained layers (the moving statistics too), Final.kernel first"""
        return [self.net.Final.kernel] + [v for blk, _, _, _ in self._parts() for v in blk.variables]

    # ---- FinalLayerTrainer's hooks: the state and Adam run on the packed block ---------------------------------------------
    def _host_weights(self):
        return self._pack()

    def _version_key(self):
        return self._versions()

    def _state_view(self, a):
        return self._unpack(a)

    def _zero_state(self):
        return np.zeros(self._floats(), np.float32)

    def _features_workspace_bytes(self, query, n, h, w, k, semi, with_raw):
        """a semi call's workspace holds the packed target plane of the undistorted frames when there are any"""
        return query(n, h, w, k, with_raw) if semi else query(n, h, w, k)

    def _trained_tail(self):
        return len(self._trained_variables())

    def _adam_ranges(self):
        """part by part, each part's variables merged where they touch and share the flag; Final.kernel after the first"""
        out = []
        for part in self._parts():
            out += _merged((off, off + int(np.prod(var.shape)), reg) for _, var, off, reg in self._part_named(*part))
            if not part[3]:
                out.append((_FINAL_OFFSET, _FINAL_OFFSET + 144 * int(self.net.classes), True))
        return tuple(out)

    def _write_back(self, host):
        for name, var, off, _ in self._named():
            var.assign(host[off:off + int(np.prod(var.shape))].reshape(var.shape))

    def load_state(self, state):
        names = set(self.variable_names)
        for key in ("m", "v"):
            if not isinstance(state[key], dict) or set(state[key]) != names:
                raise ValueError("state[%r] must map exactly the %d variable names to arrays" % (key, len(names)))
        self._set_state(self._pack(state["m"]), self._pack(state["v"]), state["t"])

    # ---- arguments, judged on the host -----------------------------------------------------------------------------------
    def _check_params(self, params):
        params = dict(params or {})
        unknown = set(params) - set(self.variable_names)
        if unknown:
            raise ValueError("unknown variables %s (the moving statistics always come from the model)" % sorted(unknown))
        return params

    def _packed_with(self, params):
        """the packed block of the host variables with ``params`` (name -> array) laid over it"""
        params = self._check_params(params)
        packed = self._pack()
        for name, var, off, _ in self._named():
            if name in params:
                a = params[name]
                a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a, dtype=np.float32)
                if a.shape != var.shape:
                    raise ValueError("%s must have shape %s (got %s)" % (name, var.shape, a.shape))
                packed[off:off + a.size] = a.reshape(-1)
        return packed

    def _check_inputs(self, inputs):
        """the leading arguments of a features call (features[, pooling indices]) after their host-side checks"""
        return tuple(inputs)

    def _raw_host(self, inputs, raw):
        """the undistorted frames' side of a features call, judged on the host before any device work: None when there is
        none (not given, or the very objects of ``inputs``), else its leading arguments after their checks"""
        if len({r is None for r in raw}) > 1:
            raise ValueError("features_raw and argmax1_raw are given together or not at all (the undistorted frame's "
                             "pooling indices are its own)")
        if raw[0] is None or all(r is i for r, i in zip(raw, inputs)):
            return None
        if tuple(np.shape(raw[0])) != tuple(np.shape(inputs[0])):
            raise ValueError("features_raw must have the shape of the features %s (got %s)"
                             % (tuple(np.shape(inputs[0])), tuple(np.shape(raw[0]))))
        return self._check_inputs(raw)

    @staticmethod
    def _on_device(inputs, device=None):
        x = _lib.as_device_f32(inputs[0])
        x = x if device is None else x.to(device)
        return (x,) + tuple(t.to(device=x.device).contiguous() for t in inputs[1:])

    # ---- gradients and steps ---------------------------------------------------------------------------------------------
    def _grad_dict(self, grad):
        return {name: grad[off:off + int(np.prod(var.shape))].view(var.shape) for name, var, off, _ in self._named()}

    def _features_on_device(self, inputs, raw, semi):
        """(the leading arguments of a features call on the device, those of the undistorted frames or Nones), after the
        host-side checks of both"""
        checked = self._check_inputs(inputs)
        raw = self._raw_host(inputs, raw) if semi is not None else None
        x = self._on_device(checked)
        return x, ((None,) * len(x) if raw is None else self._on_device(raw, x[0].device))

    def _gradient(self, inputs, raw, labels, mask, params, semi, confusion, return_pseudo_pixels, extra=()):
        """``gradient_features`` behind its keywords: (loss [1], {name: gradient}[, pseudo pixels])"""
        packed = self._packed_with(params)
        x, xr = self._features_on_device(inputs, raw, semi)
        params_dev = _lib.require_gpu().from_numpy(packed).to(x[0].device)
        loss, grad, pp = self._grad_call(x, xr, labels, mask, params_dev, semi, confusion, return_pseudo_pixels, extra)
        return (loss, self._grad_dict(grad), pp) if return_pseudo_pixels else (loss, self._grad_dict(grad))

    def _step_from_features(self, inputs, raw, labels, mask, semi, confusion, return_pseudo_pixels, extra=()):
        """``step_features`` behind its keywords: loss before the step[, pseudo pixels]"""
        x, xr = self._features_on_device(inputs, raw, semi)
        dev = self._device_state(x[0].device)
        loss, grad, pp = self._grad_call(x, xr, labels, mask, dev["w"], semi, confusion, return_pseudo_pixels, extra)
        self._apply(dev, grad)
        return (loss[0], pp) if return_pseudo_pixels else loss[0]

    def gradient_features(self, features5_0, labels, mask, params=None, labelled=None, measure=None, threshold=None,
                          features_raw=None, confusion=None, return_pseudo_pixels=False):
        """(loss float64 [1], {name: gradient}) on the device for Bottleneck5_0's output [N, h, w, 16] and labels / mask
        [N, 2h, 2w].  ``params``: a name -> array mapping that overrides any of the 13 variables (the others, and the
        moving statistics, are the model's).  No update.  The packed gradient is 0 in the statistics and padding slots.
        The keywords after ``params`` are the semi-supervised ones (``SemiSupervisedBlockTrainer``)."""
        semi = self._semi_call(features5_0, labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels,
                               features_raw=features_raw)
        return self._gradient((features5_0,), (features_raw,), labels, mask, params, semi, confusion, return_pseudo_pixels)

    def features(self, images):
        """Bottleneck5_0's output [N, H/2, W/2, 16] for ``images`` (a copy): what ``step_features`` and
        ``gradient_features`` take.  One forward pass of the frozen trunk; the frozen layers never change, so the result
        can be cached across steps."""
        return self._workspace_features(images, "ssal_enet_train_block_features_offset", 2, 16)

    def _workspace_features(self, images, offset_entry, down, channels):
        """[N, H / down, W / down, channels] fp32 (a copy) out of the net's workspace after one forward pass on ``images``;
        ``offset_entry``: the C query of the slice's byte offset"""
        net = self.net
        x = net._prepare(images, False)
        n, h, w, _ = x.shape
        net(x, training=False)
        off = getattr(_lib.lib(), offset_entry)(net._handle, n, h, w)
        if off < 0:
            raise ValueError("bad input dims %s" % (tuple(x.shape),))
        torch = _lib.require_gpu()
        shape = (n, h // down, w // down, channels)
        return net._ws[off:off + 4 * int(np.prod(shape))].view(torch.float32).view(shape).clone()

    def step_features(self, features5_0, labels, mask, labelled=None, measure=None, threshold=None, features_raw=None,
                      confusion=None, return_pseudo_pixels=False):
        """one Adam step from cached Bottleneck5_0 features [N, h, w, 16]; returns the loss (float64 device scalar) BEFORE
        the step, as ``sess.run([loss, train_op])`` does"""
        semi = self._semi_call(features5_0, labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels,
                               features_raw=features_raw)
        return self._step_from_features((features5_0,), (features_raw,), labels, mask, semi, confusion,
                                        return_pseudo_pixels)

    def step(self, images, labels, mask, labelled=None, measure=None, threshold=None, images_raw=None, confusion=None,
             return_pseudo_pixels=False):
        """one Adam step from images [N, H, W, C] (fp32 or decoded uint8) and labels / mask [N, H, W]: the frozen trunk up
        to Bottleneck5_0, the training kernels, Adam.  Returns the loss (float64 device scalar) before the step."""
        semi = self._semi_call(images, labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels,
                               images_raw=images_raw)
        return self._step_images(images, images_raw, labels, mask, semi, confusion, return_pseudo_pixels)


# ---- the last stage: Bottleneck5_0 + Bottleneck5_1 + Final ------------------------------------------
class LastStageTrainer(LastBlockTrainer):
    """Adam on the 26 variables of ENet's last decoder stage: the 13 of ``LastBlockTrainer`` and ``Bottleneck5_0``'s
    ``proj_kernel``, ``proj_gamma``, ``proj_beta``, ``proj_alpha``, ``conv_kernel``, ``conv_gamma``, ``conv_beta``,
    ``conv_alpha``, ``exp_kernel``, ``exp_gamma``, ``exp_beta``, ``res_kernel`` and ``residual_alpha``: the backward pass
    through the network's last upsampling block (a transposed convolution, a max-unpool, a resolution change).

    The deviation from the reference is ``LastBlockTrainer``'s: everything below Bottleneck5_0 is frozen and runs with
    ``training=False``; both trained blocks run in INFERENCE mode (constant moving statistics, never written; no spatial
    dropout; batch-norm ``y = gamma (x - mean) / sqrt(var + 1e-3) + beta`` with ``gamma`` / ``beta`` trainable).  The
    unpool's backward is the gather of the gradient at each element's pooling position.

    Regulariser: the Keras ``l1_l2`` gradient goes, next to ``LastBlockTrainer``'s set, to the variables of Bottleneck5_0 the
    reference passes a regulariser to (enet_modules.py:1070-1214): ``proj_kernel``, ``proj_alpha``, ``conv_kernel``,
    ``conv_alpha``, ``exp_kernel``, ``res_kernel``, ``residual_alpha``; ``gamma`` / ``beta`` get the plain Adam update.

    The inputs are Bottleneck4_2's output [N, h, w, 64] and ``argmax1`` [N, h, w, 16] int64, the pooling indices of
    Bottleneck1_0 in the reference's per-image form ``(y * 2w + x) * 16 + c`` (``features(images)`` returns both)."""

    _C_FEATURES = ("ssal_train_stage_grad", "ssal_train_stage_grad_semi")
    _C_IMAGES = ("ssal_enet_train_stage", "ssal_enet_train_stage_semi")
    _CHANNELS, _UP = 64, 4
    _LIMIT = ("kernels'", "kernels'")
    _PARTS = LastBlockTrainer._PARTS + (("Bottleneck5_0", _UPSAMPLE16),)

    # ---- arguments, judged on the host ---------------------------------------------------------------------------------------
    def _check_argmax(self, name, feature_channels, index_channels, feature_shape, argmax):
        """the pooling indices ``argmax`` (``name`` in the messages: "argmax1" / "argmax2") as an int64 tensor (on whatever
        device it lives) after the checks: shape [N, h, w, index_channels] next to features [N, h, w, feature_channels], every
        index inside its own 2 x 2 window and channel.  A torch tensor that passed is remembered under its name, so a cached
        one is checked once."""
        import torch
        a = argmax if isinstance(argmax, torch.Tensor) else torch.as_tensor(np.asarray(argmax))
        shape, ch = tuple(feature_shape), index_channels
        if len(shape) != 4 or shape[-1] != feature_channels:
            raise ValueError("features must be [N,h,w,%d] (got %s)" % (feature_channels, shape))
        want = shape[:3] + (ch,)
        if tuple(a.shape) != want:
            raise ValueError("%s must have shape %s (got %s)" % (name, want, tuple(a.shape)))
        if a.dtype != torch.int64:
            if a.dtype.is_floating_point or a.dtype == torch.bool:
                raise ValueError("%s must be an integer tensor (got %s)" % (name, a.dtype))
            a = a.to(torch.int64)
        # name -> (the caller's tensor itself, its version): kept alive, so never confused
        memo = vars(self).setdefault("_argmax_ok", {})
        seen = memo.get(name)
        if not (seen is not None and seen[0] is argmax and seen[1] == argmax._version):
            _, h, w, _ = want
            c = torch.arange(ch, device=a.device).view(1, 1, 1, ch)
            i = torch.arange(h, device=a.device).view(1, h, 1, 1)
            j = torch.arange(w, device=a.device).view(1, 1, w, 1)
            pix = torch.div(a, ch, rounding_mode="floor")
            y, x = torch.div(pix, 2 * w, rounding_mode="floor"), pix % (2 * w)
            ok = (a >= 0) & (a % ch == c) & (torch.div(y, 2, rounding_mode="floor") == i) & \
                 (torch.div(x, 2, rounding_mode="floor") == j)
            if not bool(ok.all()):
                raise ValueError("%s holds %d indices outside their own 2x2 window / channel" % (name, int((~ok).sum())))
            memo[name] = (argmax, argmax._version) if isinstance(argmax, torch.Tensor) else None
        return a

    def _check_inputs(self, inputs):
        return inputs[0], self._check_argmax("argmax1", 64, 16, np.shape(inputs[0]), inputs[1])

    def _check_params(self, params):
        unknown = set(params or {}) - set(self.variable_names)
        lowest = self._PARTS[-1][0]
        frozen = self.net._layer_names[:self.net._layer_names.index(lowest)]
        below = sorted(n for n in unknown if n.split(".")[0] in frozen)
        if below:
            raise NotImplementedError("training below %s is not implemented (got %s)" % (lowest, below))
        return super()._check_params(params)

    @staticmethod
    def _check_workgroups(max_workgroups):
        if int(max_workgroups) < 0:
            raise ValueError("max_workgroups must be >= 0 (got %r)" % (max_workgroups,))
        return int(max_workgroups)

    # ---- gradients -------------------------------------------------------------------------------------------------------
    def gradient_features(self, features4_2, argmax1, labels, mask, params=None, max_workgroups=0, labelled=None,
                          measure=None, threshold=None, features_raw=None, argmax1_raw=None, confusion=None,
                          return_pseudo_pixels=False):
        """(loss float64 [1], {name: gradient}) on the device for Bottleneck4_2's output [N, h, w, 64], the pooling indices
        ``argmax1`` [N, h, w, 16] and labels / mask [N, 4h, 4w].  ``params``: a name -> array mapping that overrides any of
        the 26 variables (the others, and the moving statistics, are the model's).  ``max_workgroups``: 0 = the default,
        min(tiles, 1024); a tuning knob.  No update.  The keywords after it are the semi-supervised ones
        (``SemiSupervisedStageTrainer``)."""
        semi = self._semi_call(features4_2, labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels,
                               features_raw=features_raw, argmax1_raw=argmax1_raw)
        extra = (self._check_workgroups(max_workgroups),)
        return self._gradient((features4_2, argmax1), (features_raw, argmax1_raw), labels, mask, params, semi, confusion,
                              return_pseudo_pixels, extra)

    def features(self, images):
        """(Bottleneck4_2's output [N, H/4, W/4, 64] (a copy), argmax1 [N, H/4, W/4, 16] int64) for ``images``: what
        ``step_features`` and ``gradient_features`` take.  One forward pass of the frozen trunk; the frozen layers never
        change, so the result can be cached across steps."""
        return self._workspace_features(images, "ssal_enet_train_stage_features_offset", 4, 64), self.net.pooling_argmax()[0]

    def step_features(self, features4_2, argmax1, labels, mask, max_workgroups=0, labelled=None, measure=None,
                      threshold=None, features_raw=None, argmax1_raw=None, confusion=None, return_pseudo_pixels=False):
        """one Adam step from cached Bottleneck4_2 features and pooling indices (``features(images)``); returns the loss
        (float64 device scalar) BEFORE the step, as ``sess.run([loss, train_op])`` does"""
        semi = self._semi_call(features4_2, labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels,
                               features_raw=features_raw, argmax1_raw=argmax1_raw)
        extra = (self._check_workgroups(max_workgroups),)
        return self._step_from_features((features4_2, argmax1), (features_raw, argmax1_raw), labels, mask, semi, confusion,
                                        return_pseudo_pixels, extra)

    def step(self, images, labels, mask, max_workgroups=0, labelled=None, measure=None, threshold=None, images_raw=None,
             confusion=None, return_pseudo_pixels=False):
        """one Adam step from images [N, H, W, C] (fp32 or decoded uint8) and labels / mask [N, H, W]: the frozen trunk up
        to Bottleneck4_2, the stage's forward and training kernels, Adam.  Returns the loss (float64 device scalar) before
        the step."""
        semi = self._semi_call(images, labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels,
                               images_raw=images_raw)
        extra = (self._check_workgroups(max_workgroups),)
        return self._step_images(images, images_raw, labels, mask, semi, confusion, return_pseudo_pixels, extra)


# ---- the decoder tail: Bottleneck4_2 + the last stage ------------------------------------------------
class DecoderTailTrainer(LastStageTrainer):
    """Adam on the variables of ENet's decoder tail: the 26 of ``LastStageTrainer`` and ``Bottleneck4_2``'s ``proj_kernel``,
    ``proj_gamma``, ``proj_beta``, ``proj_alpha``, ``conv_kernel``, ``conv_gamma``, ``conv_beta``, ``conv_alpha``,
    ``exp_kernel``, ``exp_gamma``, ``exp_beta`` and ``residual_alpha`` (4 640 floats): the backward pass through a regular
    64-channel bottleneck (1 x 1 projection 64 -> 16, 3 x 3 convolution, 1 x 1 expansion 16 -> 64, identity residual).

    The deviation from the reference is ``LastBlockTrainer``'s: everything below Bottleneck4_2 is frozen and runs with
    ``training=False``; the three trained blocks run in INFERENCE mode (constant moving statistics, never written; no spatial
    dropout; batch-norm ``y = gamma (x - mean) / sqrt(var + 1e-3) + beta`` with ``gamma`` / ``beta`` trainable).

    Regulariser: the Keras ``l1_l2`` gradient goes, next to ``LastStageTrainer``'s set, to the variables of Bottleneck4_2 the
    reference attaches a regulariser to in ``Bottleneck`` (the list of Bottleneck5_1): ``proj_kernel``, ``proj_alpha``,
    ``conv_kernel``, ``conv_alpha``, ``exp_kernel``, ``residual_alpha``; ``gamma`` / ``beta`` get the plain Adam update.

    The inputs are Bottleneck4_1's output [N, h, w, 64] and ``argmax1`` [N, h, w, 16] int64 as ``LastStageTrainer`` takes it
    (``features(images)`` returns both)."""

    _C_FEATURES = ("ssal_train_tail_grad", "ssal_train_tail_grad_semi")
    _C_IMAGES = ("ssal_enet_train_tail", "ssal_enet_train_tail_semi")
    _PARTS = LastStageTrainer._PARTS + (("Bottleneck4_2", _REGULAR64),)

    def gradient_features(self, features4_1, argmax1, labels, mask, params=None, max_workgroups=0, **semi_keywords):
        """(loss float64 [1], {name: gradient}) on the device for Bottleneck4_1's output [N, h, w, 64], the pooling indices
        ``argmax1`` [N, h, w, 16] and labels / mask [N, 4h, 4w]; everything else as ``LastStageTrainer.gradient_features``
        (``features_raw`` of the semi-supervised form is Bottleneck4_1 of the undistorted frames)."""
        return super().gradient_features(features4_1, argmax1, labels, mask, params=params, max_workgroups=max_workgroups,
                                         **semi_keywords)

    def features(self, images):
        """(Bottleneck4_1's output [N, H/4, W/4, 64] (a copy), argmax1 [N, H/4, W/4, 16] int64) for ``images``: what
        ``step_features`` and ``gradient_features`` take.  One forward pass of the frozen trunk."""
        return self._workspace_features(images, "ssal_enet_train_tail_features_offset", 4, 64), self.net.pooling_argmax()[0]

    def step_features(self, features4_1, argmax1, labels, mask, max_workgroups=0, **semi_keywords):
        """one Adam step from cached Bottleneck4_1 features and pooling indices (``features(images)``); returns the loss
        (float64 device scalar) BEFORE the step"""
        return super().step_features(features4_1, argmax1, labels, mask, max_workgroups=max_workgroups, **semi_keywords)


# ---- the deep tail: Bottleneck4_1 + the decoder tail --------------------------------------------------
class DeepTailTrainer(DecoderTailTrainer):
    """Adam on 50 variables: the 38 of ``DecoderTailTrainer``, then ``Bottleneck4_1``'s twelve (``proj_kernel`` ..
    ``residual_alpha``, 4 640 floats).  Bottleneck4_2's backward also yields its input gradient, and the second regular
    64-channel bottleneck is a second launch of the same kernel on it: the regular-bottleneck backward as a chain link.

    The deviation from the reference is ``LastBlockTrainer``'s: everything below Bottleneck4_1 is frozen and runs with
    ``training=False``; the four trained blocks run in INFERENCE mode (constant moving statistics, never written; no spatial
    dropout; batch-norm ``y = gamma (x - mean) / sqrt(var + 1e-3) + beta`` with ``gamma`` / ``beta`` trainable).

    Regulariser: the Keras ``l1_l2`` gradient goes, next to ``DecoderTailTrainer``'s set, to the variables of Bottleneck4_1
    the reference attaches a regulariser to in ``Bottleneck``: ``proj_kernel``, ``proj_alpha``, ``conv_kernel``,
    ``conv_alpha``, ``exp_kernel``, ``residual_alpha``; ``gamma`` / ``beta`` get the plain Adam update.

    The inputs are Bottleneck4_0's output [N, h, w, 64] and ``argmax1`` [N, h, w, 16] int64 as ``LastStageTrainer`` takes it
    (``features(images)`` returns both)."""

    _C_FEATURES = ("ssal_train_tail2_grad", "ssal_train_tail2_grad_semi")
    _C_IMAGES = ("ssal_enet_train_tail2", "ssal_enet_train_tail2_semi")
    _PARTS = DecoderTailTrainer._PARTS + (("Bottleneck4_1", _REGULAR64),)

    def gradient_features(self, features4_0, argmax1, labels, mask, params=None, max_workgroups=0, **semi_keywords):
        """(loss float64 [1], {name: gradient}) on the device for Bottleneck4_0's output [N, h, w, 64], the pooling indices
        ``argmax1`` [N, h, w, 16] and labels / mask [N, 4h, 4w]; everything else as ``LastStageTrainer.gradient_features``
        (``features_raw`` of the semi-supervised form is Bottleneck4_0 of the undistorted frames)."""
        return super().gradient_features(features4_0, argmax1, labels, mask, params=params, max_workgroups=max_workgroups,
                                         **semi_keywords)

    def features(self, images):
        """(Bottleneck4_0's output [N, H/4, W/4, 64], argmax1 [N, H/4, W/4, 16] int64) for ``images``: what
        ``step_features`` and ``gradient_features`` take.  One forward pass of the frozen trunk, whose later layers write over
        Bottleneck4_0's output, and the model's own Bottleneck4_0 on the Bottleneck3_8 endpoint it leaves."""
        net = self.net
        x = net._prepare(images, False)
        net(x, training=False)
        a38 = net.endpoint_outputs[-1][3].clone()
        argmax1, argmax2 = net.pooling_argmax()
        return net.Bottleneck4_0(a38, argmax2, training=False), argmax1

    def step_features(self, features4_0, argmax1, labels, mask, max_workgroups=0, **semi_keywords):
        """one Adam step from cached Bottleneck4_0 features and pooling indices (``features(images)``); returns the loss
        (float64 device scalar) BEFORE the step"""
        return super().step_features(features4_0, argmax1, labels, mask, max_workgroups=max_workgroups, **semi_keywords)


# ---- the decoder: Bottleneck4_0 + the deep tail --------------------------------------------------------
class DecoderTrainer(DeepTailTrainer):
    """Adam on 63 variables: the 50 of ``DeepTailTrainer``, then ``Bottleneck4_0``'s thirteen (``proj_kernel`` ..
    ``residual_alpha``, 18 256 floats): the backward pass through the 128 -> 64 upsampling block that opens the decoder.  The
    trained part is exactly ENet's decoder over a frozen encoder.

    The deviation from the reference is ``LastBlockTrainer``'s: everything below Bottleneck4_0 is frozen and runs with
    ``training=False``; the five trained blocks run in INFERENCE mode (constant moving statistics, never written; no spatial
    dropout; batch-norm ``y = gamma (x - mean) / sqrt(var + 1e-3) + beta`` with ``gamma`` / ``beta`` trainable).  The unpool's
    backward is the gather of the gradient at each element's pooling position; no gradient is produced for Bottleneck3_8's
    output.

    Regulariser: the Keras ``l1_l2`` gradient goes, next to ``DeepTailTrainer``'s set, to the variables of Bottleneck4_0 the
    reference passes a regulariser to in ``BottleneckUpsample``: ``proj_kernel``, ``proj_alpha``, ``conv_kernel``,
    ``conv_alpha``, ``exp_kernel``, ``res_kernel``, ``residual_alpha``; ``gamma`` / ``beta`` get the plain Adam update.

    The inputs are Bottleneck3_8's output [N, h, w, 128], ``argmax2`` [N, h, w, 64] int64, the pooling indices of Bottleneck2_0
    in the reference's per-image form ``(y * 2w + x) * 64 + c`` (``ENet.pooling_argmax()[1]``), and ``argmax1`` [N, 2h, 2w, 16]
    as ``LastStageTrainer`` takes it (``features(images)`` returns the three)."""

    _C_FEATURES = ("ssal_train_decoder_grad", "ssal_train_decoder_grad_semi")
    _C_IMAGES = ("ssal_enet_train_decoder", "ssal_enet_train_decoder_semi")
    _CHANNELS, _UP = 128, 8
    _PARTS = DeepTailTrainer._PARTS + (("Bottleneck4_0", _UPSAMPLE64),)

    # ---- arguments, judged on the host ---------------------------------------------------------------------------------------
    def _check_inputs(self, inputs):
        shape = tuple(np.shape(inputs[0]))
        a2 = self._check_argmax("argmax2", 128, 64, shape, inputs[1])
        return inputs[0], a2, self._check_argmax("argmax1", 64, 16, (shape[0], 2 * shape[1], 2 * shape[2], 64), inputs[2])

    def _raw_host(self, inputs, raw):
        if len({r is None for r in raw}) > 1:
            raise ValueError("features_raw, argmax2_raw and argmax1_raw are given together or not at all (the undistorted "
                             "frame's pooling indices are its own)")
        return super()._raw_host(inputs, raw)

    # ---- gradients and steps -------------------------------------------------------------------------------------------------
    def gradient_features(self, features3_8, argmax2, argmax1, labels, mask, params=None, max_workgroups=0, labelled=None,
                          measure=None, threshold=None, features_raw=None, argmax2_raw=None, argmax1_raw=None,
                          confusion=None, return_pseudo_pixels=False):
        """(loss float64 [1], {name: gradient}) on the device for Bottleneck3_8's output [N, h, w, 128], the pooling indices
        ``argmax2`` [N, h, w, 64] and ``argmax1`` [N, 2h, 2w, 16], and labels / mask [N, 8h, 8w]; everything else as
        ``LastStageTrainer.gradient_features`` (``features_raw`` / ``argmax2_raw`` / ``argmax1_raw`` of the semi-supervised
        form are those of the undistorted frames)."""
        semi = self._semi_call(features3_8, labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels,
                               features_raw=features_raw, argmax2_raw=argmax2_raw, argmax1_raw=argmax1_raw)
        extra = (self._check_workgroups(max_workgroups),)
        return self._gradient((features3_8, argmax2, argmax1), (features_raw, argmax2_raw, argmax1_raw), labels, mask, params,
                              semi, confusion, return_pseudo_pixels, extra)

    def features(self, images):
        """(Bottleneck3_8's output [N, H/8, W/8, 128] (a copy), argmax2 [N, H/8, W/8, 64], argmax1 [N, H/4, W/4, 16], both
        int64) for ``images``: what ``step_features`` and ``gradient_features`` take.  One forward pass of the frozen encoder;
        the frozen layers never change, so the result can be cached across steps."""
        feats = self._workspace_features(images, "ssal_enet_train_decoder_features_offset", 8, 128)
        argmax1, argmax2 = self.net.pooling_argmax()
        return feats, argmax2, argmax1

    def step_features(self, features3_8, argmax2, argmax1, labels, mask, max_workgroups=0, labelled=None, measure=None,
                      threshold=None, features_raw=None, argmax2_raw=None, argmax1_raw=None, confusion=None,
                      return_pseudo_pixels=False):
        """one Adam step from cached Bottleneck3_8 features and pooling indices (``features(images)``); returns the loss
        (float64 device scalar) BEFORE the step"""
        semi = self._semi_call(features3_8, labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels,
                               features_raw=features_raw, argmax2_raw=argmax2_raw, argmax1_raw=argmax1_raw)
        extra = (self._check_workgroups(max_workgroups),)
        return self._step_from_features((features3_8, argmax2, argmax1), (features_raw, argmax2_raw, argmax1_raw), labels, mask,
                                        semi, confusion, return_pseudo_pixels, extra)


# ---- the semi-supervised step of the two deeper trainers ---------------------------------------------
class _SemiKeywords:
    """The semi-supervised keywords of ``FinalLayerTrainer`` (``labelled``, ``measure``, ``threshold``, ``features_raw`` /
    ``images_raw``, ``confusion``, ``return_pseudo_pixels``; meaning, defaults and validation are its ``_semi`` /
    ``_semi_device``) are accepted, not refused: the head kernel builds the targets of an unlabelled image from the logits it
    holds (or reads the packed targets a target-only launch wrote from the undistorted frame), counts the tile's pixels into
    the confusion matrix and the pseudo pixels per image.  With none of the keywords given a call goes through the plain
    entry exactly as the class below it in the MRO does."""

    _semi_keywords = True


class SemiSupervisedBlockTrainer(_SemiKeywords, LastBlockTrainer):
    """``LastBlockTrainer`` with the reference's semi-supervised step (active_learning.py:226-275, 339-342) built into its
    head kernel: ``gradient_features``, ``step_features`` and ``step`` accept ``labelled``, ``measure``, ``threshold``,
    ``features_raw`` / ``images_raw``, ``confusion`` and ``return_pseudo_pixels`` with ``FinalLayerTrainer``'s meaning,
    defaults and validation (the pseudo annotation is that of the logits under the variables being trained).  Loss and the
    13 gradients are bit-identical to ``LastBlockTrainer`` on the composed targets.  ``state`` /
    ``load_state`` are interchangeable with ``LastBlockTrainer``'s."""


class SemiSupervisedStageTrainer(_SemiKeywords, LastStageTrainer):
    """``LastStageTrainer`` with the semi-supervised step built into the head kernel (see ``SemiSupervisedBlockTrainer``);
    the undistorted frame's side of the feature entries is ``features_raw`` [N, h, w, 64] with its own pooling indices
    ``argmax1_raw`` (what ``features(images_raw)`` returns).  Loss and the 26 gradients are bit-identical to
    ``LastStageTrainer`` on the composed targets; ``state`` / ``load_state`` are interchangeable with its."""


class SemiSupervisedTailTrainer(_SemiKeywords, DecoderTailTrainer):
    """``DecoderTailTrainer`` with the semi-supervised step built into the head kernel (see ``SemiSupervisedBlockTrainer``);
    the undistorted frame's side of the feature entries is ``features_raw`` [N, h, w, 64] (Bottleneck4_1) with its own pooling
    indices ``argmax1_raw``.  Loss and the gradients are bit-identical to ``DecoderTailTrainer`` on the composed targets;
    ``state`` / ``load_state`` are interchangeable with its."""


class SemiSupervisedDeepTailTrainer(_SemiKeywords, DeepTailTrainer):
    """``DeepTailTrainer`` with the semi-supervised step built into the head kernel (see ``SemiSupervisedBlockTrainer``);
    the undistorted frame's side of the feature entries is ``features_raw`` [N, h, w, 64] (Bottleneck4_0) with its own pooling
    indices ``argmax1_raw``.  Loss and the gradients are bit-identical to ``DeepTailTrainer`` on the composed targets;
    ``state`` / ``load_state`` are interchangeable with its."""


class SemiSupervisedDecoderTrainer(_SemiKeywords, DecoderTrainer):
    """``DecoderTrainer`` with the semi-supervised step built into the head kernel (see ``SemiSupervisedBlockTrainer``); the
    undistorted frame's side of the feature entries is ``features_raw`` [N, h, w, 128] (Bottleneck3_8) with its own pooling
    indices ``argmax2_raw`` and ``argmax1_raw``.  Loss and the gradients are bit-identical to ``DecoderTrainer`` on the composed
    targets; ``state`` / ``load_state`` are interchangeable with its."""


# ---- ICNet's trainers: a class per depth of ``_icnet_depths.DEPTHS`` --------------------------------------
# ``@_icnet_depth(stem)`` gives a class what its depth's row states: the class attributes the shared code reads and the public
# methods ``gradient_features``, ``features``, ``step_features``, ``step`` (and ``gradient`` where the row has it), whose leading
# parameters are the row's features under their own names.  What a class body still holds is the depth's own.
def _shape(f, unit=None):
    """a feature's shape as a docstring writes it: in the first feature's h x w, or (``unit``: the depth's label up-factor) in
    the frame's H x W"""
    c = "C_in" if f.channels is None else f.channels
    if unit is None:
        m = "" if f.factor == 1 else str(f.factor)
        return "[N, %sh, %sw, %s]" % (m, m, c)
    return "[N, H/%d, W/%d, %s]" % (unit // f.factor, unit // f.factor, c)


def _listed(words):
    return ", ".join(words[:-1]) + " and " + words[-1] if len(words) > 1 else words[0]


def _method(name, lead, optional, target, feature_names, doc):
    """the public method ``name(self, *lead, *optional)`` -- ``optional``: (name, default) pairs; every parameter passable by
    position or by name -- which calls ``self.<target>([the tuple of the parameters feature_names, ]**the others by name)``"""
    P = inspect.Parameter
    sig = inspect.Signature([P(n, P.POSITIONAL_OR_KEYWORD) for n in ("self",) + tuple(lead)]
                            + [P(n, P.POSITIONAL_OR_KEYWORD, default=d) for n, d in optional])

    def method(*args, **kwargs):
        bound = sig.bind(*args, **kwargs)  # (TypeError for a call the signature does not take, as for any method)
        bound.apply_defaults()
        a = bound.arguments
        self = a.pop("self")
        feats = tuple(a.pop(n) for n in feature_names)
        return getattr(self, target)(*((feats,) if feature_names else ()), **a)

    method.__name__, method.__doc__, method.__signature__ = name, doc, sig
    return method


def _public_methods(d, variables, semi):
    """the public methods of depth ``d`` (a row of ``_icnet_depths.DEPTHS``; ``variables``: its packed (layer, attribute,
    regularised) rows) as the plain class has them, or with ``semi`` the semi-supervised one"""
    names = tuple(f.name for f in d.features)
    maps = [f for f in d.features if f.kind == _depths.MAP]
    has_frame = len(maps) < len(d.features)
    layers = list(collections.OrderedDict.fromkeys(layer for layer, _, _ in variables))
    inputs = ", ".join("``%s`` %s%s" % (f.name, _shape(f), " (fp32 or decoded uint8)" if f.kind == _depths.FRAME else "")
                       for f in d.features)
    targets = "labels / mask [N, %dh, %dw]" % (d.up, d.up)
    trunk = "the frozen trunk up to %s, then %s" % (
        _listed(["``%s``" % f.name for f in maps]), _listed(["``%s``" % layer for layer in layers]))
    raw = "``sub12_sum`` of the undistorted frames" if d.parent is None else \
        "the tuple (%s) of the undistorted frames, given whole or not at all" % ", ".join(n + "_raw" for n in names)
    if semi:
        knobs = [("labelled", None), ("measure", None), ("threshold", None), ("features_raw", None), ("confusion", None),
                 ("return_pseudo_pixels", False)]
        knobs_doc = ("  The semi-supervised keywords are those of ``FinalLayerTrainer.gradient_features``: ``labelled`` [N], "
                     "``measure`` / ``threshold`` (defaults: the trainer's), ``features_raw`` (%s), ``confusion`` (int64 [K, K] "
                     "device tensor, added to), ``return_pseudo_pixels`` (appends the int64 [N] counts to the result)." % raw)
        again = ("  The keywords are those of ``gradient_features``; with ``return_pseudo_pixels`` the result is ``(loss, "
                 "pseudo_pixels)``.")
        raw_frames = ("  ``images_raw``: the undistorted frames (same shape and dtype as ``images``) -- the trunk and the trained "
                      "layers run on them first and the pseudo annotation comes from their logits (active_learning.py:231).")
    else:
        knobs = [("labelled", None), ("confusion", None), ("return_pseudo_pixels", False)]
        knobs_doc = again = ("  ``labelled``, ``confusion`` and ``return_pseudo_pixels`` are semi-supervised keywords: refused "
                             "unless left as they are (%s).%s"
                             % (d.noun, "" if d.semi else "  There is no semi-supervised form yet."))
        raw_frames = ""
    image_knobs = [(n, v) for n, v in knobs if n != "features_raw"]
    image_knobs[3:3] = [("images_raw", None)] if semi else []
    mw = ("max_workgroups", 0)
    out = [
        _method("gradient_features", names + ("labels", "mask"), [("params", None), mw] + knobs, "_gradient_from", names,
                "(loss float64 [1], {name: gradient} for ``variable_names``) on the device for %s and %s.  ``params`` overrides "
                "any of the %d tensors; ``max_workgroups``: 0 = the default grids, a tuning knob.  No update.%s"
                % (inputs, targets, len(variables), knobs_doc)),
        _method("features", ("images",), [], "_features", (),
                "%s for ``images`` (%s): what ``step_features`` and ``gradient_features`` take%s.  One forward pass of the frozen "
                "trunk; it never changes, so the result can be cached across steps."
                % (", ".join("``%s`` %s" % (f.name, _shape(f, d.up)) for f in maps), "copies" if len(maps) > 1 else "a copy",
                   " next to the frames" if has_frame else "")),
        _method("step_features", names + ("labels", "mask"), [mw] + knobs, "_step_from", names,
                "one Adam step from cached features (``features(images)``%s): %s and %s.  Returns the loss (float64 device "
                "scalar) BEFORE the step, as ``sess.run([loss, train_op])`` does.%s"
                % (" and the frames" if has_frame else "", inputs, targets, again)),
        _method("step", ("images", "labels", "mask"), [mw] + image_knobs, "_step_from_images", (),
                "one Adam step from images [N, H, W, C] (fp32 or decoded uint8) and labels / mask [N, H, W]: %s on the weights "
                "being trained, their gradient kernels, Adam.  Returns the loss (float64 device scalar) before the step.%s%s"
                % (trunk, raw_frames, again)),
    ]
    if d.image_gradient:
        out.append(_method("gradient", ("images", "labels", "mask"), [("params", None), mw] + image_knobs,
                           "_gradient_from_images", (),
                           "``gradient_features(*features(images), ...)`` through the images entry, ``(loss, {name: gradient})``: "
                           "%s and their gradient kernels, on the host variables overridden by ``params``.  No update.%s"
                           % (trunk, again)))
    return out


def _icnet_depth(stem, semi=False):
    """class decorator: the class is the trainer of depth ``stem`` (``semi``: its semi-supervised form, on the ``_semi`` entries
    next to the plain ones)"""
    d = _depths.DEPTHS[stem]
    assert d.semi or not semi, "depth %s has no semi-supervised entries" % stem

    def describe(cls):
        cls._DEPTH = d
        cls._VARS, cls._STATS = _depths.variables(stem), _depths.stats(stem)  # (layer, attribute[, regularised]), packed order
        cls.variable_names = ["%s.%s" % (layer, attr) for layer, attr, _ in cls._VARS]
        cls._FEATURE_NAMES = tuple(f.name for f in d.features if f.kind == _depths.MAP)  # the endpoints features() returns
        cls._SEMI_NOUN = d.noun                                                          # in the refusal of a semi keyword
        cls._CHANNELS, cls._UP = d.features[0].channels, d.up
        grad, train = "ssal_icnet_%s_grad" % stem, "ssal_icnet_train_%s" % stem
        cls._C_FEATURES = (grad, grad + "_semi" if semi else None)
        cls._C_IMAGES = (train, train + "_semi" if semi else None)
        cls._C_UPDATE = "ssal_icnet_update_%s" % stem
        for m in _public_methods(d, cls._VARS, semi):
            m.__qualname__ = "%s.%s" % (cls.__qualname__, m.__name__)
            setattr(cls, m.__name__, m)
        return cls
    return describe


# ---- ICNet's output layer: conv6_cls over a frozen trunk ------------------------------------------------
_HEAD = _depths.HEAD
_HEAD_NAMES = (_HEAD + ".kernel", _HEAD + ".bias")


@_icnet_depth("head")
class ICNetHeadTrainer(FinalLayerTrainer):
    """Adam on ``net.conv6_cls.kernel`` [1, 1, 128, K] and ``net.conv6_cls.bias`` [K] of an ``ICNet``: the reference's
    ``-r/--reinitialize-output-layer`` slice (active_learning.py:905-909, 461-462) for the second model -- the only weights
    whose shape depends on the class count.  The trunk is frozen and runs with ``training=False`` up to ``sub12_sum``
    [N, H/8, W/8, 128]; the head is the fused 2x bilinear + 1x1 convolution + bias of the forward path (on the weights
    being trained), the loss is ``masked_softmax_cross_entropy`` on its 4x bilinear up-sampling (``conv6_interp``), which is
    evaluated inside the gradient kernel.  Hyper-parameters, Adam, the beta powers and the learning-rate decay are
    ``FinalLayerTrainer``'s; the Keras ``l1_l2`` regulariser goes to the kernel, not to the bias.

    The head travels packed as ``[128 K | K]`` floats (kernel, then bias); ``gradient_features`` returns and ``state`` /
    ``load_state`` use ``{"conv6_cls.kernel": ..., "conv6_cls.bias": ...}``.  The semi-supervised keywords, ``softmax.multiscale``
    and ``weight_reg.glorot_scaling`` are refused."""

    _semi_keywords = False

    @staticmethod
    def _check_model(net):
        from .models.icnet.icnet import ICNet
        if not isinstance(net, ICNet):
            raise NotImplementedError("ICNetHeadTrainer trains ICNet's conv6_cls (got %s; ENet: FinalLayerTrainer)"
                                      % type(net).__name__)

    @classmethod
    def from_params(cls, net, params, decay_steps=None):
        hp = params.get("hyperparams", params)
        if (hp.get("weight_reg", {}) or {}).get("glorot_scaling", False):
            raise NotImplementedError("weight_reg.glorot_scaling: the per-kernel regulariser scaling is not implemented")
        return super().from_params(net, params, decay_steps=decay_steps)

    # ---- the packed head ---------------------------------------------------------------------------------------------------
    def _vars(self):
        if not self.net.built:
            raise RuntimeError("build the model (call it once, or .build(input_shape)) before training")
        layer = getattr(self.net, _HEAD)
        return layer.kernel, layer.bias

    def _split(self):
        return 128 * int(self.net.classes)

    def _pack(self, arrays=None):
        out = np.zeros(129 * int(self.net.classes), np.float32)
        for name, var, lo in zip(_HEAD_NAMES, self._vars(), (0, self._split())):
            a = var.numpy() if arrays is None else arrays[name]
            a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a, dtype=np.float32)
            if a.shape != tuple(var.shape):
                raise ValueError("%s must have shape %s (got %s)" % (name, tuple(var.shape), a.shape))
            out[lo:lo + a.size] = a.reshape(-1)
        return out

    def _unpack(self, packed):
        k, s = int(self.net.classes), self._split()
        return {_HEAD_NAMES[0]: packed[:s].reshape(1, 1, 128, k), _HEAD_NAMES[1]: packed[s:].reshape(k)}

    # FinalLayerTrainer's hooks
    def _kernel_var(self):
        return self._vars()[0]

    def _host_weights(self):
        return self._pack()

    def _zero_state(self):
        return np.zeros(129 * int(self.net.classes), np.float32)

    def _version_key(self):
        return tuple(v.version for v in self._vars())

    def _state_view(self, a):
        return {n: np.array(v) for n, v in self._unpack(np.asarray(a)).items()}

    def _trained_tail(self):
        return 2  # conv6_cls is the last layer: kernel and bias close ``net.variables``

    def _adam_ranges(self):
        s = self._split()
        return ((0, s, True), (s, s + int(self.net.classes), False))

    def _write_back(self, host):
        """the host variables take the new head; a handle that held the weights as they were below the head gets exactly
        these two tensors (``ssal_icnet_update_head``), not the whole weight set"""
        net, s = self.net, self._split()
        kern, bias = self._vars()
        before = tuple(v.version for v in net.variables)
        kern.assign(host[:s].reshape(kern.shape))
        bias.assign(host[s:])
        torch = _lib.require_gpu()
        device = self._dev["w"].device
        with net._state_lock:
            ent = net._handles.get(device.index)
            if ent is not None and ent[1] is not None and ent[1][:-2] == before[:-2]:
                k32, b32 = np.ascontiguousarray(host[:s], np.float32), np.ascontiguousarray(host[s:], np.float32)
                with torch.cuda.device(device):
                    _lib.check(_lib.lib().ssal_icnet_update_head(ent[0], k32.ctypes.data, b32.ctypes.data, _lib.stream_ptr()))
                ent[1] = tuple(v.version for v in net.variables)

    def reinitialize(self, seed=None):
        """``sess.run`` of the output layer's initializers: glorot-uniform kernel drawn from ``seed``, zero bias (the layer's
        defaults); the optimizer state is reset too"""
        self._vars()[1].assign(np.zeros(int(self.net.classes), np.float32))
        super().reinitialize(seed)

    def load_state(self, state):
        for key in ("m", "v"):
            if not isinstance(state[key], dict) or set(state[key]) != set(_HEAD_NAMES):
                raise ValueError("state[%r] must map %s to arrays" % (key, list(_HEAD_NAMES)))
        self._set_state(self._pack(state["m"]), self._pack(state["v"]), state["t"])

    # ---- arguments, judged on the host before any device work -----------------------------------------------------------------
    def _no_semi(self, **kw):
        """``_semi_call``'s refusal for the plain ICNet trainers"""
        for name, value in kw.items():
            if value is not None and value is not False:
                raise NotImplementedError("%s: the semi-supervised step is not implemented for %s" % (name, self._SEMI_NOUN))

    def _features_workspace_bytes(self, query, n, h, w, k, semi, with_raw):
        """a semi call's workspace holds the packed target plane of the undistorted frames when there are any"""
        return query(n, h, w, k, with_raw) if semi else query(n, h, w, k)

    def _check_call(self, batch, up, labels, mask, max_workgroups, channels):
        if self._semi_keywords and (labels is None or mask is None):
            # the planes a semi call may leave out (``_semi`` has judged that) are not looked at
            shape = tuple(np.shape(batch))
            labels = mask = np.zeros((shape[0], up * shape[1], up * shape[2]), np.uint8) if len(shape) == 4 else None
        if int(max_workgroups) < 0:
            raise ValueError("max_workgroups must be >= 0 (got %r)" % (max_workgroups,))
        shape = tuple(np.shape(batch))
        if len(shape) != 4 or (channels is not None and shape[-1] != channels):
            raise ValueError("expected a [N,h,w,%s] batch (got %s)" % (channels or "C", shape))
        dt = str(getattr(batch, "dtype", ""))
        if channels is not None and not ("float" in dt):
            raise ValueError("%s must be a floating-point tensor (got %s)"
                             % (self._DEPTH.features[0].name, dt or type(batch).__name__))
        want = (shape[0], up * shape[1], up * shape[2])
        for name, t in (("labels", labels), ("mask", mask)):
            if tuple(np.shape(t)) != want:
                raise ValueError("%s must have shape %s (got %s)" % (name, want, tuple(np.shape(t))))
        dt = str(getattr(labels, "dtype", ""))
        if "int" not in dt:
            raise ValueError("labels must be an integer tensor (got %s)" % (dt or type(labels).__name__))
        dt = str(getattr(mask, "dtype", ""))
        if not ("float" in dt or "int" in dt or "bool" in dt):
            raise ValueError("mask must be a numeric tensor (got %s)" % (dt or type(mask).__name__))
        return int(max_workgroups)

    def _packed_with(self, params):
        params = dict(params or {})
        unknown = set(params) - set(_HEAD_NAMES)
        if unknown:
            raise ValueError("unknown variables %s (the head is %s)" % (sorted(unknown), list(_HEAD_NAMES)))
        packed = self._pack()
        if params:
            over = self._pack({n: params.get(n, v) for n, v in self._unpack(packed).items()})
            packed = over
        return packed

    def _check_features(self, feats, labels, mask, max_workgroups):
        """the features of a call against the depth's row: the first one with the targets (``_check_call``), then each other
        one's shape -- the first one's by its factor, its channel count -- and type, in entry order"""
        first = self._DEPTH.features[0]
        mw = self._check_call(feats[0], self._UP, labels, mask, max_workgroups, first.channels)
        shape = n, h, w, _ = tuple(np.shape(feats[0]))
        for f, t in zip(self._DEPTH.features[1:], feats[1:]):
            channels, types, kind = f.channels, ("float",), "a floating-point"
            if f.kind == _depths.FRAME:  # the caller's frames: the model's channel count, fp32 or decoded uint8
                self._vars()  # (the model is built)
                channels, types, kind = int(self.net._c_in), ("float", "uint8"), "a floating-point or uint8"
                if channels not in (3, 4):
                    raise ValueError("the high-resolution trainer takes 3 or 4 input channels (the model has %d)" % channels)
            want = (n, f.factor * h, f.factor * w, channels)
            if tuple(np.shape(t)) != want:
                raise ValueError("%s must be %s for %s %s (got %s)" % (f.name, want, first.name, shape, tuple(np.shape(t))))
            dt = str(getattr(t, "dtype", ""))
            if not any(word in dt for word in types):
                raise ValueError("%s must be %s tensor (got %s)" % (f.name, kind, dt or type(t).__name__))
        return mw

    def _check_raw(self, feats, features_raw, semi):
        """``features_raw`` as given -> its members (None: no raw side), judged on the host: the tuple ``features()`` returns"""
        if features_raw is None:
            return None
        names = self._FEATURE_NAMES
        if not isinstance(features_raw, (tuple, list)) or len(features_raw) != len(names) or any(t is None for t in features_raw):
            raise ValueError("features_raw must be the %d tensors features() returns, (%s), given whole or not at all"
                             % (len(names), ", ".join(names)))
        for name, t, f in zip(names, features_raw, feats):
            if tuple(np.shape(t)) != tuple(np.shape(f)):
                raise ValueError("features_raw: %s must have the shape of its counterpart %s (got %s)"
                                 % (name, tuple(np.shape(f)), tuple(np.shape(t))))
        return tuple(features_raw)

    def _extra_c_args(self, batch):
        """the entries' arguments between the loss' knobs and ``max_workgroups``, for a call on ``batch``'s device: none here"""
        return ()

    def _feature_to_device(self, i, t):
        """member ``i`` of ``feats`` / ``features_raw`` as the features entry takes it: a float32 map"""
        return _lib.as_device_f32(t)

    def _feature_c_args(self, xs, xr):
        """``_extra_c_args`` of a features call on the device tensors ``xs`` (``xr``: their raw side, or Nones)"""
        return self._extra_c_args(xs[0])

    # ---- gradients and steps: one path for every depth, plain and semi-supervised -----------------------------------------
    def _feature_call(self, feats, labels, mask, params, step, max_workgroups, labelled=None, measure=None, threshold=None,
                      features_raw=None, confusion=None, return_pseudo_pixels=False):
        """the features entry on the tuple ``feats``: -> (loss [1], packed gradient, pseudo pixels or None, device state or
        None); ``step``: on the weights of the device state, else on the host variables overridden by ``params``.  A plain
        class refuses the semi-supervised keywords here (``_no_semi``); everything is judged before any device work."""
        semi = self._semi_call(feats[0], labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels,
                               features_raw=features_raw)
        mw = self._check_features(feats, labels, mask, max_workgroups)
        raw = self._check_raw(feats, features_raw, semi)
        packed = None if step else self._packed_with(params)
        x = self._feature_to_device(0, feats[0])
        xs = (x,) + tuple(self._feature_to_device(i, t).to(x.device) for i, t in enumerate(feats[1:], 1))
        xr = (None,) * len(xs)
        if semi is not None and raw is not None and any(r is not f for r, f in zip(raw, feats)):
            xr = tuple(self._feature_to_device(i, t).to(x.device) for i, t in enumerate(raw))
        extra = self._feature_c_args(xs, xr) + (mw,)
        dev = self._device_state(x.device) if step else None
        vec = dev["w"] if step else _lib.require_gpu().from_numpy(packed).to(x.device)
        loss, grad, pp = self._grad_call(xs, xr, labels, mask, vec, semi, confusion, return_pseudo_pixels, extra)
        return loss, grad, pp, dev

    def _gradient_from(self, feats, labels, mask, params, max_workgroups, return_pseudo_pixels=False, **semi_kw):
        loss, grad, pp, _ = self._feature_call(feats, labels, mask, params, False, max_workgroups,
                                               return_pseudo_pixels=return_pseudo_pixels, **semi_kw)
        return (loss, self._unpack(grad), pp) if return_pseudo_pixels else (loss, self._unpack(grad))

    def _step_from(self, feats, labels, mask, max_workgroups, return_pseudo_pixels=False, **semi_kw):
        loss, grad, pp, dev = self._feature_call(feats, labels, mask, None, True, max_workgroups,
                                                 return_pseudo_pixels=return_pseudo_pixels, **semi_kw)
        self._apply(dev, grad)
        return (loss[0], pp) if return_pseudo_pixels else loss[0]

    def _step_from_images(self, images, labels, mask, max_workgroups, labelled=None, measure=None, threshold=None,
                          images_raw=None, confusion=None, return_pseudo_pixels=False):
        semi = self._semi_call(images, labels, mask, labelled, measure, threshold, confusion, return_pseudo_pixels)
        mw = self._check_call(images, 1, labels, mask, max_workgroups, None)
        return self._step_images(images, images_raw, labels, mask, semi, confusion, return_pseudo_pixels,
                                 self._extra_c_args(images) + (mw,))

    def _gradient_from_images(self, images, labels, mask, params, max_workgroups, labelled, confusion, return_pseudo_pixels):
        """the images entry on the host variables overridden by ``params``, without the update -> (loss [1], {name: gradient})"""
        semi = self._semi_call(images, labels, mask, labelled, None, None, confusion, return_pseudo_pixels)
        mw = self._check_call(images, 1, labels, mask, max_workgroups, None)
        packed = self._packed_with(params)
        torch = _lib.require_gpu()
        x = self.net._prepare(images, False)
        vec = torch.from_numpy(packed).to(x.device)
        loss, _, dev = self._images_call(x, None, labels, mask, semi, confusion, return_pseudo_pixels,
                                         self._extra_c_args(x) + (mw,), weights=vec)
        with torch.cuda.device(x.device):
            grad = torch.empty_like(dev["grad"])
            grad.copy_(dev["grad"])
        return loss, self._unpack(grad)

    def _features(self, images):
        """copies of the endpoints the features entry takes, after one forward pass (the head's one endpoint comes bare)"""
        self.net(images, training=False)
        out = tuple(self.net.endpoint(name).clone() for name in self._FEATURE_NAMES)
        return out if len(out) > 1 else out[0]


# ---- the semi-supervised step of ICNet's output-layer trainer --------------------------------------------
@_icnet_depth("head", semi=True)
class SemiSupervisedICNetHeadTrainer(_SemiKeywords, ICNetHeadTrainer):
    """``ICNetHeadTrainer`` with the reference's semi-supervised step (active_learning.py:226-275, 339-342) built into its
    gradient kernel: ``gradient_features``, ``step_features`` and ``step`` accept ``labelled``, ``measure``, ``threshold``,
    ``features_raw`` / ``images_raw``, ``confusion`` and ``return_pseudo_pixels`` with ``FinalLayerTrainer``'s meaning, defaults
    and validation (the pseudo annotation is that of the full-resolution logits under the head being trained; with a raw
    side, of the undistorted frames' logits).  Loss, dKernel and dBias are bit-identical to ``ICNetHeadTrainer`` on the
    composed targets; with none of the keywords a call goes through the plain entry.  ``state`` /
    ``load_state`` are interchangeable with ``ICNetHeadTrainer``'s."""

    def _check_raw(self, feats, features_raw, semi):
        """the head's raw side is one tensor, looked at only in a call that is semi-supervised"""
        if semi is None or features_raw is None:
            return None
        if tuple(np.shape(features_raw)) != tuple(np.shape(feats[0])):
            raise ValueError("features_raw must have the shape of sub12_sum %s (got %s)"
                             % (tuple(np.shape(feats[0])), tuple(np.shape(features_raw))))
        return (features_raw,)


# ---- ICNet's last fusion stage: conv_sub2 + conv3_sub1_proj + conv6_cls over a frozen trunk -------------
@_icnet_depth("fusion")
class ICNetFusionTrainer(ICNetHeadTrainer):
    """Adam on ICNet's last cascade-feature-fusion block and its output layer: ``sub12_sum = relu(BN(conv_sub2(resize_2x(
    sub24_sum))) + BN(conv3_sub1_proj(conv3_sub1)))`` (ICNET_SPEC section 4) and ``conv6_cls``, over a trunk frozen below
    them (``training=False`` up to ``sub24_sum`` [N, H/16, W/16, 128] and ``conv3_sub1`` [N, H/8, W/8, 64]; nothing below
    the block gets a gradient).  Batch-norm is inference-mode: ``gamma`` and ``beta`` are trained, the moving mean and
    variance stay frozen.  Hyper-parameters, ``from_params``, Adam, the beta powers and the learning-rate decay are the
    parent's; the Keras ``l1_l2`` regulariser goes to the three kernels only.

    The eight variables travel as one packed float32 vector in the order of ``variable_names``; ``gradient_features``
    returns and ``state`` / ``load_state`` use a dict keyed by those names.  The semi-supervised keywords,
    ``softmax.multiscale`` and ``weight_reg.glorot_scaling`` are refused."""

    _LIMIT = ("kernels'", "kernels'")

    # ---- the packed vector ---------------------------------------------------------------------------------------------------
    def _vars(self):
        if not self.net.built:
            raise RuntimeError("build the model (call it once, or .build(input_shape)) before training")
        return tuple(getattr(getattr(self.net, layer), attr) for layer, attr, _ in self._VARS)

    def _offsets(self):
        """(lo, hi) of every variable in the packed vector"""
        out, lo = [], 0
        for var in self._vars():
            size = int(np.prod(var.shape))
            out.append((lo, lo + size))
            lo += size
        return out

    def _floats(self):
        return self._offsets()[-1][1]

    def _pack(self, arrays=None):
        out = np.zeros(self._floats(), np.float32)
        for name, var, (lo, hi) in zip(self.variable_names, self._vars(), self._offsets()):
            a = var.numpy() if arrays is None else arrays[name]
            a = np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a, dtype=np.float32)
            if a.shape != tuple(var.shape):
                raise ValueError("%s must have shape %s (got %s)" % (name, tuple(var.shape), a.shape))
            out[lo:hi] = a.reshape(-1)
        return out

    def _unpack(self, packed):
        return {name: packed[lo:hi].reshape(tuple(var.shape))
                for name, var, (lo, hi) in zip(self.variable_names, self._vars(), self._offsets())}

    def _kernel_var(self):
        return getattr(self.net, _HEAD).kernel  # what ``reinitialize`` re-draws

    def _zero_state(self):
        return np.zeros(self._floats(), np.float32)

    def _adam_ranges(self):
        return tuple((lo, hi, reg) for (lo, hi), (_, _, reg) in zip(self._offsets(), self._VARS))

    def _stats(self, device):
        """the frozen moving statistics, ``_STATS``' rows concatenated unpadded at their own widths, on the device (pushed again only when one of them changed)"""
        torch = _lib.require_gpu()
        stat_vars = [getattr(getattr(self.net, layer), attr) for layer, attr in self._STATS]
        key = (device, tuple(v.version for v in stat_vars))
        if getattr(self, "_stats_dev", None) is None or self._stats_dev[0] != key:
            host = np.concatenate([np.asarray(v.numpy(), np.float32).reshape(-1) for v in stat_vars])
            self._stats_dev = (key, torch.from_numpy(host).to(device))
        return self._stats_dev[1]

    # ---- the handle: the trained variables are not a tail of ``net.variables`` ---------------------------------------------------
    def _frozen_versions(self, versions):
        """of a ``net.variables``-ordered version tuple, the entries of the variables that are NOT trained"""
        trained = {id(v) for v in self._vars()}
        return tuple(ver for var, ver in zip(self.net.variables, versions) if id(var) not in trained)

    def _handle_reusable(self, ent, versions):
        """a handle entry ``[handle, pushed versions]`` holds every frozen variable as ``versions`` has it"""
        return (ent is not None and ent[1] is not None and len(ent[1]) == len(versions)
                and self._frozen_versions(ent[1]) == self._frozen_versions(versions))

    def _trunk_handle(self):
        torch = _lib.require_gpu()
        net = self.net
        ent = net._handles.get(torch.cuda.current_device())
        if self._handle_reusable(ent, tuple(v.version for v in net.variables)):
            return ent[0]
        return net._sync_handle()

    def _write_back(self, host):
        """the host variables take the new weights; a handle that held the frozen variables as they were gets exactly the
        trained layers (``ssal_icnet_update_fusion`` / ``_cascade``), not the whole weight set"""
        net = self.net
        before = tuple(v.version for v in net.variables)
        for var, (lo, hi) in zip(self._vars(), self._offsets()):
            var.assign(host[lo:hi].reshape(var.shape))
        torch = _lib.require_gpu()
        device = self._dev["w"].device
        with net._state_lock:
            ent = net._handles.get(device.index)
            if self._handle_reusable(ent, before):
                p32 = np.ascontiguousarray(host, np.float32)
                with torch.cuda.device(device):
                    _lib.check(getattr(_lib.lib(), self._C_UPDATE)(ent[0], p32.ctypes.data, _lib.stream_ptr()))
                ent[1] = tuple(v.version for v in net.variables)

    def reinitialize(self, seed=None):
        """``sess.run`` of the output layer's initializers, as the parent does (glorot-uniform ``conv6_cls`` kernel drawn
        from ``seed``, zero bias; the fusion block keeps its weights); all eight Adam slots are reset"""
        getattr(self.net, _HEAD).bias.assign(np.zeros(int(self.net.classes), np.float32))
        FinalLayerTrainer.reinitialize(self, seed)

    def load_state(self, state):
        for key in ("m", "v"):
            if not isinstance(state[key], dict) or set(state[key]) != set(self.variable_names):
                raise ValueError("state[%r] must map %s to arrays" % (key, self.variable_names))
        self._set_state(self._pack(state["m"]), self._pack(state["v"]), state["t"])

    # ---- arguments, judged on the host before any device work -----------------------------------------------------------------
    def _packed_with(self, params):
        params = dict(params or {})
        unknown = set(params) - set(self.variable_names)
        if unknown:
            raise ValueError("unknown variables %s (the trained variables are %s)" % (sorted(unknown), self.variable_names))
        packed = self._pack()
        if params:
            packed = self._pack({n: params.get(n, v) for n, v in self._unpack(packed).items()})
        return packed

    def _extra_c_args(self, batch):
        """the frozen moving statistics, on ``batch``'s device (a host batch: the current device)"""
        torch = _lib.require_gpu()
        device = batch.device if getattr(batch, "is_cuda", False) else torch.device("cuda", torch.cuda.current_device())
        return (_lib.dev_ptr(self._stats(device)),)


# ---- ICNet's whole cascade head: both fusion blocks + conv6_cls over the three frozen branches -----------
@_icnet_depth("cascade")
class ICNetCascadeTrainer(ICNetFusionTrainer):
    """Adam on ICNet's cascade head -- everything ICNET_SPEC section 4 defines: ``sub24_sum = relu(BN(conv_sub4(resize_2x(
    conv5_4_k1))) + BN(conv3_1_sub2_proj(conv3_1)))``, the last fusion block of ``ICNetFusionTrainer`` and ``conv6_cls`` --
    over the three frozen branches (``training=False`` up to ``conv5_4_k1`` [N, H/32, W/32, 256], ``conv3_1`` [N, H/16, W/16,
    256] and ``conv3_sub1`` [N, H/8, W/8, 64]; nothing below them gets a gradient).  Batch-norm, hyper-parameters, Adam and the
    refusals are the parent's; the ``l1_l2`` regulariser goes to the five kernels only.

    The fourteen variables travel as one packed float32 vector in the order of ``variable_names``: the new block's six, then the
    parent's eight in the parent's order."""


# ---- ICNet's high-resolution branch down to the image, with the cascade head ----------------------------
@_icnet_depth("highres")
class ICNetHighResTrainer(ICNetCascadeTrainer):
    """Adam on ICNet's high-resolution branch (ICNET_SPEC section 3) and the cascade head above it: ``conv1_sub1``,
    ``conv2_sub1`` and ``conv3_sub1`` -- three 3 x 3 stride-2 convolutions + batch-norm + ReLU, ``C_in -> 32 -> 32 -> 64`` on
    the full-resolution frame -- then everything ``ICNetCascadeTrainer`` trains.  The two backbone branches stay frozen
    (``training=False`` up to ``conv5_4_k1`` [N, H/32, W/32, 256] and ``conv3_1`` [N, H/16, W/16, 256]) and can be cached
    across steps; the backward pass ends at the frame, which gets no gradient.  Batch-norm, hyper-parameters, Adam and the
    refusals are the parent's; the ``l1_l2`` regulariser goes to the eight kernels only.  ``C_in`` is 3 or 4.

    The 23 variables travel as one packed float32 vector in the order of ``variable_names``: the branch's nine, then the
    parent's fourteen in the parent's order."""

    def _feature_to_device(self, i, t):
        """the frames are the third input: they stay uint8 when they are (the entry converts them as the forward path does)"""
        return _lib.as_device_image(t) if i == 2 else _lib.as_device_f32(t)

    def _feature_c_args(self, xs, xr):
        """the parent's, then the frames' type and channel count: one type for both sides of the call"""
        if xr[2] is not None and xr[2].dtype != xs[2].dtype:
            raise ValueError("features_raw: images_raw must have the dtype of images %s (got %s)" % (xs[2].dtype, xr[2].dtype))
        return self._extra_c_args(xs[0]) + (int(xs[2].dtype == _lib.require_gpu().uint8), int(self.net._c_in))

    def _check_raw(self, feats, features_raw, semi):
        """the parent's on the triple ``(conv5_4_k1_raw, conv3_1_raw, images_raw)``: the frame is this trainer's third feature
        input, so the raw frames come with the raw features; each member is shaped and typed like its counterpart"""
        names = self._FEATURE_NAMES + ("images",)
        if features_raw is None:
            return None
        if not isinstance(features_raw, (tuple, list)) or len(features_raw) != 3 or any(t is None for t in features_raw):
            raise ValueError("features_raw must be the triple (conv5_4_k1_raw, conv3_1_raw, images_raw): features(images_raw) "
                             "and the raw frames, given whole or not at all")
        for name, t, f in zip(names, features_raw, feats):
            if tuple(np.shape(t)) != tuple(np.shape(f)):
                raise ValueError("features_raw: %s must have the shape of its counterpart %s (got %s)"
                                 % (name, tuple(np.shape(f)), tuple(np.shape(t))))
        dt, want = str(getattr(features_raw[2], "dtype", "")), str(getattr(feats[2], "dtype", ""))
        if ("uint8" in dt) != ("uint8" in want) or not ("float" in dt or "uint8" in dt):
            raise ValueError("features_raw: images_raw must have the dtype of images %s (got %s)" % (want, dt or "none"))
        for name, t in zip(names[:2], features_raw[:2]):
            if "float" not in str(getattr(t, "dtype", "")):
                raise ValueError("features_raw: %s must be a floating-point tensor" % name)
        return tuple(features_raw)


# ---- ICNet's pyramid head: conv5_4_k1 over the pyramid-pooling sum, with the cascade head ----------------
@_icnet_depth("pyramid")
class ICNetPyramidTrainer(ICNetCascadeTrainer):
    """Adam on ``conv5_4_k1`` -- the 1 x 1 convolution (1024 -> 256) + batch-norm + ReLU over the pyramid-pooling sum
    ``conv5_3_sum``, the low-resolution branch's only path into the cascade (ICNET_SPEC section 2) -- and the cascade head
    above it: everything ``ICNetCascadeTrainer`` trains.  Frozen (``training=False``): everything up to and including
    ``conv5_3_sum`` [N, H/32, W/32, 1024] (the pyramid pooling and its sum have no parameters), ``conv3_1`` [N, H/16, W/16, 256]
    and ``conv3_sub1`` [N, H/8, W/8, 64]; nothing below them gets a gradient.  Batch-norm, hyper-parameters, Adam and the
    refusals are the parent's; the ``l1_l2`` regulariser goes to the six kernels only.  A sibling of ``ICNetHighResTrainer``:
    both extend the cascade trainer, neither contains the other.

    The 17 variables travel as one packed float32 vector in the order of ``variable_names``: ``conv5_4_k1``'s three, then the
    parent's fourteen in the parent's order.  The semi-supervised keywords are refused."""


# ---- ICNet through its pyramid pooling: conv5_3's increase layer under the pyramid head -----------------
@_icnet_depth("pool")
class ICNetPoolingTrainer(ICNetPyramidTrainer):
    """Adam on ``conv5_3_1x1_increase`` -- the 1 x 1 convolution (256 -> 1024) + batch-norm that, with the identity shortcut
    ``conv5_2`` and a ReLU, closes the backbone's last bottleneck ``conv5_3`` (ICNET_SPEC section 2) -- through the
    parameter-free pyramid pooling ``conv5_3_sum`` above it, and the pyramid head above that: everything
    ``ICNetPyramidTrainer`` trains.  Frozen (``training=False``): everything up to and including ``conv5_3_3x3``
    [N, H/32, W/32, 256] and ``conv5_2`` [N, H/32, W/32, 1024], ``conv3_1`` [N, H/16, W/16, 256] and ``conv3_sub1``
    [N, H/8, W/8, 64]; nothing below them gets a gradient.  Batch-norm, hyper-parameters, Adam and the refusals are the
    parent's; the ``l1_l2`` regulariser goes to the seven kernels only.

    The 20 variables travel as one packed float32 vector in the order of ``variable_names``: the increase layer's three,
    then the parent's seventeen in the parent's order.  The semi-supervised keywords are refused."""


# ---- ICNet's last backbone bottleneck: conv5_3's reduce layer and 3 x 3 under the pooling trainer --------
@_icnet_depth("bneck")
class ICNetBottleneckTrainer(ICNetPoolingTrainer):
    """Adam on the whole of ``conv5_3``, the backbone's last bottleneck (ICNET_SPEC section 2): ``conv5_3_1x1_reduce`` (1 x 1,
    1024 -> 256, batch-norm, ReLU) and ``conv5_3_3x3`` (3 x 3 at dilation 4, 256 -> 256, batch-norm, ReLU) under everything
    ``ICNetPoolingTrainer`` trains.  Frozen (``training=False``): everything up to and including ``conv5_2``
    [N, H/32, W/32, 1024] -- the reduce layer's input and the bottleneck's identity shortcut --, ``conv3_1`` [N, H/16, W/16, 256]
    and ``conv3_sub1`` [N, H/8, W/8, 64]; nothing below them gets a gradient.  Batch-norm, hyper-parameters, Adam and the
    refusals are the parent's; the ``l1_l2`` regulariser goes to the nine kernels only.

    The 26 variables travel as one packed float32 vector in the order of ``variable_names``: the reduce layer's three, the
    3 x 3's three, then the parent's twenty in the parent's order.  The semi-supervised keywords are refused."""


# ---- ICNet through conv5_2: the last bottleneck but one under the bottleneck trainer ----------------------
@_icnet_depth("bneck2")
class ICNetDeepBottleneckTrainer(ICNetBottleneckTrainer):
    """Adam on ``conv5_2`` and ``conv5_3``, the backbone's last two bottlenecks (ICNET_SPEC section 2): ``conv5_2_1x1_reduce``
    (1 x 1, 1024 -> 256), ``conv5_2_3x3`` (3 x 3 at dilation 4, 256 -> 256) and ``conv5_2_1x1_increase`` (1 x 1, 256 -> 1024,
    + ``conv5_1``), each with batch-norm and a ReLU, under everything ``ICNetBottleneckTrainer`` trains.  Frozen
    (``training=False``): everything up to and including ``conv5_1`` [N, H/32, W/32, 1024] -- the block's input and identity
    shortcut --, ``conv3_1`` [N, H/16, W/16, 256] and ``conv3_sub1`` [N, H/8, W/8, 64]; nothing below them gets a gradient.
    Batch-norm, hyper-parameters, Adam and the refusals are the parent's; the ``l1_l2`` regulariser goes to the twelve kernels
    only.

    The 35 variables travel as one packed float32 vector in the order of ``variable_names``: the reduce layer's three, the
    3 x 3's three, the increase layer's three, then the parent's 26 in the parent's order.  The semi-supervised keywords are
    refused."""


# ---- the semi-supervised step of ICNet's fusion and cascade trainers --------------------------------------
@_icnet_depth("fusion", semi=True)
class SemiSupervisedICNetFusionTrainer(_SemiKeywords, ICNetFusionTrainer):
    """``ICNetFusionTrainer`` with the reference's semi-supervised step (active_learning.py:226-275, 339-342) built into the
    head's gradient kernel: ``gradient_features``, ``step_features`` and ``step`` accept ``labelled``, ``measure``,
    ``threshold``, ``features_raw`` / ``images_raw``, ``confusion`` and ``return_pseudo_pixels`` with ``FinalLayerTrainer``'s
    meaning, defaults and validation (the pseudo annotation is that of the full-resolution logits under the variables being
    trained; with a raw side, of the undistorted frames' logits under them).  ``features_raw`` is the tuple ``features()``
    returns for the undistorted frames, given whole or not at all.  Loss and the eight gradients are bit-identical to
    ``ICNetFusionTrainer`` on the composed targets; with none of the keywords a call goes through the
    plain entry.  ``state`` / ``load_state`` are interchangeable with ``ICNetFusionTrainer``'s."""


@_icnet_depth("cascade", semi=True)
class SemiSupervisedICNetCascadeTrainer(_SemiKeywords, ICNetCascadeTrainer):
    """``ICNetCascadeTrainer`` with the semi-supervised step built into the head's gradient kernel (see
    ``SemiSupervisedICNetFusionTrainer``); ``features_raw`` is the three tensors ``features(images_raw)`` returns.  Loss and
    the fourteen gradients are bit-identical to ``ICNetCascadeTrainer`` on the composed targets; ``state`` / ``load_state``
    are interchangeable with its."""


# ---- the semi-supervised step of ICNet's high-resolution trainer -----------------------------------------
@_icnet_depth("highres", semi=True)
class SemiSupervisedICNetHighResTrainer(_SemiKeywords, ICNetHighResTrainer):
    """``ICNetHighResTrainer`` with the semi-supervised step built into the head's gradient kernel (see
    ``SemiSupervisedICNetFusionTrainer``).  ``features_raw`` is the triple ``(conv5_4_k1_raw, conv3_1_raw, images_raw)``:
    ``features(images_raw)`` plus the undistorted frames themselves, because the frame is this trainer's third feature input;
    it is given whole or not at all, each member shaped and typed like its counterpart (the raw frames stay uint8 when they
    are).  With a raw side the branch, both fusion blocks and the head run on the undistorted frames first, under the variables
    being trained.  Loss and the 23 gradients are bit-identical to ``ICNetHighResTrainer`` on the composed targets (DESIGN.md
    section 37); with none of the keywords a call goes through the plain entry.  ``state`` / ``load_state`` are interchangeable
    with ``ICNetHighResTrainer``'s."""


__all__ = ["FinalLayerTrainer", "LastBlockTrainer", "LastStageTrainer", "DecoderTailTrainer", "SemiSupervisedBlockTrainer",
           "SemiSupervisedStageTrainer", "SemiSupervisedTailTrainer", "DeepTailTrainer", "SemiSupervisedDeepTailTrainer",
           "DecoderTrainer", "SemiSupervisedDecoderTrainer", "ICNetHeadTrainer", "SemiSupervisedICNetHeadTrainer",
           "ICNetFusionTrainer", "ICNetCascadeTrainer", "SemiSupervisedICNetFusionTrainer",
           "SemiSupervisedICNetCascadeTrainer", "ICNetHighResTrainer", "SemiSupervisedICNetHighResTrainer",
           "ICNetPyramidTrainer", "ICNetPoolingTrainer", "ICNetBottleneckTrainer",
           "ICNetDeepBottleneckTrainer"]
