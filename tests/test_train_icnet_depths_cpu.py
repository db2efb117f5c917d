"""ICNet's trainers as their depth table describes them, without a GPU: every public method has the
signature it had while each class spelled it out by hand (the table below is read from that source), a docstring that names its
inputs, the packed variables and statistics chain as before, a call binds by position and by name alike, and the first
feature's type refusal names the depth's own first feature."""
import inspect

import numpy as np
import pytest

import semanticsegmentationactivelearning_amd as ssal
from semanticsegmentationactivelearning_amd import _icnet_depths, _lib, training

# ---- the signatures, as the hand-written methods had them: (name, default) after ``self`` ---------------------------------------
E = inspect.Parameter.empty
PLAIN = [("labelled", None), ("confusion", None), ("return_pseudo_pixels", False)]
SEMI_FEATURES = [("labelled", None), ("measure", None), ("threshold", None), ("features_raw", None), ("confusion", None),
                 ("return_pseudo_pixels", False)]
SEMI_IMAGES = [("labelled", None), ("measure", None), ("threshold", None), ("images_raw", None), ("confusion", None),
               ("return_pseudo_pixels", False)]
TARGETS = [("labels", E), ("mask", E)]
PARAMS, MAX_WORKGROUPS = ("params", None), ("max_workgroups", 0)
# class -> (the features entry's inputs in order, semi-supervised class, has ``gradient(images)``)
CLASSES = {
    "ICNetHeadTrainer": (("sub12_sum",), False, False),
    "SemiSupervisedICNetHeadTrainer": (("sub12_sum",), True, False),
    "ICNetFusionTrainer": (("sub24_sum", "conv3_sub1"), False, False),
    "SemiSupervisedICNetFusionTrainer": (("sub24_sum", "conv3_sub1"), True, False),
    "ICNetCascadeTrainer": (("conv5_4_k1", "conv3_1", "conv3_sub1"), False, False),
    "SemiSupervisedICNetCascadeTrainer": (("conv5_4_k1", "conv3_1", "conv3_sub1"), True, False),
    "ICNetHighResTrainer": (("conv5_4_k1", "conv3_1", "images"), False, False),
    "SemiSupervisedICNetHighResTrainer": (("conv5_4_k1", "conv3_1", "images"), True, False),
    "ICNetPyramidTrainer": (("conv5_3_sum", "conv3_1", "conv3_sub1"), False, True),
    "ICNetPoolingTrainer": (("conv5_3_3x3", "conv5_2", "conv3_1", "conv3_sub1"), False, True),
    "ICNetBottleneckTrainer": (("conv5_2", "conv3_1", "conv3_sub1"), False, True),
    "ICNetDeepBottleneckTrainer": (("conv5_1", "conv3_1", "conv3_sub1"), False, True),
}


def _signatures(features, semi, gradient):
    feats = [(name, E) for name in features]
    out = {"gradient_features": feats + TARGETS + [PARAMS, MAX_WORKGROUPS] + (SEMI_FEATURES if semi else PLAIN),
           "features": [("images", E)],
           "step_features": feats + TARGETS + [MAX_WORKGROUPS] + (SEMI_FEATURES if semi else PLAIN),
           "step": [("images", E)] + TARGETS + [MAX_WORKGROUPS] + (SEMI_IMAGES if semi else PLAIN)}
    if gradient:
        out["gradient"] = [("images", E)] + TARGETS + [PARAMS, MAX_WORKGROUPS] + PLAIN
    return out


METHODS = [(cls, method) for cls, spec in CLASSES.items() for method in _signatures(*spec)]


def test_the_table_covers_every_icnet_trainer():
    assert sorted(CLASSES) == sorted(n for n in training.__all__ if "ICNet" in n)
    assert list(_icnet_depths.DEPTHS) == ["head", "fusion", "cascade", "highres", "pyramid", "pool", "bneck", "bneck2"]
    for name, (_, _, gradient) in CLASSES.items():
        assert hasattr(getattr(training, name), "gradient") == gradient, name


@pytest.mark.parametrize("cls,method", METHODS)
def test_signature_is_the_hand_written_one(cls, method):
    want = [("self", E)] + _signatures(*CLASSES[cls])[method]
    params = list(inspect.signature(getattr(getattr(training, cls), method)).parameters.values())
    assert [(p.name, p.default) for p in params] == want
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params)


@pytest.mark.parametrize("cls,method", METHODS)
def test_docstring_names_the_inputs(cls, method):
    fn = getattr(getattr(training, cls), method)
    assert fn.__doc__ and fn.__doc__.strip()
    assert fn.__name__ == method and fn.__qualname__ == "%s.%s" % (cls, method)
    features = CLASSES[cls][0]
    # (``features`` returns the endpoints, not the caller's frames; the images entries take the frames alone)
    named = [f for f in features if f != "images"] if method == "features" else features
    for name in named:
        assert name in fn.__doc__, (cls, method, name)
    if method in ("step", "gradient", "features"):
        assert "images" in fn.__doc__


# ---- the packed variables and statistics, chained from the rows ------------------------------------------------------------------
def _bn(layer):
    return [(layer, "kernel", True), (layer, "gamma", False), (layer, "beta", False)]


HEAD_VARS = [("conv6_cls", "kernel", True), ("conv6_cls", "bias", False)]
BNECK2_LAYERS = ["conv5_2_1x1_reduce", "conv5_2_3x3", "conv5_2_1x1_increase", "conv5_3_1x1_reduce", "conv5_3_3x3",
                 "conv5_3_1x1_increase", "conv5_4_k1", "conv_sub4", "conv3_1_sub2_proj", "conv_sub2", "conv3_sub1_proj"]
BNECK2_VARS = sum((_bn(layer) for layer in BNECK2_LAYERS), []) + HEAD_VARS
PARENT = {"ICNetFusionTrainer": "ICNetHeadTrainer", "ICNetCascadeTrainer": "ICNetFusionTrainer",
          "ICNetHighResTrainer": "ICNetCascadeTrainer", "ICNetPyramidTrainer": "ICNetCascadeTrainer",
          "ICNetPoolingTrainer": "ICNetPyramidTrainer", "ICNetBottleneckTrainer": "ICNetPoolingTrainer",
          "ICNetDeepBottleneckTrainer": "ICNetBottleneckTrainer"}


def test_head_and_deep_bottleneck_variables_written_out():
    head, deep = training.ICNetHeadTrainer, training.ICNetDeepBottleneckTrainer
    assert list(head._VARS) == HEAD_VARS and head._STATS == ()
    assert head.variable_names == ["conv6_cls.kernel", "conv6_cls.bias"] and head._FEATURE_NAMES == ("sub12_sum",)
    assert list(deep._VARS) == BNECK2_VARS and len(BNECK2_VARS) == 35
    assert deep.variable_names == ["%s.%s" % (layer, attr) for layer, attr, _ in BNECK2_VARS]
    assert list(deep._STATS) == [(layer, attr) for layer in BNECK2_LAYERS for attr in ("mean", "variance")]
    assert deep._FEATURE_NAMES == ("conv5_1", "conv3_1", "conv3_sub1")
    assert (deep._C_FEATURES, deep._C_IMAGES, deep._C_UPDATE) == (
        ("ssal_icnet_bneck2_grad", None), ("ssal_icnet_train_bneck2", None), "ssal_icnet_update_bneck2")
    assert (head._CHANNELS, head._UP, deep._CHANNELS, deep._UP) == (128, 8, 1024, 32)


@pytest.mark.parametrize("cls", sorted(PARENT))
def test_a_depth_ends_in_its_parent(cls):
    c, p = getattr(training, cls), getattr(training, PARENT[cls])
    assert issubclass(c, p)
    n = len(c._VARS) - len(p._VARS)
    assert n > 0 and n % 3 == 0 and c._VARS[n:] == p._VARS and c.variable_names[n:] == p.variable_names
    assert all(attr == ("kernel", "gamma", "beta")[i % 3] and reg == (attr == "kernel")
               for i, (_, attr, reg) in enumerate(c._VARS[:n]))
    m = 2 * n // 3
    assert c._STATS[m:] == p._STATS and len(c._STATS) == m + len(p._STATS)
    assert [layer for layer, _ in c._STATS[:m]] == [layer for layer, attr, _ in c._VARS[:n] if attr != "kernel"]
    assert c._SEMI_NOUN != p._SEMI_NOUN


@pytest.mark.parametrize("cls", [c for c, spec in sorted(CLASSES.items()) if spec[1]])
def test_a_semi_supervised_class_shares_its_plain_class_description(cls):
    semi, plain = getattr(training, cls), getattr(training, cls.replace("SemiSupervised", ""))
    assert issubclass(semi, plain) and semi._semi_keywords is True and plain._semi_keywords is False
    for attr in ("_VARS", "_STATS", "variable_names", "_FEATURE_NAMES", "_C_UPDATE", "_CHANNELS", "_UP", "_SEMI_NOUN"):
        assert getattr(semi, attr) == getattr(plain, attr), attr
    assert semi._C_FEATURES == (plain._C_FEATURES[0], plain._C_FEATURES[0] + "_semi") and plain._C_FEATURES[1] is None
    assert semi._C_IMAGES == (plain._C_IMAGES[0], plain._C_IMAGES[0] + "_semi") and plain._C_IMAGES[1] is None
    assert all(name in _lib.PROTOTYPES for name in (semi._C_FEATURES[1] + "_nhwc", semi._C_IMAGES[1] + "_workspace_bytes"))


# ---- calls ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def icnet19():
    net = ssal.ICNet(19)
    net.build((None, None, None, 3))
    return net


def _inputs(cls, n=1, h=1, w=2):
    """host inputs of the class' features entry at the first feature's n x h x w, and its targets"""
    d = getattr(training, cls)._DEPTH
    feats = [np.zeros((n, f.factor * h, f.factor * w, 3 if f.channels is None else f.channels), np.float32) for f in d.features]
    return feats, np.zeros((n, d.up * h, d.up * w), np.uint8), np.ones((n, d.up * h, d.up * w), np.float32)


@pytest.mark.parametrize("cls", [c for c, spec in sorted(CLASSES.items()) if len(spec[0]) > 1])
def test_positional_and_keyword_calls_bind_alike(cls, icnet19, monkeypatch):
    def no_gpu():
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    tr = getattr(training, cls)(icnet19, 1e-3)
    feats, labels, mask = _inputs(cls)
    feats[1] = feats[1][:, :, :1]  # the second feature is not the first one's multiple
    with pytest.raises(ValueError) as by_position:
        tr.gradient_features(*feats, labels, mask, None, 2)
    with pytest.raises(ValueError) as by_name:
        tr.gradient_features(*feats, labels=labels, mask=mask, max_workgroups=2, params=None)
    assert str(by_position.value) == str(by_name.value)
    second, first = CLASSES[cls][0][1], CLASSES[cls][0][0]
    assert str(by_name.value).startswith("%s must be " % second) and " for %s " % first in str(by_name.value)
    # ... and everything by name, in another order; max_workgroups is judged before the features
    kw = dict(zip(CLASSES[cls][0], feats), mask=mask, labels=labels)
    with pytest.raises(ValueError, match="max_workgroups must be >= 0"):
        tr.gradient_features(max_workgroups=-1, **kw)
    with pytest.raises(ValueError, match="max_workgroups must be >= 0"):
        tr.step_features(*feats, labels, mask, -1)
    with pytest.raises(TypeError):
        tr.gradient_features(*feats, labels, mask, None, 2, None, None, None, None, None, None, None)  # too many
    with pytest.raises(TypeError):
        tr.step_features(*feats, labels, mask, params=None)  # ``step_features`` has no ``params``


def test_a_plain_class_does_not_take_the_semi_supervised_parameters(icnet19):
    tr = training.ICNetCascadeTrainer(icnet19, 1e-3)
    feats, labels, mask = _inputs("ICNetCascadeTrainer")
    for kw in ({"measure": "entropy"}, {"threshold": 0.5}, {"features_raw": tuple(feats)}):
        with pytest.raises(TypeError):
            tr.gradient_features(*feats, labels, mask, **kw)
    with pytest.raises(TypeError):
        tr.step(np.zeros((1, 32, 64, 3), np.float32), labels, mask, images_raw=None)


def test_the_type_refusal_names_the_depths_own_first_feature(icnet19, monkeypatch):
    def no_gpu():
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    tr = training.ICNetBottleneckTrainer(icnet19, 1e-3)
    feats, labels, mask = _inputs("ICNetBottleneckTrainer")
    with pytest.raises(ValueError, match=r"^conv5_2 must be a floating-point tensor \(got int32\)$"):
        tr.gradient_features(feats[0].astype(np.int32), feats[1], feats[2], labels, mask)
    for cls in sorted(CLASSES):
        tr = getattr(training, cls)(icnet19, 1e-3)
        feats, labels, mask = _inputs(cls)
        with pytest.raises(ValueError, match="^%s must be a floating-point tensor" % CLASSES[cls][0][0]):
            tr.step_features(feats[0].astype(np.uint8), *feats[1:], labels, mask)
