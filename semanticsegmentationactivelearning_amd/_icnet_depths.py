"""ICNet's training depths, each described once for the Python side: what ``training``'s ICNet classes
and ``_lib.PROTOTYPES`` read.  The C side has its own table, the ``*Depth`` structs of ``csrc/ssal_icnet_api.hip`` (DESIGN.md
section 38).  Plain data: no behaviour beyond the chaining of rows at the bottom.

A depth trains the layers it ``adds`` and everything its ``parent`` trains; its entries are ``ssal_icnet_<stem>_grad`` (from
features) and ``ssal_icnet_train_<stem>`` (from images), with ``_semi`` forms where ``semi`` is set, and
``ssal_icnet_update_<stem>``.
"""
import collections

MAP, FRAME = "float32 map", "frame"
# one input of the features entry: ``channels`` x (``factor`` times the first input's height and width).  A MAP is a float32
# endpoint of the trunk, which ``features()`` returns; the FRAME is the caller's image batch (``channels`` None: the model's
# C_in, 3 or 4), fp32 or decoded uint8, which it does not return
Feature = collections.namedtuple("Feature", "name channels factor kind")
Depth = collections.namedtuple("Depth", "stem parent features up adds semi noun image_gradient")

_C3_1, _C3_SUB1 = Feature("conv3_1", 256, 2, MAP), Feature("conv3_sub1", 64, 4, MAP)
HEAD = "conv6_cls"  # the one layer with a bias and no batch-norm: (kernel, bias), no moving statistics

#   stem, parent, features in entry order, label pixels per pixel of the first feature, layers added in front of the parent's
#   (packed order), semi-supervised entries exist, the class' noun in the refusal of a semi-supervised keyword,
#   ``gradient(images)`` exists
DEPTHS = collections.OrderedDict((d.stem, d) for d in (
    Depth("head", None, (Feature("sub12_sum", 128, 1, MAP),), 8, (HEAD,), True, "ICNet's output layer", False),
    Depth("fusion", "head", (Feature("sub24_sum", 128, 1, MAP), Feature("conv3_sub1", 64, 2, MAP)), 16,
          ("conv_sub2", "conv3_sub1_proj"), True, "ICNet's fusion trainer", False),
    Depth("cascade", "fusion", (Feature("conv5_4_k1", 256, 1, MAP), _C3_1, _C3_SUB1), 32,
          ("conv_sub4", "conv3_1_sub2_proj"), True, "ICNet's cascade trainer", False),
    Depth("highres", "cascade", (Feature("conv5_4_k1", 256, 1, MAP), _C3_1, Feature("images", None, 32, FRAME)), 32,
          ("conv1_sub1", "conv2_sub1", "conv3_sub1"), True, "ICNet's high-resolution trainer", False),
    Depth("pyramid", "cascade", (Feature("conv5_3_sum", 1024, 1, MAP), _C3_1, _C3_SUB1), 32,
          ("conv5_4_k1",), False, "ICNet's pyramid trainer", True),
    Depth("pool", "pyramid", (Feature("conv5_3_3x3", 256, 1, MAP), Feature("conv5_2", 1024, 1, MAP), _C3_1, _C3_SUB1), 32,
          ("conv5_3_1x1_increase",), False, "ICNet's pooling trainer", True),
    Depth("bneck", "pool", (Feature("conv5_2", 1024, 1, MAP), _C3_1, _C3_SUB1), 32,
          ("conv5_3_1x1_reduce", "conv5_3_3x3"), False, "ICNet's bottleneck trainer", True),
    Depth("bneck2", "bneck", (Feature("conv5_1", 1024, 1, MAP), _C3_1, _C3_SUB1), 32,
          ("conv5_2_1x1_reduce", "conv5_2_3x3", "conv5_2_1x1_increase"), False, "ICNet's deep bottleneck trainer", True),
))


def variables(stem):
    """((layer, attribute, regularised), ...) of the depth's packed vector, in packed order: its own layers' (kernel, gamma,
    beta) triples, then its parent's"""
    d = DEPTHS[stem]
    if d.parent is None:
        return ((HEAD, "kernel", True), (HEAD, "bias", False))
    return tuple((layer, attr, attr == "kernel") for layer in d.adds for attr in ("kernel", "gamma", "beta")) + variables(d.parent)


def stats(stem):
    """((layer, attribute), ...) of the depth's frozen moving statistics: rows of each layer's own width, concatenated
    unpadded in this order"""
    d = DEPTHS[stem]
    if d.parent is None:
        return ()
    return tuple((layer, attr) for layer in d.adds for attr in ("mean", "variance")) + stats(d.parent)
