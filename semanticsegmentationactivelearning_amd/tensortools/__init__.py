"""Mirror of the reference's ``tensortools`` package: the TFRecord front-end of the scoring path
(``input``, ``tfrecord``), the forward value of ``losses`` and the validation ``metrics`` (confusion matrix on the
device, the derived metrics on the host).  checkpoint_manager and the metric summaries are out of scope."""
from . import input, losses, metrics, tfrecord  # noqa: F401
from .input import InputStage, NumpyCapsule, generate_mask  # noqa: F401
from .metrics import Metrics, confusion_mat, create_metrics  # noqa: F401
