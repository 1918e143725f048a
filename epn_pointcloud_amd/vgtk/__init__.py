"""Mirror of the reference package `vgtk` (vgtk/vgtk/__init__.py:1-13), hot-path subset:
functional, point3d, pc, spconv, so3conv, utils, loss (TripletBatchLoss, the 3DMatch trainer's loss, MultiTaskDetectionLoss,
the rotation trainer's, alignment branch, and CrossEntropyLoss / AttentionCrossEntropyLoss, the classification trainer's) and the
extension namespace `cuda`.  pc also carries the device form of the ModelNet loaders' per-sample work (pc.modelnet_batch,
pc.modelnet_alignment_batch: resample, normalise, rotate, label).
Out of scope: app (trainer/logger), transform, mesh, voxel (upstream's package of that name is
empty; the voxel-grid downsampling the reference takes from open3d is pc.voxel_down_sample)."""
from . import cuda  # noqa: F401
from . import functional  # noqa: F401
from . import point3d  # noqa: F401
from . import pc  # noqa: F401
from . import spconv  # noqa: F401
from . import so3conv  # noqa: F401
from . import loss  # noqa: F401
from .utils import batch_gather, batch_zip, LearningRateScheduler  # noqa: F401
from .loss import TripletBatchLoss, MultiTaskDetectionLoss, CrossEntropyLoss, AttentionCrossEntropyLoss  # noqa: F401
