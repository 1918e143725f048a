"""epn_pointcloud_amd -- MI355X-native hot path of EPN's SE(3) separable point convolution.

Holds only what the path needs:
  csrc/      hand-written HIP kernels for gfx950 + the C ABI (include/epn_so3conv.h)
  _lib.py    ctypes binding on torch device tensors (no CPU / eager fallback)
  vgtk/      host-side mirror of the reference's `vgtk` operator / nn.Module API for this path
  ops.py     autograd Functions over the C ABI (channels-last feature tensors)
  matching.py  descriptor matching, the 3DMatch inlier ratio / recall and pairwise registration on the device (after models.describe)
  alignment.py  rotation decode, chordal mean and angular error on the device (after RegSO3ConvModel.forward)
  classification.py  the classification trainer's evaluation loop on the device (after ClsSO3ConvModel.forward)
  optim.py   the trainers' optimiser on the device: Adam over all parameters in two launches (after backward)
  data.py    training batches on the device: ModelNet (resample, normalise, rotate, label) and 3DMatch (keypoint pairs, patches,
             augmentation), before the models' forward

`install_vgtk_alias()` registers the mirror under the reference's import names (`vgtk`,
`vgtk.spconv`, `vgtk.so3conv`, `vgtk.cuda.grouping`, ...) so SPConvNets-style code imports unchanged.
"""
import sys

__version__ = "0.1.0"


def install_vgtk_alias():
    """Make `import vgtk`, `import vgtk.spconv as zptk`, `import vgtk.so3conv as sptk` resolve here."""
    from . import vgtk as _v
    prefix = _v.__name__
    for name, mod in list(sys.modules.items()):
        if name == prefix or name.startswith(prefix + "."):
            sys.modules["vgtk" + name[len(prefix):]] = mod
    return _v


_MATCHING = ("match_descriptors", "evaluate_fragment_pair", "evaluate_scene", "register_scene", "register_fragment_pair",
             "registration_errors", "registration_recall", "RegistrationResult", "refine_registration", "refine_scene", "IcpResult")
_ALIGNMENT = ("decode_rotation", "evaluate_alignment")
_DATA = ("pack_clouds", "modelnet_batch", "modelnet_alignment_batch", "ModelNetBatch", "pack_correspondences",
         "fragment_pair_batch", "FragmentPairBatch")
_CLASSIFICATION = ("evaluate_classification",)
_OPTIM = ("FlatAdam",)


def __getattr__(name):
    """`epn_pointcloud_amd.match_descriptors` / `.evaluate_fragment_pair` / `.evaluate_scene` / `.register_scene` /
    `.register_fragment_pair` / `.registration_errors` / `.registration_recall` / `.refine_registration` / `.refine_scene`
    (matching.py) and
    `.decode_rotation` / `.evaluate_alignment` (alignment.py) and `.pack_clouds` / `.modelnet_batch` /
    `.modelnet_alignment_batch` / `.pack_correspondences` / `.fragment_pair_batch` (data.py) and `.evaluate_classification` (classification.py) and `.FlatAdam` (optim.py), resolved on first use so that importing the package -- the
    build recipe does -- still needs no torch."""
    if name in _MATCHING:
        from . import matching
        return getattr(matching, name)
    if name in _ALIGNMENT:
        from . import alignment
        return getattr(alignment, name)
    if name in _DATA:
        from . import data
        return getattr(data, name)
    if name in _CLASSIFICATION:
        from . import classification
        return getattr(classification, name)
    if name in _OPTIM:
        from . import optim
        return getattr(optim, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
