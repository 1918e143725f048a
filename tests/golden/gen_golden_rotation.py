"""Golden fixture for the rotation-estimation stage: the reference's own label_relative_rotation_np and so3_mean
(vgtk/vgtk/functional/rotation.py:481-526) and acos_safe (vgtk/vgtk/spconv/functional.py:138-143) run on small seeded inputs
-> rotation_decode.npz (arrays only).

Run:  python tests/golden/gen_golden_rotation.py       (needs /root/reference; CPU only, never runs on the GPU box)

The reference package is imported with gen_golden.py's ``sys.modules`` stand-ins.  Recorded, for A = 60 anchors and b = 4:
  labels   label_relative_rotation_np(anchors, T_p) for four random rotations T_p (fp32 inputs, so an fp32 einsum)
  means    so3_mean(Rs, weights) and so3_mean(Rs) on Rs [4,60,3,3]: rotations within about 0.5 rad of a centre per row, so
           that torch.svd in fp32 determines the mean to about 1e-7 (margin near 2)
  acos     acos_safe at x = -1, -1 + 5e-5, 0, 1 - 5e-5, 1 and one fp32 step outside [-1, 1] on either side, on a float64 tensor
           (acos_safe): the reference's code is dtype-agnostic, and in fp64 it is its own formula to 1e-15.  On float32
           tensors (acos_safe_f32, what its trainer feeds it) the same code is up to 2.35e-6 away from that formula at these
           points: its anchor value acos(1 - 1e-4) is taken at fp32(1 - 1e-4), 1.7e-8 off, where acos has slope 70.7, while
           its slope constant is computed in fp64.  The library evaluates the formula in fp64, so the fp64 run is the one the
           tests hold it to within 1e-6; the fp32 run is kept to bound that known difference (3e-6).
NOT recorded: the two rotation maps (compute_rotation_matrix_from_quaternion / _from_ortho6d, rotation.py:379-478).  Both
build their clamp with torch.FloatTensor([1e-8]).cuda() and cannot run without a CUDA device, which this machine does not have;
tests/rotation_ref.py restates their formulas (rotation.py:400-415, :466-477) and they are pinned by that restatement only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G          # noqa: E402


def main():
    G.install_reference()
    import vgtk.functional.rotation as RR
    from vgtk.spconv.functional import acos_safe
    sys.path.insert(0, os.path.join(G.ROOT, "tests"))
    import rotation_ref as Rf

    rng = np.random.default_rng(4201)
    import vgtk.so3conv.functional as L
    anchors = np.asarray(L.get_anchors(60)).astype(np.float32)
    shipped = np.load(os.path.join(G.ROOT, "epn_pointcloud_amd", "vgtk", "data", "so3_anchors60.npy")).astype(np.float32)
    assert np.array_equal(anchors, shipped), "the shipped anchor table is not the reference's"

    T = Rf.random_rotations(rng, 4).astype(np.float32)
    R_target, label = zip(*(RR.label_relative_rotation_np(anchors, t) for t in T))
    R_target, label = np.stack(R_target).astype(np.float32), np.stack(label).astype(np.int64)

    Rs = np.empty((4, 60, 3, 3))
    for p in range(4):
        q = np.concatenate((np.ones((60, 1)), 0.25 * rng.standard_normal((60, 3))), axis=1)
        Rs[p] = Rf.random_rotations(rng, 1)[0] @ Rf.quat_matrix(q)
    Rs = Rs.astype(np.float32)
    weights = rng.uniform(0.05, 1.0, (4, 60)).astype(np.float32)
    mean_w = RR.so3_mean(torch.from_numpy(Rs), torch.from_numpy(weights)).numpy()
    mean_1 = RR.so3_mean(torch.from_numpy(Rs)).numpy()

    one = np.float32(1.0)
    x = np.array([-1.0, -1.0 + 5e-5, 0.0, 1.0 - 5e-5, 1.0, np.nextafter(one, np.float32(2.0)),
                  np.nextafter(-one, np.float32(-2.0))], dtype=np.float64)
    acos = acos_safe(torch.from_numpy(x)).numpy()
    acos_f32 = acos_safe(torch.from_numpy(x.astype(np.float32))).numpy()
    assert acos.dtype == np.float64 and acos_f32.dtype == np.float32

    out = os.path.join(HERE, "rotation_decode.npz")
    np.savez(out, anchors=anchors, T=T, R_target=R_target, label=label, Rs=Rs, weights=weights, mean_weighted=mean_w,
             mean_plain=mean_1, acos_x=x, acos_safe=acos, acos_safe_f32=acos_f32)
    print(f"{out}: {os.path.getsize(out)} bytes; labels {label[0][:6]}..., acos_safe {acos}, "
          f"max |fp32 - fp64| {np.abs(acos_f32 - acos).max():.3e}")


if __name__ == "__main__":
    main()
