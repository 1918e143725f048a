"""Golden fixture for the ModelNet batch stage: the reference's own p3dtk.normalize_np (vgtk/vgtk/point3d/normalize.py:30-34),
pctk.rotate_point_cloud(pc, R) (vgtk/vgtk/pc/augmentation.py:58-89), rotation_distance_np and label_relative_rotation_np
(vgtk/vgtk/functional/rotation.py:350-369, :521-526), called the way its loaders call them (SPConvNets/datasets/modelnet40.py:
58-70 and :120-152), on three small clouds -> modelnet_batch.npz (arrays only).

Run:  python tests/golden/gen_golden_modelnet_batch.py       (needs the reference checkout gen_golden.py points to; CPU only)

The reference package is imported with gen_golden.py's ``sys.modules`` stand-ins.  The reference's random parts
(np.random.choice in uniform_resample_np, scipy's Rotation.random) cannot be shared with a counter-based generator, so the
SELECTED INDICES AND R ARE TAKEN FROM THE RESTATEMENT (tests/modelnet_batch_ref.py: select, random_rotation) and everything
after them is the reference's arithmetic, in fp64 on the fp32 inputs:
  points, offsets   the raw clouds (modelnet_batch_ref.golden_clouds: n_b == n_sample, above it, below it)
  idx, R            the restatement's selection (seed GOLDEN_SEED, ids 0..2) and rotations
  plain             normalize_np(pc.T).T of the selected rows
  pc                rotate_point_cloud(plain, R)[0]
  label, res        rotation_distance_np(R, anchors): its arg max and diff_r[label] (what flag == 'rotation' trains on)
  lrr_R, lrr_label  label_relative_rotation_np(anchors, R): the alignment loader's R and R_label"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G          # noqa: E402


def main():
    G.install_reference()
    import vgtk.pc as pctk
    import vgtk.point3d as p3dtk
    from vgtk.functional import rotation_distance_np, label_relative_rotation_np
    import vgtk.so3conv.functional as L
    sys.path.insert(0, os.path.join(G.ROOT, "tests"))
    import modelnet_batch_ref as Mr

    anchors = np.asarray(L.get_anchors(60)).astype(np.float32)
    points, offsets = Mr.golden_clouds()
    B, ns = len(Mr.GOLDEN_SIZES), Mr.GOLDEN_NSAMPLE
    idx = np.stack([Mr.select(int(offsets[c + 1] - offsets[c]), c, ns, Mr.GOLDEN_SEED) for c in range(B)])
    R = np.stack([Mr.random_rotation(c, Mr.GOLDEN_SEED) for c in range(B)])
    plain, pc, label, res, lrr_R, lrr_label = [], [], [], [], [], []
    for c in range(B):
        rows = points[offsets[c]:offsets[c + 1]][idx[c]].astype(np.float64)
        p = p3dtk.normalize_np(rows.T).T
        rotated, R_used = pctk.rotate_point_cloud(p, R[c].astype(np.float64))
        assert np.array_equal(R_used, R[c])
        _, lab, diff_r = rotation_distance_np(R[c].astype(np.float64), anchors)
        rr, rl = label_relative_rotation_np(anchors, R[c].astype(np.float64))
        plain.append(p); pc.append(rotated); label.append(lab); res.append(diff_r[lab]); lrr_R.append(rr); lrr_label.append(rl)
    out = os.path.join(HERE, "modelnet_batch.npz")
    np.savez(out, points=points, offsets=offsets, idx=idx.astype(np.int32), R=R, plain=np.stack(plain), pc=np.stack(pc),
             label=np.asarray(label, dtype=np.int64), res=np.stack(res), lrr_R=np.stack(lrr_R),
             lrr_label=np.stack(lrr_label).astype(np.int64))
    print(f"{out}: {os.path.getsize(out)} bytes; labels {label}, idx[1][:8] {idx[1][:8]}")


if __name__ == "__main__":
    main()
