"""Golden fixture for the 3DMatch batch stage: the reference's own R_from_euler_np and rotate_point_cloud(pc, R)
(vgtk/vgtk/pc/augmentation.py:16-33, :58-89), RigidMatrix(pose).R (vgtk/vgtk/functional/rotation.py:6-21) and scipy's
KDTree.query_ball_point, called the way its loader calls them (SPConvNets/datasets/match_3dmatch.py:154-177 and :301-354), on
three small fragments -> pair_batch.npz (arrays only).

Run:  python tests/golden/gen_golden_pair_batch.py       (needs the reference checkout gen_golden.py points to; CPU only)

The reference's random parts (np.random.choice for the keypoints and the resampling, np.random.randint for the degrees) cannot be
shared with a counter-based generator, so THE CHOICES, THE DEGREES AND THE SELECTED INDICES ARE TAKEN FROM THE RESTATEMENT
(tests/pair_batch_ref.py) and everything after them is the reference's arithmetic, in fp64 on the fp32 inputs:
  points .. poses    the inputs (pair_batch_ref.golden_inputs: fragment 0 serves both samples)
  choice, deg        the restatement's keypoint choices [B,npt] and Euler degrees [B,2,3]
  member             int8 [B,2,npt,max n]: query_ball_point(keypoint, radius) on a KDTree of the side's fragment, as a mask
  R                  f64 [B,2,3,3]: R_from_euler_np(deg * np.pi / 180.0)
  T                  f64 [B,3,3]: RigidMatrix(poseA).R.T @ RigidMatrix(poseB).R
  idx                the restatement's selection among the members [B,2,npt,n_sample]
  src, tgt           f64 [B,npt,n_sample,3]: rotate_point_cloud(fragment[idx], R rounded to fp32)[0]; zeros where len(members) <= 1
The fp32 in-radius rule and the KD-tree's fp64 rule can only differ at the boundary: the generator asserts that no point lies
within a relative GOLDEN_BOUNDARY of the radius of any chosen keypoint -- a condition on the inputs, checked here."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G          # noqa: E402


def main():
    G.install_reference()
    from scipy.spatial import KDTree
    import vgtk.pc as pctk
    from vgtk.pc.augmentation import R_from_euler_np
    from vgtk.functional.rotation import RigidMatrix
    sys.path.insert(0, os.path.join(G.ROOT, "tests"))
    import pair_batch_ref as Pr

    points, offsets, pairs, corr, corr_offsets, poses = Pr.golden_inputs()
    B, npt, ns, radius = pairs.shape[0], Pr.GOLDEN_NPT, Pr.GOLDEN_NSAMPLE, Pr.GOLDEN_RADIUS
    ref = Pr.fragment_pair_batch(points, offsets, pairs, corr, corr_offsets, poses, ns, npt, radius, seed=Pr.GOLDEN_SEED,
                                 max_degree=Pr.GOLDEN_MAX_DEGREE)
    assert (ref["status"] == 0).all()
    deg = np.array([[Pr.degrees(b, s, npt, Pr.GOLDEN_SEED, Pr.GOLDEN_MAX_DEGREE) for s in (0, 1)] for b in range(B)], dtype=np.int64)
    nmax = int(np.diff(offsets).max())
    member = np.zeros((B, 2, npt, nmax), dtype=np.int8)
    R = np.zeros((B, 2, 3, 3))
    T = np.zeros((B, 3, 3))
    out = {"src": np.zeros((B, npt, ns, 3)), "tgt": np.zeros((B, npt, ns, 3))}
    for b in range(B):
        T[b] = RigidMatrix(poses[pairs[b, 0]]).R.T @ RigidMatrix(poses[pairs[b, 1]]).R
        for s, name in ((0, "src"), (1, "tgt")):
            R[b, s] = R_from_euler_np(deg[b, s] * np.pi / 180.0)
            frag = points[offsets[pairs[b, s]]:offsets[pairs[b, s] + 1]].astype(np.float64)
            tree = KDTree(frag)
            for j in range(npt):
                kpt = corr[corr_offsets[b] + ref["choice"][b, j], s].astype(np.float64)
                d = np.linalg.norm(frag - kpt, axis=1)
                assert (np.abs(d - radius) > Pr.GOLDEN_BOUNDARY * radius).all(), "a point of the fixture lies on the boundary"
                indices = tree.query_ball_point(kpt, radius)
                member[b, s, j, indices] = 1
                if len(indices) > 1:
                    rotated, _ = pctk.rotate_point_cloud(frag[ref["idx"][b, s, j]], ref["R_aug"][b, s].astype(np.float64))
                    out[name][b, j] = rotated
    counts = member.sum(axis=3)
    print("counts", counts.reshape(-1).tolist(), "deg", deg.reshape(-1).tolist())
    assert counts.min() <= 1 < counts.max() and (counts > ns).any() and ((counts > 1) & (counts < ns)).any()
    path = os.path.join(HERE, "pair_batch.npz")
    np.savez_compressed(path, points=points, offsets=offsets, pairs=pairs, corr=corr, corr_offsets=corr_offsets, poses=poses,
                        choice=ref["choice"], deg=deg, member=member, R=R, T=T, idx=ref["idx"], src=out["src"], tgt=out["tgt"])
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
