"""Golden fixture for descriptor matching: the reference's evaluate_fragment_pair
(SPConvNets/datasets/evaluation_3dmatch.py:56-123) run on one synthetic fragment pair -> match_pair.npz (data only).

Run:  python tests/golden/gen_golden_match.py       (needs /root/reference and sklearn; never runs on the GPU box)

The reference module is imported with gen_golden.py's ``sys.modules`` stand-ins (plyfile is absent here); its three file
readers -- pctk.load_ply, read_key_point, read_feature -- are replaced by look-ups into in-memory arrays keyed by the "path"
strings handed to evaluate_fragment_pair.  Everything after the readers is the reference's own code: two sklearn KDTrees,
the mutual mask tgt -> src -> tgt, hom_transform, distances < tau1.

Inputs (seeded): 300 src and 300 tgt keypoints, 64-d unit descriptors.  The two counts are equal because the reference's mutual
mask compares np.arange(n_src) with an array of n_tgt entries (:87) and raises for unequal counts (3DMatch fragments all carry
5000 keypoints); unequal counts are covered by the tests against tests/match_ref.py.  150 tgt descriptors are noisy copies of
distinct src rows (75 of them with their keypoint at the ground-truth place plus 2 cm of noise: inliers; 75 displaced by
0.3-0.6 m: outliers), the other 150 tgt rows are fresh unit vectors at unrelated places.  Asserted before saving: 30-80 % of the tgt
rows are mutual, inliers and outliers both occur, and no matched distance lies within 1e-6 tau1 of tau1 (keypoints are moved
until that holds), so that the inlier decision does not hang on a rounding."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G          # noqa: E402

N_SRC, N_TGT, C, N_COPY, TAU1 = 300, 300, 64, 150, 0.1


def unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def load_reference_evaluation(arrays):
    G.install_reference()
    path = os.path.join(G.REF, "SPConvNets", "datasets", "evaluation_3dmatch.py")
    spec = importlib.util.spec_from_file_location("ref_evaluation_3dmatch", path)
    E = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(E)

    class _Pctk:
        load_ply = staticmethod(lambda p: arrays[p])
    E.pctk = _Pctk
    E.read_key_point = lambda p: arrays[p]
    E.read_feature = lambda p, descriptor_name="ours": arrays[p]
    return E


def make_inputs(rng):
    src_feats = unit(rng.standard_normal((N_SRC, C)))
    copied = rng.choice(N_SRC, N_COPY, replace=False)
    tgt_feats = np.concatenate((unit(src_feats[copied] + 0.05 * rng.standard_normal((N_COPY, C))),
                                unit(rng.standard_normal((N_TGT - N_COPY, C)))))
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    q *= np.sign(np.linalg.det(q))
    gt = np.eye(4)
    gt[:3, :3], gt[:3, 3] = q, rng.uniform(-1, 1, 3)
    src_kp = rng.uniform(0, 2, (N_SRC, 3))
    at_src = src_kp[copied].copy()                                  # where the copies belong, in src coordinates
    at_src[:N_COPY // 2] += 0.02 * rng.standard_normal((N_COPY // 2, 3))
    shift = unit(rng.standard_normal((N_COPY - N_COPY // 2, 3))) * rng.uniform(0.3, 0.6, (N_COPY - N_COPY // 2, 1))
    at_src[N_COPY // 2:] += shift
    at_src = np.concatenate((at_src, rng.uniform(0, 2, (N_TGT - N_COPY, 3))))
    tgt_kp = (at_src - gt[:3, 3]) @ gt[:3, :3]                      # inverse of x -> R x + t
    order = rng.permutation(N_TGT)                                  # copies and strangers interleaved
    return (src_kp.astype(np.float32), tgt_kp[order].astype(np.float32), src_feats.astype(np.float32),
            tgt_feats[order].astype(np.float32), gt)


def main():
    rng = np.random.default_rng(3101)
    src_kp, tgt_kp, src_feats, tgt_feats, gt = make_inputs(rng)
    arrays = {"src.ply": src_kp, "tgt.ply": tgt_kp, "src.kp": np.arange(N_SRC), "tgt.kp": np.arange(N_TGT),
              "src.npy": src_feats, "tgt.npy": tgt_feats}
    E = load_reference_evaluation(arrays)
    sys.path.insert(0, os.path.join(G.ROOT, "tests"))
    import match_ref as M

    for _ in range(20):                                             # move keypoints off the tau1 boundary
        _, _, matches, dist = M.evaluate_fragment_pair(src_kp, tgt_kp, src_feats, tgt_feats, gt, TAU1)
        near = np.abs(dist - TAU1) < 1e-6 * TAU1
        if not near.any():
            break
        tgt_kp[matches[near, 1]] += np.float32(1e-3)
        arrays["tgt.ply"] = tgt_kp
    else:
        raise AssertionError("matched distances stay on the tau1 boundary")

    n_inlier, inlier_ratio, result_log, kpts = E.evaluate_fragment_pair(0, 1, "src.ply", "tgt.ply", "src.kp", "tgt.kp", "src.npy",
                                                                        "tgt.npy", gt, tau1=TAU1, descriptor="ours")
    n_match = int(round(n_inlier / inlier_ratio))
    assert 0.3 * N_TGT <= n_match <= 0.8 * N_TGT, n_match
    assert 0 < n_inlier < n_match, (n_inlier, n_match)
    assert n_match == matches.shape[0] and not (np.abs(dist - TAU1) < 1e-6 * TAU1).any()
    out = os.path.join(HERE, "match_pair.npz")
    np.savez(out, src_kp=src_kp, tgt_kp=tgt_kp, src_feats=src_feats, tgt_feats=tgt_feats, gt=gt, tau1=np.float64(TAU1),
             n_inlier=np.int64(n_inlier), inlier_ratio=np.float64(inlier_ratio), n_match=np.int64(n_match),
             inlier_pairs=np.asarray(kpts, dtype=np.int64))
    print(f"{out}: {os.path.getsize(out)} bytes; {n_match} of {N_TGT} tgt rows mutual, {n_inlier} inliers, "
          f"inlier_ratio {inlier_ratio:.6f}")


if __name__ == "__main__":
    main()
