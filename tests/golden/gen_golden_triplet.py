"""Golden fixture for the descriptor network's training loss: the reference's own TripletBatchLoss (vgtk/vgtk/loss.py:239-445) run
on small seeded inputs -> triplet_loss.npz (arrays only).

Run:  python tests/golden/gen_golden_triplet.py       (needs /root/reference; CPU only, never runs on the GPU box)

The reference package is imported with gen_golden.py's ``sys.modules`` stand-ins; `opt` is a namespace with device = "cpu".
Recorded:
  batch-hard   N = 8, D = 32, unit-norm descriptors, tgt a perturbed src (tests/triplet_ref.py: descriptors, seed 4301), for
               loss_type hard, soft and contrastive with the margins of triplet_ref.margin_for (hard: some rows active, some
               not): the four outputs of forward() with alpha = 0 (that is _forward_invariance), the debug attributes fpos, cneg
               and match_idx, and the autograd gradients of the loss with respect to src and tgt.
  interpolate  _interpolate on nb = 1 inputs -- the only batch size it runs at (loss.py:423-424 raises for nb >= 2) -- for four
               random T, C = 4, A = 60, sigma = 0.2: the output, and the three largest traces and their indices from
               _rotation_distance.
  dist_err     the largest difference between the reference's fp32 expansion-form distance matrix (its all_dist attribute) and
               the fp64 restatement from the differences on these inputs.  MEASURED here when the fixture is written:
               5.69e-07 on these inputs (smallest distance 0.283).  trace_err is the same for the top-3 traces: 2.82e-07.
               Both are stored in the fixture; the tests read them from there.
NOT recorded: _forward_equivariance (it calls _interpolate at the batch size of the descriptors, which raises for N >= 2, and N
= 1 has no negative to mine) and _forward_attention (forward() never calls it; its attention_params are commented out in the
constructor, so it raises AttributeError).  all_dist itself is not recorded: the library never forms it."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G          # noqa: E402


def main():
    G.install_reference()
    from vgtk.loss import TripletBatchLoss
    sys.path.insert(0, os.path.join(G.ROOT, "tests"))
    import triplet_ref as Tf
    import rotation_ref as Rf

    anchors = Rf.anchors_for(60)
    src, tgt = Tf.descriptors(np.random.default_rng(4301), 8, 32)
    out = dict(src=src, tgt=tgt, anchors=anchors)
    dist_ref, _ = Tf.distances(src, tgt)
    dist_err = 0.0
    for mode in Tf.MODES:
        margin = Tf.margin_for(src, tgt, mode)
        opt = types.SimpleNamespace(device="cpu", train_loss=types.SimpleNamespace(loss_type=mode, margin=margin))
        crit = TripletBatchLoss(opt, torch.from_numpy(anchors))
        s, t = torch.from_numpy(src).requires_grad_(), torch.from_numpy(tgt).requires_grad_()
        loss, acc, pos, neg = crit(s, t, None)
        loss.backward()
        dist_err = max(dist_err, float(np.abs(crit.all_dist.detach().numpy().astype(np.float64) - dist_ref).max()))
        out.update({f"{mode}_margin": np.float64(margin),
                    f"{mode}_out": np.array([loss.item(), acc.item(), pos.item(), neg.item()], dtype=np.float32),
                    f"{mode}_fpos": crit.fpos.detach().numpy(), f"{mode}_cneg": crit.cneg.detach().numpy(),
                    f"{mode}_match_idx": crit.match_idx.numpy().astype(np.int64),
                    f"{mode}_dsrc": s.grad.numpy(), f"{mode}_dtgt": t.grad.numpy()})

    rng = np.random.default_rng(4302)
    T = np.ascontiguousarray(Rf.random_rotations(rng, 4).astype(np.float32))
    feature = rng.standard_normal((4, 4, 60)).astype(np.float32)
    opt = types.SimpleNamespace(device="cpu", train_loss=types.SimpleNamespace(loss_type="hard", margin=1.0))
    crit = TripletBatchLoss(opt, torch.from_numpy(anchors))
    outs, tops, idxs = [], [], []
    with torch.no_grad():
        for b in range(4):
            Tb = torch.from_numpy(T[b:b + 1])
            outs.append(crit._interpolate(torch.from_numpy(feature[b:b + 1]), Tb, sigma=Tf.SIGMA).numpy()[0])
            r_anchors = torch.einsum('bij,njk->bnik', Tb.transpose(1, 2), crit.anchors)
            val, idx = crit._rotation_distance(r_anchors, crit.anchors, k=3)
            tops.append(val.numpy()[0])
            idxs.append(idx.numpy()[0])
    tr = np.sort(Tf.traces(T, anchors), axis=2)[:, :, ::-1][:, :, :3]
    trace_err = float(np.abs(np.stack(tops).astype(np.float64) - tr).max())
    out.update(interp_T=T, interp_feature=feature, interp_out=np.stack(outs), interp_top=np.stack(tops),
               interp_idx=np.stack(idxs).astype(np.int64), dist_err=np.float64(dist_err), trace_err=np.float64(trace_err))

    path = os.path.join(HERE, "triplet_loss.npz")
    np.savez(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes; dist_err {dist_err:.3e} (smallest distance {dist_ref.min():.3f}), "
          f"trace_err {trace_err:.3e}; hard out {out['hard_out']}")


if __name__ == "__main__":
    main()
