"""Golden fixture for the rotation network's training loss: the reference's own MultiTaskDetectionLoss (vgtk/vgtk/loss.py:94-210),
alignment branch, run on small seeded inputs -> rotation_loss.npz (arrays only).

Run:  python tests/golden/gen_golden_rotation_loss.py       (needs /root/reference; CPU only, never runs on the GPU box)

The reference package is imported with gen_golden.py's ``sys.modules`` stand-ins.  Its two rotation maps build their clamp with
torch.FloatTensor([1e-8]).cuda() (rotation.py:384, :447); for the duration of this script torch.Tensor.cuda returns the tensor
itself, so that line yields the same constant on the host and the reference's code runs unchanged on CPU tensors.
Recorded, for A = 60 anchors, b = 2 pairs and nr = 4 and 6 (inputs: tests/rotation_loss_ref.py: golden_inputs, i.e.
rotation_ref.decode_case(60, 2, nr, 800 + nr) with R_target from label_relative_rotation; pair 0 looks like a trained head's
output, pair 1 is noise):
  q_* / o_*   wts, y, label, R_target, T, the five outputs of forward(wts, label, y, R_target, T) with w = 10 (out: the four
              scalars; err: the angular error per pair) and the autograd gradients of the loss with respect to wts and y.
  fwd_err     the largest difference between the reference's fp32 scalars (loss, cls_loss, w * l2_loss) and the fp64
              restatement on these inputs; grad_err the same for the gradients.  MEASURED here when the fixture is written and
              stored in the fixture; the tests read them from there.  (Printed below; see the fixture for the values.)"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G          # noqa: E402


def main():
    G.install_reference()
    from vgtk.loss import MultiTaskDetectionLoss
    sys.path.insert(0, os.path.join(G.ROOT, "tests"))
    import rotation_loss_ref as Lf

    torch.Tensor.cuda = lambda self, *a, **k: self            # the clamp constant of the rotation maps, on the host
    out = {}
    fwd_err = grad_err = 0.0
    for nr, key in ((4, "q"), (6, "o")):
        wts, y, label, R_target, anchors, T = Lf.golden_inputs(nr)
        crit = MultiTaskDetectionLoss(torch.from_numpy(anchors), nr=nr, w=Lf.W)
        tw, ty = torch.from_numpy(wts).requires_grad_(), torch.from_numpy(y).requires_grad_()
        loss, cls_loss, reg, r_acc, err = crit(tw, torch.from_numpy(label).long(), ty, torch.from_numpy(R_target), torch.from_numpy(T))
        loss.backward()
        scal = np.array([loss.item(), cls_loss.item(), reg.item(), r_acc.item()], dtype=np.float32)
        fwd, (dwts, dy, _, _) = Lf.evaluate(wts, y, label, R_target, 1.0, Lf.W)
        assert scal[3] == np.float32(fwd["scalars"][3])
        fwd_err = max(fwd_err, float(np.abs(scal[:3].astype(np.float64) - fwd["scalars"][:3]).max()))
        grad_err = max(grad_err, float(np.abs(tw.grad.numpy() - dwts).max()), float(np.abs(ty.grad.numpy() - dy).max()))
        out.update({f"{key}_wts": wts, f"{key}_y": y, f"{key}_label": label.astype(np.int64), f"{key}_R_target": R_target,
                    f"{key}_T": T, f"{key}_out": scal, f"{key}_err": err.detach().numpy().astype(np.float32),
                    f"{key}_dwts": tw.grad.numpy(), f"{key}_dy": ty.grad.numpy()})
        print(f"nr = {nr}: out {scal}, err {out[f'{key}_err']}, max |dwts| {np.abs(dwts).max():.3e}, max |dy| {np.abs(dy).max():.3e}")
    out.update(anchors=anchors, w=np.float64(Lf.W), fwd_err=np.float64(fwd_err), grad_err=np.float64(grad_err))
    path = os.path.join(HERE, "rotation_loss.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes; fwd_err {fwd_err:.3e}, grad_err {grad_err:.3e}")


if __name__ == "__main__":
    main()
