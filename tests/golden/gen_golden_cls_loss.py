"""Golden fixture for the classification network's training loss: the reference's own CrossEntropyLoss and
AttentionCrossEntropyLoss (vgtk/vgtk/loss.py:18-75), run on small seeded inputs -> cls_loss.npz (arrays only).

Run:  python tests/golden/gen_golden_cls_loss.py       (needs /root/reference; CPU only, never runs on the GPU box)

The reference package is imported with gen_golden.py's ``sys.modules`` stand-ins.  Recorded, for the three input sets of
tests/cls_loss_ref.py: golden_inputs -- "a": pred [6,40] with wts [6,60] and rlabel [6], the shipped trainer's layout; "b": wts
[6,40,60] with rlabel [6,60], the slice path; "c": wts [3,70,12] with rlabel [3,60], the repeat path:
  {key}_pred, _label, _wts, _rlabel   the inputs
  {key}_ce                            CrossEntropyLoss()(pred, label): (loss, acc), with {key}_ce_dpred its gradient
  {key}_{type}_{counter}_out          the five outputs of AttentionCrossEntropyLoss(type, 0.5) in training mode with iter_counter
                                      set to 0, 1000 and 2500 before the call (pretrain_step = 2000), for 'schedule', 'default'
                                      and 'no_reg'; _dpred and _dwts the autograd gradients of the loss (zeros where autograd
                                      returns None: 'no_reg' does for wts), _counter the counter after the call
  fwd_err     the largest difference between the reference's fp32 loss values (loss, cls_loss, r_loss) and the fp64 restatement
              on these inputs; grad_err the same for the gradients.  MEASURED here when the fixture is written and stored in the
              fixture; the tests read them from there.  (Printed below; see the fixture for the values.)"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G          # noqa: E402


def main():
    G.install_reference()
    from vgtk.loss import AttentionCrossEntropyLoss, CrossEntropyLoss
    sys.path.insert(0, os.path.join(G.ROOT, "tests"))
    import cls_loss_ref as Cf

    out = {}
    fwd_err = grad_err = 0.0
    for key in "abc":
        pred, label, wts, rlabel = Cf.golden_inputs(key)
        out.update({f"{key}_pred": pred, f"{key}_label": label, f"{key}_wts": wts, f"{key}_rlabel": rlabel})
        lab2 = Cf.expand_rlabel(wts, rlabel) if wts.ndim == 3 else rlabel
        tp = torch.from_numpy(pred).requires_grad_()
        loss, acc = CrossEntropyLoss()(tp, torch.from_numpy(label))
        loss.backward()
        ref = Cf.forward(pred, label)
        assert np.float32(ref["scalars"][3]) == np.float32(acc.item())
        fwd_err = max(fwd_err, abs(float(loss.item()) - ref["scalars"][1]))
        grad_err = max(grad_err, float(np.abs(tp.grad.numpy() - Cf.backward(1.0, pred, label)[0]).max()))
        out[f"{key}_ce"] = np.array([loss.item(), acc.item()], dtype=np.float32)
        out[f"{key}_ce_dpred"] = tp.grad.numpy()
        for loss_type, m in Cf.GOLDEN_TYPES:
            for counter in Cf.GOLDEN_COUNTERS:
                crit = AttentionCrossEntropyLoss(loss_type, m).train()
                crit.iter_counter = counter
                tp, tw = torch.from_numpy(pred).requires_grad_(), torch.from_numpy(wts).requires_grad_()
                res = crit(tp, torch.from_numpy(label), tw, torch.from_numpy(rlabel), 2000)
                res[0].backward()
                scal = np.array([r.item() for r in res], dtype=np.float32)
                dwts = np.zeros_like(wts) if tw.grad is None else tw.grad.numpy()
                coef = Cf.schedule_coefficients(loss_type, m, counter)
                ref = Cf.forward(pred, label, wts, lab2, coef)
                dpred, datt = Cf.backward(1.0, pred, label, wts, lab2, coef)
                assert np.array_equal(scal[3:], ref["scalars"][3:].astype(np.float32)) and crit.iter_counter == counter + 1
                fwd_err = max(fwd_err, float(np.abs(scal[:3].astype(np.float64) - ref["scalars"][:3]).max()))
                grad_err = max(grad_err, float(np.abs(tp.grad.numpy() - dpred).max()), float(np.abs(dwts - datt).max()))
                tag = f"{key}_{loss_type}_{counter}"
                out.update({f"{tag}_out": scal, f"{tag}_dpred": tp.grad.numpy(), f"{tag}_dwts": dwts,
                            f"{tag}_counter": np.int64(crit.iter_counter)})
                print(f"{tag}: out {scal}, max |dpred| {np.abs(dpred).max():.3e}, max |dwts| {np.abs(dwts).max():.3e}")
    out.update(margin=np.float64(Cf.GOLDEN_TYPES[0][1]), fwd_err=np.float64(fwd_err), grad_err=np.float64(grad_err))
    path = os.path.join(HERE, "cls_loss.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes; fwd_err {fwd_err:.3e}, grad_err {grad_err:.3e}")


if __name__ == "__main__":
    main()
