"""numpy fp64 restatement of the Adam step of csrc/adam_step.hip (include/epn_so3conv.h, epn_adam_step_f32), used
by test_adam_spec.py and test_gpu_adam.py.  Everything is fp64 on the fp32 inputs, numpy has no fused multiply-add, and every
stored value is rounded once (`.astype(np.float32)`: to nearest, subnormals kept).

The one thing restated loosely is the ORDER of the fp64 sum of squares: numpy's pairwise sum here, the kernel's fixed partition
there.  Both are sums of n non-negative fp64 terms, so each lies within n 2^-53 relative of the exact sum and the two norms within
about n 2^-53 of each other: 1e-10 at a million elements, against the 6e-8 of the fp32 ulp the outputs are held to."""
import numpy as np

SPAN = 1024          # EPN_ADAM_SPAN


class State:
    """p, m, v: flat float32 arrays of one length; counters = [steps_applied, steps_skipped]."""

    def __init__(self, p, m=None, v=None, counters=(0, 0)):
        self.p = np.array(p, dtype=np.float32).ravel()
        self.m = np.zeros_like(self.p) if m is None else np.array(m, dtype=np.float32).ravel()
        self.v = np.zeros_like(self.p) if v is None else np.array(v, dtype=np.float32).ravel()
        self.counters = [int(counters[0]), int(counters[1])]

    def copy(self):
        return State(self.p, self.m, self.v, self.counters)


def clip_factor(norm, max_norm):
    """c of the step: 1 when clipping is off (None, <= 0, +inf); else max_norm / (norm + 1e-6) where that is < 1, else 1 (a NaN
    quotient compares false)."""
    max_norm = 0.0 if max_norm is None else float(max_norm)
    if not (max_norm > 0.0 and max_norm < np.inf):
        return 1.0
    with np.errstate(all="ignore"):
        q = np.float64(max_norm) / (np.float64(norm) + np.float64(1e-6))
    return float(q) if q < 1.0 else 1.0


def step(st, g, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0, max_norm=None):
    """One call of epn_adam_step_f32 on `st` (changed in place) -> info as four fp64 values (norm, c, lr as read, skip); round
    them with np.float32 to compare.  lr is rounded to fp32 first: the kernel reads a float32."""
    g = np.asarray(g, dtype=np.float32).ravel()
    assert g.shape == st.p.shape
    s = np.float64(grad_scale)
    lr32 = np.float64(np.float32(lr))
    with np.errstate(all="ignore"):
        sg = s * g.astype(np.float64)
        sumsq = np.sum(sg * sg)
        norm = np.sqrt(sumsq)
        nonfinite = int((~np.isfinite(g)).sum())
        skip = nonfinite > 0 or not np.isfinite(norm)
        c = clip_factor(norm, max_norm)
        info = [float(norm), c, float(lr32), 1.0 if skip else 0.0]
        if skip:
            st.counters[1] += 1
            return info
        t = np.float64(st.counters[0] + 1)
        b1, b2 = np.float64(beta1), np.float64(beta2)
        bias1, bias2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        step_size, root2 = lr32 / bias1, np.sqrt(bias2)
        sc = s * np.float64(c)
        p = st.p.astype(np.float64)
        gd = sc * g.astype(np.float64) + np.float64(weight_decay) * p
        m = (b1 * st.m.astype(np.float64) + (1.0 - b1) * gd).astype(np.float32)
        v = (b2 * st.v.astype(np.float64) + (1.0 - b2) * (gd * gd)).astype(np.float32)
        den = np.sqrt(v.astype(np.float64)) / root2 + np.float64(eps)
        st.p = (p - step_size * m.astype(np.float64) / den).astype(np.float32)
        st.m, st.v = m, v
        st.counters[0] += 1
    return info


def offsets(lengths):
    out = [0]
    for n in lengths:
        out.append(out[-1] + int(n))
    return out
