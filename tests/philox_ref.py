"""numpy restatement of the dropout mask of the block-glue kernels (csrc/glue.hip), independent of the kernels.

Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants).  An element at
flat channels-last offset e of a [b, c, p, a] tensor is DROPPED iff

    Philox4x32-10(counter = {lo32(e >> 2), hi32(e >> 2), lo32(call), hi32(call)}, key = {lo32(seed), hi32(seed)})[e & 3]
        < floor(rate * 2^32)

so the mask is a function of (seed, call, e, rate) alone."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of 32-bit words, key: 2 ints -> 4 uint32 arrays."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & _MASK32 for w in counter]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK32,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [w.astype(np.uint32) for w in c]


def threshold(rate):
    return int(math.floor(float(rate) * 4294967296.0))


def keep_mask_flat(numel, rate, seed, call):
    """bool[numel]: True where the element at flat offset e is KEPT."""
    seed, call = int(seed) & (2 ** 64 - 1), int(call) & (2 ** 64 - 1)
    q = np.arange((numel + 3) // 4, dtype=np.uint64)
    words = philox4x32_10([q & _MASK32, q >> np.uint64(32), call & 0xFFFFFFFF, call >> 32], [seed & 0xFFFFFFFF, seed >> 32])
    flat = np.stack(words, axis=1).reshape(-1)[:numel]
    return flat >= np.uint32(threshold(rate)) if threshold(rate) < 2 ** 32 else np.zeros(numel, dtype=bool)


def keep_mask(b, c, p, a, rate, seed, call):
    """Logical [b, c, p, a] bool array (True = kept) of a channels-last tensor: e = ((b_i*p + p_i)*a + a_i)*c + ch."""
    return np.ascontiguousarray(keep_mask_flat(b * c * p * a, rate, seed, call).reshape(b, p, a, c).transpose(0, 3, 1, 2))


# ---- the mask statistics that tests/test_gpu_dropout.py asserts on the kernels' masks (and tests/test_dropout_cpu.py on this
# restatement, for the same fixed seed)
STAT_SHAPE = (3, 64, 37, 60)
STAT_RATE = 0.3
STAT_SEED = (1 << 40) + 2913


def mask_statistics_failures(keep_of_call, shape, rate):
    """keep_of_call(k) -> logical [b, c, p, a] bool array (True = kept) of call k.  Checks, each within 5 sigma of a binomial
    with its own n: the overall kept fraction against 1 - rate, every channel's kept fraction against 1 - rate, and the
    fraction on which calls 0 and 1 agree against rate^2 + (1 - rate)^2.  Returns the list of violated bounds."""
    b, c, p, a = shape
    k0, k1 = np.asarray(keep_of_call(0)), np.asarray(keep_of_call(1))
    out = []
    n = k0.size
    sigma = math.sqrt(rate * (1 - rate) / n)
    if abs(k0.mean() - (1 - rate)) > 5 * sigma:
        out.append(("overall", float(k0.mean()), 1 - rate, 5 * sigma))
    n_c = b * p * a
    sigma_c = math.sqrt(rate * (1 - rate) / n_c)
    per_c = k0.transpose(1, 0, 2, 3).reshape(c, -1).mean(axis=1)
    for ch in np.nonzero(np.abs(per_c - (1 - rate)) > 5 * sigma_c)[0]:
        out.append((f"channel {ch}", float(per_c[ch]), 1 - rate, 5 * sigma_c))
    q = rate * rate + (1 - rate) * (1 - rate)
    sigma_q = math.sqrt(q * (1 - q) / n)
    agree = float((k0 == k1).mean())
    if abs(agree - q) > 5 * sigma_q:
        out.append(("agreement of two calls", agree, q, 5 * sigma_q))
    return out
