"""numpy fp64 restatement of the classification loss and the evaluation tallies (include/epn_so3conv.h: epn_cls_loss_f32,
epn_cls_loss_bwd_f32, epn_cls_tally_i32) and the case tables of tests/test_cls_loss_spec.py and tests/test_gpu_cls_loss.py.

Everything is computed in fp64 from the fp32 inputs and left unrounded, except where the specification itself rounds: the
scalars are means of the per-row values ROUNDED to fp32.  The inputs of every case are built so that the restatement alone is
unambiguous: the two largest values of a row are either bitwise equal (a built tie) or at least GAP = 1e-3 apart."""
import numpy as np

FLAG_BAD_LABEL, FLAG_NONFINITE = 1, 2
GAP = 1e-3
WIDTHS = (1, 2, 40, 60, 63, 64, 65, 130, 4096)              # class widths n
ROWS = (1, 2, 5, 33, 257)
CHANNELS = (3, 60, 70)                                      # C of the [B,C,A] layout: below, at and above rlabel's 60 columns
UPSTREAM = 1.0


# ----------------------------------------------------------------------------------------------- the specification
def rows_forward(x, label):
    """x f32 [R,n], label int [R] -> (row_ce f64 [R] unrounded, pred int32 [R], flags int32 [R])."""
    x64 = np.asarray(x, dtype=np.float64)
    R, n = x64.shape
    label = np.asarray(label).astype(np.int64)
    finite = np.isfinite(x64).all(axis=1)
    in_range = (label >= 0) & (label < n)
    safe = np.where(finite[:, None], x64, 0.0)
    m = safe.max(axis=1)
    pred = safe.argmax(axis=1).astype(np.int32)              # numpy: the first (lowest) index of the maximum
    s = np.exp(safe - m[:, None]).sum(axis=1)
    xl = safe[np.arange(R), np.where(in_range, label, 0)]
    ce = (m - xl) + np.log(s)
    ce = np.where(finite, ce, np.nan)
    ce = np.where(in_range, ce, 0.0)
    flags = (~in_range * FLAG_BAD_LABEL + ~finite * FLAG_NONFINITE).astype(np.int32)
    return ce, np.where(finite, pred, -1).astype(np.int32), flags


def rows_backward(c, x, label):
    """c: g * coef / rows, already formed -> dx f64 [R,n]."""
    x64 = np.asarray(x, dtype=np.float64)
    R, n = x64.shape
    label = np.asarray(label).astype(np.int64)
    finite = np.isfinite(x64).all(axis=1)
    in_range = (label >= 0) & (label < n)
    safe = np.where(finite[:, None], x64, 0.0)
    e = np.exp(safe - safe.max(axis=1)[:, None])
    p = e / e.sum(axis=1)[:, None]
    onehot = np.arange(n)[None, :] == label[:, None]
    d = c * (p - onehot)
    d = np.where(finite[:, None], d, np.nan)
    return np.where(in_range[:, None], d, 0.0)


def flatten_attention(att, att_label):
    """The two layouts of wts -> (rows f32 [R,A], labels [R]): [B,A] with [B]; [B,C,A] with [B,C] (row b C + c)."""
    att = np.asarray(att)
    return att.reshape(-1, att.shape[-1]), np.asarray(att_label).reshape(-1)


def expand_rlabel(wts, rlabel):
    """AttentionCrossEntropyLoss.forward's label handling for the [B,C,A] layout (vgtk/vgtk/loss.py:48-53): rlabel [B,60] cut to
    [:, :C], or tiled ten times first when C exceeds its width."""
    C = wts.shape[1]
    return rlabel[:, :C] if C <= rlabel.shape[1] else np.tile(rlabel, (1, 10))[:, :C]


def forward(logits, label, att=None, att_label=None, coef=(1.0, 1.0)):
    """-> dict: row_ce, preds, row_flags (class set), att_row_ce, att_preds, att_row_flags (None without attention), scalars f64
    [5] = (loss, cls_loss, att_loss, acc, att_acc) from the ROUNDED rows."""
    out = {}
    c = [float(np.float32(v)) for v in coef]
    ce, pred, fl = rows_forward(logits, label)
    out.update(row_ce=ce, preds=pred, row_flags=fl)
    B = len(ce)
    with np.errstate(invalid="ignore"):
        cls = ce.astype(np.float32).astype(np.float64).sum() / B
    acc = float(((pred == np.asarray(label)) & (pred >= 0)).sum()) / B
    att_loss = att_acc = 0.0
    loss = c[0] * cls
    out.update(att_row_ce=None, att_preds=None, att_row_flags=None)
    if att is not None:
        a2, l2 = flatten_attention(att, att_label)
        ce2, pred2, fl2 = rows_forward(a2, l2)
        R = len(ce2)
        att_loss = ce2.astype(np.float32).astype(np.float64).sum() / R
        att_acc = float(((pred2 == l2) & (pred2 >= 0)).sum()) / R
        loss = loss + c[1] * att_loss
        shape = np.asarray(att).shape[:-1]
        out.update(att_row_ce=ce2.reshape(shape), att_preds=pred2.reshape(shape), att_row_flags=fl2.reshape(shape))
    out["scalars"] = np.array([loss, cls, att_loss, acc, att_acc], dtype=np.float64)
    return out


def backward(g, logits, label, att=None, att_label=None, coef=(1.0, 1.0)):
    """-> (dlogits f64 [B,k], datt f64 in att's shape or None); the factor g * c / rows formed first, in that order."""
    c = [float(np.float32(v)) for v in coef]
    g = float(np.float32(g))
    dlogits = rows_backward(g * c[0] / logits.shape[0], logits, label)
    datt = None
    if att is not None:
        a2, l2 = flatten_attention(att, att_label)
        datt = rows_backward(g * c[1] / a2.shape[0], a2, l2).reshape(np.asarray(att).shape)
    return dlogits, datt


def tally(preds, label, flags, k, att_preds=None, att_flags=None, att_label=None, A=0, tables=None):
    """Adds one batch into tables = (confusion [k,k], anchor_table [k,A] or None, totals [4]) (made here when None) -> tables."""
    if tables is None:
        tables = (np.zeros((k, k), np.int32), np.zeros((k, A), np.int32) if A else None, np.zeros(4, np.int32))
    confusion, anchor_table, totals = tables
    for i in range(len(preds)):
        bad = flags[i] != 0 or not 0 <= label[i] < k or not 0 <= preds[i] < k
        if att_preds is not None:
            bad = bad or att_flags[i] != 0 or not 0 <= att_preds[i] < A
        if bad:
            totals[3] += 1
            continue
        totals[0] += 1
        totals[1] += int(preds[i] == label[i])
        confusion[label[i], preds[i]] += 1
        if att_preds is not None:
            anchor_table[label[i], att_preds[i]] += 1
            if att_label is not None:
                totals[2] += int(att_preds[i] == att_label[i])
    return tables


def schedule_coefficients(loss_type, m, counter, pretrain_step=2000):
    """(c_cls, c_att) of AttentionCrossEntropyLoss at iter_counter = counter (loss.py:59-68)."""
    if loss_type == "schedule":
        t = min(float(counter) / pretrain_step, 1.0)
        return t, m + 1.0 - t
    return (1.0, float(m)) if loss_type == "default" else (1.0, 0.0)


# ----------------------------------------------------------------------------------------------- inputs
def top_gap(x):
    """The distance between the two largest values of every row (inf for one column)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, np.asarray(x).shape[-1])
    if x.shape[1] == 1:
        return np.full(x.shape[0], np.inf)
    part = np.partition(x, x.shape[1] - 2, axis=1)
    return part[:, -1] - part[:, -2]


RESEEDED = 0


def logits_for(rows, n, seed, scale=2.0):
    """f32 [rows,n] Gaussian logits whose two largest values per row are at least GAP apart (a row that is not is redrawn from
    the same stream; RESEEDED counts them) and int32 labels in range, half of them the arg max."""
    global RESEEDED
    rng = np.random.default_rng(seed)
    x = (scale * rng.standard_normal((rows, n))).astype(np.float32)
    for r in np.nonzero(top_gap(x) < GAP)[0]:
        while top_gap(x[r:r + 1])[0] < GAP:
            RESEEDED += 1
            x[r] = (scale * rng.standard_normal(n)).astype(np.float32)
    label = rng.integers(0, n, size=rows).astype(np.int32)
    hit = rng.random(rows) < 0.5
    label[hit] = x.argmax(axis=1)[hit]
    return x, label


# (B, k, R, A, seed): every width and every row count on either side, the attention set absent once per width
CASES = []
for _i, _n in enumerate(WIDTHS):
    for _j, _r in enumerate(ROWS):
        _n2, _r2 = WIDTHS[(_i + 3 + _j) % len(WIDTHS)], ROWS[(_j + 2) % len(ROWS)]
        CASES.append((_r, _n, 0 if _j == _i % len(ROWS) else _r2, _n2, 7000 + 10 * _i + _j))
CASES = tuple(CASES)


def case(B, k, R, A, seed):
    """-> (logits, label, att or None, att_label or None, coef)."""
    logits, label = logits_for(B, k, seed)
    att = att_label = None
    if R:
        att, att_label = logits_for(R, A, seed + 5000)
    rng = np.random.default_rng(seed + 1)
    coef = (float(np.float32(rng.uniform(0.25, 1.0))), float(np.float32(rng.uniform(0.5, 2.0))))
    return logits, label, att, att_label, coef


def layout_case(C, seed=7700):
    """The [B,C,A] layout: wts f32 [4,C,12], rlabel int32 [4,60] -> (logits [4,40], label, wts, rlabel as forward() expands it)."""
    logits, label = logits_for(4, 40, seed + C)
    flat, _ = logits_for(4 * C, 12, seed + C + 100)
    wts = flat.reshape(4, C, 12)
    rlabel = np.random.default_rng(seed + C + 200).integers(0, 12, size=(4, 60)).astype(np.int32)
    return logits, label, wts, rlabel


def built_case(name):
    """-> (logits, label, att, att_label, coef).  B = 6, k = 40, A = 60 unless said."""
    logits, label, att, att_label, _ = case(6, 40, 6, 60, 7900)
    coef = (1.0, 0.5)
    if name == "tie":                                        # exact ties at the first, a middle and the last index
        for r, (lo, hi) in enumerate(((0, 17), (13, 29), (22, 39))):
            logits[r, lo] = logits[r, hi] = logits[r].max() + 1.0
        att[1, 59] = att[1, 30] = att[1].max() + 1.0
        att[2, :] = 0.25                                     # a constant row: every index ties, index 0 wins
    elif name == "label_edges":
        label[:] = (0, 39, 0, 39, 0, 39)
        att_label[:] = (0, 59, 59, 0, 0, 59)
    elif name == "bad":                                      # labels -1, n and -100
        label[1], label[3], label[4] = -1, 40, -100
        att_label[0], att_label[5] = 60, -100
    elif name == "big":                                      # +-1e4: the naive form overflows, the result stays finite
        logits[0, :] = -1e4
        logits[0, 7] = 1e4
        label[0] = 7
        logits[1, :] = -1e4
        logits[1, 3] = 1e4
        label[1] = 5
        att[2, :] = 1e4
        att[2, 11] = -1e4
        att_label[2] = 11
    elif name == "nonfinite":
        logits[2, 9] = np.nan
        logits[4, 0] = np.inf
        att[3, 59] = -np.inf
        att[5, 20] = np.nan
        label[4] = -1                                        # both bits: the bad label wins for the values
    elif name == "c_att0":
        coef = (1.0, 0.0)
    else:
        raise KeyError(name)
    return logits, label, att, att_label, coef


BUILT = ("tie", "label_edges", "bad", "big", "nonfinite", "c_att0")

GOLDEN_TYPES = (("schedule", 0.5), ("default", 0.5), ("no_reg", 0.5))
GOLDEN_COUNTERS = (0, 1000, 2500)                            # iter_counter at 0, at the midpoint, past pretrain_step = 2000


def golden_inputs(key):
    """The inputs recorded in tests/golden/cls_loss.npz (gen_golden_cls_loss.py writes what this returns):
    "a" [6,40] with wts [6,60] and rlabel [6]; "b" wts [6,40,60] with rlabel [6,60] (the slice path); "c" wts [3,70,12] with
    rlabel [3,60] (the repeat path) -> (pred, label, wts, rlabel)."""
    if key == "a":
        logits, label, att, att_label, _ = case(6, 40, 6, 60, 8100)
        return logits, label.astype(np.int64), att, att_label.astype(np.int64)
    B, C, A = (6, 40, 60) if key == "b" else (3, 70, 12)
    logits, label = logits_for(B, 40, 8200 + C)
    flat, _ = logits_for(B * C, A, 8300 + C)
    rlabel = np.random.default_rng(8400 + C).integers(0, A, size=(B, 60))
    return logits, label.astype(np.int64), flat.reshape(B, C, A), rlabel.astype(np.int64)
