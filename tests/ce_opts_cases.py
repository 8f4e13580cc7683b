"""The cross-entropy with options (mla_cross_entropy_den / mla_cross_entropy_opts, csrc/ce_core.h) restated in float64 numpy, and
the inputs its CPU and GPU tests share. The restatement is the closed form of nn.CrossEntropyLoss with class weights w, label
smoothing e, ignore_index i and reduction "mean" | "sum" (tests/test_ce_opts_cpu.py pins it to torch in float64):

  counted rows: y_b != i.  A counted label outside [0, K) is BAD: never an index, zero dx row, NaN loss, counted in counts[1].
  loss_b = (1 - e) w[y_b] (lse_b - x[b, y_b]) + (e / K) sum_k w_k (lse_b - x[b, k])
  mean: sum_b loss_b / den, den = sum over the counted in-range rows of w[y_b] (may be handed in: the global batch's);  sum: s = 1
  dx[b, k] = s [ p_k ((1 - e) w[y_b] + (e / K) W) - (1 - e) w[y_b] [k == y_b] - (e / K) w_k ],  W = sum_k w_k, s = 1 / den
  counts = [first-argmax hits among the counted in-range rows, bad labels, counted rows]
"""

import numpy as np


def restated(x, y, w=None, ignore_index=-100, eps=0.0, reduction="mean", den=None):
    """x (B, K) and w (K,) are taken to float64. -> dict(loss, dx, counts, den)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    B, K = x.shape
    w = np.ones(K) if w is None else np.asarray(w, dtype=np.float64)
    counted = y != ignore_index
    bad = counted & ((y < 0) | (y >= K))
    valid = counted & ~bad
    ys = np.where(valid, y, 0)
    m = x.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))[:, 0]
    p = np.exp(x - lse[:, None])
    wy = np.where(valid, w[ys], 0.0)
    rows = np.arange(B)
    loss_b = (1.0 - eps) * wy * (lse - x[rows, ys]) + (eps / K) * (w[None, :] * (lse[:, None] - x)).sum(axis=1)
    total = float(loss_b[valid].sum())
    own_den = float(wy.sum())
    den = own_den if den is None else float(den)
    if bad.any():
        loss = float("nan")
    elif reduction == "mean":
        loss = total / den if den != 0 else float("nan")
    else:
        loss = total
    onehot = np.zeros((B, K))
    onehot[rows, ys] = 1.0
    g = p * ((1.0 - eps) * wy + (eps / K) * w.sum())[:, None] - ((1.0 - eps) * wy)[:, None] * onehot - (eps / K) * w[None, :]
    dx = np.zeros((B, K))
    if valid.any():
        s = 1.0 / den if reduction == "mean" else 1.0
        dx[valid] = s * g[valid]
    hits = int((valid & (np.argmax(x, axis=1) == y)).sum())
    return {"loss": loss, "dx": dx, "counts": [hits, int(bad.sum()), int(counted.sum())], "den": own_den}


def bounds():
    """(loss, dscores): the project's own bounds for these two quantities, in tests/test_train_kernels_gpu.py's metrics."""
    from test_train_kernels_gpu import MEASURED
    return MEASURED["cross_entropy loss"][1], MEASURED["cross_entropy dscores"][1]


def loss_err(got, ref):
    """|got - ref| / max(|ref|, 1); 0 when both are NaN, inf when one is."""
    if np.isnan(got) or np.isnan(ref):
        return 0.0 if np.isnan(got) and np.isnan(ref) else float("inf")
    return abs(float(got) - float(ref)) / max(abs(float(ref)), 1.0)


def rel(got, ref):
    """max|got - ref| / max|ref| (the difference itself when ref is all zero)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d, m = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    return d / m if m > 0 else d


def ignored_rows(rows):
    """A quarter of the rows, row 0 and the last among them; fewer than three rows: none (the batch would be all ignored)."""
    if rows < 3:
        return []
    return sorted(set(range(0, rows, 4)) | {rows - 1})


def make_case(rows, K, seed, spread=4.0, ignore_index=-100, ignore=True):
    """float32 scores with planted exact ties of the row maximum (every fifth row; in half of them the label is the first tied
    index) and int64 labels with ignored_rows(rows) set to ignore_index."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-spread, spread, (rows, K)).astype(np.float32)
    y = rng.integers(0, K, rows).astype(np.int64)
    if K >= 2:
        for r in range(0, rows, 5):
            i, j = (r // 5) % K, (r // 5 + 1 + (r // 35) % (K - 1)) % K
            x[r, i] = x[r, j] = np.float32(x[r].max() + 0.25)
        for r in range(0, rows, 10):
            y[r] = int(np.argmax(x[r]))
    if ignore:
        y[ignored_rows(rows)] = ignore_index
    return x, y


def make_weights(K, seed=1):
    """float32 class weights spanning 0.25 to 4, one of them zero (three classes or more)."""
    rng = np.random.default_rng(1000 + seed + K)
    w = (0.25 * 16.0 ** rng.uniform(0, 1, K)).astype(np.float32)
    w[0] = 0.25
    if K >= 2:
        w[K - 1] = 4.0
    if K >= 3:
        w[K // 2] = 0.0
    return w


OPTIONS = [(weighted, eps, reduction) for weighted in (False, True) for eps in (0.0, 0.1) for reduction in ("mean", "sum")]

HOSTSIM_SHAPES = [(rows, K) for K in (1, 63, 64, 65, 527, 1024) for rows in (1, 5)]

# every K at rows = 5 (below, at and above one and several strides of the 64 lanes), every row count at K = 10 and 65 (fewer
# rows than a workgroup's four waves, exactly four, one more, many); 257 x 10 carries logits spread over +-80
GPU_SHAPES = [(5, K) for K in (1, 2, 10, 63, 64, 65, 527, 1024)] + [(rows, K) for K in (10, 65) for rows in (1, 3, 4, 257)]


def spread_of(rows, K):
    return 80.0 if (rows, K) == (257, 10) else 4.0
