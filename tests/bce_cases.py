"""The binary cross-entropy (mla_bce, csrc/bce_core.h) restated in float64 numpy, and the inputs its CPU and GPU tests share. The
restatement is nn.BCELoss(weight, reduction) as ATen defines it (tests/test_bce_cpu.py pins it to torch in float64):

  term[b, k] = w_k ((y - 1) max(log(1 - p), -100) - y max(log p, -100))
  loss = s sum term,  s = 1 / (rows K) for "mean" (or the inv_total handed in: the global batch's), 1 for "sum"
  dp[b, k] = s w_k (p - y) / max((1 - p) p, 1e-12)
  A BAD cell (target NaN or outside [0, 1], or p outside [0, 1]): no logarithm, dp exactly zero, counted; the loss is then NaN.
  A NaN in p is not bad: NaN loss, NaN in that cell of dp.
  counts = [rows with every cell on the right side of 0.5, bad cells, cells on the right side]; right: (p >= 0.5) == (y >= 0.5)
"""

import numpy as np


def restated(p, y, w=None, reduction="mean", inv_total=None):
    """p, y (rows, K) and w (K,) are taken to float64. -> dict(loss, dp, counts)."""
    p = np.asarray(p, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    rows, K = p.shape
    w = np.ones(K) if w is None else np.asarray(w, dtype=np.float64)
    s = 1.0 if reduction == "sum" else (1.0 / (rows * K) if inv_total is None else float(inv_total))
    with np.errstate(invalid="ignore"):
        bad = ~((y >= 0.0) & (y <= 1.0)) | (p < 0.0) | (p > 1.0)
    ps, ys = np.where(bad, 0.5, p), np.where(bad, 0.5, y)             # never a logarithm of a bad cell
    with np.errstate(divide="ignore", invalid="ignore"):
        term = w[None, :] * ((ys - 1.0) * np.maximum(np.log(1.0 - ps), -100.0) - ys * np.maximum(np.log(ps), -100.0))
        dp = s * w[None, :] * (ps - ys) / np.maximum((1.0 - ps) * ps, 1e-12)
    term, dp = np.where(bad, 0.0, term), np.where(bad, 0.0, dp)
    loss = float("nan") if bad.any() else float(s * term.sum())
    with np.errstate(invalid="ignore"):
        right = ((p >= 0.5) == (y >= 0.5)) & ~bad
    return {"loss": loss, "dp": dp, "counts": [int(right.all(axis=1).sum()), int(bad.sum()), int(right.sum())]}


def loss_err(got, ref):
    """|got - ref| / max(|ref|, 1); 0 when both are NaN, inf when one is."""
    if np.isnan(got) or np.isnan(ref):
        return 0.0 if np.isnan(got) and np.isnan(ref) else float("inf")
    return abs(float(got) - float(ref)) / max(abs(float(ref)), 1.0)


def rel(got, ref):
    """max|got - ref| / max|ref| (the difference itself when ref is all zero), as ce_opts_cases.rel."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d, m = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    return d / m if m > 0 else d


def make_case(rows, K, seed, soft=0.25):
    """float32 probabilities in [0.02, 0.98] and float32 multi-hot targets, about a quarter of them soft, inside (0, 1)."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.02, 0.98, (rows, K)).astype(np.float32)
    y = (rng.uniform(0, 1, (rows, K)) < 0.3).astype(np.float32)
    is_soft = rng.uniform(0, 1, (rows, K)) < soft
    y = np.where(is_soft, rng.uniform(0.05, 0.95, (rows, K)), y).astype(np.float32)
    return p, y


def make_weights(K, seed=1):
    """float32 class weights spanning 0.25 to 4, one of them zero (three classes or more)."""
    rng = np.random.default_rng(2000 + seed + K)
    w = (0.25 * 16.0 ** rng.uniform(0, 1, K)).astype(np.float32)
    w[0] = 0.25
    if K >= 2:
        w[K - 1] = 4.0
    if K >= 3:
        w[K // 2] = 0.0
    return w


# the four corners of the saturation: (p, y); the loss terms are 100 w, 100 w, 0 and 0, the gradients -1e12 w, 1e12 w, 0 and 1e-18 w
CORNERS = [(0.0, 1.0), (1.0, 0.0), (1.0, 1.0), (1e-30, 0.0)]

OPTIONS = [(weighted, reduction) for weighted in (False, True) for reduction in ("mean", "sum")]

# the smallest shapes at which the lane striding (K below, at and above one stride of 64 lanes, and in a third stride), the
# row-to-workgroup map (fewer rows than a workgroup's four waves, exactly four, one more, three workgroups) and the finish can go wrong
HOSTSIM_SHAPES = [(rows, K) for rows in (1, 3, 4, 5, 9) for K in (1, 10, 63, 64, 65, 130)]

# and: more rows than the finish workgroup has threads (257), the AudioSet head (527), all 16 strides (1024), and more than four
# times the finish workgroup's threads (1030 x 3)
GPU_SHAPES = HOSTSIM_SHAPES + [(257, 10), (5, 527), (6, 1024), (1030, 3)]
