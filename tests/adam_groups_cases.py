"""Cases and float64 restatement of the grouped Adam step (csrc/train_kernels.hip adam_grouped_kernel, mla_grad_norm), shared by
tests/test_adam_groups_cpu.py (the restatement against torch.optim.Adam / AdamW in float64) and tests/test_adam_groups_gpu.py
(the kernels against the restatement).

The restatement is torch's single-tensor step (torch/optim/adam.py _single_tensor_adam) written out in numpy float64, with the
first moment in the kernel's form b1 m + (1 - b1) g (torch: m.lerp_(g, 1 - b1); the same number up to float64 rounding)."""

import numpy as np

EPS32 = 2.0 ** -24                     # unit roundoff of float32

# Bound of one step, per element: |p_gpu - p_ref| <= C_P * 2^-24 * (|p| + |u|), u = the restatement's update p_ref_before - p_ref.
# Derivation: tests/test_adam_groups_gpu.py test_kernel_against_the_float64_restatement.
C_P = 6.0
C_M = 12.0                             # |m_gpu - m_ref| <= C_M * 2^-24 * m_abs (m_abs: the recursion on |g|)
C_V = 20.0                             # |v_gpu - v_ref| <= C_V * 2^-24 * v_lin (v_lin: the recursion on g_abs |g'|; = v without L2 cancellation)

SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1025]

# the new kernel's sweep: 2048 workgroups x 2048 elements (adam_groups.h kAdamMaxGrid x kAdamChunk); the old one wraps at 8192 x 256
ADAM_SWEEP = 2048 * 2048
NORM_SWEEP = 1024 * 4096               # mla_grad_norm: kNormMaxGrid x kNormChunk


def f32(x):
    """A hyper-parameter as the C ABI carries it (mla_adam_group_t holds floats), back as a Python float."""
    return float(np.float32(x))


def groups3():
    """L2 decay | decoupled decay with its own betas and eps | amsgrad -- hyper-parameters already rounded to float32."""
    return [dict(lr=f32(1e-3), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=f32(1e-2), decoupled=False, amsgrad=False),
            dict(lr=f32(3e-3), betas=(f32(0.8), f32(0.99)), eps=f32(1e-6), weight_decay=f32(5e-2), decoupled=True, amsgrad=False),
            dict(lr=f32(3e-4), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=0.0, decoupled=False, amsgrad=True)]


def plain_group(lr=1e-3):
    return dict(lr=f32(lr), betas=(f32(0.9), f32(0.999)), eps=f32(1e-8), weight_decay=0.0, decoupled=False, amsgrad=False)


def pad4(k):
    return (k + 3) // 4 * 4


def layout_small():
    """(numel, group) per tensor: the odd sizes, round-robin over three groups."""
    return [(k, i % 3) for i, k in enumerate(SIZES)]


def layout_wrapped():
    """A flat size past one sweep of the grouped kernel by an odd count, with a group boundary (and odd-sized tensors) inside
    the wrapped part: the chunks there are second iterations of the first workgroups."""
    return [(ADAM_SWEEP - 1024, 0), (1023, 1), (777, 2), (1302, 0), (5, 1)]          # 2083 elements past the sweep


def offsets(layout):
    off, out = 0, []
    for k, _ in layout:
        out.append(off)
        off += pad4(k)
    return out, off


def expected_runs(layout):
    """[(end, group)] of the maximal runs, restated independently of csrc/adam_groups.h."""
    runs, off = [], 0
    for k, g in layout:
        off += pad4(k)
        if runs and runs[-1][1] == g:
            runs[-1] = (off, g)
        else:
            runs.append((off, g))
    return runs


def real_mask(layout):
    """bool over the padded flat buffer: True where a tensor's element lives, False on padding."""
    offs, total = offsets(layout)
    mask = np.zeros(total, dtype=bool)
    for (k, _), o in zip(layout, offs):
        mask[o:o + k] = True
    return mask


def group_index(layout):
    offs, total = offsets(layout)
    idx = np.zeros(total, dtype=np.int64)
    for (k, g), o in zip(layout, offs):
        idx[o:o + pad4(k)] = g
    return idx


def make_params(layout, seed):
    """float32 parameters with 0.05 <= |p| <= 1 on the real elements (the derivation of C_P needs |p| >= 16 lr), 0 on padding."""
    rng = np.random.default_rng(seed)
    mask = real_mask(layout)
    p = (rng.uniform(0.05, 1.0, mask.size) * rng.choice([-1.0, 1.0], mask.size)).astype(np.float32)
    p[~mask] = 0.0
    return p


def make_grads(layout, seed):
    """float32 gradients, log-uniform magnitudes from 1e-6 to 1e2 with random signs; 0 on padding."""
    rng = np.random.default_rng(seed)
    mask = real_mask(layout)
    g = (10.0 ** rng.uniform(-6.0, 2.0, mask.size) * rng.choice([-1.0, 1.0], mask.size)).astype(np.float32)
    g[~mask] = 0.0
    return g


def clip_coef(g, max_norm):
    """torch.nn.utils.clip_grad_norm_: (norm, min(1, max_norm / (norm + 1e-6))) in float64."""
    norm = float(np.sqrt(np.sum(np.asarray(g, dtype=np.float64) ** 2)))
    c = max_norm / (norm + 1e-6)
    return norm, (c if c != c else min(1.0, c))                # a NaN norm: torch.clamp keeps the NaN


def restated_step(state, g, groups, idx, t, coef=None):
    """One step on float64 arrays. state: dict p, m, v, vmax, m_abs, v_lin (all float64, updated in place); g: the gradient;
    groups: list of dicts (lr, betas, eps, weight_decay, decoupled, amsgrad); idx: group index per element; t: step number from 1.
    Returns (u, u_abs, aux): the update p_before - p_after, its majorant with every term of the first moment taken in absolute
    value, and what a caller needs to carry an error of p through the next step (aux: b1, b2, wd_l2 = the L2 coefficient or 0,
    g_eff = |g'|, step_size, den).
    m_abs and v_lin are the moments' recursions on g_abs = |coef g| + |wd p| and on g_abs |g'|: what the rounding errors of
    g' = coef g + wd p (L2 decay, which can cancel) are proportional to."""
    p, m, v, vmax, m_abs, v_lin = state["p"], state["m"], state["v"], state["vmax"], state["m_abs"], state["v_lin"]
    g = np.asarray(g, dtype=np.float64)
    if coef is not None:
        g = g * coef
    col = lambda key: np.array([grp[key] for grp in groups], dtype=np.float64)[idx]            # noqa: E731
    lr, eps, wd = col("lr"), col("eps"), col("weight_decay")
    b1 = np.array([grp["betas"][0] for grp in groups], dtype=np.float64)[idx]
    b2 = np.array([grp["betas"][1] for grp in groups], dtype=np.float64)[idx]
    dec = np.array([grp["decoupled"] for grp in groups], dtype=bool)[idx]
    ams = np.array([grp["amsgrad"] for grp in groups], dtype=bool)[idx]
    before = p.copy()
    g_abs = np.abs(g) + np.where(~dec, np.abs(wd * p), 0.0)
    g = np.where(~dec, g + wd * p, g)                          # grad.add(param, alpha=weight_decay); wd = 0 adds nothing
    p[:] = np.where(dec, p * (1.0 - lr * wd), p)               # param.mul_(1 - lr * weight_decay)
    decayed = p.copy()
    m[:] = b1 * m + (1.0 - b1) * g
    m_abs[:] = b1 * m_abs + (1.0 - b1) * g_abs
    v[:] = b2 * v + (1.0 - b2) * g * g
    v_lin[:] = b2 * v_lin + (1.0 - b2) * g_abs * np.abs(g)
    vmax[:] = np.where(ams, np.maximum(vmax, v), vmax)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    den = np.sqrt(np.where(ams, vmax, v)) / np.sqrt(bc2) + eps
    p[:] = decayed - (lr / bc1) * m / den
    aux = {"b1": b1, "b2": b2, "wd_l2": np.where(~dec, wd, 0.0), "g_eff": np.abs(g), "step_size": lr / bc1, "den": den}
    return before - p, np.abs(before - decayed) + (lr / bc1) * m_abs / den, aux


def fresh_state(p):
    p = np.asarray(p, dtype=np.float64).copy()
    return {"p": p, "m": np.zeros_like(p), "v": np.zeros_like(p), "vmax": np.zeros_like(p), "m_abs": np.zeros_like(p),
            "v_lin": np.zeros_like(p)}
