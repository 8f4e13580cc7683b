"""Cases, float64 reference, tolerances and planted defects of the head at model_conf other than [2, 1] (tests/test_head_conf_gpu.py,
tests/test_head_conf_cases_cpu.py, tests/_head_conf_dp_worker.py). No GPU code is imported here, so the CPU test evaluates all of it.

Inputs, weights, running statistics moved off their initial values, loss weights and masks are weights.py streams, built as
test_wide_head_matches_the_oracle_in_float64 builds them (its _masks / _install are imported). The reference is
oracle.model.mla_forward on float64 copies of the same state_dict, differentiated by torch autograd.

Tolerances (test_autograd_gpu.py, test_wide_head_gpu.py): outputs and running statistics rtol 1e-4, atol 1e-6; gradients rtol 2e-3,
atol 2e-5 x (largest entry of that tensor) + 2e-5 x (largest gradient entry of the model); input gradient rtol 2e-3, atol 2e-5 x
its largest entry. share() is |got - ref| / (atol + rtol |ref|) at its worst element: <= 1 is numpy's assert_allclose.
"""

import numpy as np
import torch
import torch.nn.functional as F

from test_train_kernels_gpu import MEASURED as KERNEL_MEASURED
from test_wide_head_gpu import _install, _masks  # noqa: F401  (_install: re-exported to the GPU tests and the worker)

CONTROL = (2, 1)
CONFS = [(1,), (3,), (1, 1), (1, 1, 2), (2, 2, 1), (1, 1, 1, 1)]
BAGS = 6                                      # head cases
OUT_RTOL, OUT_ATOL, GRAD_RTOL, GRAD_ATOL = 1e-4, 1e-6, 2e-3, 2e-5
STATS = ("running_mean", "running_var", "num_batches_tracked")
WIDE = dict(classes=17, slots=12, hidden=64)  # the wide pooling / BatchNorm path; odd K: slices of conc are 4-byte aligned only


def _case(conf, width=128, **kw):
    return dict(conf=tuple(conf), width=width, kw=kw)


HEAD_CASES = ([_case(c) for c in CONFS + [CONTROL]] +
              [_case((1,), 10), _case((1, 1, 2), 10)] +          # ResNet just_bottlenecks=False width: linear_small at level 0
              [_case((3,), **WIDE), _case((1, 1, 2), **WIDE)] +
              [_case((1, 1, 2), classes=50)])


def case_id(case):
    s = "conf" + "".join(str(n) for n in case["conf"]) + "-m%d" % case["width"]
    return s + "".join("-%s%d" % (k[0], v) for k, v in sorted(case["kw"].items()))


def dims(kw):
    """(classes, slots, hidden) of a head's keyword arguments."""
    return kw.get("classes", 10), kw.get("slots", 10), kw.get("hidden", 600)


def move_running_stats(W, sd):
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = W.uniform(5, W.stream_id(k), sd[k].size, lo=-0.5, hi=0.5).astype(np.float32).reshape(sd[k].shape)
        if k.endswith("running_var"):
            sd[k] = W.uniform(5, W.stream_id(k), sd[k].size, lo=0.5, hi=2.0).astype(np.float32).reshape(sd[k].shape)
    return sd


def head_state(W, case):
    """numpy state_dict with the prefix 'mla.', running statistics away from (0, 1)."""
    K, T, H = dims(case["kw"])
    return move_running_stats(W, W.make_state_dict(3, W.mla_shapes(list(case["conf"]), case["width"], prefix="mla.", T=T, H=H, K=K)))


def head_inputs(W, case, train):
    """x (BAGS, T, width) in [0, 2), loss weights (BAGS, K) in [-1, 1), masks (train mode) or None."""
    K, T, H = dims(case["kw"])
    m = case["width"]
    x = torch.from_numpy(W.uniform(4, W.stream_id("mla_in/m%d" % m), BAGS * T * m, lo=0.0, hi=2.0)).reshape(BAGS, T, m)
    wgt = torch.from_numpy(W.uniform(4, W.stream_id("loss_w"), BAGS * K, lo=-1.0, hi=1.0)).reshape(BAGS, K)
    return x, wgt, (_masks(W, 5, case["conf"], BAGS, T, H) if train else None)


def leaves(sd, dtype=torch.float64):
    """{key: tensor of dtype (counters stay int64)}; everything that trains requires grad (fcf included: it must receive none)."""
    return {k: (torch.as_tensor(v).to(dtype) if not k.endswith("num_batches_tracked") else torch.as_tensor(v)).clone()
            .requires_grad_(not k.endswith(STATS)) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------- planted defects ----

DEFECTS = ("no_grad_from_above", "swapped_slices", "mask_of_first")


def defect_applies(defect, conf, train):
    """(a) and (b) need two levels; (c) needs a level with two layers and dropout, i.e. train mode."""
    if defect == "mask_of_first":
        return train and max(conf) >= 2
    return len(conf) >= 2


def forward(sd, x, conf, train, masks, stats_out, defect=None):
    """oracle.model.mla_forward, or a small variant of it that is wrong on purpose:
      no_grad_from_above  (a) the gradient from the level above is dropped: the input of levels >= 1 is detached;
      swapped_slices      (b) the final Linear reads attention module 1's slice where module 0's belongs and the reverse;
      mask_of_first       (c) Dropout (lvl, j) uses the mask of (lvl, 0);
      restated            no defect: the loop the first two are planted in, which must equal mla_forward bit for bit."""
    from oracle import model as omodel
    if defect is None:
        return omodel.mla_forward(sd, x, tuple(conf), train=train, masks=masks, stats_out=stats_out)
    if defect == "mask_of_first":
        first = {k: masks[k.rsplit(".", 1)[0] + ".0"] for k in masks}
        return omodel.mla_forward(sd, x, tuple(conf), train=train, masks=first, stats_out=stats_out)
    assert defect in ("no_grad_from_above", "swapped_slices", "restated"), defect
    embs, cur = [], x
    for lvl, n_fc in enumerate(conf):
        if defect == "no_grad_from_above" and lvl >= 1:
            cur = cur.detach()
        cur = omodel.embedded_mapping(sd, "mla.embedded_mappings.%d." % lvl, cur, n_fc, train, masks, stats_out)
        embs.append(cur)
    ys = [omodel.attention_module(sd, "mla.attention_modules.%d." % lvl, embs[lvl], train, stats_out) for lvl in range(len(conf))]
    if defect == "swapped_slices":
        ys[0], ys[1] = ys[1], ys[0]
    out = F.linear(torch.cat(ys, dim=1), sd["mla.fc.weight"], sd["mla.fc.bias"])
    return torch.sigmoid(omodel.bn_t(sd, "mla.norm", out, train, stats_out))


# ------------------------------------------------------------------------------------------------- reference ----

def run_oracle(sd, x, wgt, conf, train, masks, dtype=torch.float64, defect=None):
    """One forward and backward of sum(out * wgt) through the oracle in `dtype` -> {"out", "running" (the running statistics after
    a train-mode forward, {} in eval mode), "dx", "grads" {name without 'mla.': gradient or None}}, all detached."""
    ref_sd = leaves(sd, dtype)
    xr = x.to(dtype).requires_grad_(True)
    stats = {} if train else None
    out = forward(ref_sd, xr, conf, train, masks, stats, defect)
    (out * wgt.to(dtype)).sum().backward()
    running = {}
    for key, (mean, unbiased) in (stats or {}).items():
        running[key[4:] + ".running_mean"] = 0.9 * ref_sd[key + ".running_mean"] + 0.1 * mean
        running[key[4:] + ".running_var"] = 0.9 * ref_sd[key + ".running_var"] + 0.1 * unbiased
    return {"out": out.detach(), "running": running, "dx": xr.grad,
            "grads": {k[4:]: v.grad for k, v in ref_sd.items() if v.requires_grad}}


_REFERENCES = {}


def reference(W, case, train):
    """The float64 reference of a head case, computed once and shared (nobody writes into it)."""
    key = (case_id(case), bool(train))
    if key not in _REFERENCES:
        x, wgt, masks = head_inputs(W, case, train)
        _REFERENCES[key] = run_oracle(head_state(W, case), x, wgt, case["conf"], train, masks)
    return _REFERENCES[key]


def share(got, ref, rtol, atol):
    """Worst |got - ref| / (atol + rtol |ref|): the fraction of an assert_allclose tolerance that is used."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if ref.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


def grad_floor(grads):
    """2e-5 of the model's largest gradient entry: mathematically zero gradients (biases in front of a train-mode BatchNorm,
    normv.bias under the softmax's shift invariance) are rounding noise of the format on either side."""
    return GRAD_ATOL * max(float(g.abs().max()) for g in grads.values() if g is not None)


def grad_shares(got, ref):
    """{name: share} of every gradient the reference has, by the gradient tolerance; got and ref map names to tensors."""
    floor = grad_floor(ref)
    return {n: share(got[n], r, GRAD_RTOL, GRAD_ATOL * float(r.abs().max()) + floor) for n, r in ref.items() if r is not None}


def shares(got, ref):
    """{tensor name: share of its tolerance} of a whole result (run_oracle's layout) against the float64 reference."""
    out = {"out": share(got["out"], ref["out"], OUT_RTOL, OUT_ATOL)}
    for k, r in ref["running"].items():
        out[k] = share(got["running"][k], r, OUT_RTOL, OUT_ATOL)
    if got.get("dx") is not None:
        out["dx"] = share(got["dx"], ref["dx"], GRAD_RTOL, GRAD_ATOL * float(ref["dx"].abs().max()))
    out.update(grad_shares(got["grads"], ref["grads"]))
    return out


def group_of(name):
    """The MEASURE line a tensor is counted under."""
    if name in ("out", "dx"):
        return name
    if name.endswith(STATS[:2]):
        return "running statistics"
    return "gradients"


def report(tag, sh, limit=1.0, limits=None):
    """One MEASURE line per tensor group (worst share and where), then the assertion: every share <= limit (limits: {name: its own})."""
    worst = {}
    for name, v in sh.items():
        g = group_of(name)
        if g not in worst or v > worst[g][0]:
            worst[g] = (v, name)
    for g, (v, name) in sorted(worst.items()):
        print("MEASURE %s %s: worst share of the tolerance %.3g (%s)" % (tag, g, v, name))
    bad = {n: v for n, v in sh.items() if not v <= (limits or {}).get(n, limit)}
    assert not bad, (tag, bad)


# ------------------------------------------------------------------------------------------------- TrainStep ----

CNN_CONF = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=False,
                cnn_trainable=False, first_cnn_layer_trainable=False, in_channels=1)
STEP_BAGS, STEPS, LR = 4, 3, 1e-3
STEP_CASES = [_case((1,)), _case((3,)), _case((1, 1, 2)), _case((2, 2, 1)), _case((1, 1, 2), **WIDE)]
GRAPH_CASES = [_case((1,)), _case((3,)), _case((1, 1, 2))]
DP_CASE = _case((1, 1, 2))
MARGIN = 1e-4                                 # top-2 score margin above which the hit count is unambiguous
# inputs of step s: weights.py seed STEP_SEED + s, masks STEP_SEED + 100 + s. The seed is one at which every row's top-2 margin of
# the float64 reference is above MARGIN in all STEP_CASES (the smallest is 7e-4; at seed 100 the (1,) head has one of 3e-5 in its
# third step): tests/test_head_conf_cases_cpu.py asserts it
STEP_SEED = 400
LOSS_REL = 1e-4
# mla.fc.bias in the TrainStep cases: its gradient is mathematically zero (a bias in front of the train-mode BatchNorm over the 4
# bags, whose batch variance goes down to 8e-4 and scales the terms that cancel by 36), so what either side holds is rounding
# noise, and its size depends on the order of the sums: the float32 oracle alone is 1.09 to 2.28 of the gradient tolerance away from
# float64 there, depending on the host and its thread count (wide (1, 1, 2), step 0; every other tensor at most 0.40). This one
# tensor's tolerance is therefore 4 x the float32 oracle's worst distance; all others stay as they are. The 6-bag head cases need
# none of this: the float32 oracle uses at most 0.31 of any tolerance there (tests/test_head_conf_cases_cpu.py).
STEP_FC_BIAS_F32 = 2.28
STEP_LIMITS = {"mla.fc.bias": 4 * STEP_FC_BIAS_F32}

_VGG = {}


def ensemble_state(W, case):
    """numpy state_dict of Ensemble(frozen VGGish, case): seed 7 as the other TrainStep tests; the VGGish part is generated once."""
    K, T, H = dims(case["kw"])
    if not _VGG:
        _VGG.update(W.make_state_dict(7, W.vggish_shapes("cnn.cnn_model.")))
    sd = W.make_state_dict(7, W.mla_shapes(list(case["conf"]), 128, prefix="mla.", T=T, H=H, K=K))
    sd.update(_VGG)
    return sd


def step_bags(W, s, classes, slots, bags=STEP_BAGS):
    """Step s: (bags, slots, 1, 96, 64) inputs in the front-end's value range; labels over all classes, the last one the highest class."""
    x = W.uniform(STEP_SEED + s, W.stream_id("bags"), bags * slots * 96 * 64, lo=-1.4, hi=4.6)
    y = W.bits24(STEP_SEED + s, W.stream_id("labels"), bags) % classes
    y[-1] = classes - 1
    return torch.as_tensor(x).reshape(bags, slots, 1, 96, 64), torch.as_tensor(y.astype(np.int64))


def step_masks(W, s, case, bags=STEP_BAGS):
    K, T, H = dims(case["kw"])
    return _masks(W, STEP_SEED + 100 + s, case["conf"], bags, T, H)


def step_reference(state, feats, y, conf, masks):
    """The float64 reference of ONE training step restarted from `state` (the model's current 'mla.' state_dict, any float dtype):
    mla_forward(train=True) + F.cross_entropy on `feats` (bags, slots, 128) -> {"loss", "hits", "margin" (smallest top-2 score
    margin of a row), "grads" {key with 'mla.': gradient or None}, "running" {key: value after the step}}."""
    from oracle import model as omodel
    sd = leaves({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in state.items() if k.startswith("mla.")})
    stats = {}
    out = omodel.mla_forward(sd, feats.double().cpu(), tuple(conf), train=True, masks=masks, stats_out=stats)
    loss = F.cross_entropy(out, y)
    loss.backward()
    top = out.detach().topk(2, dim=1).values
    running = {}
    for key, (mean, unbiased) in stats.items():
        running[key + ".running_mean"] = 0.9 * sd[key + ".running_mean"] + 0.1 * mean
        running[key + ".running_var"] = 0.9 * sd[key + ".running_var"] + 0.1 * unbiased
    return {"loss": float(loss.detach()), "hits": int((out.detach().argmax(dim=1) == y).sum()),
            "margin": float((top[:, 0] - top[:, 1]).min()), "running": running,
            "grads": {k: v.grad for k, v in sd.items() if v.requires_grad}}


# The parameter update on its own: the step's float32 gradients fed to a float64 torch.optim.Adam. The kernel's update agrees with
# float64 to MEASURED["adam update"] of the largest update (tests/test_train_kernels_gpu.py, parameters of size 0.05). What a test
# can observe is p_after - p_before of float32 parameters, which also holds the ONE rounding of storing p_after: at most half a
# float32 spacing of the parameter, 6e-8 for a BatchNorm weight near 1 against updates of lr = 1e-3, i.e. 6e-5 of the update and
# above the kernel's bound whatever the kernel does. Both terms per element; nothing here comes from a HIP result.
ADAM_UPDATE = KERNEL_MEASURED["adam update"][1]


def adam_update_bound(update_ref, p_before, p_after):
    """Per element: ADAM_UPDATE x the tensor's largest reference update + half the float32 spacing at the parameter."""
    big = torch.maximum(p_before.detach().abs(), p_after.detach().abs()).float().cpu().numpy()
    half_ulp = torch.from_numpy(np.spacing(big).astype(np.float64)) / 2
    return ADAM_UPDATE * float(update_ref.abs().max()) + half_ulp
