"""The grouped Adam step on the GPU (mla_adam_grouped_step, mla_adam_groups_prepare, mla_grad_norm; TrainStep(optimizer=,
max_grad_norm=); train_model(extended_optimizer=True)): the kernels against the float64 restatement of tests/adam_groups_cases.py
and against the one-group kernel, the step against torch's own optimizer on identical gradients, eager against graph replays,
group routing at model scale, checkpoints, the epoch loop and two data-parallel ranks."""

import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adam_groups_cases as C
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

ops = importlib.import_module(PKG + ".ops")
M = importlib.import_module(PKG + ".model")
TR = importlib.import_module(PKG + ".train")

DEV = torch.device("cuda")


# ------------------------------------------------------------------ the kernels --------------------------------------------------

class Flat:
    """The flat device buffers of one layout, stepped by the grouped kernel."""

    def __init__(self, layout, groups, p0):
        self.groups, self.t = groups, 0
        tab = ops.adam_groups_table([k for k, _ in layout], [g for _, g in layout], len(groups))
        assert tab["total"] == p0.size
        self.table, self.runs, self.pads = tab["table"].to(DEV), tab["runs"], tab["pads"]
        self.p = torch.from_numpy(p0.copy()).to(DEV)
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.vmax = torch.zeros_like(self.p) if any(g["amsgrad"] for g in groups) else None
        self.rows = torch.zeros(8 * len(groups), device=DEV)

    def step(self, g, coef=None):
        self.t += 1
        ops.adam_groups_prepare(self.rows, self.groups, self.t)
        ops.adam_grouped_step(self.p, g, self.m, self.v, self.vmax, self.table, self.runs, self.pads, self.rows, len(self.groups), coef)


@pytest.fixture(scope="module")
def cases():
    """Per layout: parameters, three gradients and the float64 restatement's trajectory (computed once, read only)."""
    out = {}
    for name, layout in (("small", C.layout_small()), ("wrapped", C.layout_wrapped())):
        groups, idx = C.groups3(), C.group_index(layout)
        p0 = C.make_params(layout, 5)
        grads = [C.make_grads(layout, 20 + s) for s in range(3)]
        state, traj = C.fresh_state(p0), []
        for t, g in enumerate(grads, 1):
            before = state["p"].copy()
            norm, coef = C.clip_coef(g, 10.0)
            u, u_abs, aux = C.restated_step(state, g, groups, idx, t, coef)
            traj.append({k: v.copy() for k, v in state.items()} | {"before": before, "u": u, "u_abs": u_abs, "coef": coef, "norm": norm, "aux": aux})
        out[name] = dict(layout=layout, groups=groups, p0=p0, grads=grads, traj=traj, mask=C.real_mask(layout))
    return out


@pytest.mark.parametrize("name", ["small", "wrapped"])
def test_kernel_against_the_float64_restatement(cases, name):
    """Three groups (L2 decay | decoupled decay with its own betas and eps | amsgrad), clipping on, three steps, on tensors of
    [1, 3, 4, 5, 255, 256, 257, 1023, 1025] elements dealt round-robin to the groups, and on a flat size of 4 194 304 + 2083
    elements: one sweep of the grouped kernel is 2048 workgroups x 2048 elements = 4 194 304 (the one-group kernel wraps at 8192 x
    256 = 2 097 152), and the tensors past it belong to three different groups and have odd sizes.

    The bound, per step and element, with e = 2^-24 (float32 unit roundoff), first order in e; the inputs are float32 numbers and
    the restatement gets the hyper-parameters as the C ABI carries them (rounded to float32):
      p path: p (1 - lr wd) costs the rounded factor and the product, 2 e |p|; the final subtraction e |p'| <= e (|p| + |u|).
      u path, relative to u_abs (u with every term of the first moment taken in absolute value, u_abs <= 1.6 lr over three steps
      by Cauchy-Schwarz on m / sqrt(v)): g' = coef g: coef carries 3 e (norm, + 1e-6, division) and the product e; g' + wd p: 2 e
      more, 6 e; m: (1 - b1), its product and the fma, 3 e, plus e per later step: 11 e; v: 2 * 6 + 1 for g'^2, 3 for the update,
      e per later step: 18 e, halved by the root, 2 e for v_sqrt_f32 (1 ulp): 11 e; the denominator's scalar and fma: 13 e;
      step_size and its product on m: 13 e; the division (<= 1 ulp): 2 e. Together 28 e u_abs.
    So |p_gpu - p_ref| <= 3 e (|p| + |u|) + 28 e * 1.6 lr. The cases draw |p| >= 0.05 and lr <= 3e-3: 28 * 1.6 * 3e-3 = 0.134 <=
    3 * 0.05, which makes the whole 6 e |p| at most: C_P = 6 in c * 2^-24 * (|p| + |u|). The device runs on from its own values,
    so after step t the bound is the sum over the steps so far. m and v get their own bounds from the same count (which already
    holds the three steps): 12 e m_abs and 20 e v_lin.
    One thing the count above takes for granted does not hold everywhere: in the L2 group g' = coef g + wd p CANCELS where the two
    terms have opposite signs and like size, to any depth among millions of elements, and then the 6 e is relative to g_abs = |coef
    g| + |wd p|, not to |g'| (float32 torch has the same property: it is the conditioning of L2 decay, not of the kernel). With
    kappa = v_lin / v >= 1 (v's recursion on g_abs |g'| over v itself; 1 without cancellation) the u path reads, written out,
    13 e u_abs for the numerator, (10 kappa + 4) e |u| for the denominator, 2 e |u| for the division:
        step bound = e * max(C_P (|p| + |u|),  3 (|p| + |u|) + 15 u_abs + (10 kappa + 6) |u|)
    where the second form is below the first whenever kappa = 1 (u_abs, |u| <= 1.6 lr: 50 lr <= 3 * 0.05), so the well-conditioned
    elements keep the plain bound; the test prints how many elements the second form governs. Where that form has let p drift
    by more than roundoff, the next step's g' = coef g + wd p starts from the drifted p: wd times the bound so far enters m, v
    (m_in, v_in below, their recursions on it) and through them u, to first order.
    Worst observed ratio to the bound: DESIGN.md section 4."""
    c = cases[name]
    flat = Flat(c["layout"], c["groups"], c["p0"])
    clip = torch.zeros(2, device=DEV)
    bound = np.zeros(c["p0"].size)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    m_in, v_in = np.zeros_like(bound), np.zeros_like(bound)
    for t, (g, ref) in enumerate(zip(c["grads"], c["traj"]), 1):
        gd = torch.from_numpy(g).to(DEV)
        ops.grad_norm(gd, 10.0, out=clip)
        flat.step(gd, clip[1:2])
        assert torch.equal(gd, torch.from_numpy(g).to(DEV)), "the gradient is only read"
        pu = np.abs(ref["before"]) + np.abs(ref["u"])
        kappa = np.where(ref["v"] > 0, ref["v_lin"] / np.where(ref["v"] > 0, ref["v"], 1.0), 1.0)
        cond = 3 * pu + 15 * ref["u_abs"] + (10 * kappa + 6) * np.abs(ref["u"])
        print("%s step %d: %d of %d elements are governed by the conditioned form" % (name, t, int((cond > C.C_P * pu).sum()), pu.size))
        a = ref["aux"]
        g_in = a["wd_l2"] * bound                                   # what the error of p so far adds to g'
        m_in = a["b1"] * m_in + (1 - a["b1"]) * g_in
        v_in = a["b2"] * v_in + (1 - a["b2"]) * (2 * a["g_eff"] * g_in + g_in ** 2)
        drift = a["step_size"] * m_in / a["den"] + np.abs(ref["u"]) * np.where(ref["v"] > 0, v_in / (2 * np.where(ref["v"] > 0, ref["v"], 1.0)), 0.0)
        bound += C.EPS32 * np.maximum(C.C_P * pu, cond) + drift
        got = {k: getattr(flat, k).cpu().numpy().astype(np.float64) for k in ("p", "m", "v", "vmax")}
        assert float(clip[1]) < 1.0 and abs(float(clip[1]) - ref["coef"]) <= 4 * C.EPS32 * ref["coef"]
        for k, b in (("p", bound), ("m", C.C_M * C.EPS32 * ref["m_abs"] + m_in), ("v", C.C_V * C.EPS32 * ref["v_lin"] + v_in)):
            err = np.abs(got[k] - ref[k])
            ratio = float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))))
            worst[k] = max(worst[k], ratio)
            print("%s step %d: worst |%s - ref| / bound = %.3f" % (name, t, k, ratio))
        ams = np.array([grp["amsgrad"] for grp in c["groups"]])[C.group_index(c["layout"])]
        assert np.array_equal(got["vmax"][~ams], np.zeros((~ams).sum())), "groups without amsgrad never touch vmax"
        assert np.all(np.abs(got["vmax"][ams] - ref["vmax"][ams]) <= C.C_V * C.EPS32 * ref["vmax"][ams])       # (the amsgrad group has no decay: v_lin = v)
        for k in ("p", "m", "v", "vmax"):
            assert not got[k][~c["mask"]].any(), "padding of %s stays exactly 0" % k
    assert worst["p"] <= 1.0 and worst["m"] <= 1.0 and worst["v"] <= 1.0, worst


@pytest.mark.parametrize("name", ["small", "wrapped"])
def test_one_plain_group_equals_the_old_kernel_bit_for_bit(cases, name):
    c = cases[name]
    layout1 = [(k, 0) for k, _ in c["layout"]]
    flat = Flat(layout1, [C.plain_group(1e-3)], c["p0"])
    p = torch.from_numpy(c["p0"].copy()).to(DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t, g in enumerate(c["grads"], 1):
        gd = torch.from_numpy(g).to(DEV)
        ops.adam_step(p, gd, m, v, 1e-3, 0.9, 0.999, 1e-8, t)
        flat.step(gd)
        assert torch.equal(flat.p, p) and torch.equal(flat.m, m) and torch.equal(flat.v, v), t
    assert flat.vmax is None


@pytest.mark.parametrize("n", [1, 255, 257, C.NORM_SWEEP + 2083])
def test_grad_norm_against_float64(n):
    """Sums of squares are exact products added in double: only the final rounding to float32 counts, 2^-23 relative leaves
    room for the double sum's own 1e-13. Past 1024 x 4096 elements the blocks take second iterations."""
    rng = np.random.default_rng(n)
    g = (10.0 ** rng.uniform(-6, 2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    gd = torch.from_numpy(g).to(DEV)
    ref, ref_coef = C.clip_coef(g, 0.5)
    a, b = ops.grad_norm(gd, 0.5), ops.grad_norm(gd, 0.5)
    assert torch.equal(a, b), "two runs agree bit for bit"
    assert abs(float(a[0]) - ref) <= 2.0 ** -23 * ref
    assert abs(float(a[1]) - ref_coef) <= 4 * C.EPS32 * ref_coef
    big = ops.grad_norm(gd, 2.0 * ref + 1.0)
    assert float(big[1]) == 1.0 and float(big[0]) == float(a[0])


def test_unclipped_coefficient_changes_no_bit_and_inf_acts_as_in_torch(cases):
    c = cases["small"]
    g = torch.from_numpy(c["grads"][0]).to(DEV)
    clip = ops.grad_norm(g, 1e6)
    assert float(clip[1]) == 1.0
    a, b = Flat(c["layout"], c["groups"], c["p0"]), Flat(c["layout"], c["groups"], c["p0"])
    a.step(g, clip[1:2]); b.step(g)
    assert torch.equal(a.p, b.p) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and torch.equal(a.vmax, b.vmax)
    # one Inf element: norm Inf, coefficient 0, 0 * Inf = NaN in that entry only -- what clip_grad_norm_ + Adam give
    layout1 = [(k, 0) for k, _ in c["layout"]]
    offs, _ = C.offsets(layout1)
    gi = c["grads"][1].copy()
    gi[offs[6] + 100] = np.inf
    gd = torch.from_numpy(gi).to(DEV)
    clip = ops.grad_norm(gd, 1.0)
    assert float(clip[0]) == float("inf") and float(clip[1]) == 0.0
    flat = Flat(layout1, [C.plain_group(1e-3)], c["p0"])
    flat.step(gd, clip[1:2])
    params = [torch.nn.Parameter(torch.from_numpy(c["p0"][o:o + k].copy()).to(DEV)) for (k, _), o in zip(layout1, offs)]
    for q, (k, _), o in zip(params, layout1, offs):
        q.grad = gd[o:o + k].clone()
    opt = torch.optim.Adam(params, lr=1e-3, foreach=False)
    torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=False)
    opt.step()
    for q, (k, _), o in zip(params, layout1, offs):
        assert torch.equal(torch.isnan(flat.p[o:o + k]), torch.isnan(q.detach())), "the same entries are NaN"
    assert int(torch.isnan(flat.p).sum()) == 1 and not flat.p[torch.from_numpy(~c["mask"]).to(DEV)].any()
    # a NaN norm gives a NaN coefficient (torch.clamp keeps it)
    gi[offs[6] + 100] = np.nan
    clip = ops.grad_norm(torch.from_numpy(gi).to(DEV), 1.0)
    assert bool(torch.isnan(clip).all())


# ------------------------------------------------------------------ the step -----------------------------------------------------

def vggish(mk, W, finetune=False, ordinals=None):
    torch.manual_seed(77)                                        # Dropout reads the seed at construction
    ens = M.Ensemble("repeat", dict(mk.CNN_CONF), [2, 1], DEV, precision="f32")
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in W.make_state_dict(7, W.ensemble_shapes((2, 1), False)).items()})
    ens.cuda()
    drops = [m for m in ens.mla.modules() if type(m).__name__ == "Dropout"]
    if ordinals is not None:
        for d, o in zip(drops, ordinals):
            d.ordinal = o
    if finetune:
        M.set_requires_grad(ens, True)
    return ens, [d.ordinal for d in drops]


def install(ens, masks):
    for lvl, em in enumerate(ens.mla.embedded_mappings):
        for j, d in enumerate(em.dropouts):
            d.mask = masks["mla.embedded_mappings.%d.dropouts.%d" % (lvl, j)]


def head_groups(ens, amsgrad_on_biases=False, swap=False):
    """Head weights: decay, lr 1e-3 | biases and BatchNorm: no decay, lr 3e-4."""
    named = [(n, p) for n, p in ens.named_parameters() if p.requires_grad and n.startswith("mla.")]
    is_w = lambda n, p: (p.dim() >= 2 and ".norm" not in n) != swap                                # noqa: E731
    return [dict(params=[p for n, p in named if is_w(n, p)], lr=1e-3, weight_decay=1e-2),
            dict(params=[p for n, p in named if not is_w(n, p)], lr=3e-4, weight_decay=0.0, amsgrad=amsgrad_on_biases)]


def test_step_against_torch_adamw_on_identical_gradients(mk, W):
    """After each of three steps the step's own unclipped gradients go to a float32 copy of the parameters, stepped by
    clip_grad_norm_ + torch.optim.AdamW(foreach=False): the optimizer alone is compared. Tolerance: the kernel test's bound
    C_P * 2^-24 * (|p| + |u|), summed over the steps (p, u: the torch copy's value before the step and its update)."""
    ens, _ = vggish(mk, W)
    copies = {n: torch.nn.Parameter(p.detach().clone()) for n, p in ens.named_parameters() if n.startswith("mla.") and p.requires_grad}
    by_id = {id(p): n for n, p in ens.named_parameters()}
    groups = head_groups(ens)
    twin = torch.optim.AdamW([dict(g, params=[copies[by_id[id(p)]] for p in g["params"]]) for g in groups], foreach=False)
    step = TR.TrainStep(ens, optimizer=torch.optim.AdamW(groups), max_grad_norm=0.05, graph=False)
    assert set(step.grads) == {n for n in copies if ".fcf." not in n}
    bound = {n: torch.zeros_like(p, dtype=torch.float64) for n, p in copies.items()}
    live = dict(ens.named_parameters())
    worst = 0.0
    for s in range(3):
        x, y = mk.synth_bags(100 + s, 8)
        install(ens, mk.make_masks(200 + s, [2, 1], 8))
        step(x.cuda(), y.cuda())
        before = {n: p.detach().clone() for n, p in copies.items()}
        for n, p in copies.items():
            p.grad = step.grads[n].clone() if n in step.grads else None
        norm = torch.nn.utils.clip_grad_norm_([p for p in copies.values() if p.grad is not None], 0.05, foreach=False)
        twin.step()
        assert float(step.clip_coef) < 1.0 and abs(float(step.grad_norm) - float(norm)) <= 1e-6 * float(norm)
        for n, p in copies.items():
            bound[n] += C.C_P * C.EPS32 * (before[n].double().abs() + (before[n].double() - p.detach().double()).abs())
            err = (live[n].detach().double() - p.detach().double()).abs()
            if ".fcf." in n:
                assert torch.equal(live[n].detach(), p.detach())
                continue
            ratio = float((err / bound[n].clamp_min(1e-300)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (s, n, ratio)
    print("TrainStep vs torch AdamW: worst |p - p_torch| / bound = %.3f" % worst)


def test_eager_steps_equal_graph_replays_with_a_scheduler(mk, W):
    runs = {}
    ords = None
    for graph in (False, True):
        ens, ords = vggish(mk, W, ordinals=ords)
        opt = torch.optim.AdamW(head_groups(ens, amsgrad_on_biases=True))
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
        step = TR.TrainStep(ens, optimizer=opt, max_grad_norm=0.05, graph=graph)
        trace = []
        for s in range(4):
            x, y = mk.synth_bags(300 + s, 8)
            loss, hits = step(x.cuda(), y.cuda())
            trace.append((float(loss), hits.tolist(), float(step.grad_norm), float(step.clip_coef), [g["lr"] for g in opt.param_groups]))
            sched.step()                                             # halves both lr between steps 2 and 3
        runs[graph] = (trace, step)
    (ref, step_e), (got, step_g) = runs[False], runs[True]
    assert ref[1][4] != ref[2][4], "the lr changed between steps 2 and 3"
    assert got == ref, (got, ref)
    assert step_e._graph is None and step_g._graph is not None and step_g.captures == 1, "a changed lr forces no re-capture"
    for k in ("flat_p", "flat_m", "flat_v", "flat_vmax"):
        assert torch.equal(getattr(step_g, k), getattr(step_e, k)), k
    assert bool(step_g.flat_vmax.any())


def routing(ens, split):
    named = [(n, p) for n, p in ens.named_parameters() if p.requires_grad]
    lrs = {"cnn": 1e-4, "mla": 1e-3}
    opt = torch.optim.Adam([dict(params=[p for n, p in named if split(n) == k], lr=lr) for k, lr in lrs.items()])
    before = {n: p.detach().clone() for n, p in named}
    return TR.TrainStep(ens, optimizer=opt, graph=False), lrs, before


def check_routing(ens, step, lrs, before, split):
    """Adam's first step moves an entry by at most its group's lr (and by nearly lr wherever |g| >> eps): the update u obeys
    |u| <= lr (1 + 1e-5). What the test can see is the stored float32 p' = fl(p - u), half a unit in the last place of p' away
    from p - u, and at |p| = 1 that half unit (6e-8) is 6e-4 of the trunk's lr = 1e-4: measured, the BatchNorm weights near 1 move
    by 1.000047 lr (head, lr 1e-3) and conv1's largest weights by 1.00017 lr (lr 1e-4), each exactly this rounding. The bound on
    the move therefore carries the half unit of the element itself; a wrong group's lr would miss it by a factor of 10."""
    top = {k: 0.0 for k in lrs}
    over = []
    for n, p in ens.named_parameters():
        if n not in step.grads:
            assert n not in before or torch.equal(p.detach(), before[n]), n
            continue
        lr = lrs[split(n)]
        now = p.detach()
        half_ulp = 0.5 * (torch.nextafter(now.abs(), torch.full_like(now, float("inf"))) - now.abs()).double()
        move = (now.double() - before[n].double()).abs()
        excess = float((move - lr * (1 + 1e-5) - half_ulp).max())
        if excess > 0:
            over.append((n, float(move.max()) / lr, excess))
        top[split(n)] = max(top[split(n)], float(move.max()) / lr)
    print("largest move per group, in units of its lr:", top)
    assert not over, over[:8]
    assert all(v > 0.5 for v in top.values()), top


def test_groups_reach_their_tensors_in_the_vggish_finetune(mk, W):
    ens, _ = vggish(mk, W, finetune=True)
    split = lambda n: "cnn" if n.startswith("cnn.") else "mla"                  # noqa: E731
    step, lrs, before = routing(ens, split)
    x, y = mk.synth_bags(100, 2)
    step(x.cuda(), y.cuda())
    check_routing(ens, step, lrs, before, split)


def test_groups_reach_their_tensors_in_the_resnet_trunk():
    from test_resnet_finetune_golden_gpu import RUNS, build
    from test_resnet_golden_gpu import images, labels
    ens = build(RUNS["a"])
    split = lambda n: "cnn" if n.startswith("cnn.") else "mla"                  # noqa: E731
    step, lrs, before = routing(ens, split)
    assert step.rn_trunk
    step(images(10, 2), labels(2, 0))
    check_routing(ens, step, lrs, before, split)


def test_checkpoint_resumes_bit_for_bit_and_refuses_another_layout(mk, W, tmp_path):
    def make(swap=False):
        ens, _ = vggish(mk, W)
        return ens, TR.TrainStep(ens, optimizer=torch.optim.AdamW(head_groups(ens, amsgrad_on_biases=True, swap=swap)), max_grad_norm=0.05)

    def run(ens, step, first, last):
        for s in range(first, last):
            x, y = mk.synth_bags(100 + s, 8)
            install(ens, mk.make_masks(200 + s, [2, 1], 8))
            step(x.cuda(), y.cuda())

    ens_a, step_a = make()
    run(ens_a, step_a, 0, 5)
    ens_b, step_b = make()
    run(ens_b, step_b, 0, 3)
    path = str(tmp_path / "ck.pt")
    torch.save({"model": ens_b.state_dict(), "optimizer": step_b.state_dict()}, path)
    ck = torch.load(path, weights_only=True)                          # tensors only
    assert set(ck["optimizer"]) == {"adam_m", "adam_v", "adam_vmax", "step", "groups", "layout"}
    ens_c, step_c = make()
    ens_c.load_state_dict(ck["model"])
    for g in step_c.groups:
        g["lr"] = 123.0                                               # restored from the checkpoint
    step_c.load_state_dict(ck["optimizer"])
    assert [g["lr"] for g in step_c.groups] == [1e-3, 3e-4] and step_c.t == 3
    run(ens_c, step_c, 3, 5)
    for k in ("flat_p", "flat_m", "flat_v", "flat_vmax"):
        assert torch.equal(getattr(step_c, k), getattr(step_a, k)), k
    for (k, a), (_, b) in zip(ens_c.state_dict().items(), ens_a.state_dict().items()):
        assert torch.equal(a, b), k
    _, other = make(swap=True)
    with pytest.raises(ValueError, match="another layout"):
        other.load_state_dict(ck["optimizer"])
    plain_ens, _ = vggish(mk, W)
    with pytest.raises(ValueError, match="optimizer groups"):
        TR.TrainStep(plain_ens).load_state_dict(ck["optimizer"])
    assert set(TR.TrainStep(vggish(mk, W)[0]).state_dict()) == {"adam_m", "adam_v", "step", "lr", "betas", "eps"}


def test_refusals_of_the_grouped_step(mk, W):
    ens, _ = vggish(mk, W)
    params = [p for p in ens.mla.parameters() if p.requires_grad]
    with pytest.raises(ValueError, match="not both"):
        TR.TrainStep(ens, optimizer=torch.optim.Adam(params), params=params)
    with pytest.raises(ValueError, match="optimizer="):
        TR.TrainStep(ens, max_grad_norm=1.0)
    with pytest.raises(TypeError):
        TR.TrainStep(ens, optimizer=torch.optim.SGD(params, lr=0.1))
    for kw in (dict(maximize=True), dict(capturable=True), dict(differentiable=True), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(NotImplementedError):
            TR.TrainStep(ens, optimizer=torch.optim.Adam(params, **kw))
    opt = torch.optim.Adam([dict(params=params[:2]), dict(params=params[2:])])
    opt.param_groups[1]["params"].append(params[0])
    with pytest.raises(ValueError, match="two optimizer groups"):
        TR.TrainStep(ens, optimizer=opt)


def test_train_model_with_groups_scheduler_and_clipping(mk, W, tmp_path):
    from torch.utils.data import DataLoader, TensorDataset
    x, y = mk.synth_bags(5, 8)
    ds = TensorDataset(torch.as_tensor(x), torch.as_tensor(y))
    loaders = lambda: {"train": DataLoader(ds, batch_size=8), "val": DataLoader(ds, batch_size=8)}          # noqa: E731
    real_eval = TR._evaluate
    # the best-validation weights are restored at the end: pin the accuracy so that the one epoch counts (as tests/test_train_gpu.py does)
    TR._evaluate = lambda *a, **k: (lambda r: (r[0], 0.5) + tuple(r[2:]))(real_eval(*a, **k))
    finals = {}
    try:
        for wd in (1e-1, 0.0):
            ens, _ = vggish(mk, W)
            groups = head_groups(ens)
            groups[0]["weight_decay"] = wd
            opt = torch.optim.AdamW(groups)
            sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
            path = str(tmp_path / ("wd%g.pt" % wd))
            out, hist, tested = TR.train_model(ens, loaders(), torch.nn.CrossEntropyLoss(), opt, num_epochs=1, patience=None,
                                               save_model_path=path, extended_optimizer=True, scheduler=sched, max_grad_norm=1.0)
            assert [g["lr"] for g in opt.param_groups] == [5e-4, 1.5e-4], "the scheduler was stepped once"
            assert len(hist) == 1 and tested is None and not opt.state, "the torch optimizer itself is never stepped"
            assert "layout" in torch.load(path, weights_only=True)["optimizer"]
            finals[wd] = out.mla.fc.weight.detach().clone()
        with pytest.raises(ValueError, match="extended_optimizer"):
            TR.train_model(ens, loaders(), torch.nn.CrossEntropyLoss(), torch.optim.Adam(ens.mla.parameters()), num_epochs=1, max_grad_norm=1.0)
    finally:
        TR._evaluate = real_eval
    assert not torch.equal(finals[1e-1], finals[0.0])


def test_two_ranks_clip_like_one_process_on_the_global_batch(mk, W, tmp_path):
    """Head training under two gloo ranks on one GPU with max_grad_norm low enough to clip: the norm is taken on the all-reduced
    gradient, so both ranks form the same coefficient without a collective of their own. Tolerances: those of
    tests/test_train_gpu.py test_two_ranks_equal_one_rank_on_the_global_batch (there against the reference's losses)."""
    from test_train_gpu import free_port
    import _adam_groups_dp_worker as worker
    steps, B = 4, 8
    out = str(tmp_path / "dp")
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_adam_groups_dp_worker.py"), out, str(steps), str(B)],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    r0, r1 = np.load(out + ".rank0.npz"), np.load(out + ".rank1.npz")
    one = worker.run(steps, B, 0, B, None)
    for k in r0.files:
        np.testing.assert_array_equal(r0[k], r1[k], err_msg=k)          # replicas stay bit-identical, clip_coef included
    assert np.all(r0["clip_coef"] < 1.0) and np.all(one["clip_coef"] < 1.0)
    np.testing.assert_allclose(r0["losses"][:3], one["losses"][:3], rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(r0["losses"], one["losses"], rtol=2e-3, atol=1e-5)
    np.testing.assert_allclose(r0["grad_norm"][0], one["grad_norm"][0], rtol=2e-5)
    for k in r0.files:
        if k.startswith("mla.") and "num_batches" not in k:             # as the frozen-head curve of tests/test_train_gpu.py
            np.testing.assert_allclose(r0[k], one[k], rtol=1e-3, atol=1e-2 if k.endswith("running_mean") else 2e-4, err_msg=k)
