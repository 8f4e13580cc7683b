"""Input gradients of the VGGish branch on the GPU: mla_conv1_dgrad bit for bit against float64 autograd (operands and reference:
tests/conv1_dgrad_cases.py), the opt-in switch through the drop-in modules, Ensemble.saliency / saliency_waveforms, and the values
of a whole saliency map against the float64 CPU oracle (tests/input_grad_cases.py), f32 and bf16."""

import ctypes
import importlib

import numpy as np
import pytest
import torch

import conv1_dgrad_cases as D
import input_grad_cases as G
from conftest import PKG

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def M():
    return importlib.import_module(PKG + ".model")


def ensemble(M, mk, jb=False, precision="f32", frozen=False, **kw):
    ens = M.Ensemble("repeat", dict(mk.CNN_CONF, just_bottlenecks=jb), [2, 1], torch.device("cuda"), precision=precision, **kw)
    ens.load_state_dict(G.state_dict(jb))
    if frozen:
        M.set_requires_grad(ens, False)
    return ens.cuda()


def features_of(ens):
    return ens.cnn.cnn_model[0] if ens.just_bottlenecks else ens.cnn.cnn_model.features


def install(ens, masks):
    for lvl, em in enumerate(ens.mla.embedded_mappings):
        for j, d in enumerate(em.dropouts):
            d.mask = masks["mla.embedded_mappings.%d.dropouts.%d" % (lvl, j)]


# ------------------------------------------------------------------------------------------- 1, 2. the kernel ----

def dgrad_guarded(x, w, b, d):
    """mla_conv1_dgrad into a sentinel-filled buffer between two sentinel-filled guard images -> (dx view, guards untouched?)."""
    L = importlib.import_module(PKG + "._lib")
    n = x.shape[0]
    buf = torch.full((n + 2, 96, 64), D.SENTINEL, dtype=torch.float32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                                    # noqa: E731
    L.check(L.lib().mla_conv1_dgrad(p(x), p(w), p(b), p(d), L.BF16 if d.dtype == BF16 else L.F32, n, p(buf[1]), L.stream_ptr()))
    torch.cuda.synchronize()
    return buf[1:n + 1], bool((buf[0] == D.SENTINEL).all()) and bool((buf[n + 1] == D.SENTINEL).all())


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("n", D.NS + (D.cap_crossing_n(),))
def test_conv1_dgrad_equals_float64_autograd(ops, n, dtype):
    """Grid operands exact in bf16 (conv1_dgrad_cases): the result must EQUAL the float64 reference for an f32 and a bf16 d_pooled;
    every element is overwritten, nothing outside dx is; a second run gives the same bits. n = 97 passes the grid cap."""
    x, w, b, d = (t.cuda() for t in D.T.conv1_bwd_operands(n))
    d = d.to(dtype).contiguous()
    ref = D.reference(n)[0].float().cuda()
    dx, guards_ok = dgrad_guarded(x, w, b, d)
    assert guards_ok, "a store outside dx"
    assert not bool((dx == D.SENTINEL).any()), "an element of dx was not written"
    assert torch.equal(dx, ref)
    again = ops.conv1_dgrad(x, w, b, d)
    torch.cuda.synchronize()
    assert again.dtype == torch.float32 and tuple(again.shape) == (n, 96, 64) and torch.equal(again, dx)


@pytest.mark.parametrize("dtype", [torch.float32, BF16], ids=["f32", "bf16"])
def test_conv1_dgrad_clips_are_independent(ops, dtype):
    x2, w, b, d2 = (t.cuda() for t in D.two_clip_case())
    dx = ops.conv1_dgrad(x2, w, b, d2.to(dtype).contiguous())
    assert torch.equal(dx[0], D.reference(1)[0][0].float().cuda())
    assert not bool(dx[1].any())


# --------------------------------------------------------------------------------- 3. a frozen stack, switch on ----

def backward_names(ops, out):
    ops.profile = []
    try:
        out.sum().backward()
        torch.cuda.synchronize()
        return [n for n, _, _ in ops.profile]
    finally:
        ops.profile = None


def check_frozen(ops, model, x, set_switch):
    with torch.no_grad():
        base = model(x)
    off = model(x)                        # switch off: x.requires_grad is ignored, the call is plain inference
    assert x.grad is None and not off.requires_grad and torch.equal(off, base)
    set_switch(True)
    out = model(x)
    assert out.requires_grad and out.shape == off.shape
    names = backward_names(ops, out)
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == x.dtype and bool(torch.isfinite(x.grad).all())
    assert bool(x.grad.any())
    assert all(p.grad is None for p in model.parameters())
    assert names.count("conv1_dgrad") == 1 and "conv1_bwd" not in names and not [n for n in names if n.startswith("wgrad")], names
    # ... and off again: the same call records nothing
    set_switch(False)
    x.grad = None
    again = model(x)
    assert not again.requires_grad and x.grad is None and torch.equal(again, off)


def test_frozen_vggish_gives_the_input_gradient(ops, mk):
    V = importlib.import_module(PKG + ".torchvggish.vggish")
    torch.manual_seed(5)
    model = V.VGGish(urls=None, pretrained=False, preprocess=False, postprocess=False).cuda().eval()
    for p in model.parameters():
        p.requires_grad = False
    x = mk.synth_bags(31, 1)[0].float().reshape(-1, 1, 96, 64)[:4].cuda().requires_grad_(True)
    check_frozen(ops, model, x, model.set_input_grad)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("jb", [False, True])
def test_frozen_ensemble_gives_the_input_gradient(ops, M, mk, jb, precision):
    ens = ensemble(M, mk, jb, precision, frozen=True).eval()
    x = mk.synth_bags(32, 2)[0].float().cuda().requires_grad_(True)
    check_frozen(ops, ens, x, ens.set_input_grad)


def test_switch_is_a_constructor_keyword_too(M, mk):
    assert features_of(ensemble(M, mk, input_grad=True)).input_grad is True
    assert features_of(ensemble(M, mk)).input_grad is False


# ------------------------------------------------------------------------------------------------ 4. finetune ----

@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_finetune_gradients_do_not_change_with_the_switch(M, mk, precision):
    """All parameters trainable, train mode, injected dropout masks, 4 bags: the same kernels run in the same order, so every p.grad
    is bit for bit the one with the switch off; x.grad comes in addition."""
    x0, y = mk.synth_bags(100, 4)

    def run(flag):
        ens = ensemble(M, mk, False, precision)
        M.set_requires_grad(ens, True)
        ens.set_input_grad(flag).train()
        install(ens, mk.make_masks(200, [2, 1], 4))
        x = x0.float().cuda().requires_grad_(True)
        torch.nn.CrossEntropyLoss()(ens(x), y.cuda()).backward()
        torch.cuda.synchronize()
        return {n: p.grad for n, p in ens.named_parameters()}, x.grad

    g_off, x_off = run(False)
    g_on, x_on = run(True)
    assert x_off is None and x_on is not None and x_on.shape == x0.shape and bool(torch.isfinite(x_on).all()) and bool(x_on.any())
    assert set(g_on) == set(g_off) and sum(g is not None for g in g_off.values()) > 40
    for n, g in g_off.items():
        assert (g is None) == (g_on[n] is None), n
        if g is not None:
            assert torch.equal(g, g_on[n]), n


# ------------------------------------------------------------------------------------------------ 5. saliency ----

def test_saliency_is_autograd_through_the_same_model(M, mk):
    ens = ensemble(M, mk).eval()                               # the head's parameters require grad, the CNN is frozen
    x = mk.synth_bags(33, 2)[0].float().cuda()
    before = {k: v.clone() for k, v in ens.state_dict().items()}

    def by_hand(idx):
        ens.set_input_grad(True)
        xg = x.clone().requires_grad_(True)
        scores = ens(xg)
        idx = scores.detach().argmax(dim=1) if idx is None else idx
        g, = torch.autograd.grad(scores.gather(1, idx.view(-1, 1)).sum(), [xg])
        ens.set_input_grad(False)
        return scores.detach(), idx, g

    ref_scores, top, ref_grad = by_hand(None)
    scores, grad = ens.saliency(x)
    assert not scores.requires_grad and tuple(scores.shape) == (2, 10) and torch.equal(scores, ref_scores)
    assert grad.dtype == torch.float32 and grad.shape == x.shape and torch.equal(grad, ref_grad)       # default target: the arg-max
    assert torch.equal(ens.saliency(x, target=top)[1], ref_grad)
    k = (int(top[0]) + 3) % 10
    fixed = torch.full((2,), k, dtype=torch.long, device="cuda")
    ref_k = by_hand(fixed)[2]
    assert not torch.equal(ref_k, ref_grad)
    assert torch.equal(ens.saliency(x, target=k)[1], ref_k) and torch.equal(ens.saliency(x, target=fixed.cpu().int())[1], ref_k)
    assert torch.equal(ens.saliency(x, target=k, times_input=True)[1], ref_k * x)
    # nothing of the module moved: switch, mode, parameter gradients, parameters and buffers
    assert features_of(ens).input_grad is False and not ens.training
    assert all(p.grad is None for p in ens.parameters()) and any(p.requires_grad for p in ens.parameters())
    after = ens.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], v) for k, v in before.items())
    for bad in (10, -1, torch.tensor([0, 10]), torch.tensor([0]), torch.tensor([0.0, 1.0]), "3"):
        with pytest.raises(ValueError):
            ens.saliency(x, target=bad)
    ens.train()
    with pytest.raises(RuntimeError, match="eval mode only"):
        ens.saliency(x)


def test_saliency_refuses_precisions_and_branches_without_gradients(M, mk):
    x = mk.synth_bags(33, 2)[0].float().cuda()
    x3 = ensemble(M, mk, precision="bf16x3", frozen=True).eval()
    with pytest.raises(NotImplementedError, match="CNN gradients are built for precision"):
        x3.saliency(x)
    # with the switch off bf16x3 infers as ever, grad-requiring input or not
    assert tuple(x3(x.clone().requires_grad_(True)).shape) == (2, 10)
    x3.set_input_grad(True)
    with pytest.raises(NotImplementedError, match="CNN gradients are built for precision"):
        x3(x.clone().requires_grad_(True))
    rn = M.Ensemble("repeat", dict(mk.CNN_CONF, cnn_type="resnet", just_bottlenecks=True, in_channels=3), [2, 1], "cpu").eval()
    with pytest.raises(NotImplementedError, match="train-mode BatchNorm only.*stem has no backward-data"):
        rn.saliency(torch.zeros(1, 10, 1, 224, 224))                  # refused before the device is touched
    with pytest.raises(NotImplementedError, match="train-mode BatchNorm only.*stem has no backward-data"):
        rn.set_input_grad(True)


def test_saliency_waveforms(M, mk, W):
    fe = importlib.import_module(PKG + ".frontend")
    ens = ensemble(M, mk).eval()
    pcm = torch.as_tensor(W.waveform(21, 160000, 2)).cuda()
    scores, examples, grad = ens.saliency_waveforms(pcm, target=4, times_input=True)
    ex = fe.waveforms_to_examples(pcm)
    assert tuple(examples.shape) == (2, 10, 1, 96, 64) and torch.equal(examples.reshape(-1, 96, 64), ex)
    ref_scores, ref_grad = ens.saliency(examples, target=4, times_input=True)
    assert torch.equal(scores, ref_scores) and torch.equal(grad, ref_grad) and grad.shape == examples.shape


# --------------------------------------------------------------------------------------- 6. values, f32 ----

def hip_saliency(M, mk, jb, precision, seed):
    o = G.oracle(jb, seed)
    ens = ensemble(M, mk, jb, precision, frozen=True).eval()
    scores, grad = ens.saliency(o["x"].cuda(), target=o["target"].cuda())
    return o, scores.double().cpu(), grad.double().cpu()


@pytest.mark.parametrize("jb", [False, True])
def test_saliency_values_f32_against_the_float64_oracle(M, mk, jb):
    """Per example e_i = |g_hip,i - g_64,i| / |g_64 of its bag|; yardstick R = the f32 CPU oracle's own error per bag, its maximum
    over the two bags, at a seed where that oracle is flip-free (asserted first). Required: at least 18 of the 20 examples within
    8 R (the HIP convolutions and GEMMs sum in another order, and R differs 2x between the bags) and none above 0.05 (a missing tap or
    shifted pixel costs an example its whole share of the bag norm; a flipped unit stays at or below 1e-2).
    Measured on the MI355X: DESIGN.md section 4."""
    seed = G.SEED_JB1 if jb else G.SEED_JB0
    o = G.oracle(jb, seed)
    r = G.per_example_error(o["g32"], o["g64"])
    R = float(G.bag_error(o["g32"], o["g64"]).max())
    assert float(r.max()) <= G.FLIP_FREE, "the f32 oracle is not flip-free at seed %d" % seed
    if not jb:
        assert R <= 2.2e-5 and float(r.max()) <= 2.1e-5
    o, scores, grad = hip_saliency(M, mk, jb, "f32", seed)
    np.testing.assert_allclose(scores.numpy(), o["scores64"].numpy(), rtol=1e-4, atol=0)
    e = G.per_example_error(grad, o["g64"]).flatten()
    over = int((e > 8 * R).sum())
    print("saliency f32 jb=%s seed %d: R %.3g, e_i max %.3g median %.3g, %d of 20 over 8 R; largest five e_i / R: %s"
          % (jb, seed, R, float(e.max()), float(e.median()), over, " ".join("%.2f" % (v / R) for v in e.sort(descending=True).values[:5].tolist())))
    assert over <= 2, (over, e.tolist())
    assert float(e.max()) <= 0.05, e.tolist()


# -------------------------------------------------------------------------------------- 7. values, bf16 ----

@pytest.mark.parametrize("jb", [False, True])
def test_saliency_values_bf16_against_the_float64_oracle(M, mk, jb):
    """Elementwise agreement means nothing in bf16 (the CPU oracle under autocast sits at cosine 0.95 .. 0.96 per bag against
    float64): required per bag 1 - cos(g_hip, g_64) <= 2 (1 - cos(g_autocast, g_64)), the right-hand side computed here on the same
    inputs; 2x because the HIP bf16 path rounds at other places than autocast (f32 head, f32 master weights, bf16 activations
    between layers). The kernel's own exactness in bf16 is test_conv1_dgrad_equals_float64_autograd's job.
    Measured on the MI355X: DESIGN.md section 4."""
    seed = G.SEED_JB1 if jb else G.SEED_JB0
    o, scores, grad = hip_saliency(M, mk, jb, "bf16", seed)
    mine, yard = G.one_minus_cos(grad, o["g64"]), G.one_minus_cos(G.oracle_autocast(jb, seed), o["g64"])
    print("saliency bf16 jb=%s seed %d: cos(hip, f64) %s, cos(autocast, f64) %s" % (jb, seed, (1 - mine).tolist(), (1 - yard).tolist()))
    assert bool(torch.isfinite(grad).all())
    assert bool((mine <= 2 * yard).all()), (mine.tolist(), yard.tolist())
