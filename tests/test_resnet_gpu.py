"""cnn_type="resnet" on the GPU: the HIP ResNet-50 trunk (csrc/resnet.hip) against a float64 restatement of
torchvision's ResNet-50 v1.5 and the reference's Input normalisation (tests/resnet50_restated.py), the head on top of
it against the oracle, determinism, and the frozen-trunk training step (TrainStep, graphed and eager, and the literal
autograd loop)."""

import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet50_restated as R
from conftest import PKG
from oracle import model as omodel

pytestmark = pytest.mark.gpu

M = importlib.import_module(PKG + ".model")
W = importlib.import_module(PKG + ".weights")
ops = importlib.import_module(PKG + ".ops")
TR = importlib.import_module(PKG + ".train")

CONF = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
            first_cnn_layer_trainable=False, in_channels=3)
SEED = 21


def state_dict():
    return W.make_state_dict(SEED, W.ensemble_shapes((2, 1), True, cnn_type="resnet"))


def images(seed, bags, T=10):
    x = W.uniform(seed, W.stream_id("rn_images"), bags * T * 224 * 224, lo=0.0, hi=1.0)
    return torch.from_numpy(x.reshape(bags, T, 1, 224, 224))


def ensemble(input_conf="repeat", precision="f32", **kw):
    conf = dict(CONF, **kw)
    ens = M.Ensemble(input_conf, conf, [2, 1], torch.device("cuda"), precision=precision)
    if conf["just_bottlenecks"]:
        ens.load_state_dict({k: torch.as_tensor(v) for k, v in state_dict().items()})
    return ens.cuda()


def restated(train):
    ref = R.CNN(True).double()
    ref.load_state_dict({k[4:]: torch.as_tensor(v) for k, v in state_dict().items() if k.startswith("cnn.")})
    return ref.train(train)


def rel_max(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def rel_l2(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


# ---- 1. every conv shape class against F.conv2d in float64 -----------------------------------------------------------------

CONVS = [  # (ks, stride, cin, cout, H, n)
    (1, 1, 64, 256, 14, 3), (1, 1, 256, 64, 9, 5), (1, 2, 256, 512, 14, 3), (3, 1, 64, 64, 9, 5), (3, 2, 128, 128, 10, 3),
    (3, 1, 512, 512, 7, 3), (1, 1, 2048, 512, 7, 3),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ks,stride,cin,cout,H,n", CONVS)
def test_conv_classes(dtype, ks, stride, cin, cout, H, n):
    g = torch.Generator().manual_seed(ks * 1000 + cin + cout + H)
    x = torch.randn(n, H, H, cin, generator=g).to(dtype)
    w = (torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5).to(dtype).float()
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), stride=stride, padding=ks // 2).permute(0, 2, 3, 1)
    res = torch.randn(ref.shape, generator=g).to(dtype)
    wp = ops.rn_repack(w.cuda(), dtype)
    xd = x.cuda()
    tol = 1e-4 if dtype == torch.float32 else 1e-2
    raw = ops.rn_conv(xd, wp, stride).cpu()
    print("conv k%d s%d %d->%d %s: raw max rel %.3g" % (ks, stride, cin, cout, dtype, rel_max(raw, ref)))
    assert rel_max(raw, ref) <= tol
    bn = ref * scale.double() + shift.double()
    got = ops.rn_conv(xd, wp, stride, scale.cuda(), shift.cuda(), relu=True).cpu()
    assert rel_max(got, bn.clamp_min(0)) <= tol
    got = ops.rn_conv(xd, wp, stride, scale.cuda(), shift.cuda(), residual=res.cuda(), relu=True).cpu()
    assert rel_max(got, (bn + res.double()).clamp_min(0)) <= tol


# ---- 2. stem borders -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("conf", ["repeat", "single"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_stem_borders(conf, dtype):
    g = torch.Generator().manual_seed(5)
    x = torch.rand(1, 3, 1, 224, 224, generator=g)
    x[..., :3, :] += 40.0; x[..., -3:, :] -= 40.0; x[..., :, :3] += 25.0; x[..., :, -3:] += 60.0
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.05
    ref = F.conv2d(R.normalize_input(x.double(), conf), w.double(), stride=2, padding=3).permute(0, 2, 3, 1)
    planes = x.reshape(-1, 224, 224).contiguous().cuda()
    got = ops.rn_stem(planes, conf == "single", w.cuda(), dtype).cpu()
    print("stem %s %s: max rel %.3g" % (conf, dtype, rel_max(got, ref)))
    tol = 1e-4 if dtype == torch.float32 else 1e-2
    assert rel_max(got, ref) <= tol
    scale, shift = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g)
    got = ops.rn_stem(planes, conf == "single", w.cuda(), dtype, scale.cuda(), shift.cuda(), relu=True).cpu()
    assert rel_max(got, (ref * scale.double() + shift.double()).clamp_min(0)) <= tol


# ---- 3. whole trunk (eval and train) and the Ensemble scores ---------------------------------------------------------------

@pytest.mark.parametrize("conf", ["repeat", "single"])
def test_trunk_eval_and_scores(conf):
    x = images(1, 1)
    ref_feat = restated(False)(R.normalize_input(x.double(), conf))
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in omodel.to_torch(state_dict()).items()}
    ref_scores = omodel.mla_forward(sd64, ref_feat.reshape(1, 10, 2048))
    for prec in ("f32", "bf16"):
        ens = ensemble(conf, prec).eval()
        with torch.no_grad():
            feat = ens.cnn(ens.input(x.cuda())).cpu()
            scores = ens(x.cuda()).cpu()
        e_feat, e_sc = rel_max(feat, ref_feat), float((scores.double() - ref_scores).abs().max())
        print("eval %s %s: features max rel %.3g, rel L2 %.3g; scores max abs %.3g" % (conf, prec, e_feat, rel_l2(feat, ref_feat), e_sc))
        if prec == "f32":
            assert e_feat <= 1e-4 and e_sc <= 1e-4
        else:
            assert rel_l2(feat, ref_feat) <= 3e-2 and e_sc <= 1e-2


def test_trunk_train_mode_statistics():
    x = images(2, 1)[:, :6]                       # 6 images
    ref = restated(True)
    ref_feat = ref(R.normalize_input(x.double(), "repeat"))
    ens = ensemble().train()
    with torch.no_grad():
        feat = ens.cnn(ens.input(x.cuda())).cpu()
    e = rel_max(feat, ref_feat)
    ref_sd, got_sd = ref.state_dict(), ens.cnn.state_dict()
    n_bn, worst = 0, 0.0
    for k, v in ref_sd.items():
        if k.endswith("num_batches_tracked"):
            assert int(got_sd[k]) == 1, k
            n_bn += 1
        elif k.endswith("running_mean") or k.endswith("running_var"):
            worst = max(worst, float((got_sd[k].double().cpu() - v).abs().max() / v.abs().max()))
    print("train: features max rel %.3g, running stats worst rel %.3g" % (e, worst))
    assert n_bn == 53
    assert e <= 1e-4 and worst <= 1e-5


# ---- 4./5. determinism -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_bag_score_independent_of_batch(prec):
    x = images(3, 7).cuda()
    ens = ensemble(precision=prec).eval()
    with torch.no_grad():
        full = ens(x)
        one = ens(x[4:5].contiguous())
    assert torch.equal(full[4:5], one)


def test_train_forward_bit_identical():
    x = images(4, 1).cuda()
    ens = ensemble(precision="bf16").train()
    with torch.no_grad():
        a = ens.cnn(ens.input(x))
        b = ens.cnn(ens.input(x))
    assert torch.equal(a, b)
    assert int(ens.cnn.cnn_model[1].num_batches_tracked) == 2


# ---- 6./7. training the head on the frozen trunk ---------------------------------------------------------------------------

def labels(bags, seed=0):
    return torch.tensor([(3 * i + seed) % 10 for i in range(bags)], dtype=torch.long)


def steps_with_trainstep(graph, ordinals=None):
    torch.manual_seed(77)
    ens = ensemble(precision="bf16")
    drops = [m for m in ens.mla.modules() if type(m).__name__ == "Dropout"]
    if ordinals is not None:
        for d, o in zip(drops, ordinals):
            d.ordinal = o
    step = TR.TrainStep(ens, lr=1e-3, graph=graph)
    losses = []
    for s in range(3):
        loss, hits = step(images(10 + s, 2).cuda(), labels(2, s).cuda())
        losses.append(float(loss))
    return ens, step, losses, [d.ordinal for d in drops]


def test_trainstep_graphed_equals_eager():
    ens_e, step_e, loss_e, ords = steps_with_trainstep(False)
    ens_g, step_g, loss_g, _ = steps_with_trainstep(True, ords)
    assert step_g._graph is not None and step_e._graph is None
    print("TrainStep losses", loss_e)
    assert loss_g == loss_e and all(np.isfinite(loss_e))
    for (k, a), (_, b) in zip(ens_g.state_dict().items(), ens_e.state_dict().items()):
        assert torch.equal(a, b), k
    assert int(ens_e.cnn.cnn_model[1].num_batches_tracked) == 3
    ref = state_dict()
    for k, v in ens_e.cnn.state_dict().items():                 # trunk weights frozen
        if v.dim() == 4:
            assert torch.equal(v.cpu(), torch.as_tensor(ref["cnn." + k])), k


def test_autograd_loop_matches_trainstep():
    masks = {}
    ens_a = ensemble()
    ens_t = ensemble()
    for ens in (ens_a, ens_t):
        for lvl, em in enumerate(ens.mla.embedded_mappings):
            for j, d in enumerate(em.dropouts):
                d.mask = torch.from_numpy(W.keep_mask(5, W.stream_id("rn_mask/%d/%d" % (lvl, j)), 2 * 10 * 600, 0.4))
    params = [p for p in ens_a.parameters() if p.requires_grad]
    assert not any(p is q for p in params for q in ens_a.cnn.parameters())
    opt = torch.optim.Adam(params, lr=1e-3)
    crit = torch.nn.CrossEntropyLoss()
    step = TR.TrainStep(ens_t, lr=1e-3)
    la, lt = [], []
    ens_a.train()
    for s in range(3):
        x, y = images(10 + s, 2).cuda(), labels(2, s).cuda()
        opt.zero_grad()
        loss = crit(ens_a(x), y)
        loss.backward()
        opt.step()
        la.append(float(loss.detach()))
        lt.append(float(step(x, y)[0]))
    print("autograd losses", la, "TrainStep losses", lt)
    assert np.allclose(la, lt, rtol=1e-5, atol=1e-6)
    noisy = ("fc.bias", "fc.0.bias", "fc.1.bias", "fcv.bias")   # biases in front of a train-mode BatchNorm: zero gradient
    for (k, a), (_, b) in zip(ens_a.mla.state_dict().items(), ens_t.mla.state_dict().items()):
        if not k.endswith(noisy):                 # tolerances of test_autograd_gpu.py (torch Adam vs the fused Adam)
            assert torch.allclose(a.float(), b.float(), rtol=5e-3, atol=4e-3), k


# ---- 8. what must raise ----------------------------------------------------------------------------------------------------

def test_trunk_gradient_requests_raise():
    ens = ensemble(cnn_trainable=True)
    with pytest.raises(NotImplementedError, match="cnn.cnn_model"):
        TR.TrainStep(ens)
    with pytest.raises(NotImplementedError, match="cnn.cnn_model"):
        ens.train()(images(1, 1).cuda())
    ens = ensemble(first_cnn_layer_trainable=True)
    with pytest.raises(NotImplementedError, match="cnn.cnn_model.0.weight"):
        TR.TrainStep(ens)
    with pytest.raises(ValueError):
        ens.eval()(torch.zeros(1, 10, 1, 225, 224, device="cuda"))
