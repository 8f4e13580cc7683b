"""cnn_type="resnet" against tests/golden/resnet.npz, which the REFERENCE's own Ensemble / Input / CNN / CnnFlatten / MLA code
produced in float64 (tests/golden/make_golden_resnet.py): eval scores and features of both just_bottlenecks branches and
both channel configurations, the 53 running statistics after one train-mode forward, and three literal training steps
(frozen trunk, torch Adam; the fc of just_bottlenecks=False trained too) through TrainStep and through autograd. Also: eval
after graph-replayed training steps uses the running statistics those steps left."""

import importlib

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu

M = importlib.import_module(PKG + ".model")
W = importlib.import_module(PKG + ".weights")
TR = importlib.import_module(PKG + ".train")

SEED = 21
NOISY = ("fc.bias", "fc.0.bias", "fc.1.bias", "fcv.bias")     # biases in front of a train-mode BatchNorm: zero gradient


def conf(jb):
    return dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=jb, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)


def build(jb, input_conf="repeat", precision="f32"):
    ens = M.Ensemble(input_conf, conf(jb), [2, 1], torch.device("cuda"), precision=precision)
    sd = W.make_state_dict(SEED, W.ensemble_shapes((2, 1), jb, cnn_type="resnet", num_classes=10))
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    return ens.cuda()


def images(seed, bags, T=10):
    x = W.uniform(seed, W.stream_id("rn_images"), bags * T * 224 * 224, lo=0.0, hi=1.0)
    return torch.from_numpy(x.reshape(bags, T, 1, 224, 224)).cuda()


def labels(bags, seed=0):
    return torch.tensor([(3 * i + seed) % 10 for i in range(bags)], dtype=torch.long).cuda()


def inject(ens, seed, bags):
    for lvl, em in enumerate(ens.mla.embedded_mappings):
        for j, d in enumerate(em.dropouts):
            key = "mla.embedded_mappings.%d.dropouts.%d" % (lvl, j)
            d.mask = torch.from_numpy(W.keep_mask(seed, W.stream_id(key), bags * 10 * 600, 0.4))


@pytest.mark.parametrize("jb", [True, False])
@pytest.mark.parametrize("input_conf", ["repeat", "single"])
def test_eval_against_reference(golden, jb, input_conf):
    g = golden("resnet")
    tag = "eval/%s/%s" % ("jb" if jb else "fc", input_conf)
    x = images(1, 1)
    for prec, tol in (("f32", 1e-4), ("bf16", 1e-2)):
        ens = build(jb, input_conf, prec).eval()
        with torch.no_grad():
            feats = ens.cnn(ens.input(x)).cpu().numpy()
            scores = ens(x).cpu().numpy()
        ref_f = g[tag + "/features"]
        got_f = feats[:2] if jb else feats
        e_f = float(np.abs(got_f - ref_f).max() / np.abs(ref_f).max())
        e_s = float(np.abs(scores - g[tag + "/scores"]).max())
        print("%s %s: features max rel %.3g, scores max abs %.3g" % (tag, prec, e_f, e_s))
        assert e_s <= tol
        if prec == "f32":
            assert e_f <= 1e-4
        else:
            assert float(np.linalg.norm(got_f - ref_f) / np.linalg.norm(ref_f)) <= 3e-2


def test_running_statistics_against_reference(golden):
    g = golden("resnet")
    ens = build(True).train()
    inject(ens, 3, 2)
    with torch.no_grad():
        ens(images(2, 2))
    worst, n = 0.0, 0
    for k, v in ens.cnn.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            ref = g["trainfwd/" + k]
            worst = max(worst, float(np.abs(v.cpu().numpy() - ref).max() / np.abs(ref).max()))
        elif k.endswith("num_batches_tracked"):
            assert int(v) == int(g["trainfwd/" + k]) == 1, k
            n += 1
    print("running statistics worst rel %.3g" % worst)
    assert n == 53 and worst <= 1e-5


def _check_training(g, tag, ens, losses):
    print(tag, "losses", losses, "reference", g[tag + "/losses"].tolist())
    np.testing.assert_allclose(losses[:2], g[tag + "/losses"][:2], rtol=5e-5, atol=1e-6)
    np.testing.assert_allclose(losses, g[tag + "/losses"], rtol=2e-3, atol=1e-5)
    sd = ens.state_dict()
    checked = 0
    for key in g.files:
        if not key.startswith(tag + "/final/"):
            continue
        name = key[len(tag) + 7:]
        if name.endswith(NOISY) or name.endswith("fcf.weight") or name.endswith("fcf.bias"):
            continue
        got = sd[name[:-4]][:8] if name.endswith("[:8]") else sd[name]
        atol = 1e-2 if name.endswith("running_mean") else 4e-3
        rtol = 2e-2 if name.endswith("running_var") else 5e-3
        np.testing.assert_allclose(got.cpu().numpy(), g[key], rtol=rtol, atol=atol, err_msg=name)
        checked += 1
    assert checked >= 30
    ens.eval()
    with torch.no_grad():
        np.testing.assert_allclose(ens(images(99, 1)).cpu().numpy(), g[tag + "/eval_after"], rtol=0, atol=2e-2)


@pytest.mark.parametrize("jb", [True, False])
def test_trainstep_against_reference(golden, jb):
    g = golden("resnet")
    ens = build(jb)
    step = TR.TrainStep(ens, lr=1e-3)
    assert ("cnn.cnn_model.fc.weight" in step.grads) == (not jb)
    losses = []
    for s in range(3):
        inject(ens, 200 + s, 2)
        losses.append(float(step(images(10 + s, 2), labels(2, s))[0]))
    _check_training(g, "train/%s" % ("jb" if jb else "fc"), ens, losses)


@pytest.mark.parametrize("jb", [True, False])
def test_autograd_loop_against_reference(golden, jb):
    g = golden("resnet")
    ens = build(jb)
    params = [p for p in ens.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-3)
    crit = torch.nn.CrossEntropyLoss()
    ens.train()
    losses = []
    for s in range(3):
        inject(ens, 200 + s, 2)
        opt.zero_grad()
        loss = crit(ens(images(10 + s, 2)), labels(2, s))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    if not jb:
        assert ens.cnn.cnn_model.fc.weight.grad is not None
    _check_training(g, "train/%s" % ("jb" if jb else "fc"), ens, losses)


@pytest.mark.parametrize("jb", [True, False])
def test_eval_after_graphed_steps_sees_new_running_statistics(jb):
    torch.manual_seed(5)
    ens = build(jb, precision="bf16")
    step = TR.TrainStep(ens, lr=1e-3, graph=True)
    x, y, xe = images(30, 2), labels(2), images(31, 1)
    evals = []
    for rnd in range(2):
        for _ in range(2):
            step(x, y)
        assert step._graph is not None                  # the second step of a shape (and every later one) is a replay
        ens.eval()
        with torch.no_grad():
            got = ens(xe)
            ens.cnn._rn_cache["bn"].key = None          # coefficients recomputed from the running statistics of now
            fresh = ens(xe)
        assert torch.equal(got, fresh), rnd
        evals.append(got)
        ens.train()
    assert not torch.equal(evals[0], evals[1])
    assert int(ens.cnn.cnn_model.state_dict()["bn1.num_batches_tracked" if not jb else "1.num_batches_tracked"]) == 4
