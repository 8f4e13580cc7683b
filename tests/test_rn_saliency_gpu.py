"""Saliency maps of the ResNet branch on the GPU: the stem's data gradient (mla_rn_stem_dgrad) and the eval epilogue's backward
(mla_rn_act_bwd) kernel by kernel, the taped eval-mode trunk forward, the hand-walked input backward (resnet.trunk_input_backward)
and Ensemble.saliency_images / saliency_clips against the float64 restatement (tests/rn_saliency_cases.py)."""

import ctypes
import importlib

import numpy as np
import pytest
import torch

import rn_saliency_cases as C
from conftest import PKG

pytestmark = pytest.mark.gpu

M = importlib.import_module(PKG + ".model")
W = importlib.import_module(PKG + ".weights")
ops = importlib.import_module(PKG + ".ops")
RN = importlib.import_module(PKG + ".resnet")
_lib = importlib.import_module(PKG + "._lib")

CONF = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
            first_cnn_layer_trainable=False, in_channels=3)
DTYPES = [torch.float32, torch.bfloat16]


def tol(dtype):
    return 1e-4 if dtype == torch.float32 else 1e-2          # the bounds of test_resnet_finetune_gpu.py's stem weight gradient


def ensemble(conf="repeat", jb=True, precision="f32", **kw):
    torch.manual_seed(123)                        # just_bottlenecks=False: torch's initialisation of the fc, the same for every call
    ens = M.Ensemble(conf, dict(CONF, just_bottlenecks=jb, **kw), [2, 1], torch.device("cuda"), precision=precision, slots=C.SLOTS)
    missing = ens.load_state_dict(C.state_dict(jb), strict=False)
    assert not missing.unexpected_keys and missing.missing_keys == ([] if jb else ["cnn.cnn_model.fc.weight", "cnn.cnn_model.fc.bias"])
    return ens.cuda().eval()


def fc_of(ens):
    fc = ens.cnn.cnn_model.fc
    return fc.weight.detach().cpu().clone(), fc.bias.detach().cpu().clone()


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. mla_rn_stem_dgrad ------------------------------------------------------------------------------------------------

SENTINEL = float("nan")


def stem_dgrad_guarded(dy, w, single, y=None, scale=None):
    """The C entry writing into the middle of a sentinel-filled buffer with one guard image on either side -> dx (n, 224, 224);
    asserts that the guards kept their bits and that every element between them was written."""
    n = dy.shape[0]
    buf = torch.full((n + 2, 224, 224), SENTINEL, device="cuda")
    before = bits(buf).clone()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    _lib.check(_lib.lib().mla_rn_stem_dgrad(p(dy), n, p(y), p(scale), p(w), int(single), p(buf[1:]), ops.DT[dy.dtype], _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(bits(buf[0]), before[0]) and torch.equal(bits(buf[-1]), before[-1]), "a store outside dx"
    assert not bool(torch.isnan(buf[1:-1]).any()), "an element of dx was not written"
    return buf[1:-1].clone()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("n", [1, 3])
def test_stem_dgrad_against_float64(n, single, epilogue, dtype):
    bf16 = dtype == torch.bfloat16
    dy, y, scale = C.stem_operands(n, bf16=bf16)
    w = C.stem_weight()
    if not epilogue:
        y = scale = None
    ref = C.stem_reference(dy, w, single, y, scale)
    dev = lambda t, dt=None: None if t is None else t.to("cuda", dt)          # noqa: E731
    args = (dev(dy, dtype), dev(w), single, dev(y, dtype), dev(scale))
    dx = stem_dgrad_guarded(*args)
    e = C.rel_max(dx.cpu(), ref)
    print("stem dgrad n %d single %s epilogue %s %s: rel_max %.3g" % (n, single, epilogue, dtype, e))
    assert e <= tol(dtype)
    assert torch.equal(bits(ops.rn_stem_dgrad(*args)), bits(dx)), "the wrapper and a second run give the same bits"
    if n == 3:                                    # the bits of an image do not depend on its neighbours or on the grid
        one = ops.rn_stem_dgrad(args[0][:1].contiguous(), args[1], single, None if y is None else args[3][:1].contiguous(), args[4])
        assert torch.equal(bits(one), bits(dx[:1]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("single", [False, True])
def test_stem_dgrad_one_hot_borders(single, dtype):
    dy = C.one_hot_dy(2)
    w = C.stem_weight()
    ref = C.stem_reference(dy, w, single)
    dx = stem_dgrad_guarded(dy.to("cuda", dtype), w.cuda(), single).cpu()
    assert not bool(dx[0].any()), "an all-zero dy gives an all-zero dx"
    assert torch.equal(dx[1] != 0, ref[1] != 0) and int((dx[1] != 0).sum()) == 16 + 20 + 20 + 25 + 49
    assert C.rel_max(dx, ref) <= 1e-6             # one product per element: f32 rounding of a alone


# ---- 2. mla_rn_act_bwd ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["plain", "relu", "relu_dres"])
@pytest.mark.parametrize("shape", [(1, 7, 7, 64), (3, 14, 14, 256)])
def test_act_bwd(shape, mode, dtype):
    g = torch.Generator().manual_seed(17 + len(mode) + shape[-1])
    dy = torch.randn(shape, generator=g).to(dtype).cuda()
    y = torch.randn(shape, generator=g).clamp_min(0.0).to(dtype).cuda()
    scale = (torch.randn(shape[-1], generator=g) * 0.5 + 1.0).cuda()
    relu, want = mode != "plain", mode == "relu_dres"
    dpre, dres = ops.rn_act_bwd(dy, scale, y=y if relu else None, want_dres=want)
    masked = dy.float() * (y > 0).float() if relu else dy.float()
    assert dpre.dtype == dtype and torch.equal(dpre, (masked * scale).to(dtype))     # f32: as written; bf16: that value rounded once
    if want:
        assert dres.dtype == dtype and torch.equal(dres, masked.to(dtype))
        assert float((dres == 0).float().mean()) > 0.3
    else:
        assert dres is None


# ---- 3. the taped eval forward -------------------------------------------------------------------------------------------

def eval_forward_names():
    """What the untaped eval-mode trunk launches, written from resnet.trunk_forward as it stood before the tape existed."""
    names = ["rn_stem", "rn_maxpool"]
    for n_blocks in (3, 4, 6, 3):
        for k in range(n_blocks):
            names += ["rn_conv1x1", "rn_conv3x3"] + (["rn_conv1x1"] if k == 0 else []) + ["rn_conv1x1"]
    return names + ["rn_avgpool"]


def profiled(fn):
    ops.profile = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, [name for name, _, _ in ops.profile]
    finally:
        ops.profile = None


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_taped_eval_forward_changes_nothing(precision):
    ens = ensemble(precision=precision)
    x = ens.input(C.images().cuda())
    run = lambda tape: RN.trunk_forward(ens.cnn.cnn_model, x, precision, False, ens.cnn._rn_cache, tape=tape)     # noqa: E731
    with torch.no_grad():
        plain, names = profiled(lambda: run(None))
        tape = {}
        taped, names_taped = profiled(lambda: run(tape))
    assert names == eval_forward_names() and names_taped == names
    assert torch.equal(plain, taped)
    records = tape["bn"]
    assert tape["eval"] and len(records) == 53 and len(tape["block_in"]) == 16
    assert sum(r.y is not None for r in records.values()) == 49          # the 48 block units with a ReLU, and the stem
    assert all(r.scale is not None and r.x is None and r.mean is None and r.var is None for r in records.values())
    stem = records[id(RN.parts(ens.cnn.cnn_model)[1])]
    assert tuple(stem.y.shape) == (4, 112, 112, 64) and tape["single"] is False and tape["planes"] is x.planes
    with torch.no_grad():
        assert torch.equal(ens(C.images().cuda()), ens.mla(plain.reshape(-1, C.SLOTS, 2048)))


# ---- 4. / 5. values, f32 -------------------------------------------------------------------------------------------------

def f32_yardstick(jb, fc=None):
    """R: the LARGEST error of the float32 restatement against float64, over the bags and both input configurations."""
    return max(float(C.bag_error(C.oracle(conf, jb, fc)["g32"], C.oracle(conf, jb, fc)["g64"]).max()) for conf in C.CONFS)


def assert_close_f32(what, g, g64, R):
    e, share = C.bag_error(g, g64), C.image_share(g, g64)
    print("%s: R %.3g, e_b %s (e_b / R %s), largest image share %.3g"
          % (what, R, ["%.3g" % v for v in e.tolist()], ["%.2f" % (v / R) for v in e.tolist()], float(share.max())))
    assert bool((e <= 4 * R).all()), (e.tolist(), R)
    assert float(share.max()) <= 0.05, share.tolist()


def test_trunk_input_backward_alone():
    """Measured on the MI355X: DESIGN.md section 4."""
    ens = ensemble()
    cnn_model = ens.cnn.cnn_model
    tape = {}
    with torch.no_grad():
        RN.trunk_forward(cnn_model, ens.input(C.images().cuda()), "f32", False, ens.cnn._rn_cache, tape=tape)
    dx, names = profiled(lambda: RN.trunk_input_backward(cnn_model, tape, C.d_feats().cuda()))
    assert tape == {}, "the walk consumes the tape"
    assert names.count("rn_stem_dgrad") == 1 and names[-1] == "rn_stem_dgrad" and names.count("rn_act_bwd") == 52
    assert not [n for n in names if n.startswith(("rn_wgrad", "rn_stem_wgrad", "rn_bn_bwd"))]
    assert dx.dtype == torch.float32 and tuple(dx.shape) == (4, 224, 224)
    assert all(p.grad is None for p in ens.parameters())
    assert_close_f32("trunk_input_backward f32", dx.cpu().view(C.images().shape), C.trunk_oracle("repeat"), f32_yardstick(True))


@pytest.mark.parametrize("jb", [True, False])
@pytest.mark.parametrize("conf", C.CONFS)
def test_saliency_images_values_f32(conf, jb):
    """Per bag e_b = |g - g64| / |g64| against the float64 restatement; yardstick R = the float32 restatement's own error, the
    largest over the bags and both input configurations (about 6e-3). Required: every e_b <= 4 R (another summation order flips
    other ReLU units than the CPU f32 run did) and no image's share of its bag's norm above 0.05 (a dropped tap of 49 costs about
    14 %, a shifted pixel about 100 %). Measured on the MI355X: DESIGN.md section 4."""
    ens = ensemble(conf, jb)
    fc = None if jb else fc_of(ens)
    o = C.oracle(conf, jb, fc)
    scores, grad = ens.saliency_images(o["x"].cuda(), target=o["target"].cuda())
    np.testing.assert_allclose(scores.double().cpu().numpy(), o["scores64"].numpy(), rtol=1e-4, atol=0)
    assert grad.dtype == torch.float32 and grad.shape == o["x"].shape
    for border in (grad[..., 0, :], grad[..., -1, :], grad[..., :, 0], grad[..., :, -1]):
        assert bool((border != 0).all())
    assert_close_f32("saliency_images f32 %s jb=%s" % (conf, jb), grad.cpu(), o["g64"], f32_yardstick(jb, fc))


# ---- 6. values, bf16 -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("jb", [True, False])
@pytest.mark.parametrize("conf", C.CONFS)
def test_saliency_images_values_bf16(conf, jb):
    """Elementwise agreement means nothing in bf16 (the CPU restatement under autocast sits at cosine 0.96 .. 0.98 per bag against
    float64): required per bag 1 - cos(g_hip, g_64) <= 2 (1 - cos(g_autocast, g_64)), the right-hand side computed here on the same
    inputs; 2x because the HIP bf16 path rounds at other places than autocast (bf16 activations between layers, f32 head).
    Measured on the MI355X: DESIGN.md section 4."""
    ens = ensemble(conf, jb, "bf16")
    fc = None if jb else fc_of(ens)
    o = C.oracle(conf, jb, fc)
    scores, grad = ens.saliency_images(o["x"].cuda(), target=o["target"].cuda())
    mine, yard = C.one_minus_cos(grad.cpu(), o["g64"]), C.one_minus_cos(C.oracle_autocast(conf, jb, fc), o["g64"])
    print("saliency_images bf16 %s jb=%s: cos(hip, f64) %s, cos(autocast, f64) %s" % (conf, jb, (1 - mine).tolist(), (1 - yard).tolist()))
    assert grad.dtype == torch.float32 and bool(torch.isfinite(grad).all())
    assert bool(torch.isfinite(scores).all())
    assert bool((mine <= 2 * yard).all()), (mine.tolist(), yard.tolist())


# ---- 7. the public entries -----------------------------------------------------------------------------------------------

def test_saliency_images_api():
    ens = ensemble(cnn_trainable=True)             # every trunk parameter requires grad: the walk does not care
    assert all(p.requires_grad for p in ens.cnn.parameters())
    x = C.images().cuda()
    before = {k: v.clone() for k, v in ens.state_dict().items()}
    scores, grad = ens.saliency_images(x)
    top = scores.argmax(dim=1)
    assert not scores.requires_grad and tuple(scores.shape) == (2, 10) and grad.shape == x.shape and grad.dtype == torch.float32
    with torch.no_grad():                         # the head behind autograd and the inference head: the same f32 scores within the issue's rtol
        np.testing.assert_allclose(scores.cpu().numpy(), ens(x).cpu().numpy(), rtol=1e-4, atol=0)
    again = ens.saliency_images(x)
    assert torch.equal(again[0], scores) and torch.equal(bits(again[1]), bits(grad))
    assert torch.equal(ens.saliency_images(x, target=top)[1], grad)
    k = (int(top[0]) + 3) % 10
    g_k = ens.saliency_images(x, target=k)[1]
    assert not torch.equal(g_k, grad)
    assert torch.equal(ens.saliency_images(x, target=torch.full((2,), k, dtype=torch.int32))[1], g_k)
    assert torch.equal(ens.saliency_images(x, target=k, times_input=True)[1], g_k * x)
    # nothing of the module moved: mode, parameter gradients, parameters, running statistics
    assert not ens.training and all(p.grad is None for p in ens.parameters())
    after = ens.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[n], v) for n, v in before.items())
    for bad in (10, -1, True, torch.tensor([0, 10]), torch.tensor([0]), torch.tensor([0.0, 1.0]), "3"):
        with pytest.raises(ValueError, match="target"):
            ens.saliency_images(x, target=bad)
    for shape in ((2, 2, 224, 224), (2, 3, 1, 224, 224), (4, 1, 224, 224)):
        with pytest.raises(ValueError, match="saliency_images takes"):
            ens.saliency_images(torch.zeros(shape, device="cuda"))
    with pytest.raises(NotImplementedError, match="train-mode BatchNorm only.*stem has no backward-data"):
        ens.saliency(x)
    ens.train()
    with pytest.raises(RuntimeError, match="eval mode only"):
        ens.saliency_images(x)
    vgg = M.Ensemble("repeat", dict(CONF, cnn_type="vggish", in_channels=1, just_bottlenecks=False), [2, 1], "cpu").eval()
    for call in (lambda: vgg.saliency_images(x), lambda: vgg.saliency_clips(torch.zeros(1, 88200))):
        with pytest.raises(NotImplementedError, match=r"saliency\(\).*saliency_waveforms\(\)"):
            call()


def test_saliency_clips():
    import librosa_restated as LR
    dataset = importlib.import_module(PKG + ".dataset")
    ens = M.Ensemble("single", CONF, [2, 1], torch.device("cuda"), precision="bf16")
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in W.make_state_dict(21, W.ensemble_shapes((2, 1), True, cnn_type="resnet")).items()})
    ens.cuda()
    # running statistics that describe dB images, as in test_melspec_gpu.py::test_forward_clips (the seeded ones describe unit-scale
    # inputs, and the eval-mode head's attention underflows to NaN on images a hundred times larger, as the reference's would)
    wave = lambda name: torch.from_numpy(LR.waveform(name, 88200)[None].astype(np.float32)).cuda()      # noqa: E731
    calib = dataset.clips_to_images(torch.cat([wave("noise"), wave("tones")]))
    ens.train()
    with torch.no_grad():
        for _ in range(30):
            ens(calib)
    ens.eval()
    pcm = wave("chirp")
    scores, images, grad = ens.saliency_clips(pcm, target=4, times_input=True)
    assert tuple(images.shape) == (1, 10, 1, 224, 224) and torch.equal(images, dataset.clips_to_images(pcm))
    assert bool(torch.isfinite(scores).all()) and bool(torch.isfinite(grad).all()) and bool(grad.any())
    ref_scores, ref_grad = ens.saliency_images(images, target=4, times_input=True)
    assert torch.equal(scores, ref_scores) and torch.equal(bits(grad), bits(ref_grad)) and grad.shape == images.shape
