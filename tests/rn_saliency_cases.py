"""Operands and float64 references that tests/test_rn_stem_dgrad_cpu.py and tests/test_rn_saliency_gpu.py share, each computed once.
Device-free.

1. The stem's data gradient (mla_rn_stem_dgrad): dy / y / scale / w operands and torch's conv2d_input in float64 with Input's fold
   applied (the channels that carry x, each over its std, summed).
2. The ResNet branch's saliency maps: the gradient of scores[b, target_b] with respect to the images through
   tests/resnet50_restated.py's CNN in eval mode behind normalize_input, then oracle.model.mla_forward -- in float64 (the reference),
   in float32 (the yardstick of the f32 comparison) and under torch.autocast("cpu", bfloat16) (the yardstick of the bf16 one). 2 bags
   of 2 slots: 4 images, about 1.5 s per float64 case. ReLU and max-pool routing make the gradient discontinuous (a unit that flips
   in f32 is a discrete event), so errors are taken per bag and per image relative to the bag's gradient norm."""

import functools
import importlib

import torch
from torch.nn.grad import conv2d_input

import resnet50_restated as R
from conftest import PKG
from oracle import model as OM

W = importlib.import_module(PKG + ".weights")

SEED, IMG_SEED = 21, 31
BAGS, SLOTS = 2, 2
MODEL_CONF = (2, 1)
CONFS = ("repeat", "single")
NUMBERED = {"0": "conv1", "1": "bn1", "4": "layer1", "5": "layer2", "6": "layer3", "7": "layer4"}


# ---------------------------------------------------------------------------------------------- stem data gradient ----

def stem_weight():
    """The stem conv of the trunk the saliency tests load: (64, 3, 7, 7) f32."""
    return torch.as_tensor(W.make_state_dict(SEED, W.resnet50_shapes("cnn.cnn_model.", True))["cnn.cnn_model.0.weight"])


def stem_operands(n, bf16=False, seed=5):
    """dy, y (n, 112, 112, 64) and scale (64): random dy, a y with about half its entries <= 0 (a few exact zeros and a NaN, which
    route nothing), positive and negative scales. bf16: the values a bf16 tensor holds."""
    g = torch.Generator().manual_seed(seed * 100 + n)
    dy = torch.randn(n, 112, 112, 64, generator=g)
    y = torch.randn(n, 112, 112, 64, generator=g).clamp_min(0.0)
    y[0, 0, 0, 0] = float("nan")
    scale = torch.randn(64, generator=g) * 0.5 + 1.0
    if bf16:
        dy, y = dy.bfloat16().float(), y.bfloat16().float()
    return dy, y, scale


def one_hot_dy(n=1):
    """dy that is 1 at the four corner outputs and one interior output, each in its own channel: pins the tap map at the borders,
    where input rows / columns 0, 1, 222, 223 lose taps."""
    dy = torch.zeros(n, 112, 112, 64)
    for k, (oy, ox) in enumerate(((0, 0), (0, 111), (111, 0), (111, 111), (57, 30))):
        dy[n - 1, oy, ox, 7 * k + 3] = 1.0
    return dy


def folded_weight(w, single):
    """(64, 1, 7, 7) float64: the forward's coefficient of x per tap, a = sum over the channels that carry x of w_c / std_c."""
    w = w.double()
    chans = (0,) if single else (0, 1, 2)
    return sum(w[:, c:c + 1] / R.STD[c] for c in chans)


def stem_reference(dy, w, single, y=None, scale=None):
    """float64 dx (n, 224, 224): conv2d_input of the folded one-channel conv on g = dy [* (y > 0) * scale]."""
    g = dy.double()
    if y is not None:
        g = g * (y > 0).double() * scale.double()
    n = dy.shape[0]
    return conv2d_input((n, 1, 224, 224), folded_weight(w, single), g.permute(0, 3, 1, 2), stride=2, padding=3)[:, 0]


def rel_max(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------------------- saliency maps ----

def images():
    x = W.uniform(IMG_SEED, W.stream_id("rn_images"), BAGS * SLOTS * 224 * 224, lo=0.0, hi=1.0)
    return torch.from_numpy(x.reshape(BAGS, SLOTS, 1, 224, 224))


@functools.lru_cache(maxsize=None)
def state_dict(jb):
    """Ensemble.state_dict() entries for slots = 2: the issue's trunk and head for just_bottlenecks=True; for False the same trunk
    under torchvision's names, a head of input width 10, and NO fc (the model's own initialisation stays, see fc_of)."""
    trunk = W.make_state_dict(SEED, W.resnet50_shapes("cnn.cnn_model.", True))
    if jb:
        sd = dict(trunk)
        sd.update(W.make_state_dict(SEED, W.mla_shapes(MODEL_CONF, 2048, T=SLOTS)))
    else:
        sd = {}
        for k, v in trunk.items():
            head, rest = k[len("cnn.cnn_model."):].split(".", 1)
            sd["cnn.cnn_model.%s.%s" % (NUMBERED[head], rest)] = v
        sd.update(W.make_state_dict(SEED, W.mla_shapes(MODEL_CONF, 10, T=SLOTS)))
    return {k: torch.as_tensor(v) for k, v in sd.items()}


def restated(jb, dtype, fc=None):
    """(CNN of resnet50_restated in eval mode, head state dict) in `dtype`; fc = (weight, bias) for just_bottlenecks=False."""
    sd = state_dict(jb)
    cnn = R.CNN(jb, 10)
    own = {k[4:]: v for k, v in sd.items() if k.startswith("cnn.")}
    if not jb:
        own["cnn_model.fc.weight"], own["cnn_model.fc.bias"] = fc
    cnn.load_state_dict(own)
    cast = lambda v: v.to(dtype) if v.is_floating_point() else v          # noqa: E731
    return cnn.to(dtype).eval(), {k: cast(v) for k, v in sd.items() if k.startswith("mla.")}


def _maps(conf, jb, fc, dtype, target, autocast=False):
    cnn, head = restated(jb, dtype, fc)
    x = images().to(dtype).requires_grad_(True)

    def forward():
        feats = cnn(R.normalize_input(x, conf))
        return OM.mla_forward(head, feats.reshape(BAGS, SLOTS, -1), MODEL_CONF)

    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            scores = forward()
    else:
        scores = forward()
    scores = scores.double()
    idx = scores.detach().argmax(dim=1) if target is None else target
    g, = torch.autograd.grad(scores.gather(1, idx.view(-1, 1)).sum(), [x])
    return scores.detach(), idx, g.detach().double()


_ORACLE = {}


def oracle(conf, jb, fc=None):
    """dict: x (2, 2, 1, 224, 224) f32, target (2,) = the float64 arg-max, scores64, g64, and g32 (the float32 restatement's
    gradient for the same targets). fc: the (weight, bias) f32 CPU tensors of the model under test for just_bottlenecks=False (the
    model's own torch initialisation); cached per (conf, jb), so it must be the same at every call."""
    key = (conf, jb)
    if key not in _ORACLE:
        scores64, target, g64 = _maps(conf, jb, fc, torch.float64, None)
        _ORACLE[key] = dict(x=images(), target=target, scores64=scores64, g64=g64, fc=fc,
                            g32=_maps(conf, jb, fc, torch.float32, target)[2])
    o = _ORACLE[key]
    assert jb or (torch.equal(o["fc"][0], fc[0]) and torch.equal(o["fc"][1], fc[1])), "oracle() is cached per (conf, jb): one fc"
    return o


_AUTOCAST = {}


def oracle_autocast(conf, jb, fc=None):
    key = (conf, jb)
    if key not in _AUTOCAST:
        _AUTOCAST[key] = _maps(conf, jb, fc, torch.float32, oracle(conf, jb, fc)["target"], autocast=True)[2]
    return _AUTOCAST[key]


def d_feats():
    return torch.randn(BAGS * SLOTS, 2048, generator=torch.Generator().manual_seed(4)) * 0.05


@functools.lru_cache(maxsize=None)
def trunk_oracle(conf):
    """float64 gradient of (features * d_feats).sum() with respect to the images through the eval-mode trunk alone -> x's shape."""
    cnn, _ = restated(True, torch.float64)
    x = images().double().requires_grad_(True)
    g, = torch.autograd.grad((cnn(R.normalize_input(x, conf)) * d_feats().double()).sum(), [x])
    return g.detach()


def bag_error(g, g64):
    """e_b = |g - g64|_2 / |g64|_2 per bag -> (2,)."""
    return (g.double() - g64).flatten(1).norm(dim=1) / g64.flatten(1).norm(dim=1)


def image_share(g, g64):
    """|g_i - g64_i|_2 / |g64 of the image's bag|_2 -> (2, 2)."""
    return (g.double() - g64).flatten(2).norm(dim=2) / g64.flatten(1).norm(dim=1, keepdim=True)


def one_minus_cos(g, g64):
    a, b = g.double().flatten(1), g64.flatten(1)
    return 1.0 - (a * b).sum(dim=1) / (a.norm(dim=1) * b.norm(dim=1))
