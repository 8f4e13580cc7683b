"""Shape-only recorders for the ``ops.rn_*`` wrappers the ResNet trunk walks call (resnet.trunk_forward, trunk_backward,
trunk_input_backward), and the scenarios traced with them: which wrapper is called when, with which tensors. No value is
computed, no library and no device is needed. Shared by tests/test_resnet_walk_cpu.py and the generator of its fixture,
tests/golden/make_golden_resnet_walk.py; neither looks inside a tape (its layout is resnet.py's own business)."""

import hashlib
import inspect
import json

import torch
from torch import nn

PRECISIONS = {"f32": torch.float32, "bf16": torch.bfloat16}
CONFIGS = [(jb, precision) for jb in (True, False) for precision in PRECISIONS]
N = 2                                             # images per trace
LAYER3_2 = 3 + 4 + 2                              # index of layer3.2 among the 16 blocks


class Tracer:
    """The log of one trace: (name, {argument: value}, [results]) per call. A tensor is written as a small integer standing for
    its (data_ptr, shape), numbered by first appearance: ``conv.weight.detach().contiguous()`` is the parameter again, and a
    view of another shape is not. Every tensor seen stays alive until the next begin(), so no address is handed out twice."""

    def begin(self):
        self.log, self.keep, self.ids = [], [], {}

    def tensor(self, t):
        self.keep.append(t)
        return {"t": self.ids.setdefault((t.data_ptr(), tuple(t.shape)), len(self.ids)), "shape": list(t.shape), "dtype": str(t.dtype)}

    def value(self, v):
        if isinstance(v, torch.Tensor):
            return self.tensor(v)
        if isinstance(v, nn.Module):              # a BatchNorm2d: known by its weight
            return {"bn": self.tensor(v.weight)["t"]}
        if isinstance(v, torch.dtype):
            return str(v)
        if isinstance(v, (tuple, list)):
            return [self.value(e) for e in v]
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        return type(v).__name__                   # the Dist stand-in

    def recorder(self, fn):
        sig = inspect.signature(fn)

        def call(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            entry = [fn.__name__, {k: self.value(v) for k, v in bound.arguments.items()}, None]
            self.log.append(entry)                # logged before the results exist: the arguments are numbered first
            out = fn(*args, **kwargs)
            entry[2] = self.value(out)
            return out
        return call

    def names(self):
        return [e[0] for e in self.log]

    def sha256(self):
        return hashlib.sha256(json.dumps(self.log, sort_keys=True).encode()).hexdigest()


class LocalDist:
    bn_active = False


def _new(shape, dtype):
    return torch.empty(tuple(int(s) for s in shape), dtype=dtype)


def _like(t, want=True):
    return torch.empty_like(t) if want else None


# ---- the wrappers' signatures and result shapes, as ops.py has them ----

def _local():
    return LocalDist()


def rn_repack(w, dtype):
    return _new((w.shape[0], w.shape[2], w.shape[3], w.shape[1]), dtype)


def rn_stem(planes, single, w, dtype, scale=None, shift=None, relu=False):
    assert planes.dim() == 3 and planes.dtype == torch.float32
    return _new((planes.shape[0], 112, 112, 64), dtype)


def rn_conv(x, w_packed, stride, scale=None, shift=None, residual=None, relu=False):
    n, H, W_, cin = x.shape
    cout, ks = w_packed.shape[0], w_packed.shape[1]
    assert w_packed.shape[3] == cin and w_packed.dtype == x.dtype and (scale is None) == (shift is None)
    pad = ks // 2
    out = _new((n, (H + 2 * pad - ks) // stride + 1, (W_ + 2 * pad - ks) // stride + 1, cout), x.dtype)
    assert residual is None or (residual.shape == out.shape and residual.dtype == x.dtype)
    return out


def rn_bn_stats_sync(x, bn, dist, running=True, want_stats=False):
    assert x.shape[-1] == bn.num_features
    return tuple(_new((x.shape[-1],), torch.float32) for _ in range(4 if want_stats else 2))


def rn_bn_eval_coeffs(bn):
    return _new((bn.num_features,), torch.float32), _new((bn.num_features,), torch.float32)


def rn_bn_apply(x, scale, shift, residual=None, relu=False, out=None):
    assert residual is None or residual.shape == x.shape
    assert out is None or (out.shape == x.shape and out.dtype == x.dtype)
    return x if out is None else out


def rn_maxpool(x):
    n, H, W_, C = x.shape
    return _new((n, (H - 1) // 2 + 1, (W_ - 1) // 2 + 1, C), x.dtype)


def rn_avgpool(x):
    return _new((x.shape[0], x.shape[3]), torch.float32)


def rn_repack_dgrad(w, dtype):
    return _new((w.shape[1], w.shape[2], w.shape[3], w.shape[0]), dtype)


def rn_conv_dgrad(dy, w_dgrad, stride, in_hw, residual=None):
    assert w_dgrad.shape[3] == dy.shape[3] and w_dgrad.dtype == dy.dtype
    out = _new((dy.shape[0], in_hw[0], in_hw[1], w_dgrad.shape[0]), dy.dtype)
    assert residual is None or (residual.shape == out.shape and residual.dtype == dy.dtype)
    return out


def rn_conv_wgrad(x, dy, stride, dw):
    assert dw.dtype == torch.float32 and dw.shape[0] == dy.shape[3] and dw.shape[1] == x.shape[3] and dy.dtype == x.dtype


def rn_stem_wgrad(planes, single, dy, dw):
    assert tuple(dw.shape) == (64, 3, 7, 7) and tuple(dy.shape) == (planes.shape[0], 112, 112, 64)


def rn_bn_bwd_sync(x, dy, mean, var, bn, dist, y=None, want_dres=False, dgamma=None, dbeta=None):
    assert dy.shape == x.shape and dy.dtype == x.dtype and mean.numel() == var.numel() == x.shape[-1]
    assert y is None or (y.shape == x.shape and y.dtype == x.dtype)
    return _like(x), _like(x, want_dres)


def rn_maxpool_bwd(x, dy):
    assert dy.dtype == x.dtype and tuple(dy.shape) == tuple(rn_maxpool(x).shape)
    return _like(x)


def rn_avgpool_bwd(d, shape, dtype):
    assert tuple(d.shape) == (shape[0], shape[3]) and d.dtype == torch.float32
    return _new(shape, dtype)


def rn_act_bwd(dy, scale, y=None, want_dres=False):
    assert scale.numel() == dy.shape[-1] and (y is None or (y.shape == dy.shape and y.dtype == dy.dtype))
    return _like(dy), _like(dy, want_dres)


def rn_stem_dgrad(dy, w, single, y=None, scale=None):
    assert tuple(dy.shape[1:]) == (112, 112, 64) and (y is None) == (scale is None)
    assert y is None or (y.shape == dy.shape and y.dtype == dy.dtype and scale.numel() == 64)
    return _new((dy.shape[0], 224, 224), torch.float32)


RECORDED = [rn_repack, rn_stem, rn_conv, rn_bn_stats_sync, rn_bn_eval_coeffs, rn_bn_apply, rn_maxpool, rn_avgpool, rn_repack_dgrad,
            rn_conv_dgrad, rn_conv_wgrad, rn_stem_wgrad, rn_bn_bwd_sync, rn_maxpool_bwd, rn_avgpool_bwd, rn_act_bwd, rn_stem_dgrad]


def install(ops, setattr_):
    """Replace the 17 wrappers and ``_local`` of `ops` through setattr_(ops, name, value) (monkeypatch.setattr in a test,
    plain setattr in a script that ends afterwards) -> the Tracer they write to."""
    tracer = Tracer()
    tracer.begin()
    for fn in RECORDED:
        setattr_(ops, fn.__name__, tracer.recorder(fn))
    setattr_(ops, "_local", _local)
    return tracer


# ---- the scenarios ----

def new_model(M, jb, precision, trainable):
    return M.CNN(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=jb, cnn_trainable=trainable,
                 precision=precision, trunk_backward=True)


def stem_input(RN):
    return RN.StemInput(torch.empty(N, 224, 224), False)


def taped_eval_forward(RN, cnn, precision):
    tape = {}
    with torch.no_grad():
        RN.trunk_forward(cnn.cnn_model, stem_input(RN), precision, False, cnn._rn_cache, tape=tape)
    return tape


def grad_sets(RN, cnn_model):
    """(tag, parameters whose gradient is asked for) of the four train-mode runs, in the order they are traced."""
    conv1, _, layers, _ = RN.parts(cnn_model)
    blocks = [b for layer in layers for b in layer]
    return [("train_all", [p for _, p in RN.trunk_params(cnn_model)]),
            ("train_layer3_2_up", [p for b in blocks[LAYER3_2:] for p in b.parameters()]),
            ("train_conv1", [conv1.weight]),
            ("train_none", [])]


def scenarios(M, RN, tracer, jb, precision):
    """Yields (tag, names, sha256, tape) of the seven traces of one model configuration; tape: what the backward left of its
    tape (a walk consumes it: {}), None for a forward alone. The eval pair shares one model (the second forward finds the caches
    filled), and so do the four taped train runs."""
    def done(tag, tape=None):
        return tag, tracer.names(), tracer.sha256(), tape

    d_feats = torch.empty(N, 2048)
    cnn = new_model(M, jb, precision, False).eval()
    tracer.begin()
    with torch.no_grad():
        RN.trunk_forward(cnn.cnn_model, stem_input(RN), precision, False, cnn._rn_cache)
    yield done("eval_forward")

    tracer.begin()
    tape = taped_eval_forward(RN, cnn, precision)
    RN.trunk_input_backward(cnn.cnn_model, tape, d_feats)
    yield done("eval_input_backward", tape)

    cnn = new_model(M, jb, precision, False).train()
    tracer.begin()
    RN.trunk_forward(cnn.cnn_model, stem_input(RN), precision, True, cnn._rn_cache)
    yield done("train_forward")

    cnn = new_model(M, jb, precision, True).train()
    for tag, params in grad_sets(RN, cnn.cnn_model):
        tracer.begin()
        tape = {}
        with torch.no_grad():
            RN.trunk_forward(cnn.cnn_model, stem_input(RN), precision, True, cnn._rn_cache, tape=tape)
        grads = {id(p): torch.empty(p.shape) for p in params}
        RN.trunk_backward(cnn.cnn_model, tape, d_feats, grads)
        yield done(tag, tape)


def key(jb, precision, tag):
    return "%s/%s/%s" % ("bottlenecks" if jb else "fc", precision, tag)
