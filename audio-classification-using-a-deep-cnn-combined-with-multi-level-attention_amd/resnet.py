"""ResNet-50 v1.5 (torchvision ``resnet50``, as the reference builds it in ``model.py:128-149``) with torchvision's
attribute names, child order and parameter shapes, so that the reference's ``state_dict`` keys -- both the
``nn.Sequential(*children()[:-1], CnnFlatten)`` numbering of ``just_bottlenecks=True`` and the named keys of
``just_bottlenecks=False`` -- load unchanged.

The modules are parameter holders; ``trunk_forward`` runs the whole trunk as HIP kernels (``csrc/resnet.hip``) on NHWC
activations in the compute dtype: eval mode with the BatchNorm folded into the conv epilogues as an f32 scale/shift from
the running statistics, train mode (the frozen trunk stays in train mode, ``set_requires_grad`` does not call ``eval``)
with batch statistics and the running-statistics update. Gradients into the trunk (``trunk_backward``, csrc/resnet_bwd.hip)
are opt-in per model (``CNN.set_trunk_backward``) and raise while off; the ``fc`` of ``just_bottlenecks=False`` (trainable in
the reference) is differentiable (``fc_forward``).
"""

import collections
import math

import torch
from torch import nn

from . import ops
from .params import S_RESNET_SHAPE
from .torchvggish.vggish import _Cache

_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


class Conv2d(nn.Module):
    """Parameter holder with nn.Conv2d's names and default initialisation (bias=False, as every conv of ResNet-50)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=False):
        super().__init__()
        assert not bias
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = (kernel_size, kernel_size), (stride, stride), (padding, padding)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))

    def forward(self, x):
        raise RuntimeError("Conv2d is executed by the HIP ResNet trunk of its parent module")


class BatchNorm2d(nn.Module):
    """Parameter / buffer holder with torch.nn.BatchNorm2d's names, eps 1e-5, momentum 0.1."""

    def __init__(self, num_features):
        super().__init__()
        self.num_features, self.eps, self.momentum = num_features, 1e-5, 0.1
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))

    def forward(self, x):
        raise RuntimeError("BatchNorm2d is executed by the HIP ResNet trunk of its parent module")


class _Fused(nn.Module):
    """Parameterless torchvision child (ReLU, MaxPool2d, AdaptiveAvgPool2d): it only holds its place in the child order."""

    def forward(self, x):
        raise RuntimeError("%s is fused into the HIP ResNet trunk" % type(self).__name__)


class ReLU(_Fused):
    pass


class MaxPool2d(_Fused):
    pass


class AdaptiveAvgPool2d(_Fused):
    pass


class Linear(nn.Module):
    """nn.Linear parameter holder (ResNet.fc)."""

    def __init__(self, in_features, out_features):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.empty(out_features))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(in_features)
        nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x):
        raise RuntimeError("Linear is executed by its container")


class Bottleneck(nn.Module):
    """torchvision v1.5 Bottleneck: the stride sits on the 3x3 conv2."""

    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, 1)
        self.bn1 = BatchNorm2d(planes)
        self.conv2 = Conv2d(planes, planes, 3, stride=stride, padding=1)
        self.bn2 = BatchNorm2d(planes)
        self.conv3 = Conv2d(planes, planes * 4, 1)
        self.bn3 = BatchNorm2d(planes * 4)
        self.relu = ReLU()
        self.downsample = downsample
        self.stride = stride


class ResNet(nn.Module):
    """torchvision ResNet-50: children conv1, bn1, relu, maxpool, layer1..layer4, avgpool, fc (in that order)."""

    def __init__(self, layers=(3, 4, 6, 3), num_classes=1000):
        super().__init__()
        self.conv1 = Conv2d(3, 64, 7, stride=2, padding=3)
        self.bn1 = BatchNorm2d(64)
        self.relu = ReLU()
        self.maxpool = MaxPool2d()
        inplanes = 64
        for i, (planes, n, stride) in enumerate(zip((64, 128, 256, 512), layers, (1, 2, 2, 2))):
            ds = nn.Sequential(Conv2d(inplanes, planes * 4, 1, stride=stride), BatchNorm2d(planes * 4))
            blocks = [Bottleneck(inplanes, planes, stride, ds)] + [Bottleneck(planes * 4, planes) for _ in range(n - 1)]
            inplanes = planes * 4
            setattr(self, "layer%d" % (i + 1), nn.Sequential(*blocks))
        self.avgpool = AdaptiveAvgPool2d()
        self.fc = Linear(2048, num_classes)


def resnet50(pretrained=False, **kwargs):
    """torchvision.models.resnet50 stand-in: weights arrive through load_state_dict (no download here)."""
    if pretrained:
        raise Exception("pretrained ResNet-50 weights are not downloaded here: use pretrained=False and load_state_dict instead")
    return ResNet(**kwargs)


class StemInput:
    """What ``Input.forward`` hands to the ResNet trunk: the raw (N, 224, 224) f32 planes and the channel configuration
    (``single``: x in channel 0 only). The normalisation happens inside the stem kernel (model.py:84-94)."""

    def __init__(self, planes, single):
        self.planes, self.single = planes, single


def parts(cnn_model):
    """(conv1, bn1, [layer1..layer4], fc or None) of a ResNet or of the just_bottlenecks Sequential of its children."""
    if isinstance(cnn_model, ResNet):
        m = cnn_model
        return m.conv1, m.bn1, [m.layer1, m.layer2, m.layer3, m.layer4], m.fc
    kids = list(cnn_model.children())
    return kids[0], kids[1], kids[4:8], None


def trunk_params(cnn_model):
    """(name, parameter) of the trunk: everything but the fc of just_bottlenecks=False."""
    return [(n, p) for n, p in cnn_model.named_parameters() if not n.startswith("fc.")]


def trunk_requires_grad(cnn_model):
    return any(p.requires_grad for _, p in trunk_params(cnn_model))


def _check_frozen(cnn_model):
    if not torch.is_grad_enabled():
        return
    for name, p in trunk_params(cnn_model):
        if p.requires_grad:               # fc (just_bottlenecks=False) is trained: fc_forward
            raise NotImplementedError("gradients into the ResNet trunk are off (parameter cnn.cnn_model.%s requires grad); train with "
                                      "cnn_trainable=False / first_cnn_layer_trainable=False, or turn the HIP trunk backward on with "
                                      "CNN.set_trunk_backward(True) / Ensemble(..., trunk_backward=True)" % name)


# What a taped forward keeps per BatchNorm2d (tape["bn"][id(bn)]). y: the unit's output where a ReLU follows (its mask), else
# None. Train mode: x the raw conv output, mean / var its batch statistics, scale None. Eval mode, the BatchNorm folded into the
# conv: scale the folded per-channel scale, x / mean / var None.
BnRecord = collections.namedtuple("BnRecord", "x mean var y scale")


def trunk_forward(cnn_model, x, precision, training, cache, dist=None, tape=None):
    """StemInput -> f32 (N, 2048) bottleneck features (avgpool + flatten) of the HIP trunk. dist: the ``ops.Dist`` of a
    data-parallel training step; in train mode its SyncBN setting decides whether the 53 BatchNorm2d statistics are those of
    the global batch (one all-reduce per layer) or of this rank's shard. tape: a dict that receives what the backward of this
    forward needs (``trunk_backward`` in train mode, ``trunk_input_backward`` in eval mode, which also sets tape["eval"]): every
    block's input in tape["block_in"] and one ``BnRecord`` per BatchNorm2d in tape["bn"], both keyed by the module's id, the
    stem's bn1 included. The kernels launched and the features are those of the untaped call; in train mode the BatchNorm
    outputs then go to new tensors instead of overwriting their inputs."""
    if not isinstance(x, StemInput):
        raise TypeError("the ResNet trunk takes the output of model.Input (raw 224 x 224 planes)")
    if precision not in _DTYPES:
        raise NotImplementedError("the ResNet trunk is built for precision 'f32' and 'bf16', not %r" % precision)
    conv1, bn1, layers, _ = parts(cnn_model)
    if conv1.weight.shape != (64, 3, 7, 7):
        raise NotImplementedError("the ResNet stem kernel takes the 3-channel conv1 (in_channels=3)")
    planes = x.planes
    assert planes.dim() == 3 and tuple(planes.shape[1:]) == S_RESNET_SHAPE
    _check_frozen(cnn_model)
    dtype = _DTYPES[precision]
    blocks = [b for layer in layers for b in layer]
    convs = [c for b in blocks for c in ([b.conv1, b.conv2, b.conv3] + ([b.downsample[0]] if b.downsample is not None else []))]
    packed = cache["w"].get([c.weight for c in convs], dtype,
                            lambda: {id(c): ops.rn_repack(c.weight.detach().contiguous(), dtype) for c in convs})
    w1 = conv1.weight.detach().contiguous()
    if tape is not None:
        tape.update(dtype=dtype, planes=planes, single=x.single, bn={}, block_in={})

    def conv_of(h, conv, scale=None, shift=None, residual=None, relu=False):
        if conv is conv1:                         # the stem: it reads the raw planes, and nothing is added to it
            return ops.rn_stem(planes, x.single, w1, dtype, scale, shift, relu)
        return ops.rn_conv(h, packed[id(conv)], conv.stride[0], scale, shift, residual, relu)

    if training:
        cache["bn"].key = None                    # the running statistics change below, behind torch's version counters
        dist = dist or ops._local()

        def unit(h, conv, bn, residual=None, relu=False):
            t = conv_of(h, conv)
            if tape is None:
                return ops.rn_bn_apply(t, *ops.rn_bn_stats_sync(t, bn, dist), residual=residual, relu=relu)
            scale, shift, mean, var = ops.rn_bn_stats_sync(t, bn, dist, want_stats=True)
            y = ops.rn_bn_apply(t, scale, shift, residual=residual, relu=relu, out=torch.empty_like(t))
            tape["bn"][id(bn)] = BnRecord(t, mean, var, y if relu else None, None)
            return y
    else:
        bns = [bn1] + [n for b in blocks for n in ([b.bn1, b.bn2, b.bn3] + ([b.downsample[1]] if b.downsample is not None else []))]
        tensors = [t for n in bns for t in (n.weight, n.bias, n.running_mean, n.running_var)]
        coef = cache["bn"].get(tensors, None, lambda: {id(n): ops.rn_bn_eval_coeffs(n) for n in bns})
        if tape is not None:
            tape["eval"] = True

        def unit(h, conv, bn, residual=None, relu=False):
            scale, shift = coef[id(bn)]
            y = conv_of(h, conv, scale, shift, residual, relu)
            if tape is not None:                  # the fused outputs are new tensors anyway, the tape only keeps them
                tape["bn"][id(bn)] = BnRecord(None, None, None, y if relu else None, scale)
            return y

    h = ops.rn_maxpool(unit(None, conv1, bn1, relu=True))
    for b in blocks:
        if tape is not None:
            tape["block_in"][id(b)] = h
        o = unit(h, b.conv1, b.bn1, relu=True)
        o = unit(o, b.conv2, b.bn2, relu=True)
        idn = unit(h, b.downsample[0], b.downsample[1]) if b.downsample is not None else h
        h = unit(o, b.conv3, b.bn3, residual=idn, relu=True)
        del o, idn                                # nothing of a block but its output is held into the next one
    if tape is not None:
        tape["last_shape"] = tuple(h.shape)
    return ops.rn_avgpool(h)


def _blocks_backward(blocks, tape, d_feats, lowest, bn_bwd, wgrad):
    """What ``trunk_backward`` and ``trunk_input_backward`` share: the avg-pool backward of d_feats, then the blocks in reverse
    from the last one down to ``blocks[max(lowest, 1) - 1]`` (unit 0 is the stem, unit k is blocks[k - 1]) -> the gradient of
    the max-pool output, or None when lowest > 0 (nothing under the lowest block is wanted, so its input gradients are not
    computed). bn_bwd(bn, dy, want_dres) -> (d_pre, d_res) is the backward of one BatchNorm [+ residual] [+ ReLU]; it pops
    bn's record from tape["bn"]. wgrad(x, dy, conv) takes the conv's weight gradient, or does nothing. At a block input the
    main-path and skip-path gradients are summed by the conv1 data gradient's residual input. The ``del`` statements bound
    the peak memory of both callers: every gradient and kept output is released as soon as the walk has passed it."""
    dtype, records = tape["dtype"], tape["bn"]

    def dgrad(dy, conv, in_hw, residual=None):
        return ops.rn_conv_dgrad(dy, ops.rn_repack_dgrad(conv.weight.detach().contiguous(), dtype), conv.stride[0], in_hw, residual)

    d = ops.rn_avgpool_bwd(d_feats, tape["last_shape"], dtype)
    for k in range(len(blocks), max(lowest, 1) - 1, -1):
        b = blocks[k - 1]
        h_in = tape["block_in"].pop(id(b))
        a2 = records[id(b.bn2)].y
        do3, g3 = bn_bwd(b.bn3, d, True)
        wgrad(a2, do3, b.conv3)
        da2 = dgrad(do3, b.conv3, a2.shape[1:3])
        del do3
        a1 = records[id(b.bn1)].y
        do2, _ = bn_bwd(b.bn2, da2, False)
        del da2, a2
        wgrad(a1, do2, b.conv2)
        da1 = dgrad(do2, b.conv2, a1.shape[1:3])
        del do2
        do1, _ = bn_bwd(b.bn1, da1, False)
        del da1, a1
        wgrad(h_in, do1, b.conv1)
        below = lowest < k                                        # a unit under this block wants a gradient
        if b.downsample is not None:
            dds, _ = bn_bwd(b.downsample[1], g3, False)
            wgrad(h_in, dds, b.downsample[0])
            skip = dgrad(dds, b.downsample[0], h_in.shape[1:3]) if below else None
            del dds
        else:
            skip = g3
        del g3
        d = dgrad(do1, b.conv1, h_in.shape[1:3], residual=skip) if below else None
        del do1, skip, h_in
    return d


def trunk_input_backward(cnn_model, tape, d_feats):
    """Backward of the EVAL-mode trunk forward recorded in `tape` down to the input: d_feats (N, 2048) f32, the gradient of the
    features -> (N, 224, 224) f32, the gradient of the raw planes ``model.Input`` received. Every BatchNorm is a per-channel
    scale and shift folded into its conv's epilogue there, so its backward is ``ops.rn_act_bwd`` (the ReLU mask from the
    record's kept output, times its scale): the whole of ``_blocks_backward`` with that and without weight gradients, then the
    max-pool backward and ``ops.rn_stem_dgrad`` behind the stem's own epilogue (bn1's record). No weight gradient and no
    batch-statistics backward is launched. Runs under no_grad whatever the parameters' requires_grad flags say; no parameter's
    .grad and no buffer is touched. The tape is consumed (its tensors are released as the walk passes them)."""
    assert tape.get("eval"), "trunk_input_backward differentiates the eval-mode forward (trunk_forward(training=False, tape=...))"
    conv1, bn1, layers, _ = parts(cnn_model)
    records = tape["bn"]

    def bn_bwd(bn, dy, want_dres):
        r = records.pop(id(bn))
        return ops.rn_act_bwd(dy, r.scale, y=r.y, want_dres=want_dres)

    with torch.no_grad():
        d = _blocks_backward([b for layer in layers for b in layer], tape, d_feats, 0, bn_bwd, lambda x, dy, conv: None)
        stem = records.pop(id(bn1))
        da0 = ops.rn_maxpool_bwd(stem.y, d)                       # d: gradient of the maxpool output
        del d
        dx = ops.rn_stem_dgrad(da0, conv1.weight.detach().contiguous(), tape["single"], y=stem.y, scale=stem.scale)
    tape.clear()
    return dx


def trunk_backward(cnn_model, tape, d_feats, grads, dist=None):
    """Backward of the train-mode trunk forward recorded in `tape`: d_feats (N, 2048) f32, the gradient of the features ->
    the f32 gradients of the trunk parameters in `grads` ({id(parameter): tensor to write}); only those are computed.
    ``_blocks_backward`` walks down to the lowest unit holding a requested parameter with the train-mode BatchNorm backward
    (batch statistics and kept output from the record); weight gradients nobody asked for are skipped. Then, where the stem is
    wanted, the max-pool backward, bn1's backward and the stem's weight gradient. The tape is
    consumed (its tensors are released as the walk passes them). dist: the ``ops.Dist`` the forward ran under; with SyncBN
    active every BatchNorm2d backward all-reduces its two batch sums (one message per layer the walk passes), so dx is that of
    the global batch. Convs, weight gradients, stem and pools are per-sample linear: they stay local, and `grads` holds this
    rank's part of every parameter gradient (the caller's gradient all-reduce sums the parts)."""
    assert not tape.get("eval"), "trunk_backward differentiates the train-mode forward (trunk_forward(training=True, tape=...))"
    conv1, bn1, layers, _ = parts(cnn_model)
    blocks = [b for layer in layers for b in layer]
    units = [[conv1, bn1]] + [[b] for b in blocks]                 # unit 0: stem; unit k: blocks[k - 1]
    wanted = [any(id(p) in grads for m in u for p in m.parameters()) for u in units]
    if not any(wanted):
        tape.clear()
        return
    lowest = wanted.index(True)
    records = tape["bn"]
    dist = dist or ops._local()
    g = grads.get

    def wgrad(x, dy, conv):
        if id(conv.weight) in grads:
            ops.rn_conv_wgrad(x, dy, conv.stride[0], grads[id(conv.weight)])

    def bn_bwd(bn, dy, want_dres):
        r = records.pop(id(bn))
        return ops.rn_bn_bwd_sync(r.x, dy, r.mean, r.var, bn, dist, y=r.y, want_dres=want_dres, dgamma=g(id(bn.weight)),
                                  dbeta=g(id(bn.bias)))

    d = _blocks_backward(blocks, tape, d_feats, lowest, bn_bwd, wgrad)
    if lowest == 0:                                               # d: gradient of the maxpool output
        da0 = ops.rn_maxpool_bwd(records[id(bn1)].y, d)
        dh0, _ = bn_bwd(bn1, da0, False)
        del da0
        if id(conv1.weight) in grads:
            ops.rn_stem_wgrad(tape["planes"], tape["single"], dh0, grads[id(conv1.weight)])
    tape.clear()


def fc_forward(fc, feats):
    """ResNet.fc (model.py:148-149: Linear(2048, num_classes), assigned after the freeze, so it trains) on the f32 (N, 2048)
    features; through autograd when its parameters require grad."""
    from . import differentiable
    if torch.is_grad_enabled() and (fc.weight.requires_grad or fc.bias.requires_grad):
        return differentiable.FcFn.apply(feats, fc.weight, fc.bias)
    return ops.linear_small(feats, fc.weight.detach().contiguous(), fc.bias.detach().contiguous())


def new_cache():
    return {"w": _Cache(), "bn": _Cache()}
