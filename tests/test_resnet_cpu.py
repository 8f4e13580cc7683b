"""cnn_type="resnet" (model.py:128-149) on the host: construction, state_dict keys / shapes against a restated
torchvision ResNet-50, strict checkpoint loading, emb_input_size, requires_grad per flag combination and the
configurations that must raise. No GPU needed."""

import importlib

import pytest
import torch

import resnet50_restated as R
from conftest import PKG

M = importlib.import_module(PKG + ".model")
W = importlib.import_module(PKG + ".weights")


def conf(**kw):
    c = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
             first_cnn_layer_trainable=False, in_channels=3)
    c.update(kw)
    return c


def restated_cnn_keys(jb, num_classes=10):
    sd = R.CNN(jb, num_classes).state_dict()
    return {"cnn." + k: tuple(v.shape) for k, v in sd.items()}


@pytest.mark.parametrize("jb,n", [(True, 318), (False, 320)])
def test_state_dict_keys_match_restated_reference(jb, n):
    ens = M.Ensemble("repeat", conf(just_bottlenecks=jb), [2, 1], "cpu")
    got = {k: tuple(v.shape) for k, v in ens.state_dict().items() if k.startswith("cnn.")}
    ref = restated_cnn_keys(jb)
    assert len(ref) == n
    assert list(got) == list(ref) and got == ref
    shapes = W.ensemble_shapes((2, 1), jb, cnn_type="resnet", num_classes=10)
    assert list(ens.state_dict()) == list(shapes)
    assert all(tuple(ens.state_dict()[k].shape) == tuple(s) for k, s in shapes.items())
    assert W.resnet50_shapes("cnn.cnn_model.", jb, 10) == {k: s for k, s in ref.items()}


def test_key_numbering():
    keys = set(M.Ensemble("repeat", conf(), [2, 1], "cpu").state_dict())
    for k in ("cnn.cnn_model.0.weight", "cnn.cnn_model.1.running_var", "cnn.cnn_model.4.0.conv1.weight",
              "cnn.cnn_model.4.0.downsample.1.running_var", "cnn.cnn_model.7.2.bn3.num_batches_tracked"):
        assert k in keys
    keys = set(M.Ensemble("repeat", conf(just_bottlenecks=False), [2, 1], "cpu").state_dict())
    for k in ("cnn.cnn_model.conv1.weight", "cnn.cnn_model.layer1.0.downsample.1.running_var", "cnn.cnn_model.fc.weight"):
        assert k in keys


@pytest.mark.parametrize("jb", [True, False])
def test_restated_checkpoint_loads_strict(jb):
    torch.manual_seed(0)
    ref = R.CNN(jb, 10)
    for m in ref.modules():                       # non-default buffers so that the copy is visible
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.1, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.num_batches_tracked.fill_(3)
    ens = M.Ensemble("repeat", conf(just_bottlenecks=jb), [2, 1], "cpu")
    sd = dict(ens.state_dict())
    sd.update({"cnn." + k: v for k, v in ref.state_dict().items()})
    ens.load_state_dict(sd, strict=True)
    for k, v in ref.state_dict().items():
        assert torch.equal(ens.state_dict()["cnn." + k], v), k


def test_emb_input_size():
    assert M.Ensemble("repeat", conf(), [2, 1], "cpu").emb_input_size == 2048
    assert M.Ensemble("repeat", conf(just_bottlenecks=False, num_classes=128), [2, 1], "cpu").emb_input_size == 128


def _grad_names(**kw):
    return {n for n, p in M.Ensemble("repeat", conf(**kw), [2, 1], "cpu").named_parameters() if p.requires_grad and n.startswith("cnn.")}


def test_requires_grad_per_flags():
    assert _grad_names() == set()
    assert _grad_names(just_bottlenecks=False) == {"cnn.cnn_model.fc.weight", "cnn.cnn_model.fc.bias"}
    assert _grad_names(first_cnn_layer_trainable=True) == {"cnn.cnn_model.0.weight"}
    assert _grad_names(cnn_trainable=True) == set(restated_cnn_keys(True)) - {
        k for k in restated_cnn_keys(True) if k.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked")}
    ens = M.Ensemble("repeat", conf(first_cnn_layer_trainable=True, in_channels=1), [2, 1], "cpu")
    assert tuple(ens.cnn.cnn_model[0].weight.shape) == (64, 1, 7, 7) and ens.cnn.cnn_model[0].weight.requires_grad


def test_frozen_trunk_stays_in_train_mode():
    ens = M.Ensemble("repeat", conf(), [2, 1], "cpu")
    assert ens.training and all(m.training for m in ens.cnn.modules())


def test_rejected_configurations():
    with pytest.raises(Exception, match="load_state_dict instead"):
        M.Ensemble("repeat", conf(use_pretrained=True), [2, 1], "cpu")
    with pytest.raises(NotImplementedError):
        M.Ensemble("repeat", conf(), [2, 1], "cpu", precision="bf16x3")
    ens = M.Ensemble("repeat", conf(), [2, 1], "cpu")
    with pytest.raises(NotImplementedError):
        ens.set_precision("bf16x3")
    with pytest.raises(NotImplementedError):
        ens.forward_waveforms(torch.zeros(1, 160000))
    with pytest.raises(Exception, match="Invalid input type"):
        M.Ensemble("stereo", conf(), [2, 1], "cpu").input(torch.zeros(1, 10, 1, 224, 224))
    with pytest.raises(ValueError):
        ens.input(torch.zeros(1, 10, 1, 96, 64))


def test_seeded_resnet_bn_values():
    sd = W.make_state_dict(3, W.resnet50_shapes("cnn.cnn_model.", True))
    assert 0.9 <= sd["cnn.cnn_model.1.weight"].min() and sd["cnn.cnn_model.1.weight"].max() <= 1.1
    assert 0.17 <= sd["cnn.cnn_model.4.0.bn3.weight"].min() and sd["cnn.cnn_model.4.0.bn3.weight"].max() <= 0.23
    assert abs(sd["cnn.cnn_model.4.0.downsample.1.bias"]).max() <= 0.1
