"""The input-gradient switch and the saliency entries without a GPU: defaults, where set_input_grad reaches, and every refusal that
comes before the device is touched (train mode, the ResNet branch, bad targets, bad shapes)."""

import importlib
import inspect

import pytest
import torch

from conftest import PKG

CONF = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=False, cnn_trainable=False,
            first_cnn_layer_trainable=False, in_channels=1)


@pytest.fixture(scope="module")
def M():
    return importlib.import_module(PKG + ".model")


def features_of(ens):
    return ens.cnn.cnn_model[0] if ens.just_bottlenecks else ens.cnn.cnn_model.features


@pytest.mark.parametrize("jb", [False, True])
def test_switch_defaults_off_and_reaches_the_conv_stack(M, jb):
    conf = dict(CONF, just_bottlenecks=jb)
    ens = M.Ensemble("repeat", conf, [2, 1], "cpu")
    feats = features_of(ens)
    assert feats.input_grad is False
    assert ens.set_input_grad(True) is ens and feats.input_grad is True
    assert ens.cnn.set_input_grad(False) is ens.cnn and feats.input_grad is False
    assert feats.set_input_grad(1) is feats and feats.input_grad is True
    assert features_of(M.Ensemble("repeat", conf, [2, 1], "cpu", input_grad=True)).input_grad is True
    cnn = M.CNN(**conf, input_grad=True)
    assert (cnn.cnn_model[0] if jb else cnn.cnn_model.features).input_grad is True
    if not jb:
        vgg = ens.cnn.cnn_model
        assert vgg.set_input_grad(False) is vgg and feats.input_grad is False
    # another model's switch is its own
    assert features_of(M.Ensemble("repeat", conf, [2, 1], "cpu")).input_grad is False


def test_features_backward_keeps_its_signature_and_gains_want_dx():
    ct = importlib.import_module(PKG + ".cnn_train")
    p = inspect.signature(ct.features_backward).parameters
    assert list(p) == ["feats", "tape", "d", "grads", "keys", "done", "want_dx"] and p["want_dx"].default is False and p["done"].default is None


def test_resnet_has_no_input_gradient(M):
    conf = dict(CONF, cnn_type="resnet", just_bottlenecks=True, in_channels=3)
    rn = M.Ensemble("repeat", conf, [2, 1], "cpu").eval()
    assert rn.set_input_grad(False) is rn
    for call in (lambda: rn.set_input_grad(True), lambda: rn.cnn.set_input_grad(True), lambda: rn.saliency(torch.zeros(1, 10, 1, 224, 224)),
                 lambda: M.Ensemble("repeat", conf, [2, 1], "cpu", input_grad=True)):
        with pytest.raises(NotImplementedError, match="train-mode BatchNorm only.*stem has no backward-data"):
            call()
    with pytest.raises(NotImplementedError, match="waveform paths feed VGGish"):
        rn.saliency_waveforms(torch.zeros(1, 160000))


def test_saliency_refusals_come_before_the_device_is_touched(M):
    ens = M.Ensemble("repeat", CONF, [2, 1], "cpu")
    x = torch.zeros(2, 10, 1, 96, 64)
    assert ens.training
    with pytest.raises(RuntimeError, match="saliency runs in eval mode only"):
        ens.saliency(x)
    ens.eval()
    for bad in (10, -1, True, 2.0, "3", torch.tensor([0, 10]), torch.tensor([-1, 0]), torch.tensor([0]), torch.tensor([[0, 1]]),
                torch.tensor([0.0, 1.0]), torch.tensor([True, False])):
        with pytest.raises(ValueError, match="target"):
            ens.saliency(x, target=bad)
    for shape in ((2, 10, 96, 64), (2, 4, 1, 96, 64), (20, 1, 96, 64)):
        with pytest.raises(ValueError, match=r"saliency takes \(B, 10, 1, 96, 64\) examples"):
            ens.saliency(torch.zeros(shape))
    assert features_of(ens).input_grad is False and not ens.training
