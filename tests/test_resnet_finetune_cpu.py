"""CPU side of the ResNet-50 trunk backward: every new entry point is declared by the header and bound by _lib.py, and the
opt-in flag (Ensemble / CNN keyword trunk_backward, CNN.set_trunk_backward) is plumbed without touching the default."""

import importlib
import inspect

import numpy as np
import pytest
import torch

from conftest import PKG

NEW = ["mla_rn_repack_dgrad", "mla_rn_conv_dgrad", "mla_rn_conv_wgrad_workspace_floats", "mla_rn_conv_wgrad",
       "mla_rn_stem_wgrad_workspace_floats", "mla_rn_stem_wgrad", "mla_rn_bn_bwd_workspace_bytes", "mla_rn_bn_bwd",
       "mla_rn_maxpool_bwd", "mla_rn_avgpool_bwd"]

CONF = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=True,
            first_cnn_layer_trainable=False, in_channels=3)


@pytest.fixture(scope="module")
def L():
    importlib.import_module(PKG + ".build").build(verbose=False)
    return importlib.import_module(PKG + "._lib")


def test_header_declares_and_lib_binds_every_entry_point(L):
    declared = L.declared_symbols()
    lib = L.lib()
    for name in NEW:
        assert name in declared, name
        assert getattr(lib, name).argtypes is not None, name
    sizes = [n for n in NEW if n.endswith(("_floats", "_bytes"))]
    for name in sizes:
        assert getattr(lib, name).restype is not None, name


def test_workspace_sizes(L):
    lib = L.lib()
    # one split of 64 x 64 x 9 floats per 2048 / 9 workgroups at most; more images never shrink the workspace
    small = lib.mla_rn_conv_wgrad_workspace_floats(3, 28, 28, 128, 128, 3, L.BF16)
    big = lib.mla_rn_conv_wgrad_workspace_floats(80, 28, 28, 128, 128, 3, L.BF16)
    assert 0 < small <= big and big % (128 * 128 * 9) == 0
    assert lib.mla_rn_conv_wgrad_workspace_floats(0, 28, 28, 128, 128, 3, L.BF16) == 0
    assert lib.mla_rn_stem_wgrad_workspace_floats(20) == 747 * 64 * 49 * 2      # 2240 rows, 3 per workgroup
    assert lib.mla_rn_bn_bwd_workspace_bytes(256) == 2 * 512 * 256 * 8 + 4 * 256 * 4


def test_keyword_and_setter_plumbing():
    M = importlib.import_module(PKG + ".model")
    names = list(inspect.signature(M.Ensemble.__init__).parameters)
    assert names[names.index("precision") + 1] == "trunk_backward"
    assert inspect.signature(M.Ensemble.__init__).parameters["trunk_backward"].default is False
    names = list(inspect.signature(M.CNN.__init__).parameters)
    assert names[names.index("precision") + 1] == "trunk_backward"
    cnn = M.CNN(**CONF)
    assert cnn.trunk_backward is False
    assert cnn.set_trunk_backward(True) is cnn and cnn.trunk_backward is True
    assert cnn.set_trunk_backward(False) is cnn and cnn.trunk_backward is False
    assert M.CNN(**CONF, trunk_backward=True).trunk_backward is True
    ens = M.Ensemble("repeat", dict(CONF), [2, 1], torch.device("cpu"), "f32", True)
    assert ens.cnn.trunk_backward is True
    assert ens.set_trunk_backward(False) is ens and ens.cnn.trunk_backward is False


def test_flag_off_keeps_the_refusal_message():
    M = importlib.import_module(PKG + ".model")
    RN = importlib.import_module(PKG + ".resnet")
    cnn = M.CNN(**CONF)
    with pytest.raises(NotImplementedError, match="cnn.cnn_model.0.weight.*set_trunk_backward"):
        RN._check_frozen(cnn.cnn_model)
    assert [n for n, _ in RN.trunk_params(M.CNN(**dict(CONF, just_bottlenecks=False)).cnn_model) if n.startswith("fc.")] == []


def test_fixture_keys_and_shapes(golden):
    g = golden("resnet_finetune")
    for tag, n_trunk_grads in (("a", 159), ("b", 1)):       # a: 53 convs + 53 BatchNorm2d x (weight, bias)
        names = list(g[tag + "/names"])
        P = len(names)
        for key, shape in (("idx", (P, 32)), ("init", (P, 32)), ("grad", (P, 32)), ("final", (P, 32)), ("gnorm", (P,)),
                           ("losses", (3,)), ("scores1", (2, 10)), ("stat_idx", (106, 32)), ("stat", (106, 32))):
            assert g["%s/%s" % (tag, key)].shape == shape, (tag, key)
        assert len(g[tag + "/stat_names"]) == 106 and np.isfinite(g[tag + "/losses"]).all()
        trunk = [n for n, v in zip(names, g[tag + "/gnorm"])
                 if n.startswith("cnn.") and not n.startswith("cnn.cnn_model.fc.") and not np.isnan(v)]
        assert len(trunk) == n_trunk_grads, (tag, len(trunk))
    assert [n for n, v in zip(g["b/names"], g["b/gnorm"]) if n.startswith("cnn.") and not np.isnan(v)] == \
        ["cnn.cnn_model.conv1.weight", "cnn.cnn_model.fc.weight", "cnn.cnn_model.fc.bias"]
