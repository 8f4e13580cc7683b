"""The head's shape as constructor arguments (classes / slots / hidden instead of the params constants K / T / H): what can be
checked without a GPU -- state_dict shapes against weights.mla_shapes, the defaults, the accepted range, the refusal of the
ten-window audio entry points on another slot count, and the class names of the test report."""

import ctypes
import importlib
import inspect

import pytest
import torch

from conftest import PKG

CNN_CONF = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=False,
                cnn_trainable=False, first_cnn_layer_trainable=False, in_channels=1)
WIDE = dict(classes=50, slots=12, hidden=64)


@pytest.fixture(scope="module")
def M():
    return importlib.import_module(PKG + ".model")


def shapes_of(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def test_head_state_dict_follows_the_keywords(M, W):
    mla = M.MultiLevelAttention([2, 1], 128, **WIDE)
    want = W.mla_shapes([2, 1], 128, prefix="", T=12, H=64, K=50)
    got = shapes_of(mla)
    assert list(got) == list(want) and got == {k: tuple(s) for k, s in want.items()}
    assert (mla.classes, mla.slots, mla.hidden) == (50, 12, 64)
    am, em = mla.attention_modules[1], mla.embedded_mappings[0]
    assert (am.classes, am.slots, am.hidden) == (50, 12, 64) and (em.slots, em.hidden) == (12, 64)
    assert mla.norm.num_features == 50 and em.norm0.num_features == 12 and mla.fc.weight.shape == (50, 100)


def test_ensemble_state_dict_follows_the_keywords(M, W):
    ens = M.Ensemble("repeat", dict(CNN_CONF), [2, 1], torch.device("cpu"), **WIDE)
    want = W.mla_shapes([2, 1], 128, prefix="mla.", T=12, H=64, K=50)
    want.update(W.vggish_shapes("cnn.cnn_model."))
    assert shapes_of(ens) == {k: tuple(s) for k, s in want.items()}
    assert (ens.classes, ens.slots, ens.hidden) == (50, 12, 64)
    assert ens.num_classes == 10, "num_classes keeps its reference meaning (the ResNet fc width)"
    # beside the existing keywords
    ens = M.Ensemble("repeat", dict(CNN_CONF), [1], torch.device("cpu"), precision="bf16", trunk_backward=False, classes=527)
    assert ens.mla.norm.num_features == 527 and ens.cnn.precision == "bf16" and ens.slots == 10 and ens.hidden == 600


def test_defaults_give_the_dataset_head(M, W):
    P = importlib.import_module(PKG + ".params")
    assert (P.T, P.H, P.K) == (10, 600, 10)
    assert shapes_of(M.MultiLevelAttention([2, 1], 128)) == {k: tuple(s) for k, s in W.mla_shapes([2, 1], 128, prefix="").items()}
    ens = M.Ensemble("repeat", dict(CNN_CONF), [2, 1], torch.device("cpu"))
    assert shapes_of(ens) == {k: tuple(s) for k, s in W.ensemble_shapes((2, 1), False).items()}
    assert (ens.classes, ens.slots, ens.hidden) == (10, 10, 600)
    assert shapes_of(M.AttentionModule())["fcv.weight"] == (10, 600)
    assert shapes_of(M.EmbeddedMapping(2, True, 128))["fc.0.weight"] == (600, 128)
    # positional use is unchanged, the new arguments are keyword-only
    for cls, names in ((M.MultiLevelAttention, ("classes", "slots", "hidden")), (M.AttentionModule, ("classes", "slots", "hidden")),
                       (M.EmbeddedMapping, ("slots", "hidden"))):
        sig = inspect.signature(cls.__init__).parameters
        assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names), cls
    with pytest.raises(TypeError):
        M.MultiLevelAttention([2, 1], 128, 50)


@pytest.mark.parametrize("kw,name", [(dict(classes=0), "classes"), (dict(classes=1025), "classes"), (dict(slots=65), "slots"),
                                     (dict(slots=0), "slots"), (dict(hidden=6), "hidden"), (dict(hidden=0), "hidden")])
def test_out_of_range_shapes_are_refused_by_every_constructor(M, kw, name):
    with pytest.raises(ValueError, match=name):
        M.MultiLevelAttention([2, 1], 128, **kw)
    with pytest.raises(ValueError, match=name):
        M.Ensemble("repeat", dict(CNN_CONF), [2, 1], torch.device("cpu"), **kw)
    if name != "classes":
        with pytest.raises(ValueError, match=name):
            M.EmbeddedMapping(2, True, 128, **kw)
    with pytest.raises(ValueError, match=name):
        M.AttentionModule(**kw)


def test_limits_themselves_are_accepted(M):
    mla = M.MultiLevelAttention([1], 8, classes=1024, slots=64, hidden=4)
    assert mla.fc.weight.shape == (1024, 1024) and mla.embedded_mappings[0].norm0.num_features == 64
    assert M.MultiLevelAttention([1], 8, classes=1, slots=1, hidden=4).norm.num_features == 1


def test_audio_entry_points_refuse_another_slot_count_before_any_launch(M, monkeypatch):
    """The dataset's bags have ten windows: on a slots=12 model every method that builds them raises ValueError -- before the
    dataset code (and with it the GPU library) is reached, which the poisoned loader proves."""
    L = importlib.import_module(PKG + "._lib")

    def no_library(*a, **k):
        raise AssertionError("the GPU library was touched")
    monkeypatch.setattr(L, "lib", no_library)
    rn = M.Ensemble("repeat", dict(CNN_CONF, cnn_type="resnet", just_bottlenecks=True, in_channels=3), [2, 1], torch.device("cpu"),
                    slots=12)
    pcm = torch.zeros(2, 88200)
    for call in (lambda: rn.forward_clips(pcm), lambda: rn.forward_recordings([pcm[0].numpy()], [22050]),
                 lambda: rn.forward_wavfiles(["a.wav"]), lambda: rn.forward_audiofiles(["a.wav"])):
        with pytest.raises(ValueError, match="slots = 12"):
            call()
    vg = M.Ensemble("repeat", dict(CNN_CONF), [2, 1], torch.device("cpu"), slots=12)
    for call in (lambda: vg.forward_clips_librosa(pcm), lambda: vg.forward_recordings_librosa([pcm[0].numpy()], [16000]),
                 lambda: vg.forward_wavfiles_librosa(["a.wav"]), lambda: vg.forward_audiofiles_librosa(["a.wav"]),
                 lambda: vg.forward_recordings_native([pcm[0].numpy()], [16000]), lambda: vg.forward_wavfiles_native(["a.wav"]),
                 lambda: vg.forward_audiofiles_native(["a.wav"])):
        with pytest.raises(ValueError, match="slots = 12"):
            call()
    # the branch check still comes first, as before
    with pytest.raises(NotImplementedError):
        vg.forward_clips(pcm)


def test_report_names_default_by_class_count():
    TR = importlib.import_module(PKG + ".train")
    P = importlib.import_module(PKG + ".params")
    assert TR.default_target_names(10) == list(P.TARGET_NAMES)
    assert TR.default_target_names(3) == ["class_0", "class_1", "class_2"]
    assert len(TR.default_target_names(527)) == 527 and TR.default_target_names(527)[-1] == "class_526"
    sig = inspect.signature(TR.test_model).parameters
    assert list(sig) == ["model", "dataloader", "criterion", "optimizer", "target_names"] and sig["target_names"].default is None
    # the summary takes the names test_model hands it
    res, cm = TR.classification_summary([0, 2, 2], [0, 2, 1], TR.default_target_names(3))
    assert res["class_2"]["support"] == 2 and cm.shape == (3, 3)


def test_shape_limits_of_the_c_entry_points_are_reported_before_any_launch():
    """Validation happens on the host, so it is checkable without a GPU (every call below fails it; the pointers are never
    dereferenced): 65 slots or 1025 classes in the pooling, 1025 columns in the column-mode statistics and in the _wide backward
    pair; the row mode keeps its 64-period limit."""
    L = importlib.import_module(PKG + "._lib")
    lib = L.lib()
    fake, E_SHAPE = ctypes.c_void_p(0x1000), -2
    bn = (fake,) * 8
    for T, K in ((65, 10), (10, 1025), (0, 10), (10, 0)):
        assert lib.mla_attention_pool(fake, 4, T, K, *bn, 1e-5, fake, 2048, fake, fake, None) == E_SHAPE
        assert lib.mla_attention_pool_bwd(fake, 2048, fake, fake, 4, T, K, fake, fake, None) == E_SHAPE
    assert b"K <= 1024" in lib.mla_last_error()
    for mode, period, cols in ((1, 0, 1025), (0, 65, 8)):
        assert lib.mla_bn_stats_sums(fake, 130, cols, cols, mode, period, fake, fake, None) == E_SHAPE
        assert lib.mla_bn_stats_fused(fake, 130, cols, cols, mode, period, fake, fake, fake, fake, None, None, 0.1, None, None) == E_SHAPE
    assert lib.mla_bn_bwd_sums_wide(fake, 1025, fake, 1025, None, 0, 0, 1.0, 20, 1025, fake, fake, 1e-5, fake, fake, None) == E_SHAPE
    assert lib.mla_bn_bwd_apply_wide(fake, 1025, fake, 1025, None, 0, 0, 1.0, 20, 1025, fake, fake, fake, 1e-5, fake, fake,
                                     ctypes.c_double(20.0), fake, 1025, 0, fake, fake, None) == E_SHAPE
    assert lib.mla_bn_stats_workspace_bytes() >= (32 * 1024 + 1024) * 2 * 8
