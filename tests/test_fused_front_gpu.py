"""Fused front (PCM -> conv1's pooled output in one kernel, ops.logmel_conv1): bit-identity with the two-kernel path
conv1(waveforms_to_examples(pcm, bf16)), band edges against a torch-CPU f32 reference, the Ensemble switch, graph replay,
no state between launches; and, without a GPU, the C symbol and its argument types."""

import ctypes
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import PKG

gpu = pytest.mark.gpu

FIRST, EX = 15600, 15360          # samples for one example, and for each further one
CNN_CONF = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=False,
                cnn_trainable=False, first_cnn_layer_trainable=False, in_channels=1)


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def fe():
    return importlib.import_module(PKG + ".frontend")


@pytest.fixture(scope="module")
def conv1_wb(W):
    """conv1 weights / bias of the seeded state dict, on the device."""
    sd = W.make_state_dict(6, W.ensemble_shapes((2, 1), False))
    key = [k for k in sd if k.endswith("features.0.weight")][0]
    w = torch.as_tensor(np.asarray(sd[key])).float().cuda().contiguous()
    b = torch.as_tensor(np.asarray(sd[key[:-len("weight")] + "bias"])).float().cuda().contiguous()
    return w, b


def noise(W, seed, n_wave, n_samples, silent_last=True):
    """Seeded noise waveforms; the last one silent (all-equal rows: zero halo and ReLU edges)."""
    pcm = torch.from_numpy(W.waveform(seed, n_samples, n_wave)).clone()
    if silent_last and n_wave > 1:
        pcm[-1] = 0.0
    return pcm


def two_kernels(ops, fe, pcm, w, b):
    return ops.conv1(fe.waveforms_to_examples(pcm, out_dtype=torch.bfloat16), w, b, torch.bfloat16)


@gpu
@pytest.mark.parametrize("n_wave,n_samples", [(1, 160000), (3, 160000), (27, 160000), (2, FIRST), (2, FIRST + 2 * EX)])
def test_fused_equals_two_kernels(ops, fe, W, conv1_wb, n_wave, n_samples):
    """1 waveform x 10 examples; 3; 27 waveforms = 270 clips (more clips than CUs, uneven shares); 1 and 3 examples per waveform."""
    w, b = conv1_wb
    pcm = noise(W, 41, n_wave, n_samples).cuda()
    got = ops.logmel_conv1(pcm, w, b)
    assert tuple(got.shape) == (n_wave * fe.counts(n_samples)[1], 48, 32, 64) and got.dtype == torch.bfloat16
    assert torch.equal(got, two_kernels(ops, fe, pcm, w, b))


@gpu
def test_fused_int16_unaligned_and_strided_pcm(ops, fe, W, conv1_wb):
    w, b = conv1_wb
    f = noise(W, 42, 3, FIRST + EX)
    i16 = (f * 32767).to(torch.int16).cuda()
    assert torch.equal(ops.logmel_conv1(i16, w, b), two_kernels(ops, fe, i16, w, b))
    # odd offset: the pairwise (non-vector) PCM reads
    buf = torch.zeros(3 * (FIRST + EX) + 1).cuda()
    odd = buf[1:].view(3, FIRST + EX)
    odd.copy_(f)
    assert odd.data_ptr() % 8 != 0
    ref = two_kernels(ops, fe, f.cuda(), w, b)
    assert torch.equal(ops.logmel_conv1(odd, w, b), ref)
    # odd row stride (non-vector) and an even one with a gap between the rows (vector)
    for pad in (3, 6):
        wide = torch.full((3, FIRST + EX + pad), 7.0).cuda()
        view = wide[:, :FIRST + EX]
        view.copy_(f)
        assert view.stride(0) == FIRST + EX + pad
        assert torch.equal(ops.logmel_conv1(view, w, b), ref)


@gpu
def test_band_edges_against_torch_cpu(ops, fe, W, conv1_wb):
    """First and last pooled rows of a clip and the pooled rows on both sides of every hand-over between two 8-frame items
    (pooled rows 4 i - 1 | 4 i + 2 | 4 i + 3, which include both sides of every 16-row seam of the stand-alone kernel), against
    torch-CPU f32 conv + pool of the bf16-rounded examples and weights, at the bf16 conv1 tolerance of test_model_gpu (1e-2)."""
    w, b = conv1_wb
    pcm = noise(W, 43, 2, FIRST + EX).cuda()
    got = ops.logmel_conv1(pcm, w, b).float().cpu()
    ex = fe.waveforms_to_examples(pcm, out_dtype=torch.bfloat16).float().cpu()
    wq = w.cpu().to(torch.bfloat16).float()
    ref = F.max_pool2d(F.relu(F.conv2d(ex[:, None], wq, b.cpu(), padding=1)), 2).permute(0, 2, 3, 1)
    rows = sorted({0, 47} | {p for i in range(12) for p in (4 * i - 1, 4 * i, 4 * i + 2, 4 * i + 3) if 0 <= p < 48})
    scale = float(ref.abs().max())
    for p in rows:
        err = float((got[:, p] - ref[:, p]).abs().max()) / scale
        assert err < 1e-2, (p, err)


@gpu
def test_no_state_between_launches(ops, fe, W, conv1_wb):
    w, b = conv1_wb
    a, c = noise(W, 44, 3, 160000).cuda(), noise(W, 45, 3, 160000, silent_last=False).cuda()
    ra, rc = two_kernels(ops, fe, a, w, b), two_kernels(ops, fe, c, w, b)
    ga, gc = ops.logmel_conv1(a, w, b), ops.logmel_conv1(c, w, b)
    assert torch.equal(ga, ra) and torch.equal(gc, rc) and not torch.equal(ga, gc)


@gpu
def test_ensemble_switch_and_graph_replay(ops, W):
    model = importlib.import_module(PKG + ".model")
    ens = model.Ensemble("repeat", dict(CNN_CONF), [2, 1], torch.device("cuda"), precision="bf16")
    sd = W.make_state_dict(6, W.ensemble_shapes((2, 1), False))
    ens.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    ens.cuda().eval()
    pcm = noise(W, 46, 2, 160000, silent_last=False).cuda()
    was = ops.FUSED_FRONT
    try:
        with torch.no_grad():
            ops.FUSED_FRONT = True
            ops.profile = []
            fused = ens.forward_waveforms(pcm)
            names = [n for n, _, _ in ops.profile]
            ops.profile = None
            assert "logmel" in names and "conv1" not in names
            g = ens.capture_waveforms(pcm)
            assert torch.equal(g(pcm), fused)
            ops.FUSED_FRONT = False
            assert torch.equal(ens.forward_waveforms(pcm), fused)
    finally:
        ops.FUSED_FRONT = was
        ops.profile = None


def test_symbol_and_argtypes():
    lib = importlib.import_module(PKG + "._lib")
    fn = lib.lib().mla_logmel_conv1
    vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert list(fn.argtypes) == [vp, ci, i64, i64, i64, vp, vp, vp, vp, vp]
