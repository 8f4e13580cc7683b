"""The mel-dB backward on the GPU (csrc/melspec_bwd.hip): both kernels against the float64 reference on every case of
tests/melspec_bwd_cases.py under the bound the host simulation is held to, the product's own geometry included; one store per
element (NaN prefill, a canary behind n), exact zeros, independence of batch and strides, run-to-run bits; MelDbImagesFn behind
autograd; Ensemble.clip_saliency; one FGSM step on the audio lowers the attacked score."""

import functools
import importlib

import numpy as np
import pytest
import torch

import melspec_bwd_cases as D
from conftest import PKG

pytestmark = pytest.mark.gpu

CONF = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
            first_cnn_layer_trainable=False, in_channels=3)
N_CLIP = 88200


@pytest.fixture(scope="module")
def fe():
    return importlib.import_module(PKG + ".frontend")


@pytest.fixture(scope="module")
def ds():
    return importlib.import_module(PKG + ".dataset")


def run(fe, c, pad=0, d_pad=0):
    """The forward's first kernel and the two backward entries on case c -> (d_db, d_pcm) on the CPU. The rows of pcm lie n + pad
    elements apart (the padding holds 1e30), d_pcm's n + d_pad; both outputs come in NaN-filled: afterwards they hold no NaN and
    the padding behind n is still NaN."""
    clips, n = c.pcm.shape
    buf = torch.full((clips, n + pad), 1e30, dtype=torch.float32, device="cuda")
    buf[:, :n] = c.pcm.cuda()
    x = buf[:, :n]
    db, ws = fe.melspec_db_unclipped(x, D.SR, c.n_mels, c.hop)
    d_db = torch.full_like(db, float("nan"))
    got = fe.melspec_images_backward(c.g.cuda(), db, ws, n, c.hop, D.TOP_DB, c.n_images, c.image_w, c.stride, c.floor_grad, out=d_db)
    assert got.data_ptr() == d_db.data_ptr()
    out_buf = torch.full((clips, n + d_pad), float("nan"), dtype=torch.float32, device="cuda")
    out = out_buf[:, :n]
    got = fe.melspec_db_backward(x, d_db, D.SR, c.n_mels, c.hop, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert not bool(torch.isnan(d_db).any()) and not bool(torch.isnan(out).any()), "every element is stored"
    assert bool(torch.isnan(out_buf[:, n:]).all()), "nothing is stored at or behind n"
    return d_db.cpu(), out.cpu()


@pytest.mark.parametrize("name", D.CASES + D.GPU_ONLY)
def test_kernels_against_the_float64_reference(fe, name):
    c = D.case(name)
    d_db, d_pcm = run(fe, c, pad=D.STRIDE_PAD.get(name, 0), d_pad=3)
    for which, got in ((0, d_db), (1, d_pcm)):
        e, y = D.err(got, D.reference(name)[which]), D.yardstick(name, which)
        print("case %s %s: err %.3e, float32 restatement %.3e, ratio %.2f" % (name, ("d_db", "d_pcm")[which], e, y, e / y if y else 0.0))
        assert e <= D.YARDSTICK_FACTOR * y
        assert bool(torch.isfinite(got).all())


def test_floor_only_silence_and_zero_gradient_are_exact(fe):
    d_db, d_pcm = run(fe, D.case("floor_only"))
    assert int((d_db != 0).sum()) == 1 and bool((d_pcm != 0).any()), "the gradient is the floor term alone: one cell of d_db"
    d_db, d_pcm = run(fe, D.case("floor_only", False))
    assert bool((d_db == 0).all()) and bool((d_pcm == 0).all()), "floor_grad=False: exactly 0"
    d_db, d_pcm = run(fe, D.case("silence"))
    assert bool((d_pcm == 0).all()) and bool((d_db != 0).any()), "silence: S = 0 < amin passes nothing, no NaN"
    c = D.case("step")
    d_db, d_pcm = run(fe, c._replace(g=torch.zeros_like(c.g)))
    assert bool((d_db == 0).all()) and bool((d_pcm == 0).all())


def test_rows_do_not_depend_on_batch_or_strides_and_runs_repeat(fe):
    a, b = D.case("noise"), D.case("step")
    both = a._replace(pcm=torch.cat([a.pcm, b.pcm]), g=torch.cat([a.g, b.g]))
    ref_db, ref_pcm = run(fe, both, pad=37)
    for pad, d_pad in ((37, 0), (0, 0), (5, 11)):
        d_db, d_pcm = run(fe, both, pad=pad, d_pad=d_pad)
        assert torch.equal(d_db, ref_db) and torch.equal(d_pcm, ref_pcm)
    for r in range(3):
        d_db, d_pcm = run(fe, both._replace(pcm=both.pcm[r:r + 1], g=both.g[r:r + 1]))
        assert torch.equal(d_db[0], ref_db[r]) and torch.equal(d_pcm[0], ref_pcm[r]), "a row alone"
    d_db, d_pcm = run(fe, both._replace(pcm=both.pcm.flip(0).contiguous(), g=both.g.flip(0).contiguous()), d_pad=2)
    assert torch.equal(d_db.flip(0), ref_db) and torch.equal(d_pcm.flip(0), ref_pcm), "a row at another position"


def test_melspectrogram_db_backward(fe):
    c = D.case("runs")
    frames = D.frames_of(c.pcm.shape[1], c.hop)
    got = fe.melspectrogram_db_backward(c.pcm.cuda(), c.g.cuda().view(1, c.n_mels, frames), D.SR, c.n_mels, c.hop)
    assert torch.equal(got.cpu(), run(fe, c)[1])
    with pytest.raises(NotImplementedError, match="HTK / center=False path of the VGGish librosa branch is out of scope"):
        fe.melspectrogram_db_backward(c.pcm.cuda(), c.g.cuda().view(1, c.n_mels, frames), D.SR, c.n_mels, c.hop, center=False)


@pytest.mark.parametrize("overlap", (True, False))
def test_mel_db_images_fn_is_the_forward_and_the_backward_kernels(ds, overlap):
    c = D.case("dataset" if overlap else "dataset39")
    x = c.pcm.cuda().requires_grad_(True)
    images = ds.clips_to_images_differentiable(x, overlap)
    assert images.requires_grad and torch.equal(images.detach(), ds.clips_to_images(c.pcm.cuda(), overlap))
    g = c.g.cuda()
    grad, = torch.autograd.grad((2.0 * images * g).sum(), [x])                       # a torch op on top
    assert torch.equal(grad, ds.clips_to_images_backward(c.pcm.cuda(), 2.0 * g, overlap))
    assert not ds.clips_to_images(x, overlap).requires_grad, "the plain entry keeps returning a leaf"
    with pytest.raises(TypeError, match="float32 waveform"):
        ds.clips_to_images_differentiable(c.pcm.cuda().double(), overlap)


@functools.lru_cache(maxsize=None)
def ensemble(conf, jb, precision):
    """A random-weight ResNet Ensemble whose BatchNorm running statistics describe dB images (thirty train-mode passes over two
    other clips, as tests/test_melspec_gpu.py::test_forward_clips does and explains)."""
    import librosa_restated as LR
    M = importlib.import_module(PKG + ".model")
    W = importlib.import_module(PKG + ".weights")
    ds = importlib.import_module(PKG + ".dataset")
    torch.manual_seed(123)                          # just_bottlenecks=False: torch's initialisation of the fc
    ens = M.Ensemble(conf, dict(CONF, just_bottlenecks=jb), [2, 1], torch.device("cuda"), precision=precision)
    sd = W.make_state_dict(21, W.ensemble_shapes((2, 1), jb, cnn_type="resnet"))
    missing = ens.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
    assert not missing.unexpected_keys and all(k.startswith("cnn.cnn_model.fc.") for k in missing.missing_keys)
    ens.cuda()
    wave = lambda name: torch.from_numpy(LR.waveform(name, N_CLIP)[None].astype(np.float32)).cuda()      # noqa: E731
    calib = ds.clips_to_images(torch.cat([wave("noise"), wave("tones")]))
    ens.train()
    with torch.no_grad():
        for _ in range(30):
            ens(calib)
    return ens.eval(), torch.cat([wave("chirp"), wave("burst")])


@pytest.mark.parametrize("conf,jb,precision", (("repeat", False, "f32"), ("single", True, "bf16")))
def test_clip_saliency(ds, conf, jb, precision):
    ens, pcm = ensemble(conf, jb, precision)
    before = {k: v.clone() for k, v in ens.state_dict().items()}
    for target in (None, 4, torch.tensor([1, 7])):
        scores, grad = ens.clip_saliency(pcm, target=target)
        ref_scores, _, image_grad = ens.saliency_clips(pcm, target)
        assert grad.dtype == torch.float32 and tuple(grad.shape) == (2, N_CLIP) and tuple(scores.shape) == (2, 10)
        assert torch.equal(scores, ref_scores)
        assert torch.equal(grad, ds.clips_to_images_backward(pcm, image_grad))
        assert bool(torch.isfinite(grad).all()) and bool(grad.abs().max() > 0)
    _, timed = ens.clip_saliency(pcm, target=torch.tensor([1, 7]), times_input=True)
    assert torch.equal(timed, grad * pcm), "times_input multiplies by the waveform"
    _, constant = ens.clip_saliency(pcm, target=4, floor_grad=False)
    assert torch.equal(constant, ds.clips_to_images_backward(pcm, ens.saliency_clips(pcm, 4)[2], floor_grad=False))
    _, contiguous = ens.clip_saliency(pcm, target=4, overlap=False)
    assert torch.equal(contiguous, ds.clips_to_images_backward(pcm, ens.saliency_clips(pcm, 4, overlap=False)[2], overlap=False))
    assert not ens.training and all(p.grad is None for p in ens.parameters())
    after = ens.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[n], v) for n, v in before.items())


def test_clip_saliency_refuses_train_mode_and_the_vggish_branch():
    M = importlib.import_module(PKG + ".model")
    ens, pcm = ensemble("single", True, "bf16")
    ens.train()
    try:
        with pytest.raises(RuntimeError, match="eval mode only"):
            ens.clip_saliency(pcm)
    finally:
        ens.eval()
    vgg = M.Ensemble("repeat", dict(CONF, cnn_type="vggish", in_channels=1, just_bottlenecks=False), [2, 1], "cpu").eval()
    with pytest.raises(NotImplementedError, match=r"clip_saliency differentiates the ResNet branch.*waveform_saliency\(\)"):
        vgg.clip_saliency(torch.zeros(1, N_CLIP))


def test_one_fgsm_step_lowers_the_attacked_score():
    """A direction check, not a tolerance: eps = 1e-3 along -sign(grad) lowers the picked score of both bags."""
    ens, pcm = ensemble("repeat", False, "f32")
    with torch.no_grad():
        before = ens.forward_clips(pcm)
    target = before.argmax(dim=1)
    _, grad = ens.clip_saliency(pcm, target=target)
    with torch.no_grad():
        after = ens.forward_clips(pcm - 1e-3 * grad.sign())
    picked = lambda s: s.gather(1, target.view(-1, 1)).view(-1)                                 # noqa: E731
    print("picked scores before", picked(before).tolist(), "after", picked(after).tolist())
    assert bool((picked(after) < picked(before)).all())
