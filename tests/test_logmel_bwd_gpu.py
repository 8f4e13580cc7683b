"""The log-mel backward on the GPU (csrc/logmel_bwd.hip): the kernel against the float64 reference on every case of
tests/logmel_bwd_cases.py under the bound the host simulation is held to; one store per element (NaN prefill, guard columns),
zero tail, silence, G = 0, independence of batch and strides, run-to-run bits, the grid-cap crossing; LogMelFn behind autograd;
Ensemble.waveform_saliency; one FGSM step lowers the attacked score."""

import importlib

import pytest
import torch

import input_grad_cases as G
import logmel_bwd_cases as D
from conftest import PKG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    return importlib.import_module(PKG + ".frontend")


@pytest.fixture(scope="module")
def M():
    return importlib.import_module(PKG + ".model")


def ensemble(M, mk, precision="f32", **kw):
    ens = M.Ensemble("repeat", dict(mk.CNN_CONF, just_bottlenecks=False), [2, 1], torch.device("cuda"), precision=precision, **kw)
    ens.load_state_dict(G.state_dict(False))
    M.set_requires_grad(ens, False)
    return ens.cuda().eval()


def strided(t, pad, fill):
    """A (W, n) device view whose rows lie n + pad elements apart, inside a buffer filled with `fill`."""
    W, n = t.shape
    buf = torch.full((W, n + pad), fill, dtype=t.dtype, device="cuda")
    buf[:, :n] = t.cuda()
    return buf, buf[:, :n]


def run(fe, pcm, g, pad=0, d_pad=0):
    """The kernel on rows n + pad apart into NaN-filled rows n + d_pad apart -> the (W, n) result on the CPU; the padding of the
    output must still be NaN and the valid part must hold none."""
    _, x = strided(pcm, pad, 7 if pcm.dtype == torch.int16 else 1e30)
    out_buf = torch.full((pcm.shape[0], pcm.shape[1] + d_pad), float("nan"), dtype=torch.float32, device="cuda")
    out = out_buf[:, :pcm.shape[1]]
    got = fe.waveforms_to_examples_backward(x, g.cuda(), out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out_buf[:, pcm.shape[1]:]).all()), "nothing is stored outside the rows"
    assert not bool(torch.isnan(out).any()), "every element is stored"
    return out.cpu()


@pytest.mark.parametrize("name", D.CASES + ("cap",))
def test_kernel_against_the_float64_reference(fe, name):
    pcm, g = D.case(name)
    got = run(fe, pcm, g, pad=D.STRIDE_PAD.get(name, 0))
    e, bound = D.err(got, D.reference(name)), D.bound(name)
    print("case %s: err %.3e, float32 restatement %.3e, bound %.3e" % (name, e, D.yardstick(name), bound))
    assert e <= bound
    assert bool(torch.isfinite(got).all())


def test_zero_tail_silence_and_zero_gradient(fe):
    pcm, g = D.case("b")
    got = run(fe, pcm, g, d_pad=5)
    assert bool((got[:, 15600:] == 0).all()) and bool((got[:, :15600] != 0).float().mean() > 0.99)
    pcm, g = D.case("g")
    got = run(fe, pcm, g, pad=37)
    assert bool((got[2] == 0).all()), "silence: A_k = 0 passes nothing, no NaN"
    assert bool((got[1, 15600 + D.WIN:] == 0).all())
    assert bool((run(fe, pcm, torch.zeros_like(g)) == 0).all())
    short = torch.rand(2, 15599) - 0.5
    assert bool((run(fe, short, torch.zeros(0, 96, 64), pad=3, d_pad=1) == 0).all()), "no example: zeros everywhere"


def test_rows_do_not_depend_on_batch_or_strides_and_runs_repeat(fe):
    pcm, g = D.case("g")
    ref = run(fe, pcm, g, pad=37)
    assert torch.equal(run(fe, pcm, g, pad=37), ref), "two calls give the same bits"
    for pad, d_pad in ((0, 0), (5, 11), (1, 0)):
        assert torch.equal(run(fe, pcm, g, pad=pad, d_pad=d_pad), ref)
    per = g.shape[0] // 3
    for r in range(3):
        assert torch.equal(run(fe, pcm[r:r + 1], g[r * per:(r + 1) * per])[0], ref[r])
    big, gbig = D.case("cap")
    last = run(fe, big, gbig)[-1]
    assert torch.equal(run(fe, big[-1:], gbig[-10:])[0], last), "a row computed on a workgroup's second trip equals the row alone"


def test_logmel_fn_is_the_forward_and_the_backward_kernel(fe):
    pcm, g = D.case("c")
    x = pcm.cuda().requires_grad_(True)
    ex = fe.waveforms_to_examples_differentiable(x)
    assert ex.requires_grad and torch.equal(ex.detach(), fe.waveforms_to_examples(pcm.cuda()))
    (ex * g.cuda()).sum().backward()
    assert torch.equal(x.grad, fe.waveforms_to_examples_backward(pcm.cuda(), g.cuda()))
    plain = fe.waveforms_to_examples(x)
    assert not plain.requires_grad, "the plain entry keeps returning a leaf"
    with pytest.raises(TypeError, match="float32 waveform"):
        fe.waveforms_to_examples_differentiable(D.case("f")[0].cuda())


def test_literal_loop_fills_the_waveform_gradient(fe, M, mk, W):
    ens = ensemble(M, mk)
    ens.set_input_grad(True)
    pcm = torch.as_tensor(W.waveform(23, 160000, 2)).cuda().requires_grad_(True)
    ex = fe.waveforms_to_examples_differentiable(pcm)
    scores = ens(ex.view(2, 10, 1, 96, 64))
    scores[:, 3].sum().backward()
    ens.set_input_grad(False)
    ref_scores, ref = ens.waveform_saliency(pcm.detach(), target=3)
    assert torch.equal(scores.detach(), ref_scores) and torch.equal(pcm.grad, ref) and bool(pcm.grad.abs().max() > 0)
    assert all(p.grad is None for p in ens.parameters())


@pytest.mark.parametrize("precision", ("f32", "bf16"))
def test_waveform_saliency(fe, M, mk, W, precision):
    ens = ensemble(M, mk, precision)
    feats = ens.cnn.cnn_model.features
    was = feats.input_grad
    pcm = torch.as_tensor(W.waveform(21, 160000, 2)).cuda()
    for target in (None, 4, torch.tensor([1, 7])):
        scores, grad = ens.waveform_saliency(pcm, target=target)
        ref_scores, _, ex_grad = ens.saliency_waveforms(pcm, target)
        assert grad.dtype == torch.float32 and tuple(grad.shape) == (2, 160000)
        assert torch.equal(scores, ref_scores)
        assert torch.equal(grad, fe.waveforms_to_examples_backward(pcm, ex_grad.reshape(-1, 96, 64)))
        assert bool(torch.isfinite(grad).all()) and bool(grad.abs().max() > 0)
    _, timed = ens.waveform_saliency(pcm, target=torch.tensor([1, 7]), times_input=True)
    assert torch.equal(timed, grad * pcm)
    assert all(p.grad is None for p in ens.parameters()) and feats.input_grad == was
    i16 = (pcm * 32768).round().clamp(-32768, 32767).to(torch.int16)
    _, raw16 = ens.waveform_saliency(i16, target=4)
    _, timed16 = ens.waveform_saliency(i16, target=4, times_input=True)
    assert torch.equal(timed16, raw16 * (i16.float() / 32768.0)), "int16: times the float waveform pcm / 32768"


def test_waveform_saliency_refuses_train_mode_and_the_resnet_branch(M, mk, W):
    ens = ensemble(M, mk)
    pcm = torch.as_tensor(W.waveform(21, 160000, 1)).cuda()
    ens.train()
    with pytest.raises(RuntimeError, match="eval mode only"):
        ens.waveform_saliency(pcm)
    rn = M.Ensemble("repeat", dict(mk.CNN_CONF, cnn_type="resnet", just_bottlenecks=True, in_channels=3), [2, 1], "cpu").eval()
    with pytest.raises(NotImplementedError, match="the waveform paths feed VGGish log-mel examples"):
        rn.waveform_saliency(torch.zeros(1, 160000))


def test_one_fgsm_step_lowers_the_attacked_score(M, mk, W):
    """A direction check, not a tolerance: eps = 1e-3 along -sign(grad) lowers the picked score of both bags."""
    ens = ensemble(M, mk)
    pcm = torch.as_tensor(W.waveform(29, 160000, 2)).cuda()
    with torch.no_grad():
        before = ens.forward_waveforms(pcm)
    target = before.argmax(dim=1)
    _, grad = ens.waveform_saliency(pcm, target=target)
    with torch.no_grad():
        after = ens.forward_waveforms(pcm - 1e-3 * grad.sign())
    picked = lambda s: s.gather(1, target.view(-1, 1)).view(-1)                                 # noqa: E731
    print("picked scores before", picked(before).tolist(), "after", picked(after).tolist())
    assert bool((picked(after) < picked(before)).all())
