"""GPU tests of the bf16 finetune path (csrc/cnn_train_bf16.hip, the bf16 instantiations of csrc/cnn_train.hip's maxpool, of
csrc/train_kernels.hip's Linear-backward helpers and of csrc/conv.hip's generic conv entry and dgrad repack; shared rules in csrc/cnn_train_core.h):
every kernel against a float64 torch-CPU computation on the SAME bf16-rounded operands (so the only differences are the
f32 accumulation order and the final rounding), then the whole step against the loss curve the reference produced
(tests/golden/train.npz 'finetune'), with the measured bf16 deviation stated next to the bound."""

import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import PKG

pytestmark = pytest.mark.gpu

SHAPES = [(64, 128, 48, 32), (128, 256, 24, 16), (256, 256, 24, 16), (256, 512, 12, 8), (512, 512, 12, 8)]   # conv2..conv6


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


def bf(t):
    return t.to(torch.bfloat16)


def rnd(W, seed, stream, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(W.uniform(seed, stream, int(np.prod(shape)), lo=lo, hi=hi)).reshape(shape)


@pytest.mark.parametrize("cin,cout,H,Wd", SHAPES)
def test_wgrad_bf16_matches_float64(ops, W, cin, cout, H, Wd):
    """dW = sum_pixels dZ (x) shifted A on v_mfma_f32_16x16x32_bf16 through ds_read_b64_tr_b16, against autograd of
    F.conv2d in float64 on the same bf16 values. n = 3 images exercises the split over images (3 splits) and its reduction."""
    n = 3
    a = bf(rnd(W, 61, cin, (n, H, Wd, cin), -0.5, 1.5))                # NHWC, bf16-representable
    dz = bf(rnd(W, 62, cout, (n, H, Wd, cout)))
    dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device="cuda")
    ops.conv_wgrad(dz.cuda(), a.cuda(), dw)
    x64 = a.double().permute(0, 3, 1, 2).contiguous()
    w64 = torch.zeros((cout, cin, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, w64, padding=1).backward(dz.double().permute(0, 3, 1, 2).contiguous())
    ref = w64.grad
    err = float((dw.cpu().double() - ref).abs().max() / ref.abs().max())
    assert err < 2e-5, err                                              # f32 accumulation over n*H*W <= 4608 exact products


def test_wgrad_bf16_equals_the_f32_kernel_on_the_same_values(ops, W):
    """Same operands through the exact-f32 wgrad kernel: both see identical products; only the summation tree differs."""
    cin, cout, H, Wd, n = 256, 256, 24, 16, 5
    a = bf(rnd(W, 63, 1, (n, H, Wd, cin), -0.5, 1.5)).cuda()
    dz = bf(rnd(W, 64, 2, (n, H, Wd, cout))).cuda()
    d16 = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device="cuda")
    d32 = torch.empty_like(d16)
    ops.conv_wgrad(dz, a, d16)
    ops.conv_wgrad(dz.float(), a.float(), d32)
    assert float((d16 - d32).abs().max() / d32.abs().max()) < 1e-5


def test_maxpool_and_relu_pool_bwd_bf16(ops, W):
    """First-maximum routing and ReLU mask are decided on the bf16 values themselves: identical to torch on the same
    values (ties included: bf16 activations tie often); the bias gradient is the column sum of dZ."""
    n, H, Wd, C = 3, 12, 8, 512
    a = bf(rnd(W, 65, 1, (n, H, Wd, C), -1.0, 1.0)).clamp_min(0)       # post-ReLU: many exact zeros and ties
    a[0, :2, :2, :7] = 0.5                                              # a window of equal positive values -> first position wins
    pooled = ops.maxpool2x2(a.cuda()).cpu()
    ref_pool, idx = F.max_pool2d(a.float().permute(0, 3, 1, 2), 2, return_indices=True)
    assert torch.equal(pooled.float(), ref_pool.permute(0, 2, 3, 1))
    d = bf(rnd(W, 66, 2, (n, H // 2, Wd // 2, C)))
    db = torch.empty(C, dtype=torch.float32, device="cuda")
    dz = ops.relu_pool_bwd(a.cuda(), d.cuda(), pool=True, db=db).cpu()
    assert dz.dtype == torch.bfloat16
    x = a.float().permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(F.relu(x), 2).backward(d.float().permute(0, 3, 1, 2))
    # torch routes to the first maximum in scan order, and relu'(0) = 0: windows of zeros get nothing
    assert torch.equal(dz.float(), x.grad.permute(0, 2, 3, 1))
    np.testing.assert_allclose(db.cpu().numpy(), x.grad.double().sum(dim=(0, 2, 3)).numpy(), rtol=1e-6, atol=1e-6)
    # un-pooled layer
    d2 = bf(rnd(W, 67, 3, (n, H, Wd, C)))
    dz2 = ops.relu_pool_bwd(a.cuda(), d2.cuda(), pool=False, db=db).cpu()
    assert torch.equal(dz2, torch.where(a > 0, d2, torch.zeros_like(d2)))
    np.testing.assert_allclose(db.cpu().numpy(), dz2.double().sum(dim=(0, 1, 2)).numpy(), rtol=1e-6, atol=1e-6)
    # the last Linear: float32 output and incoming gradient, bf16 dZ
    h = rnd(W, 68, 4, (40, 128)).clamp_min(0)
    g = rnd(W, 69, 5, (40, 128))
    dz3 = ops.relu_pool_bwd(h.cuda(), g.cuda(), pool=False, bf16=True).cpu()
    assert torch.equal(dz3, bf(torch.where(h > 0, g, torch.zeros_like(g))))


def test_transpose_and_col_sum_bf16(ops, W):
    for R, C in ((40, 128), (77, 200), (5120, 96)):
        x = bf(rnd(W, 70, R, (R, C)))
        t = ops.transpose_padded(x.cuda()).cpu()
        ld = (R + 7) // 8 * 8
        assert tuple(t.shape) == (C, ld) and torch.equal(t[:, :R], x.t()) and bool((t[:, R:] == 0).all())
        out = torch.empty(C, dtype=torch.float32, device="cuda")
        ops.col_sum(x.cuda(), out)
        np.testing.assert_allclose(out.cpu().numpy(), x.double().sum(dim=0).numpy(), rtol=1e-6, atol=1e-6)


def test_relu_bwd_of_an_f32_linear_output_gives_bf16_dz_and_its_column_sums(ops, W):
    """relu_pool_bwd_bf16_kernel<float, float> with the bias slots, un-pooled, at (5, 128): 80 lanes of 8 channels, every other
    slot stays zero. dZ = where(a > 0, d_out, 0) rounded to bf16, bit for bit; db is the column sum of THOSE bf16 values (what the
    layer's weight gradient is formed from): 5 terms of 8 significant bits are exact in double, one rounding to f32. The f32 inputs
    hold bf16-representable values, as the activations and gradients of the bf16 step do: the kernel sums its slots before it rounds
    dZ for the store, so only on such values are "the column sum of dZ" and "the column sum of what was stored" the same number."""
    h, g = bf(rnd(W, 94, 1, (5, 128))).float().clamp_min(0), bf(rnd(W, 95, 2, (5, 128))).float()
    db = torch.full((128,), 9.0, device="cuda")
    dz = ops.relu_pool_bwd(h.cuda(), g.cuda(), pool=False, db=db, bf16=True).cpu()
    ref = bf(torch.where(h > 0, g, torch.zeros_like(g)))
    assert dz.dtype == torch.bfloat16 and torch.equal(dz, ref)
    assert torch.equal(db.cpu(), ref.double().sum(dim=0).float())


def test_col_sum_bf16_of_a_strided_column_slice(ops, W):
    """colsum_partial_kernel<bf16_t> on columns 40 .. 169 of a (1000, 200) matrix (row pitch 200): 1000 // 256 = 3 row chunks of 334
    rows (the last one 332: neither a multiple of the 4 row groups), three 64-column tiles of which the last holds 2 columns.
    1000 bf16 values of |v| < 1 add exactly in double (8 + 10 bits of 53), so the result is the float64 sum rounded once to f32."""
    wide = bf(rnd(W, 96, 1, (1000, 200)))
    x, out = wide[:, 40:170], torch.full((130,), 9.0, device="cuda")
    ops.col_sum(wide.cuda()[:, 40:170], out)
    assert torch.equal(out.cpu(), x.double().sum(dim=0).float())


@pytest.mark.parametrize("cin,cout,H,Wd,act", [(64, 128, 48, 32, True), (256, 256, 24, 16, True), (512, 512, 12, 8, True),
                                               (512, 512, 12, 8, False), (512, 256, 12, 8, False), (256, 256, 24, 16, False),
                                               (256, 128, 24, 16, False), (128, 64, 48, 32, False)])
def test_generic_conv_bf16_training_and_dgrad_shapes(ops, W, cin, cout, H, Wd, act):
    """The bf16 instantiations of mla_conv3x3 the finetune step adds: un-pooled training forward (bias + ReLU kept) and the
    five transposed convolutions (plain store), against float64 on the same bf16 operands; 3 images (one tile has two images
    for W = 8, so the last tile is half empty)."""
    n = 3
    x = bf(rnd(W, 71, cin, (n, H, Wd, cin), -0.5, 1.0))
    w = rnd(W, 72, cout, (cout, cin, 3, 3)) * (6.0 / (9 * cin)) ** 0.5
    b = rnd(W, 73, cout, (cout,)) * 0.1 if act else None
    if act:
        wp = ops.repack_conv_weight(w.cuda(), torch.bfloat16)
        ref_w = bf(w).double()
    else:                       # dgrad: `w` is the forward weight (cin_fwd = cout here): out[ci] = sum dZ[co] * W[co][ci][flipped]
        wf = rnd(W, 72, cout, (cin, cout, 3, 3)) * (6.0 / (9 * cin)) ** 0.5           # forward layer cout_fwd = cin, cin_fwd = cout
        wp = ops.repack_dgrad(wf.cuda(), torch.bfloat16)
        ref_w = bf(wf).double()
    got = ops.conv3x3(x.cuda(), wp, b.cuda() if act else None, cout, pool=False, act=act).cpu()
    x64 = x.double().permute(0, 3, 1, 2)
    if act:
        ref = F.relu(F.conv2d(x64, ref_w, b.double(), padding=1))
    else:
        ref = F.conv_transpose2d(x64, ref_w, padding=1)
    ref = ref.permute(0, 2, 3, 1)
    err = float((got.double() - ref).abs().max() / ref.abs().max())
    assert err < 6e-3, err                                             # bf16 output rounding (2^-9) on top of exact-product f32 sums


def test_finetune_bf16_curve_against_the_reference_golden(golden, mk, W):
    """train.py:96-97 + :124-138 with the CNN in bf16 (f32 master weights, f32 head): 4 steps on 4 bags against the
    reference's float32 run. Step 1 differs only by the bf16 forward (scores measured ~3e-3 off -> loss ~1e-3); afterwards
    Adam's normalised updates (~+-lr per weight whatever the gradient's precision) keep the curves together: measured
    worst relative loss deviation 4e-3, bound 2e-2. The f32 path keeps its 2e-3 bound (tests/test_train_gpu.py)."""
    g = golden("train")
    TR = importlib.import_module(PKG + ".train")
    M = importlib.import_module(PKG + ".model")
    ens = M.Ensemble("repeat", dict(mk.CNN_CONF), [2, 1], torch.device("cuda"), precision="bf16")
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in W.make_state_dict(7, W.ensemble_shapes((2, 1), False)).items()})
    ens.cuda()
    M.set_requires_grad(ens, True)
    step = TR.TrainStep(ens, lr=1e-3)
    assert step.finetune and step.n_params == 72964234 - 2 * 6010
    losses = []
    for s in range(4):
        x, y = mk.synth_bags(100 + s, 4)
        masks = mk.make_masks(200 + s, [2, 1], 4)
        for lvl, em in enumerate(ens.mla.embedded_mappings):
            for j, d in enumerate(em.dropouts):
                d.mask = masks["mla.embedded_mappings.%d.dropouts.%d" % (lvl, j)]
        loss, hits = step(x.cuda(), y.cuda())
        losses.append(float(loss))
        if s == 0:
            grads0 = {n: gr.double().cpu() for n, gr in step.grads.items()}
    dev = np.abs(np.array(losses) / g["finetune/losses"] - 1).max()
    print("bf16 finetune: losses %s vs reference %s (worst relative deviation %.3g)" % (losses, g["finetune/losses"], dev))
    np.testing.assert_allclose(losses, g["finetune/losses"], rtol=2e-2, atol=0)
    assert all(p.dtype == torch.float32 for p in ens.parameters()), "master weights stay float32"
    # first-step gradients against the exact-f32 path of the same step (which itself matches the reference's autograd to
    # 1e-4, tests/test_train_gpu.py). What bf16 changes is not the arithmetic of a layer (each kernel is checked against
    # float64 above) but (a) the embeddings by ~3e-3, which this model's train-mode BatchNorms over 4 bags amplify, and
    # (b) the max-pool routing wherever two window entries agree to bf16's 8 bits: a fraction f of the gradient mass moving
    # to a neighbouring pixel changes the gradient VECTOR by sqrt(2 f). Measured: cosine 0.969 ... 0.99995, norms within 15 %.
    ens32 = M.Ensemble("repeat", dict(mk.CNN_CONF), [2, 1], torch.device("cuda"), precision="f32")
    ens32.load_state_dict({k: torch.as_tensor(v) for k, v in W.make_state_dict(7, W.ensemble_shapes((2, 1), False)).items()})
    ens32.cuda()
    M.set_requires_grad(ens32, True)
    step32 = TR.TrainStep(ens32, lr=1e-3)
    x, y = mk.synth_bags(100, 4)
    masks = mk.make_masks(200, [2, 1], 4)
    for lvl, em in enumerate(ens32.mla.embedded_mappings):
        for j, d in enumerate(em.dropouts):
            d.mask = masks["mla.embedded_mappings.%d.dropouts.%d" % (lvl, j)]
    step32(x.cuda(), y.cuda())
    worst_cos, worst_norm = 1.0, 0.0
    for name, gr in step32.grads.items():
        a, b = gr.double().cpu(), grads0[name]
        if float(a.norm()) < 1e-4:
            continue
        assert float(a.norm()) == pytest.approx(float(g["finetune/gradnorm0/" + name]), rel=2e-3), name
        cos = float((a * b).sum() / (a.norm() * b.norm()))
        worst_cos, worst_norm = min(worst_cos, cos), max(worst_norm, abs(float(b.norm() / a.norm()) - 1))
        assert cos > 0.95 and abs(float(b.norm() / a.norm()) - 1) < 0.2, (name, cos)
    print("bf16 finetune gradients vs the f32 path: worst cosine %.4f, worst norm deviation %.3g" % (worst_cos, worst_norm))
    # The scores themselves after 3 Adam steps are compared only loosely, and eval-mode scores not at all: every lr 1e-3 Adam
    # step moves each of the 73 M weights by ~+-lr (2-10 % of its size) in the SIGN of its gradient, whatever the gradient's
    # magnitude; with 4 bags most of those gradients are small sums whose sign flips with any change of rounding (cosine 0.97
    # between the bf16 and f32 gradient vectors), so two runs that differ in rounding drift apart step by step -- the
    # cross-entropy of the sigmoid scores (above) is what stays pinned. Control (profiles/r02_finetune_bf16_control.txt): the exact
    # f32 path with its inputs perturbed by 1e-4 relative moves these scores by mean 0.045 / max 0.18 and the loss by 1e-2.
    # Measured here: mean |d score| 0.05, max 0.37.
    dsc = np.abs(step.last_out.cpu().numpy() - g["finetune/out_last"])
    print("bf16 finetune: train-mode scores of step 4 vs the reference: mean |d| %.3g, max %.3g" % (dsc.mean(), dsc.max()))
    assert dsc.mean() < 0.1 and dsc.max() < 0.5
    # and it is deterministic
    ens2 = M.Ensemble("repeat", dict(mk.CNN_CONF), [2, 1], torch.device("cuda"), precision="bf16")
    ens2.load_state_dict({k: torch.as_tensor(v) for k, v in W.make_state_dict(7, W.ensemble_shapes((2, 1), False)).items()})
    ens2.cuda()
    M.set_requires_grad(ens2, True)
    step2 = TR.TrainStep(ens2, lr=1e-3)
    l2 = []
    for s in range(2):
        x, y = mk.synth_bags(100 + s, 4)
        masks = mk.make_masks(200 + s, [2, 1], 4)
        for lvl, em in enumerate(ens2.mla.embedded_mappings):
            for j, d in enumerate(em.dropouts):
                d.mask = masks["mla.embedded_mappings.%d.dropouts.%d" % (lvl, j)]
        l2.append(float(step2(x.cuda(), y.cuda())[0]))
    assert l2 == losses[:2]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cin,cout,H,Wd", [(64, 128, 48, 32), (256, 256, 24, 16), (512, 512, 12, 8)])
def test_conv3x3_train_writes_prepool_and_pooled(ops, W, dtype, cin, cout, H, Wd):
    """mla_conv3x3_train == the un-pooled forward followed by mla_maxpool2x2, bit for bit (same accumulators, the pool is taken on
    the stored values' source registers; bf16: max commutes with the rounding because rounding is monotone)."""
    n = 3
    x = rnd(W, 91, cin, (n, H, Wd, cin), -0.5, 1.0).to(dtype).cuda()
    w = (rnd(W, 92, cout, (cout, cin, 3, 3)) * (6.0 / (9 * cin)) ** 0.5).cuda()
    b = (rnd(W, 93, cout, (cout,)) * 0.1).cuda()
    wp = ops.repack_conv_weight(w, dtype)
    a_ref = ops.conv3x3(x, wp, b, cout, pool=False, act=True)
    p_ref = ops.maxpool2x2(a_ref)
    a, p = ops.conv3x3_train(x, wp, b, cout)
    assert torch.equal(a, a_ref) and torch.equal(p, p_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n,tol", [(3, 4e-2), (130, 3e-3)])
def test_conv1_backward_on_the_matrix_cores_matches_autograd(n, tol):
    """mla_conv1_bwd_bf16 recomputes conv1 + ReLU + max-pool as the forward's patch GEMM (bf16 operands) and forms dW as a second
    GEMM over pixels. Reference: torch autograd on the CPU with x and w rounded to bf16 (what the forward multiplied), the incoming
    gradient in bf16. Measured 4.5e-4 / 1.0e-5 at 512 clips (the f32-recompute kernel this replaces: 4e-2 against the same reference).
    What remains are single routing flips at near-ties of the arg-max / ReLU threshold (the MFMA and torch's conv2d sum the nine
    products in different orders): each moves one |g x| <= 2.3 between taps, visible only against the small sums of a 3-clip batch
    (1.4e-2 there). Also bit-deterministic."""
    ops = importlib.import_module(PKG + ".ops")
    g = torch.Generator().manual_seed(5)
    x = torch.rand((n, 96, 64), generator=g) * 6 - 1.4
    w = (torch.rand((64, 1, 3, 3), generator=g) - 0.5) * 0.6
    b = (torch.rand(64, generator=g) - 0.5) * 0.2
    d = (torch.rand((n, 48, 32, 64), generator=g) - 0.5).to(torch.bfloat16)
    dw = torch.empty((64, 1, 3, 3), device="cuda")
    db = torch.empty(64, device="cuda")
    ops.conv1_bwd(x.cuda(), w.cuda(), b.cuda(), d.cuda(), dw, db)
    wr = w.to(torch.bfloat16).float().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    y = torch.nn.functional.max_pool2d(torch.relu(torch.nn.functional.conv2d(x.to(torch.bfloat16).float()[:, None], wr, br, padding=1)), 2)
    y.backward(d.float().permute(0, 3, 1, 2))
    rel = lambda a, c: float((a - c).abs().max() / c.abs().max())
    assert rel(dw.cpu(), wr.grad) < tol and rel(db.cpu(), br.grad) < tol, (rel(dw.cpu(), wr.grad), rel(db.cpu(), br.grad))
    dw2 = torch.empty_like(dw)
    db2 = torch.empty_like(db)
    ops.conv1_bwd(x.cuda(), w.cuda(), b.cuda(), d.cuda(), dw2, db2)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(64, 128, 48, 32), (256, 256, 24, 16), (512, 512, 12, 8)])
def test_window_codes_route_gradients_like_the_prepool_activation(shape):
    """bf16 training forward of the pooled layers keeps ONE byte per pooled element (mla_conv3x3_train_codes: position of the window's
    first maximum, or "ReLU off") instead of the pre-pool activation (mla_conv3x3_train). Both forms must give the same pooled output
    bit for bit, the same gradient mass per window and the same bias gradient; the routed position may differ only where two f32
    pre-activations of a window round to the same bf16 value (the codes compare the f32 accumulators, the activation path the stored
    bf16 values): a fraction of a percent of the windows."""
    ops = importlib.import_module(PKG + ".ops")
    cin, cout, H, W_ = shape
    n = 6
    g = torch.Generator().manual_seed(11)
    x = (torch.rand((n, H, W_, cin), generator=g) * 2 - 0.6).clamp_min(0).to(torch.bfloat16).cuda()
    w = ((torch.rand((cout, cin, 3, 3), generator=g) - 0.5) * (2.0 / (9 * cin) ** 0.5)).cuda()
    b = ((torch.rand(cout, generator=g) - 0.5) * 0.1).cuda()
    d = (torch.rand((n, H // 2, W_ // 2, cout), generator=g) - 0.5).to(torch.bfloat16).cuda()
    wp = ops.repack_conv_weight(w, torch.bfloat16)
    a, pooled_a = ops.conv3x3_train(x, wp, b, cout)
    codes, pooled_c = ops.conv3x3_train_codes(x, wp, b, cout)
    assert codes.dtype == torch.uint8 and int(codes.max()) <= 4 and torch.equal(pooled_a.view(torch.int16), pooled_c.view(torch.int16))
    assert torch.equal(codes == 4, pooled_c == 0)                                     # ReLU off <=> the pooled output is zero
    db_a = torch.empty(cout, device="cuda")
    db_c = torch.empty(cout, device="cuda")
    dz_a = ops.relu_pool_bwd(a, d, pool=True, db=db_a)
    dz_c = ops.pool_bwd_codes(codes, d, db=db_c)
    win = lambda t: t.float().reshape(n, H // 2, 2, W_ // 2, 2, cout).sum(dim=(2, 4))
    assert torch.equal(win(dz_a), win(dz_c)) and torch.equal(db_a, db_c)              # same gradient mass per window, same bias gradient
    differ = float((dz_a != dz_c).float().mean())
    assert differ < 5e-3, differ


def test_config4_full_size_finetune_bf16_is_deterministic_and_shards(tmp_path, mk, W):
    """BASELINE config 4 at its literal size in the finetune variant (train.py:96-97: every parameter trainable): the step on
    512 bags (5 120 clips of 96 x 64 log-mel), CNN in bf16 with f32 master weights, the configuration bench.py's train_step leg
    times. Size-independent properties (the CPU reference cannot run this in seconds):
    (1) two runs give identical bits -- losses, hit counts, every updated parameter;
    (2) two ranks with 256 bags each (gloo, sharing the test GPU; SyncBN sums + the five gradient buckets on the second
        stream) stay bit-identical replicas and reproduce the one-process run: the first loss to float32 rounding of the
        statistics' summation tree; the second, after one Adam step of +-lr on 73 M weights whose small gradients change sign
        with the summation order of the two half-batch weight gradients, to 2e-3."""
    import os, subprocess, sys
    from conftest import ROOT
    TR = importlib.import_module(PKG + ".train")
    M = importlib.import_module(PKG + ".model")
    B, steps = 512, 2

    def install(ens, masks):
        for lvl, em in enumerate(ens.mla.embedded_mappings):
            for j, d in enumerate(em.dropouts):
                d.mask = masks["mla.embedded_mappings.%d.dropouts.%d" % (lvl, j)]

    def one_process():
        ens = M.Ensemble("repeat", dict(mk.CNN_CONF), [2, 1], torch.device("cuda"), precision="bf16")
        ens.load_state_dict({k: torch.as_tensor(v) for k, v in W.make_state_dict(7, W.ensemble_shapes((2, 1), False)).items()})
        ens.cuda()
        M.set_requires_grad(ens, True)
        step = TR.TrainStep(ens, lr=1e-3)
        losses, hits_all = [], []
        for s in range(steps):
            x, y = mk.synth_bags(100 + s, B)
            install(ens, mk.make_masks(200 + s, [2, 1], B))
            loss, hits = step(x.cuda(), y.cuda())
            losses.append(float(loss)); hits_all.append(hits.tolist())
        return losses, hits_all, step.flat_p.clone()

    l1, h1, p1 = one_process()
    torch.cuda.empty_cache()
    l2, h2, p2 = one_process()
    assert l1 == l2 and h1 == h2 and torch.equal(p1, p2), "the bf16 finetune step must be bit-deterministic at full size"
    assert all(np.isfinite(l1)) and abs(l1[0] - np.log(10.0)) < 0.2 and all(0 <= h[0] <= B and h[1] == 0 for h in h1)
    del p1, p2
    torch.cuda.empty_cache()

    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "dpft512")
    env = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_dp_worker.py"), out, str(steps), str(B), "bf16", "finetune"],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=1200) == 0
    r0, r1 = np.load(out + ".rank0.npz"), np.load(out + ".rank1.npz")
    for k in r0.files:
        np.testing.assert_array_equal(r0[k], r1[k], err_msg=k)                    # replicas: bit-identical, CNN biases included
    assert any(k.startswith("cnn.") for k in r0.files)
    np.testing.assert_allclose(r0["losses"][:1], l1[:1], rtol=2e-6, atol=0)
    np.testing.assert_allclose(r0["losses"], l1, rtol=2e-3, atol=0)
    print("config 4 finetune bf16, 2 ranks vs 1 process: losses %s vs %s" % (r0["losses"], l1))


def test_composed_bf16_backward_against_float64_autograd_on_the_same_activations(W):
    """The whole bf16 CNN backward (cnn_train.backward: pool / ReLU backward from window codes, wgrad, dgrad, conv1's MFMA backward,
    the three Linear layers) composed, against torch autograd in float64 whose forward is FORCED onto the GPU's own bf16 activations
    (straight-through: every layer output is replaced by the value the HIP forward produced, gradients flow through the float64 graph)
    and whose weights are the bf16-rounded ones. What remains different is f32 accumulation order and the bf16 storage of the
    gradient tensors between layers -- no routing, indexing or layer-wiring error can hide: per parameter tensor the relative L2
    error must stay below 1e-2 (measured: printed) where the end-to-end check against the f32 path only asks for cosine 0.95."""
    cnn_train = importlib.import_module(PKG + ".cnn_train")
    V = importlib.import_module(PKG + ".torchvggish.vggish")
    n = 3
    vg = V.VGGish(urls={}, pretrained=False, preprocess=False, postprocess=False, precision="bf16")
    sd = W.make_state_dict(1, W.vggish_shapes())
    vg.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    vg.cuda()
    x = torch.from_numpy(W.uniform(91, 1, n * 96 * 64, lo=-1.4, hi=4.6)).reshape(n, 96, 64)
    d_out = torch.from_numpy(W.uniform(91, 2, n * 128, lo=-1.0, hi=1.0)).reshape(n, 128)
    with torch.no_grad():
        emb, tape = cnn_train.forward(vg, x.cuda(), "bf16")
        grads = {k: torch.zeros_like(p, dtype=torch.float32) for k, p in vg.named_parameters()}
        cnn_train.backward(vg, tape, d_out.cuda(), grads, "")
    # float64 reference on the GPU's activations
    conv_idx, pooled = [0, 3, 6, 8, 11, 13], {0, 3, 8, 13}
    params = {k: bf(torch.as_tensor(v)).double().requires_grad_(k.endswith("weight")) if k.endswith("weight")
              else torch.as_tensor(v).double().requires_grad_(True) for k, v in sd.items()}
    nhwc_to_nchw = lambda t: t.double().permute(0, 3, 1, 2).cpu()
    h = bf(x).double()[:, None]
    layer_inputs = {2: tape["layers"][2][0], 3: tape["layers"][3][0], 4: tape["layers"][4][0], 5: tape["layers"][5][0], 6: tape["layers"][6][0]}
    for li, idx in enumerate(conv_idx):
        z = F.relu(F.conv2d(h, params["features.%d.weight" % idx], params["features.%d.bias" % idx], padding=1))
        if idx in pooled:
            z = F.max_pool2d(z, 2, 2)
        gpu = nhwc_to_nchw(layer_inputs[li + 2]) if li + 2 <= 6 else nhwc_to_nchw(tape["fc"][0][0].reshape(n, 6, 4, 512))
        assert float((z.detach() - gpu).abs().max()) <= 2e-2 * float(gpu.abs().max()) + 1e-3, idx     # the forwards agree to bf16 rounding
        h = z + (gpu - z).detach()
    h = h.permute(0, 2, 3, 1).reshape(n, -1)
    for i, idx in enumerate((0, 2, 4)):
        z = F.relu(F.linear(h, params["embeddings.%d.weight" % idx], params["embeddings.%d.bias" % idx]))
        gpu = (tape["fc"][i][1] if i < 2 else emb).double().cpu()
        h = z + (gpu - z).detach()
    h.backward(d_out.double())
    worst = 0.0
    for k, g_gpu in grads.items():
        ref = params[k].grad
        err = float((g_gpu.cpu().double() - ref).norm() / (ref.norm() + 1e-30))
        worst = max(worst, err)
        assert err < 1e-2, (k, err)
    print("composed bf16 backward vs float64 autograd on the same activations: worst relative L2 error %.3g" % worst)
