"""The comparison rule, the injection patterns and the float64 references of tests/test_nonfinite_gpu.py and
tests/test_nonfinite_cpu.py: how a kernel must treat NaN and Inf.

ONE RULE (same_nonfinite): for a kernel output `got` and the float64 reference `ref` of the same stored operands (for bf16: the
bf16-rounded values), isnan(got) == isnan(ref) element by element, got == +inf exactly where ref == +inf, the same for -inf, and
where ref is finite `got` meets the criterion of the kernel's existing finite test (bit-equality on the dyadic grid, or the derived
bound) -- the caller passes that criterion as `finite(got, ref)`; both arrive with 0 at the reference's non-finite positions, so
the criterion needs no masking of its own. The rule catches a kernel that DROPS a NaN (fmaxf(x, 0) returns 0 for NaN, where
nn.ReLU, nn.MaxPool2d, torch.clamp and np.maximum return NaN) and one that INVENTS one (an out-of-range operand masked by a
multiplication with 0 instead of being skipped: NaN * 0 = NaN).

One exception: precision "bf16x3" fed an Inf operand splits it into hi = inf and lo = inf - inf = NaN, so there only "non-finite
wherever the reference is, finite elsewhere" is required (x3_inf=True). NaN operands in bf16x3 obey the full rule.

Operands come from the generators of the sibling finite tests (infer_kernel_cases.py, cnn_train_bf16_cases.py,
test_resnet_kernels_gpu.py, test_train_kernels_gpu.py): no tolerance is introduced here. Magnitudes stay small: every finite
reference value is asserted to lie below the largest finite bf16.

Injection patterns (the names the tests use):
  a  one NaN in an interior input element of image 0 / row tile 0: the rest of the batch is bit-identical to the clean run
  b  one NaN in the last pixel / row / column of a tail tile
  c  +Inf and -Inf elements: relu(-inf) = 0, relu(+inf) = +inf, pooling over -inf
  d  one NaN in a weight, bias or BatchNorm parameter: that output channel is NaN everywhere and no other is
  e  NaN in memory the result must not depend on (row padding, rows behind M, images behind n, K padding, a workspace): the
     output is bit-identical to the clean run
"""

import numpy as np
import torch
import torch.nn.functional as F

import infer_kernel_cases as K
from infer_kernel_cases import BF16, F32

NAN, INF = float("nan"), float("inf")
BF16_MAX = float(torch.finfo(torch.bfloat16).max)


def _bits(t):
    """The stored bits as integers (NaN == NaN, -0 != +0)."""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


def same_nonfinite(got, ref, what, finite=None, x3_inf=False):
    """The rule of this module's docstring. got: the kernel's output (any float type, any device), ref: float64 of the same shape.
    finite(g, r): the sibling test's criterion on float64 copies in which the reference's non-finite positions are 0."""
    got = torch.as_tensor(got)
    ref = torch.as_tensor(ref).to(got.device)
    assert ref.dtype == torch.float64 and tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape, ref.dtype)
    g = got.double()
    fin = torch.isfinite(ref)
    assert float(ref[fin].abs().max()) <= BF16_MAX if bool(fin.any()) else True, "%s: a finite reference value exceeds bf16" % what
    if x3_inf:
        bad = torch.isfinite(g) != fin
        assert not bool(bad.any()), "%s: %d elements are finite where the reference is not, or the reverse" % (what, int(bad.sum()))
    else:
        for label, a, b in (("NaN", torch.isnan(g), torch.isnan(ref)), ("+inf", g == INF, ref == INF), ("-inf", g == -INF, ref == -INF)):
            lost, made = int((b & ~a).sum()), int((a & ~b).sum())
            assert lost == 0 and made == 0, "%s: %d of the reference's %d %s are missing, %d appear where it has none" % (
                what, lost, int(b.sum()), label, made)
    if finite is not None:
        zero = torch.zeros((), dtype=torch.float64, device=g.device)
        finite(torch.where(fin, g, zero), torch.where(fin, ref, zero))
    return fin


def exact(dtype):
    """Criterion of the dyadic-grid tests: the output is the float64 value, cast once (f32, or round-to-nearest-even bf16)."""
    def check(g, r):
        want = K.cast(r, dtype).double()
        bad = g != want
        assert not bool(bad.any()), "%d finite elements differ from the exact value" % int(bad.sum())
    return check


def bounded(bound, what):
    """Criterion of the derived-bound tests: |got - ref| <= bound per element (the bound is taken as 0 where it is not finite)."""
    def check(g, r):
        b = torch.nan_to_num(torch.as_tensor(bound).double().to(g.device), nan=0.0, posinf=0.0, neginf=0.0)
        ratio = float(((g - r).abs() / (b + 1e-300)).max())
        print("%s: worst |error| / bound on the finite elements = %.3g" % (what, ratio))
        assert ratio <= 1.0, (what, ratio)
    return check


def assert_channels(ref, channel, what, axis=-1):
    """Pattern d on the REFERENCE: exactly `channel` along `axis` is NaN everywhere, nothing else is."""
    nan = torch.isnan(ref).movedim(axis, -1)
    assert bool(nan[..., channel].all()) and int(nan.sum()) == nan[..., channel].numel(), what


# ---------------------------------------------------------------------------------------------- VGGish convs ----

def conv_stored(x, w, mode):
    """infer_kernel_cases.conv_operands without its exactness assertions (they fail on NaN): the stored images and packed weights."""
    if mode == "bf16x3":
        xh, xl = K.planes(x)
        wp = K.packed_weight(w, F32)
        cout, _, cin = wp.shape
        wh, wl = K.planes(wp.view(cout, 9, cin // 64, 64))
        return torch.cat([xh, xl], dim=-1).contiguous(), torch.stack([wh, wl, wh], dim=3).reshape(cout, 9, 3 * cin).contiguous()
    dtype = F32 if mode == "f32" else BF16
    return x.to(dtype), K.packed_weight(w, dtype)


def conv_reference(x, w, b, pool, x3=False, relu=True):
    """float64 conv + bias (+ ReLU) (+ 2 x 2 max-pool) of NHWC x, as infer_kernel_cases.conv_case computes it; x3: the three-product
    sum of the stored planes. Returns (output NHWC, pre-activation NHWC), on the CPU."""
    dev = K.ref_device()
    nchw = lambda t: t.double().permute(0, 3, 1, 2).contiguous().to(dev)                          # noqa: E731
    if x3:
        (xh, xl), (wh, wl) = K.planes(x), K.planes(w)
        wh, wl = wh.double().to(dev), wl.double().to(dev)
        pre = K.conv_matmul(nchw(xh), wh + wl) + K.conv_matmul(nchw(xl), wh)
    else:
        pre = K.conv_matmul(nchw(x), w.double().to(dev))
    pre = pre + b.double().to(dev).view(1, -1, 1, 1)
    y = F.relu(pre) if relu else pre
    if pool:
        y = F.max_pool2d(y, 2)
    return y.permute(0, 2, 3, 1).contiguous().cpu(), pre.permute(0, 2, 3, 1).contiguous().cpu()


def merged(got_split):
    """[hi | lo] planes along the last axis -> hi + lo in float64 (NaN where either plane is)."""
    c = got_split.shape[-1] // 2
    return got_split[..., :c].double() + got_split[..., c:].double()


def assert_split_planes(got_split, ref, fin, what):
    """bf16x3 outputs, after same_nonfinite(merged(got), ref) returned `fin`: where the reference is finite the stored planes are
    hi = bf16(v), lo = bf16(v - hi) of the exact value, plane by plane."""
    ref, fin = ref.cpu(), fin.cpu()
    want = K.split_out(torch.where(fin, ref, torch.zeros((), dtype=torch.float64)))
    bad = (got_split.cpu().double() != want.double()) & torch.cat([fin, fin], dim=-1)
    assert not bool(bad.any()), "%s: %d plane elements differ from the exact split" % (what, int(bad.sum()))


CONV_PATTERNS = ("a", "b", "c", "d-weight", "d-bias", "e")


def conv_inject(case, pattern, n):
    """Operands of one VGGish conv launch: the first n images of `case` with `pattern` applied. Returns x (n or n + 1 images: e keeps
    a NaN image behind the batch), w, b, the images whose output must keep the clean run's bits, and the poisoned channel (d)."""
    x, w, b = case["x"][:n].clone(), case["w"].clone(), case["b"].clone()
    _, H, Wd, cin = x.shape
    keep, channel = slice(0, 0), None
    if pattern == "a":
        x[0, H // 2, Wd // 2, cin // 2] = NAN
        keep = slice(1, n)
    elif pattern == "b":
        x[n - 1, H - 1, Wd - 1, cin - 1] = NAN
        keep = slice(0, n - 1)
    elif pattern == "c":
        x[0, 1, 1, 0], x[n - 1, H - 2, Wd - 2, cin - 1] = INF, -INF
        keep = slice(1, n - 1)
    elif pattern == "d-weight":
        channel = w.shape[0] - 3
        w[channel, cin // 2, 1, 1] = NAN                   # the centre tap: no output pixel lacks it
    elif pattern == "d-bias":
        channel = 1
        b[channel] = NAN
    elif pattern == "e":
        x = torch.cat([x, torch.full_like(x[:1], NAN)])
        keep = slice(0, n)
    else:
        raise KeyError(pattern)
    return x, w, b, keep, channel


# ------------------------------------------------------------------------------------------------- waveforms ----

def nan_sample(x, index):
    """A copy of the float waveform(s) x with one NaN sample at `index` (a tuple for 2-D input)."""
    y = np.array(x, dtype=np.float32, copy=True)
    y[index] = np.nan
    return y


def frames_touching(index, n_frames, hop, win, pad=0):
    """The frames f with f * hop - pad <= index < f * hop - pad + win."""
    f = np.arange(n_frames)
    return (f * hop - pad <= index) & (index < f * hop - pad + win)
