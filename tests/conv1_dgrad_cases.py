"""Operands, image counts and the float64 reference of conv1's input gradient (csrc/conv1_dgrad.hip, csrc/conv1_dgrad_core.h),
callable without a device: tests/test_conv1_dgrad_cpu.py (host simulation, C ABI) and tests/test_input_grad_gpu.py share them.

Operands are cnn_train_bf16_cases.conv1_bwd_operands(n): x multiples of 2^-2, w of 2^-4, bias of 2^-4, d_pooled of 2^-3, all exact in
bf16, with planted ties, an "off" channel and a single-centre-tap channel. The recompute (bias + 9 products in units of 2^-6, |sum| <=
14 * 64 units) is exact in f32 in any order, so the routing is the same on both sides; dx is a sum of products d * w in units of
2^-7, and where sum|terms| stays below 2^24 units (asserted here) every partial sum in ANY order is an f32 value: the kernel's result
must EQUAL the float64 reference, with an f32 and with a bf16 d_pooled alike.

The only value oracle is torch float64 autograd of max_pool2d(relu(conv2d)) with respect to x. cap_crossing_n() restates the
launcher's grid (a workgroup takes a second item once n * tiles passes the cap); the constants are read from the source with _one(),
so a rewritten definition fails the regular expression instead of silently untesting the second trip."""

import functools

import torch
import torch.nn.functional as F

import cnn_train_bf16_cases as T
from infer_kernel_cases import _one, _source

UNIT = 2.0 ** -7                                  # finest product d_pooled * w
NS = T.CONV1_NS                                   # 1, 3, 65
SENTINEL = -7.0 - 2.0 ** -8                       # an f32 value off the 2^-7 grid: no gradient equals it (asserted per case)


def _constants():
    core, hip = _source("csrc/conv1_dgrad_core.h"), _source("csrc/conv1_dgrad.hip")
    c = {}
    c["tile_rows"] = int(_one(r"constexpr int kTileRows = (\d+);", core, "kTileRows"))
    c["max_wg"] = int(_one(r"constexpr int kMaxWg = (\d+);", core, "kMaxWg"))
    _one(r"constexpr int kTiles = kH / kTileRows;", core, "kTiles")
    _one(r"MLA_HD int64_t items_of\(int64_t n\) \{ return n \* kTiles; \}", core, "items_of")
    _one(r"MLA_HD int grid_of\(int64_t n\) \{ return int\(items_of\(n\) < kMaxWg \? items_of\(n\) : kMaxWg\); \}", core, "grid_of")
    _one(r"dim3\(cd::grid_of\(n\)\), dim3\(cd::kThreads\), 0, s, x, w, bias, d_pooled, cd::items_of\(n\), dx\);", hip, "launch_conv1_dgrad")
    _one(r"for \(int64_t item = blockIdx\.x; item < n_items; item \+= gridDim\.x\) \{", hip, "conv1_dgrad_kernel: item loop")
    return c


C = _constants()
TILES = 96 // C["tile_rows"]


def grid_of(n):
    return min(n * TILES, C["max_wg"])


def cap_crossing_n():
    """The smallest n at which a workgroup of the capped grid takes a second item."""
    n = C["max_wg"] // TILES + 1
    assert n * TILES > C["max_wg"] >= (n - 1) * TILES
    return n


@functools.lru_cache(maxsize=None)
def reference(n, chunk=16):
    """(dx float64 (n, 96, 64), sum|terms| float64) by float64 autograd on the CPU in slices of `chunk` clips; the second is
    conv_transpose2d of |routed gradient| with |w|. Asserted: conv_transpose2d of the routed gradient IS autograd's dx, the 2^24
    bound, dx on the 2^-7 grid and hence an f32 value bit for bit, no element equal to the sentinel."""
    x, w, b, d = T.conv1_bwd_operands(n)
    w64, b64 = w.double(), b.double()
    dx, dabs = [], []
    for i in range(0, n, chunk):
        xs = x[i:i + chunk].double()[:, None].requires_grad_(True)
        ds = d[i:i + chunk].double().permute(0, 3, 1, 2)
        pre = F.conv2d(xs, w64, b64, padding=1)
        pre.retain_grad()
        F.max_pool2d(F.relu(pre), 2).backward(ds)
        routed = pre.grad
        assert torch.equal(F.conv_transpose2d(routed, w64, padding=1), xs.grad)
        dx.append(xs.grad[:, 0])
        dabs.append(F.conv_transpose2d(routed.abs(), w64.abs(), padding=1)[:, 0])
    dx, dabs = torch.cat(dx), torch.cat(dabs)
    T.assert_exact(dabs, UNIT)
    assert torch.equal((dx / UNIT).round() * UNIT, dx) and torch.equal(dx.float().double(), dx)
    assert not bool((dx == SENTINEL).any())
    return dx, dabs


def two_clip_case():
    """Clip 0 of the n = 1 operands followed by a second clip whose d_pooled is all zero (its x is clip 0's, shifted): dx[1] must
    be exactly 0 and dx[0] the one-clip result."""
    x, w, b, d = T.conv1_bwd_operands(1)
    x2 = torch.cat([x, x.roll(5, dims=2)]).contiguous()
    d2 = torch.cat([d, torch.zeros_like(d)]).contiguous()
    return x2, w, b, d2
