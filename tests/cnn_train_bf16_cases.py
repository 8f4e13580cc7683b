"""Shapes, operands and float64 references of tests/test_cnn_train_bf16_gpu.py (the bf16 finetune kernels of csrc/cnn_train_bf16.hip
and the bf16 forms of csrc/conv.hip's generic entry), callable without a device: tests/test_cnn_train_bf16_cases_cpu.py evaluates every
builder, reference and exactness / planted-case assertion on the CPU at an assumed 256 CUs.

Nothing here is an oracle for VALUES except torch float64 arithmetic on the stored operands. wgrad_splits(), generic_cfg() and the
constants restate the launchers' CHOICES (how many image splits mla_conv_wgrad_bf16 starts, which tile a generic conv case runs, the
fixed grids of the element-wise kernels) and serve only to choose the image counts; the lines they restate are read from the sources
with _one(), so a rewritten definition fails the regular expression instead of silently untesting a branch.

Ground rule for "exact": operands lie on a dyadic grid that bf16 holds exactly. When sum|terms| of an output, in units of the finest
product, is below 2^24, every partial sum in ANY order is an f32 value -- MFMA accumulators, per-split partials, wgrad_reduce_kernel's
f32 sum over splits, the sRed adds of conv1's backward -- and the result must equal the float64 reference bit for bit."""

import functools
import re

import torch
import torch.nn.functional as F

import infer_kernel_cases as K
from infer_kernel_cases import BF16, _one, _source, dyadic

CUS_ASSUMED = 256


# ------------------------------------------------------------------------------------------------ constants ----

def _constants():
    core, b16, conv = _source("csrc/cnn_train_core.h"), _source("csrc/cnn_train_bf16.hip"), _source("csrc/conv.hip")
    c = {}
    shapes = _one(r"#define MLA_WGRAD_SHAPES\(X\) (.*)\n", core, "MLA_WGRAD_SHAPES")
    c["wgrad_shapes"] = [tuple(int(v) for v in m) for m in re.findall(r"X\((\d+), (\d+), (\d+), (\d+)\)", shapes)]
    assert len(c["wgrad_shapes"]) == shapes.count("X("), "MLA_WGRAD_SHAPES is not in the form this test reads"
    c["tco128"] = int(_one(r"#ifndef MLA_WGRAD_TCO128\n#define MLA_WGRAD_TCO128 (\d) ", b16, "MLA_WGRAD_TCO128"))
    _one(r"static constexpr int TCO = \(MLA_WGRAD_TCO128 \|\| CIN < 128\) \? 128 : 64, TCI = \(MLA_WGRAD_TCO128 \|\| CIN < 128\) \? 64 : 128;",
         b16, "WBCfg::TCO, TCI")
    _one(r"static constexpr int TH = W == 32 \? 4 : \(W == 16 \? 8 : 12\);", b16, "WBCfg::TH")
    _one(r"const int tiles = C::TILES_CO \* C::TILES_CI;", b16, "launch_wgrad_bf16: tiles")
    _one(r"int splits = cus / tiles < 1 \? 1 : cus / tiles;", b16, "launch_wgrad_bf16: splits")
    _one(r"if \(splits > n\) splits = int\(n\);", b16, "launch_wgrad_bf16: splits <= n")
    _one(r"const int n_mine = split < n_img \? \(n_img - split \+ splits - 1\) / splits : 0;", b16, "wgrad_bf16_kernel: n_mine")
    c["c1_max_wg"] = int(_one(r"constexpr int kC1MaxWg = (\d+);", b16, "kC1MaxWg"))
    _one(r"const int wgs = \(n_seg \+ 3\) / 4 < kC1MaxWg \? \(n_seg \+ 3\) / 4 : kC1MaxWg;", b16, "mla_conv1_bwd_bf16: wgs")
    c["bias_grid8"] = int(_one(r"constexpr int kBiasGrid8 = (\d+);", b16, "kBiasGrid8"))
    # the generic conv entry: every compiled (cin, cout, H, W, pool, act) line, and the special 128 -> 64 tall tile of dgrad conv2
    lines = re.findall(r"\n    MLA_CONV_CASE(?:_TALL8?)?\((\d+), (\d+), (\d+), (\d+), (true|false), (\d), (true|false)\)", conv)
    c["generic_lines"] = [(int(ci), int(co), int(h), int(w), po == "true", ac == "true") for ci, co, h, w, po, _ns, ac in lines]
    _one(r"if constexpr \(sizeof\(T\) == 2\) return launch_conv<Cfg<T, 128, 64, 48, 32, false, 2, false, false, 4>>\(in, w, bias, out, n, s, prepool, codes\);",
         conv, "the tall dgrad conv2 tile")
    _one(r"return launch_conv<Cfg<T, CI, CO, HH, WW, PO, 4, AC, false, 4>>\(in, w, bias, out, n, s, prepool, codes\);", conv, "MLA_CONV_CASE_TALL")
    assert int(_one(r"#define MLA_CONV_DGRAD2 (\d) ", conv, "MLA_CONV_DGRAD2")) >= 1          # 1, 2: the tall 128 -> 64 tile is what bf16 runs
    return c


C = _constants()
SHAPES = C["wgrad_shapes"]                               # (cin, cout, H, W) of conv2 .. conv6


# ---------------------------------------------------------------------------------------------------- wgrad ----

def wgrad_tiles(cin, cout):
    tco, tci = (128, 64) if (C["tco128"] or cin < 128) else (64, 128)
    return (cout // tco) * (cin // tci)


def wgrad_splits(shape, cus):
    """Image splits of launch_wgrad_bf16 before it clamps them to n: one persistent workgroup per CU."""
    return max(1, cus // wgrad_tiles(shape[0], shape[1]))


def wgrad_bands(shape):
    H, W = shape[2], shape[3]
    return H // (4 if W == 32 else (8 if W == 16 else 12))


def wgrad_cases(cus):
    """(id, shape, n). n = 3: one image per workgroup. n = splits + 1: split 0 takes two images, the others one (uneven n_mine, the
    hand-over from an image's last band to the next image's band 0 in the other LDS buffer). W = 8 (BANDS == 1) also at 2 splits + 1:
    three items in one workgroup, both LDS images re-used. n = 1: fewer images than splits."""
    cases = []
    for s in SHAPES:
        tag = "%d-%d" % s[:2]
        sp = wgrad_splits(s, cus)
        cases.append((tag + "-n3", s, 3))
        cases.append((tag + "-splits+1", s, sp + 1))
        if s[3] == 8:
            cases.append((tag + "-2splits+1", s, 2 * sp + 1))
    cases.append(("256-256-n1", (256, 256, 24, 16), 1))
    return cases


def wgrad_bits(n):
    """Multiples of 2^-2 in general (worst case conv2 at 257 images: 257 * 1536 * 16 = 6.3e6 < 2^24 with every |term| = 1); the small
    cases use the finer 2^-4 grid (3 * 1536 * 256 = 1.2e6)."""
    return 4 if n <= 3 else 2


def wgrad_operands(shape, n, cus, device="cpu"):
    """A (n, H, W, cin), dZ (n, H, W, cout) in f32 holding grid values. In the first and second image of split 0 the first and last row of
    A is 1.0 (four times a typical |value| on the coarse grid): a y-halo row left over from an earlier item then adds a large
    one-signed-per-channel amount that cannot cancel."""
    cin, cout, H, W = shape
    gen = torch.Generator(device=device).manual_seed(7000 + cin + cout + n)
    bits = wgrad_bits(n)
    a, dz = dyadic(gen, (n, H, W, cin), bits, device), dyadic(gen, (n, H, W, cout), bits, device)
    for img in {0, min(n - 1, wgrad_splits(shape, cus))}:
        a[img, 0], a[img, H - 1] = 1.0, 1.0
    return a, dz, 2.0 ** (-2 * bits)


def wgrad_autograd(a, dz):
    """float64 autograd of F.conv2d on the CPU: dW (cout, cin, 3, 3)."""
    x64 = a.double().permute(0, 3, 1, 2).contiguous()
    w64 = torch.zeros((dz.shape[3], a.shape[3], 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, w64, padding=1).backward(dz.double().permute(0, 3, 1, 2).contiguous())
    return w64.grad


def wgrad_matmul(a, dz, absolute=False, chunk=32):
    """The same dW as nine shifted float64 matmuls, dW[:, :, ky, kx] = dZ_flat^T @ shift(A)_flat, per image (batched) and in slices of
    `chunk` images, on the device the operands live on. absolute=True: sum|terms| per element (the same with absolute values)."""
    n, H, W, cin = a.shape
    cout = dz.shape[3]
    dw = torch.zeros((cout, cin, 3, 3), dtype=torch.float64, device=a.device)
    for i in range(0, n, chunk):
        ap, z = F.pad(a[i:i + chunk].double(), (0, 0, 1, 1, 1, 1)), dz[i:i + chunk].double().flatten(1, 2)
        if absolute:
            ap, z = ap.abs(), z.abs()
        zt = z.transpose(1, 2).contiguous()
        for ky in range(3):
            for kx in range(3):
                dw[:, :, ky, kx] += torch.bmm(zt, ap[:, ky:ky + H, kx:kx + W].flatten(1, 2)).sum(dim=0)
    return dw


def assert_exact(abs_sum, unit):
    K.assert_exact_arithmetic(abs_sum, unit)


# ---------------------------------------------------------------------------------------------- conv1 backward ----

CONV1_NS = (1, 3, 65)
CH_TIE, CH_OFF, CH_POS = 0, 1, 2             # zero filter + positive bias; zero filter + zero bias; a single centre tap


@functools.lru_cache(maxsize=None)
def conv1_bwd_operands(n):
    """x multiples of 2^-2 in [-1, 3], w of 2^-4 in [-1/2, 1/2], bias of 2^-4 in [-1/2, 1/2], d_pooled of 2^-3 in [-1, 1]: all exact in
    bf16, bias + 9 products exact in f32 in any order (|sum| <= 14 in units of 2^-6), so the recompute and hence the routing are the
    same numbers on both sides, ties included. Planted: a constant block of x (all four window positions tie), a channel with zero
    filter and positive bias (ties everywhere), one with zero filter and zero bias (pre-activation exactly 0: nothing flows), one with a
    single centre tap (the maximum follows x to every window position)."""
    gen = torch.Generator().manual_seed(900 + n)
    x = torch.randint(-4, 13, (n, 96, 64), generator=gen, dtype=torch.int32).float() / 4.0
    w = torch.randint(-8, 9, (64, 1, 3, 3), generator=gen, dtype=torch.int32).float() / 16.0
    b = torch.randint(-8, 9, (64,), generator=gen, dtype=torch.int32).float() / 16.0
    d = dyadic(gen, (n, 48, 32, 64), 3)
    x[0, 10:20, 10:20] = 1.0
    w[CH_TIE], b[CH_TIE] = 0.0, 0.25
    w[CH_OFF], b[CH_OFF] = 0.0, 0.0
    w[CH_POS], b[CH_POS] = 0.0, 0.0
    w[CH_POS, 0, 1, 1] = 0.5
    for t in (x, w, b, d):
        assert torch.equal(t.to(BF16).float(), t)
    return x, w, b, d


def windows(t):
    """(P, C, H, W) -> (P, C, H/2, W/2, 4): the four positions of every pooling window in scan order (0,0) (0,1) (1,0) (1,1)."""
    P, Cc, H, W = t.shape
    return t.reshape(P, Cc, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(P, Cc, H // 2, W // 2, 4)


def conv1_bwd_reference(x, w, b, d, chunk=22):
    """float64 autograd of max_pool2d(relu(conv2d)) on the CPU in slices of `chunk` clips: dW, db, sum|terms| of dW and of db per
    element; the planted cases are asserted on the reference's own routing (the gradient that reaches the pre-activation)."""
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    dw_abs, db_abs = torch.zeros(64, 1, 3, 3, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)
    seen = set()
    for i in range(0, x.shape[0], chunk):
        xs, ds = x[i:i + chunk].double()[:, None], d[i:i + chunk].double().permute(0, 3, 1, 2)
        pre = F.conv2d(xs, w64, b64, padding=1)
        pre.retain_grad()
        F.max_pool2d(F.relu(pre), 2).backward(ds)
        g, p = windows(pre.grad), windows(pre.detach())
        dw_abs += torch.nn.grad.conv2d_weight(xs.abs(), (64, 1, 3, 3), pre.grad.abs(), padding=1)
        db_abs += pre.grad.abs().sum(dim=(0, 2, 3))
        # zero filter, positive bias: four equal positive values everywhere -> position 0 takes the whole gradient
        assert bool((p[:, CH_TIE] == 0.25).all()) and torch.equal(g[:, CH_TIE, ..., 0], ds[:, CH_TIE]) and not bool(g[:, CH_TIE, ..., 1:].any())
        # zero filter, zero bias: the pre-activation is exactly 0 and relu'(0) = 0
        assert bool((p[:, CH_OFF] == 0).all()) and not bool(g[:, CH_OFF].any())
        # single centre tap: a lone positive maximum at every position routes there
        top = p[:, CH_POS].max(dim=-1).values
        alone = ((p[:, CH_POS] == top.unsqueeze(-1)).sum(dim=-1) == 1) & (top > 0)
        for pos in range(4):
            here = alone & (p[:, CH_POS, ..., pos] == top)
            if bool(here.any()):
                assert torch.equal(g[:, CH_POS, ..., pos][here], ds[:, CH_POS][here])
                seen.add(pos)
        if i == 0:      # the constant block of clip 0: pooled rows 6..8, columns 6..8 see constant patches -> ties -> position 0
            blk, gb, db_ = p[0, :, 6:9, 6:9], g[0, :, 6:9, 6:9], ds[0, :, 6:9, 6:9]
            assert bool((blk == blk[..., :1]).all()) and bool((blk[..., 0] > 0).any())
            assert torch.equal(gb[..., 0], torch.where(blk[..., 0] > 0, db_, torch.zeros_like(db_))) and not bool(gb[..., 1:].any())
    assert seen == {0, 1, 2, 3}, seen
    return w64.grad, b64.grad, dw_abs, db_abs


# ------------------------------------------------------------------------------------- pool / ReLU backward ----

POOL_SHAPES = [(2, 4, 6, 8), (3, 2, 2, 16), (172, 12, 8, 512)]       # (n, H, W, C): C / 8 = 1 and 2 below the grid, the last beyond it
SENTINEL = -7.0                                                        # exact in bf16; no gradient of the grid equals it


def plant(a):
    """One window of four equal positive values (the first position must win) and one all-zero window (nothing may flow)."""
    a[0, :2, :2, :] = 0.5
    a[1, 2:4, 2:4, :] = 0.0
    return a


def pool_operands(shape, pool):
    n, H, W, Cc = shape
    gen = torch.Generator().manual_seed(500 + n + int(pool))
    a = plant(dyadic(gen, shape).clamp_min(0))                         # post-ReLU grid data: about half zeros, 9 distinct values
    d = dyadic(gen, (n, H // 2, W // 2, Cc) if pool else shape)
    return a, d


def pool_reference(a, d, pool, planted=True):
    """float64 autograd of max_pool2d(relu(a), 2) (or relu(a)) at NHWC a on the CPU: dA, NHWC."""
    x = a.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.max_pool2d(F.relu(x), 2) if pool else F.relu(x)
    y.backward(d.double().permute(0, 3, 1, 2))
    dz = x.grad.permute(0, 2, 3, 1)
    if pool and planted:    # torch's rule on the planted windows: the first of four equal values takes everything, zeros take nothing
        assert torch.equal(dz[0, 0, 0], d[0, 0, 0].double()) and not bool(dz[0, 0, 1].any() or dz[0, 1, :2].any())
        assert not bool(dz[1, 2:4, 2:4].any())
    return dz


def codes_operands(shape):
    """Codes drawn uniformly from 0..4 (the contract of mla_pool_bwd_codes_bf16) at the pooled resolution; the first eight channels of
    pixel (0, 0, 0) hold 0, 1, 2, 3, 4, 3, 2, 1: a byte order mistake inside the two 32-bit words moves those gradients."""
    n, H, W, Cc = shape
    gen = torch.Generator().manual_seed(600 + n)
    codes = torch.randint(0, 5, (n, H // 2, W // 2, Cc), generator=gen, dtype=torch.uint8)
    codes[0, 0, 0, :8] = torch.tensor([0, 1, 2, 3, 4, 3, 2, 1], dtype=torch.uint8)
    d = dyadic(gen, (n, H // 2, W // 2, Cc))
    d[0, 0, 0, :8] = torch.tensor([1.0, 0.875, 0.75, 0.625, 0.5, 0.375, 0.25, 0.125])
    return codes, d


def route_by_codes(codes, d):
    """dz[window position code] = d where code < 4, 0 elsewhere. codes, d (n, H/2, W/2, C) -> float64 (n, H, W, C)."""
    n, HO, WO, Cc = codes.shape
    dz = torch.zeros((n, 2 * HO, 2 * WO, Cc), dtype=torch.float64, device=d.device)
    for pos in range(4):
        dz[:, pos >> 1::2, pos & 1::2] = torch.where(codes == pos, d.double(), torch.zeros((), dtype=torch.float64, device=d.device))
    return dz


# --------------------------------------------------------------------------------- the generic conv entry ----

FWD_LAYERS = (2, 3, 4, 5, 6)                  # un-pooled forward, act=True: every VGGish shape (layers 3 and 5 are what the step runs)
POOLED_LAYERS = (2, 4, 6)                     # conv3x3_train / conv3x3_train_codes
DGRAD_SHAPES = [(512, 512, 12, 8), (512, 256, 12, 8), (256, 256, 24, 16), (256, 128, 24, 16), (128, 64, 48, 32)]   # channels of dZ, of dA
WIDE_LAYERS = (4, 6)                          # one W = 16 and one W = 8 layer also with MLA_CONV_TILE=wide
WIDE_DGRAD = [(256, 256, 24, 16), (512, 512, 12, 8)]
PERSISTENT_DGRAD = [(128, 64, 48, 32), (512, 512, 12, 8)]     # the special tall 128 -> 64 tile, and one W = 8 form


def layer_shape(layer):
    g = K.conv_cfg(layer, "f32", "wide")
    return g["cin"], g["cout"], g["H"], g["W"]


def generic_table():
    """Every (cin, cout, H, W, pool, act) the case table above sends through conv_generic<bf16_t>."""
    t = {layer_shape(l) + (False, True) for l in FWD_LAYERS} | {layer_shape(l) + (True, True) for l in POOLED_LAYERS}
    return t | {s + (False, False) for s in DGRAD_SHAPES}


def generic_cfg(cin, cout, H, W, tile):
    """Tile geometry of the bf16 Cfg<> conv_generic runs for an un-pooled shape: the tall tile (4 x 2 waves, NS = 4; 128 -> 64: NS = 2)
    or, with MLA_CONV_TILE=wide, the 2 x 4 one. Same derivation as infer_kernel_cases.conv_cfg."""
    wm, ns = (4, 2 if cout == 64 else 4) if tile == "tall" else (2, {64: 1, 128: 2}.get(cout, 4))
    segw = 16 if W >= 16 else 8
    g = dict(cin=cin, cout=cout, H=H, W=W, WM=wm, NS=ns, IMGS=wm if segw == 8 else 1)
    g["TH"] = 12 if segw == 8 else 6 * wm // (W // segw)
    g["BN"] = (8 // wm) * ns * 16
    g["TILES_Y"], g["n_tiles_n"] = H // g["TH"], cout // g["BN"]
    assert H % g["TH"] == 0 and cout % g["BN"] == 0
    return g


@functools.lru_cache(maxsize=None)
def dgrad_case(shape):
    """13 distinct dZ images (planted corners, dense borders), a forward weight (Cout_fwd = channels of dZ, Cin_fwd = channels of dA) on the
    2^-3 grid and dA = conv_transpose2d in float64: at most 9 * 512 products of |value| <= 1 in units of 2^-6, asserted below 2^24."""
    cz, ca, H, W = shape
    gen = torch.Generator().manual_seed(3000 + cz + ca)
    dev = K.ref_device()
    dz = K._plant(dyadic(gen, (K.P_IMAGES, H, W, cz)), gen, dyadic)
    wf = dyadic(gen, (cz, ca, 3, 3))
    z64, w64 = dz.double().permute(0, 3, 1, 2).contiguous().to(dev), wf.double().to(dev)
    y = F.conv_transpose2d(z64, w64, padding=1)
    assert_exact(F.conv_transpose2d(z64.abs(), w64.abs(), padding=1), 2.0 ** -6)
    return dict(dz=dz, wf=wf, y=y.permute(0, 2, 3, 1).contiguous().cpu())


@functools.lru_cache(maxsize=None)
def narrow_case(layer):
    """Operands for the window codes: x multiples of 2^-1 in [-1, 1], four non-zero weights of +-1/2 or +-1 per output channel, bias
    multiples of 2^-2 in [-1, 1]. |pre-activation| <= 5 in units of 2^-2: every pre-activation is a bf16 value (asserted), so the
    stored pre-pool activation orders a window exactly as the f32 accumulators do, and ties for the maximum are frequent (asserted:
    at least 1 % of the windows, and at least one window whose maximum is exactly 0)."""
    cin, cout, H, W = layer_shape(layer)
    gen = torch.Generator().manual_seed(4000 + layer)
    dev = K.ref_device()
    half = lambda gg, s: dyadic(gg, s, 1)                                                         # noqa: E731
    x = K._plant(half(gen, (K.P_IMAGES, H, W, cin)), gen, half)
    w = torch.zeros((cout, cin * 9))
    idx = torch.stack([torch.randperm(cin * 9, generator=gen)[:4] for _ in range(cout)])
    vals = torch.tensor([-1.0, -0.5, 0.5, 1.0])[torch.randint(0, 4, (cout, 4), generator=gen)]
    w = w.scatter_(1, idx, vals).reshape(cout, cin, 3, 3)
    b = dyadic(gen, (cout,), 2)
    x64 = x.double().permute(0, 3, 1, 2).contiguous().to(dev)
    pre = (K.conv_matmul(x64, w.double().to(dev)) + b.double().to(dev).view(1, -1, 1, 1)).permute(0, 2, 3, 1).contiguous().cpu()
    assert float(pre.abs().max()) <= 5.0 and torch.equal(pre.float().to(BF16).double(), pre)
    return dict(x=x, w=w, b=b, pre=pre)


def window_codes(pre):
    """pre (P, H, W, C) float64 exact pre-activations -> (codes uint8 (P, H/2, W/2, C), tie mask, maximum): the first maximum in scan
    order of the four pre-activations, or 4 where that maximum is <= 0."""
    win = windows(pre.permute(0, 3, 1, 2)).permute(0, 2, 3, 1, 4)                                 # (P, H/2, W/2, C, 4)
    top = win.max(dim=-1).values
    eq = win == top.unsqueeze(-1)
    arg = torch.full(top.shape, 3, dtype=torch.uint8)
    for pos in (2, 1, 0):
        arg = torch.where(eq[..., pos], torch.full_like(arg, pos), arg)
    codes = torch.where(top > 0, arg, torch.full_like(arg, 4))
    return codes, eq.sum(dim=-1) >= 2, top


def train_reference(pre):
    """(pre-pool post-ReLU activation, pooled activation) in bf16 = round-to-nearest-even of the exact values, and the codes."""
    codes, ties, top = window_codes(pre)
    return K.cast(pre.clamp_min(0), BF16), K.cast(top.clamp_min(0), BF16), codes, ties, top
