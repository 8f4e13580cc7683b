"""Shapes, operands and float64 references of tests/test_infer_kernels_gpu.py, callable without a device
(tests/test_infer_kernel_cases_cpu.py runs every builder and every exactness assertion on the CPU at the small sizes).

Nothing here is an oracle for VALUES except torch float64 arithmetic on the stored operands. gemm_form() and conv_cfgs() restate
the launchers' CHOICES (which tile form dispatch<> takes, how many persistent workgroups launch_conv starts) and serve only to
choose the shapes and to name the branch a case is meant to enter; the lines they restate are read from the sources with _one(), so a
rewritten definition fails the regular expression instead of silently untesting a branch."""

import functools
import os
import re

import torch
import torch.nn.functional as F

from conftest import PKG, ROOT

F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24
P_IMAGES = 13                      # distinct images of every conv batch, repeated cyclically: coprime to every tile and grid stride


def _source(name):
    with open(os.path.join(ROOT, PKG, *name.split("/"))) as f:
        return f.read()


def _one(pattern, text, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, "%s is not in the form this test reads" % what
    return found[0]


# ------------------------------------------------------------------------------------------------ constants ----

def _constants():
    mma, gemm, conv, ops_py = _source("csrc/mma_core.h"), _source("csrc/gemm.hip"), _source("csrc/conv.hip"), _source("ops.py")
    c = {}
    c["kpr"] = {BF16: int(_one(r"struct Elem<bf16_t> \{ static constexpr int kPerChunk = \d+, kPerRow = (\d+); \};", mma, "Elem<bf16_t>")),
                F32: int(_one(r"struct Elem<float> \{ static constexpr int kPerChunk = \d+, kPerRow = (\d+); \};", mma, "Elem<float>"))}
    c["per"] = {BF16: int(_one(r"struct Elem<bf16_t> \{ static constexpr int kPerChunk = (\d+),", mma, "Elem<bf16_t>")),
                F32: int(_one(r"struct Elem<float> \{ static constexpr int kPerChunk = (\d+),", mma, "Elem<float>"))}
    # dispatch<>: the lines gemm_form() restates
    _one(r"const bool wide = N > 128 && \(N % 256 == 0 \|\| N % 256 > 128\);", gemm, "dispatch: wide")
    _one(r"const bool tall = wide && M >= 4096 && N >= 1024;", gemm, "dispatch: tall")
    _one(r"const double cost256 = 64\.0 \* double\(full\) \+ \(rest == 0 \? 0\.0 : \(full >= 1 && 2 \* rest <= cus && \(full \* cus\) % n_tiles == 0 \? 48\.0 : 64\.0\)\);",
         gemm, "dispatch: cost256")
    _one(r"const double cost320 = 72\.0 \* double\(\(t320 \+ cus - 1\) / cus\);", gemm, "dispatch: cost320")
    _one(r"if \(full_rounds >= 1 && rest > 0 && 2 \* rest <= cus && \(full_rounds \* cus\) % n_tiles == 0\) m_tall = full_rounds \* cus / n_tiles \* 256;",
         gemm, "dispatch: remainder split")
    _one(r"if \(\(\(M \+ 127\) / 128\) \* \(\(N \+ 255\) / 256\) \* 2 <= cus\) \{", gemm, "dispatch: half-empty chip")
    c["ring_min"] = int(_one(r"if \(K % mma::Elem<T>::kPerRow == 0 && K / mma::Elem<T>::kPerRow >= (\d+)\)", gemm, "dispatch: ring"))
    _one(r"if \(\(\(M \+ 127\) / 128\) \* \(\(N \+ 127\) / 128\) < cus && M > 64\)", gemm, "dispatch: 64-row tiles")
    assert _one(r"constexpr int kMS = 4, NS = 2, kBM = 128, BN = 128, RING = (\d+);", gemm, "ring depth") == "4"
    caps = re.findall(r"\(total \+ 255\) / 256 < (\d+) \? \(total \+ 255\) / 256 : (\d+)\)\), dim3\(256\),\s*0, s, partial", gemm)
    assert len(caps) == 2 and len({v for pair in caps for v in pair}) == 1, "splitk_reduce_kernel's grid cap is not in the form this test reads"
    c["reduce_cap"] = int(caps[0][0]) * 256
    c["ksplit"] = int(_one(r"\nKSPLIT = (\d+) ", ops_py, "ops.KSPLIT"))
    _one(r"splits = int\(min\(64, max\(2, 256 // tiles\), K // 512\)\)", ops_py, "ops.linear's split count")
    # element-wise helpers of conv.hip: 8192 x 256 grid caps
    caps = re.findall(r"const unsigned grid = unsigned\(\((?:n|total) \+ 255\) / 256 < (\d+) \? \((?:n|total) \+ 255\) / 256 : (\d+)\);", conv)
    assert len(caps) == 6 and {v for pair in caps[2:] for v in pair} == {"8192"}, "the helpers' grid caps are not in the form this test reads"
    c["helper_cap"] = 8192 * 256
    # conv1's persistent caps
    _one(r"const int64_t blocks = n \* 12 < int64_t\(cus1\) \* 4 \? n \* 12 : int64_t\(cus1\) \* 4;", conv, "conv1_kernel's grid")
    _one(r"const int64_t tiles = n \* \(96 / MLA_CONV1_ROWS\), slots = int64_t\(cus1\) \* MLA_CONV1_WAVES;", conv, "conv1_patch_kernel's grid")
    c["conv1_waves"] = int(_one(r"#define MLA_CONV1_WAVES (\d+)", conv, "MLA_CONV1_WAVES"))
    c["conv1_rows"] = int(_one(r"#define MLA_CONV1_ROWS (\d+) ", conv, "MLA_CONV1_ROWS"))
    # Cfg<>: the tile geometry conv_cfgs() restates, and launch_conv's grid
    _one(r"static constexpr int WM = WM_, WN = kWaves / WM_;", conv, "Cfg::WN")
    assert _one(r"constexpr int kThreads = 512, kWaves = (\d+), kMS = (\d+);", conv, "kWaves, kMS") == ("8", "6")
    _one(r"static constexpr int SEGW = W >= 16 \? 16 : 8;", conv, "Cfg::SEGW")
    _one(r"static constexpr int IMGS = SEGW == 8 \? WM : 1;", conv, "Cfg::IMGS")
    _one(r"static constexpr int TH = SEGW == 8 \? 12 : kMS \* WM / SEGS;", conv, "Cfg::TH")
    _one(r"static constexpr int BN = WN \* NS \* 16;", conv, "Cfg::BN")
    _one(r"static constexpr int TILES_Y = H / TH;", conv, "Cfg::TILES_Y")
    _one(r"constexpr int per_cu = \(C::LDS_BYTES \* 2 <= 160 \* 1024 && C::MIN_WAVES >= 4\) \? 2 : 1;", conv, "launch_conv: per_cu")
    _one(r"int64_t gx = int64_t\(cus\) \* per_cu / n_tiles_n;", conv, "launch_conv: gx")
    cases = re.findall(r"case (\d): return launch_conv<Cfg<(T|bf16_t), (\d+), (\d+), (\d+), (\d+), (true|false), (\d)(?:, true, (true|false))?(?:, (\d))?>>"
                       r"\(in, w, bias, out, n, s\);", conv)
    assert len(cases) == 20, "conv_layer / conv_layer_split are not in the form this test reads"
    cfgs = {}
    for i, (layer, _t, cin, cout, h, w, pool, ns, split, wm) in enumerate(cases):
        # order in the source: conv_layer tall (bf16), conv_layer wide (f32 and bf16 wide), conv_layer_split tall, conv_layer_split wide
        group = ("bf16/tall", "wide", "bf16x3/tall", "bf16x3/wide")[i // 5]
        assert (split == "true") == group.startswith("bf16x3") and (wm == "4") == group.endswith("tall"), (group, split, wm)
        cfgs[(int(layer), group)] = dict(cin=int(cin), cout=int(cout), H=int(h), W=int(w), pool=pool == "true", NS=int(ns), WM=int(wm or 2))
    c["conv_cfgs"] = cfgs
    return c


C = _constants()
KPR, PER = C["kpr"], C["per"]


def name(dtype):
    return "f32" if dtype == F32 else "bf16"


# ------------------------------------------------------------------------------------------ common idioms ----

def dyadic(gen, shape, bits=3, device="cpu"):
    """f32 multiples of 2^-bits in [-1, 1]: exact in bf16 for bits <= 7."""
    return torch.randint(-(1 << bits), (1 << bits) + 1, shape, generator=gen, dtype=torch.int32, device=device).float() / float(1 << bits)


def sparse9(gen, shape, density):
    """f32 values n 2^-9 with |n| <= 512, a fraction `density` of them non-zero: hi = bf16(x) and lo = x - hi are both exact bf16
    values (n has at most 10 significant bits, hi keeps 8, lo at most 2), and lo is non-zero for most non-zero x."""
    v = torch.randint(-512, 513, shape, generator=gen, dtype=torch.int32).float() / 512.0
    return v * (torch.rand(shape, generator=gen) < density)


def planes(x):
    """x (f32) -> hi = bf16(x), lo = bf16(x - hi), as torch rounds (to nearest even)."""
    hi = x.to(BF16)
    return hi, (x - hi.float()).to(BF16)


def cast(ref64, dtype):
    """float64 -> f32 -> dtype: the value an exact f32 accumulator stores (round-to-nearest-even for bf16)."""
    return ref64.float().to(dtype)


def split_out(ref64):
    """The [hi | lo] planes of an exact f32 value v along the last axis: hi = bf16(v), lo = bf16(v - hi)."""
    v = ref64.float()
    assert torch.equal(v.double(), ref64)
    hi, lo = planes(v)
    return torch.cat([hi, lo], dim=-1)


def assert_exact_arithmetic(abs_sum, unit=2.0 ** -6):
    """sum|terms| (bias included) in units of the finest grid is below 2^24: every partial sum in any order is an f32 value."""
    assert float(abs_sum.max()) / unit < 2 ** 24, float(abs_sum.max())


def within(got, ref, bound, what):
    """Per-element derived bound (evaluated where the result lives); prints the worst ratio error / bound before asserting."""
    got = got.double()
    ref, bound = ref.double().to(got.device), bound.double().to(got.device)
    err = (got - ref).abs()
    assert bool(torch.isfinite(got).all()), what
    ratio = float((err / (bound + 1e-300)).max())
    print("%s: worst |error| / bound = %.3g" % (what, ratio))
    assert ratio <= 1.0, (what, ratio)


def half_ulp_bf16(ref, b32):
    """Half a bf16 ulp of any value within b32 of ref is at most 2^-9 of its binade's upper end: <= 2^-8 (|ref| + b32)."""
    return 2.0 ** -8 * (ref.abs() + b32)


def ref_device():
    return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")


# ---------------------------------------------------------------------------------------------- GEMM forms ----

def gemm_form(M, N, K, kPerRow, cus):
    """Which tile form dispatch<> (csrc/gemm.hip) launches for out (M, N) = a (M, K) . w (N, K)^T: tile rows x tile columns, '+128' for
    the 128-row remainder launch behind 256 x 256 tiles, 'ring' for the four-stage 128 x 128 ring; '/dma' when the operands go to LDS
    by LDS-DMA (K a multiple of the 128-byte row), '/reg' when they are staged through registers (K tail)."""
    cdiv = lambda a, b: (a + b - 1) // b                                                        # noqa: E731
    dma = K % kPerRow == 0
    tag = "/dma" if dma else "/reg"
    wide = N > 128 and (N % 256 == 0 or N % 256 > 128)
    tall = wide and M >= 4096 and N >= 1024
    n_tiles = cdiv(N, 256)
    if tall and dma:
        t256, t320 = cdiv(M, 256) * n_tiles, cdiv(M, 320) * n_tiles
        full = t256 // cus
        rest = t256 - full * cus
        cost256 = 64.0 * full + (0.0 if rest == 0 else (48.0 if full >= 1 and 2 * rest <= cus and (full * cus) % n_tiles == 0 else 64.0))
        if 72.0 * cdiv(t320, cus) < cost256:
            return "320x256" + tag
    if tall:
        tiles = cdiv(M, 256) * n_tiles
        full = tiles // cus
        rest = tiles - full * cus
        split = full >= 1 and rest > 0 and 2 * rest <= cus and (full * cus) % n_tiles == 0
        return ("256x256+128" if split and full * cus // n_tiles * 256 != M else "256x256") + tag
    if wide:
        if cdiv(M, 128) * n_tiles * 2 <= cus:
            return "ring" + tag if dma and K // kPerRow >= C["ring_min"] else "128x128" + tag
        return "128x256" + tag
    if cdiv(M, 128) * cdiv(N, 128) < cus and M > 64:
        return "64x128" + tag
    return "128x128" + tag


def tall_rows(M, N, cus):
    """Rows the 256 x 256 launch of a '256x256+128' case covers."""
    n_tiles = (N + 255) // 256
    return ((M + 255) // 256 * n_tiles) // cus * cus // n_tiles * 256


# id -> (M, N, K in 128-byte rows or None for the register-staged twin): M = tile rows * k + 5, the last column tile partly empty,
# the smallest K that keeps the form (two stages; the ring from eight, and nine so that the four-stage ring wraps unevenly; the twins
# one 128-byte row and one 16-byte piece). Worked out with gemm_form() for 256 CUs; the GPU test evaluates gemm_form() with the
# device's CU count and fails, saying so, when a case would enter another form there.
GEMM_CASES = {
    "64x128/dma": (133, 300, 2), "64x128/reg": (133, 300, None),
    "128x128/dma": (133, 456, 2), "128x128/reg": (133, 456, None),
    "ring/dma": (133, 456, 8), "ring/dma-9": (133, 456, 9),
    "128x256/dma": (1157, 4040, 2), "128x256/reg": (1157, 4040, None),
    "256x256/dma": (4101, 1224, 2), "256x256/reg": (4101, 1224, None),
    "256x256+128/dma": (10245, 1992, 2), "256x256+128/reg": (10245, 1992, None),
    "320x256/dma": (9925, 1992, 2),
}
GEMM_PAIRS = [(F32, F32), (BF16, F32), (BF16, BF16)]
GEMM_DERIVED = {   # one per form on uniform data at K = 2048 (the short-K 128 x 128 form through its narrow-layer route)
    "64x128/dma": (133, 300), "128x128/dma": (37, 300), "ring/dma": (133, 456), "128x256/dma": (1157, 4040),
    "256x256/dma": (4101, 1224), "256x256+128/dma": (10245, 1992), "320x256/dma": (9925, 1992),
}


def gemm_k(case_id, dtype):
    rows = GEMM_CASES[case_id][2]
    return KPR[dtype] + PER[dtype] if rows is None else rows * KPR[dtype]


def form_of(case_id):
    return case_id.split("-")[0]


def gemm_operands(seed, M, N, K, device="cpu"):
    gen = torch.Generator(device=device).manual_seed(seed)
    return dyadic(gen, (M, K), device=device), dyadic(gen, (N, K), device=device), dyadic(gen, (N,), device=device)


def gemm_reference(a, w, b):
    """float64 a . w^T (+ b) and the sum of the terms' magnitudes, on the device the operands live on."""
    a, w = a.double(), w.double()
    y, y_abs = a @ w.t(), a.abs() @ w.abs().t()
    if b is not None:
        y, y_abs = y + b.double(), y_abs + b.double().abs()
    return y, y_abs


def x3_density(K):
    """About 40 non-zero products per output whatever K: 9 % non-zeros in both operands at K = 4608."""
    return min(0.5, (40.0 / K) ** 0.5)


def seg_planes_a(a, seg):
    """(M, K) f32 -> (M, 2K) bf16, [hi | lo] per segment of `seg` columns."""
    M, K = a.shape
    hi, lo = planes(a)
    return torch.stack([hi.view(M, K // seg, seg), lo.view(M, K // seg, seg)], dim=2).reshape(M, 2 * K).contiguous()


def seg_planes_w(w, seg):
    """(N, K) f32 -> (N, 3K) bf16, [hi | lo | hi] per segment."""
    N, K = w.shape
    hi, lo = planes(w)
    hi, lo = hi.view(N, K // seg, seg), lo.view(N, K // seg, seg)
    return torch.stack([hi, lo, hi], dim=2).reshape(N, 3 * K).contiguous()


def x3_gemm_case(seed, M, N, K):
    """Sparse 2^-9 operands, their exact planes and the float64 three-product reference a_hi w_hi + a_hi w_lo + a_lo w_hi + b."""
    gen = torch.Generator().manual_seed(seed)
    a, w, b = sparse9(gen, (M, K), x3_density(K)), sparse9(gen, (N, K), x3_density(K)), dyadic(gen, (N,))
    (ah, al), (wh, wl) = planes(a), planes(w)
    assert torch.equal(ah.float() + al.float(), a) and torch.equal(wh.float() + wl.float(), w) and int((al != 0).sum()) > 0 and int((wl != 0).sum()) > 0
    ah, al, wh, wl = (t.double() for t in (ah, al, wh, wl))
    y = ah @ (wh + wl).t() + al @ wh.t() + b.double()
    y_abs = ah.abs() @ (wh.abs() + wl.abs()).t() + al.abs() @ wh.abs().t() + b.double().abs()
    return dict(a=a, w=w, b=b, y=y, y_abs=y_abs)


X3_GEMM_CASES = {   # id -> (M, N, K, seg): dispatch<> sees 3K columns of bf16
    "64x128-seg64": (133, 300, 512, 64), "64x128-segK/2": (133, 300, 512, 256),
    "128x128-seg64": (133, 456, 128, 64),
    "ring-seg64": (133, 456, 512, 64), "ring-segK/2": (133, 456, 512, 256),
}


# --------------------------------------------------------------------------------------------- conv layers ----

LAYERS = (2, 3, 4, 5, 6)
SMALL_N = 5


def conv_cfg(layer, mode, tile):
    """The Cfg<> of conv.hip that mla_vggish_conv runs for (layer, 'f32' | 'bf16' | 'bf16x3', 'tall' | 'wide'), with its derived tile
    geometry. f32 has wide tiles only."""
    key = (layer, "wide" if mode != "bf16x3" and (mode == "f32" or tile == "wide") else mode + "/" + tile)
    g = dict(C["conv_cfgs"][key])
    segw = 16 if g["W"] >= 16 else 8
    g["IMGS"] = g["WM"] if segw == 8 else 1
    g["TH"] = 12 if segw == 8 else 6 * g["WM"] // (g["W"] // segw)
    g["BN"] = (8 // g["WM"]) * g["NS"] * 16
    g["TILES_Y"] = g["H"] // g["TH"]
    g["n_tiles_n"] = g["cout"] // g["BN"]
    assert g["H"] % g["TH"] == 0 and g["cout"] % g["BN"] == 0
    return g


def conv_tiles(g, n):
    return (n + g["IMGS"] - 1) // g["IMGS"] * g["TILES_Y"]


def persistent_n(g, cus):
    """Smallest image count whose tile count exceeds twice gx_bound = 2 cus / n_tiles_n (an upper bound of launch_conv's persistent
    grid, whatever per_cu is): some workgroup takes at least three tiles, i.e. re-uses both patch buffers. The tile count is no
    multiple of the bound, the batch ends inside a tile where tiles hold several images, and in the middle of the 13-image cycle."""
    bound = max(1, 2 * cus // g["n_tiles_n"])
    n = 2 * bound * g["IMGS"] // g["TILES_Y"]
    while not (conv_tiles(g, n) > 2 * bound and conv_tiles(g, n) % bound != 0 and (g["IMGS"] == 1 or n % g["IMGS"] != 0) and n % P_IMAGES != 0):
        n += 1
    return n


def conv_matmul(x, w):
    """3 x 3, pad 1 convolution in float64 as unfold + matmul. x (P, C, H, W), w (Cout, C, 3, 3) -> (P, Cout, H, W)."""
    P, Cc, H, Wd = x.shape
    cols = F.unfold(x, 3, padding=1)                                 # (P, C * 9, H * W)
    return (w.reshape(w.shape[0], -1) @ cols).reshape(P, w.shape[0], H, Wd)


def _plant(x, gen, fill):
    """Halo handling is the point: every image gets its own corners and dense border rows / columns. Image 0 gets a 4 x 4 block of
    zeros at rows 3..6, columns 1..4: the four pre-activations of the pooling window at rows 4..5, columns 2..3 are then the bias."""
    P, H, Wd, Cc = x.shape
    for side in (x[:, 0], x[:, H - 1], x[:, :, 0], x[:, :, Wd - 1]):
        side.copy_(fill(gen, tuple(side.shape)))
    for i in range(P):
        for c, (yy, xx) in enumerate(((0, 0), (0, Wd - 1), (H - 1, 0), (H - 1, Wd - 1))):
            x[i, yy, xx, :] = (((i + 1) * (c + 2)) % 17 - 8) / 8.0
    x[0, 3:7, 1:5, :] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def conv_case(layer, kind):
    """13 distinct NHWC images, OIHW weights and a bias for VGGish conv `layer`, with the float64 reference of the layer (bias, ReLU and
    the 2 x 2 max-pool of layers 2, 4, 6) and sum|terms| per output. kind 'grid': multiples of 2^-3 (f32 and bf16 runs); 'sparse9':
    sparse multiples of 2^-9 whose hi / lo planes are exact (bf16x3 runs; the reference is the three-product sum of the planes)."""
    g = conv_cfg(layer, "f32", "wide")
    cin, cout, H, Wd, pool = g["cin"], g["cout"], g["H"], g["W"], g["pool"]
    gen = torch.Generator().manual_seed(1000 * layer + len(kind))
    dev = ref_device()
    nchw = lambda t: t.double().permute(0, 3, 1, 2).contiguous().to(dev)                         # noqa: E731
    if kind == "grid":
        x = _plant(dyadic(gen, (P_IMAGES, H, Wd, cin)), gen, dyadic)
        w, b = dyadic(gen, (cout, cin, 3, 3)), dyadic(gen, (cout,))
        pre = conv_matmul(nchw(x), w.double().to(dev))
        pre_abs = conv_matmul(nchw(x).abs(), w.double().abs().to(dev))
        unit = 2.0 ** -6
    else:
        d = x3_density(9 * cin)
        x = _plant(sparse9(gen, (P_IMAGES, H, Wd, cin), d), gen, lambda gg, s: sparse9(gg, s, min(1.0, 2 * d)))
        w, b = sparse9(gen, (cout, cin, 3, 3), d), dyadic(gen, (cout,))
        (xh, xl), (wh, wl) = planes(x), planes(w)
        assert torch.equal(xh.float() + xl.float(), x) and torch.equal(wh.float() + wl.float(), w) and int((xl != 0).sum()) > 0 and int((wl != 0).sum()) > 0
        wh, wl = wh.double().to(dev), wl.double().to(dev)
        pre = conv_matmul(nchw(xh), wh + wl) + conv_matmul(nchw(xl), wh)
        pre_abs = conv_matmul(nchw(xh).abs(), wh.abs() + wl.abs()) + conv_matmul(nchw(xl).abs(), wh.abs())
        unit = 2.0 ** -18
    bb = b.double().to(dev).view(1, -1, 1, 1)
    pre, pre_abs = pre + bb, pre_abs + bb.abs()
    assert_exact_arithmetic(pre_abs, unit)
    assert bool((pre < 0).any()) and bool((pre > 0).any())              # ReLU has something to clamp
    y = pre.clamp_min(0)
    if pool:
        win = pre.reshape(P_IMAGES, cout, H // 2, 2, Wd // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(P_IMAGES, cout, H // 2, Wd // 2, 4)
        top = win.max(dim=-1).values
        alone = (win == top.unsqueeze(-1)).sum(dim=-1) == 1
        for pos in range(4):                                               # the maximum alone at each of the four positions, and positive
            assert bool(((win[..., pos] == top) & alone & (top > 0)).any()), pos
        planted = win[0, :, 2, 1, :]                                        # the window behind the block of zeros: four times the bias
        assert torch.equal(planted, bb.view(-1, 1).expand(-1, 4)) and bool((planted > 0).any())
        y = F.max_pool2d(y, 2)
    return dict(x=x, w=w, b=b, y=y.permute(0, 2, 3, 1).contiguous().cpu(), unit=unit, g=g,
                pre=pre.permute(0, 2, 3, 1).contiguous().cpu())       # the exact pre-activations, NHWC (tests/cnn_train_bf16_cases.py)


def packed_weight(w, dtype):
    """(Cout, Cin, 3, 3) -> (Cout, 9, Cin): what mla_conv_repack_weights produces, written with torch."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1]).contiguous().to(dtype)


def conv_operands(case, mode):
    """The stored operands of one run: images (13, H, W, C | 2C) and packed weights (Cout, 9, Cin | 3 Cin), and the expected output of
    the 13 images in the output's storage type ([hi | lo] planes for bf16x3)."""
    x, w, y = case["x"], case["w"], case["y"]
    if mode == "bf16x3":
        xh, xl = planes(x)
        wp = packed_weight(w, F32)
        cout, _, cin = wp.shape
        wh, wl = planes(wp.view(cout, 9, cin // 64, 64))
        return torch.cat([xh, xl], dim=-1).contiguous(), torch.stack([wh, wl, wh], dim=3).reshape(cout, 9, 3 * cin).contiguous(), split_out(y)
    dtype = F32 if mode == "f32" else BF16
    assert torch.equal(x.to(dtype).float(), x) and torch.equal(w.to(dtype).float(), w)
    return x.to(dtype), packed_weight(w, dtype), cast(y, dtype)


# --------------------------------------------------------------------------------------------------- conv1 ----

CONV1_PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32)]


def conv1_persistent_n(cus):
    """Smallest clip count beyond both persistent caps (conv1_kernel: cus * 4 blocks of 12 per clip; conv1_patch_kernel: cus *
    MLA_CONV1_WAVES slots of 96 / MLA_CONV1_ROWS tiles per clip) that leaves a remainder against both and against the 13-clip cycle."""
    t1, cap1, t2, cap2 = 12, cus * 4, 96 // C["conv1_rows"], cus * C["conv1_waves"]
    n = 1
    while not (n * t1 > cap1 and n * t2 > cap2 and (n * t1) % cap1 != 0 and (n * t2) % cap2 != 0 and n % P_IMAGES != 0):
        n += 1
    return n


@functools.lru_cache(maxsize=None)
def conv1_case(kind):
    """13 clips (96, 64), the 64 x 1 x 3 x 3 filter and bias. 'grid': multiples of 2^-3; 'uniform': log-mel-like values in [-6, 2) and
    weights in [-0.5, 0.5) with all their mantissa bits."""
    gen = torch.Generator().manual_seed(77 + len(kind))
    if kind == "grid":
        x, w, b = dyadic(gen, (P_IMAGES, 96, 64)), dyadic(gen, (64, 1, 3, 3)), dyadic(gen, (64,))
        x[:, 0], x[:, 95], x[:, :, 0], x[:, :, 63] = 1.0, -1.0, 0.875, -0.875
        x[0, 3:7, 1:5] = 0.0
    else:
        x = torch.rand((P_IMAGES, 96, 64), generator=gen) * 8 - 6
        w, b = torch.rand((64, 1, 3, 3), generator=gen) - 0.5, torch.rand((64,), generator=gen) - 0.5
    return dict(x=x, w=w, b=b)


def conv1_reference(x, w, b):
    """float64 conv1 + bias + ReLU + 2 x 2 max-pool of the operands AS GIVEN, NHWC (P, 48, 32, 64), and the pre-pool sum|terms| + |bias|
    pooled with max (|max a - max r| <= max |a - r|, and ReLU is 1-Lipschitz: the largest bound of a window bounds its pooled value)."""
    x, w, b = x.double().unsqueeze(1), w.double(), b.double().view(1, -1, 1, 1)
    pre, pre_abs = conv_matmul(x, w) + b, conv_matmul(x.abs(), w.abs()) + b.abs()
    y, y_abs = F.max_pool2d(pre.clamp_min(0), 2), F.max_pool2d(pre_abs, 2)
    return y.permute(0, 2, 3, 1).contiguous(), y_abs.permute(0, 2, 3, 1).contiguous()


def conv1_rounds_operands_to_bf16(x_dtype, out_dtype):
    """mla_vggish_conv1 runs every pairing with a bf16 OUTPUT on conv1_patch_kernel, which multiplies bf16(x) by bf16(w) on the bf16
    matrix unit; the pairings with an f32 output keep the f32 filter (and the input as stored)."""
    return out_dtype == BF16


# ------------------------------------------------------------------------------------------------- helpers ----

def special_f32():
    """Ties to even in both directions, +-0, the largest finite bf16 and f32 values, subnormals (one exact in bf16, one that rounds),
    infinities, and values next to a tie."""
    bits = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x00000000, 0x80000000, 0x7F7F0000, 0x7F7FFFFF,
            0xFF7F0000, 0x00010000, 0x00018000, 0x00008000, 0x80018000, 0x00000001, 0x7F800000, 0xFF800000, 0x007F8000, 0x3F800000]
    return torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in bits], dtype=torch.int32).view(F32)


def split_reference(x, seg, copies):
    """mla_split_bf16x3 written with torch: (rows, cols) f32 -> (rows, copies * cols) bf16, [hi | lo (| hi)] per segment."""
    rows, cols = x.shape
    hi, lo = planes(x)
    hi, lo = hi.view(rows, cols // seg, seg), lo.view(rows, cols // seg, seg)
    return torch.stack([hi, lo, hi][:copies], dim=2).reshape(rows, copies * cols)


def merge_reference(p, seg):
    """mla_merge_bf16x3 written with torch: (rows, 2 cols) bf16 [hi | lo] per segment -> hi + lo, one f32 addition."""
    rows, c2 = p.shape
    v = p.view(rows, c2 // (2 * seg), 2, seg).float()
    return (v[:, :, 0] + v[:, :, 1]).reshape(rows, c2 // 2)
