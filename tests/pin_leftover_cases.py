"""Shapes, operands, float64 references and bounds of tests/test_pin_leftovers_gpu.py, callable without a device
(tests/test_pin_leftover_cases_cpu.py evaluates every case, every exactness assertion and every constant on the CPU).

Six kernel families: rn_stem_kernel, rn_stem_wgrad, linear_narrow_kernel<N>, linear_small_kernel / linear_small_wide_kernel,
mla_col_sum / mla_col_sum_bf16, and mla_bn_stats / mla_bn_stats_fused up to 64 channels. Nothing here is an oracle for VALUES except
torch float64 arithmetic on the stored operands. small_form(), narrow_grid(), colsum_chunks() and stats_blocks() restate the
launchers' CHOICES and serve only to choose the shapes and to name the branch a case is meant to enter; the lines they restate are
read from the sources with _one(), so a rewritten definition fails the regular expression instead of silently untesting a branch.

Two kinds of criterion, as in tests/infer_kernel_cases.py:
  exact    operands on the dyadic grid (multiples of 2^-3 in [-1, 1]); the case asserts sum|terms| / unit < 2^24 from its own float64
           reference, so every partial sum in any order is an f32 value;
  derived  |got - ref| <= P 2^-24 sum|terms| per element (P counted in the docstring of the bound), plus half a bf16 ulp for a bf16
           output; quantities reduced in double: count 2^-53 sum|terms| plus the one f32 rounding of the result."""

import functools
import re

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_weight

import infer_kernel_cases as K
import test_resnet_kernels_gpu as RK             # stem_case(): the planes and gradients of the n = 10 and n = 19 weight-gradient tests
import test_wide_head_gpu as WH                  # _stats_reference(): float64 statistics per column and their bounds
from infer_kernel_cases import BF16, F32, U, _one, _source, dyadic

D = 2.0 ** -53                                   # unit roundoff of float64


# ------------------------------------------------------------------------------------------------ constants ----

def _constants():
    head, train, core, fwd, bwd = (_source("csrc/" + n) for n in ("mla_head.hip", "train_kernels.hip", "rn_core.h", "resnet.hip", "resnet_bwd.hip"))
    c = {}
    # mla_linear_narrow: 16 rows per block, at most 2048 blocks, grid-stride over the rest
    cap = _one(r"const unsigned grid = unsigned\(\(M \+ 15\) / 16 < (\d+) \? \(M \+ 15\) / 16 : (\d+)\);", head, "mla_linear_narrow's grid")
    assert cap[0] == cap[1]
    _one(r"for \(int64_t m = int64_t\(blockIdx\.x\) \* 16 \+ grp; m < M; m \+= int64_t\(gridDim\.x\) \* 16\) \{", head, "linear_narrow_kernel's row loop")
    _one(r"for \(int kk = l; kk < k4; kk \+= 16\) \{", head, "linear_narrow_kernel's K loop")
    c["narrow_blocks"], c["narrow_rows"] = int(cap[0]), 16
    insts = [int(v) for v in re.findall(r"MLA_NARROW_CASE\((\d+)\)", head)]
    assert insts == list(range(1, 17)), "the narrow instantiations are not in the form this test reads"
    # mla_linear_small: the form switch and the wide kernel's grid cap
    sw = _one(r"if \(N % 4 == 0 && N >= (\d+) && K <= (\d+) && N \* K \* 4 <= (\d+) \* 1024 && ldo % 4 == 0 && mla::aligned\(out, 16\) && M \* N >= \(1 << (\d+)\)\) \{",
              head, "mla_linear_small's form switch")
    c["small_min_n"], c["small_max_k"], c["small_lds"], c["small_min_out"] = int(sw[0]), int(sw[1]), int(sw[2]) * 1024, 1 << int(sw[3])
    _one(r"const int64_t blocks = \(M \* \(N / 4\) \+ 255\) / 256;", head, "the wide kernel's block count")
    cap = _one(r"hipLaunchKernelGGL\(linear_small_wide_kernel, dim3\(unsigned\(blocks < (\d+) \? blocks : (\d+)\)\), dim3\(256\)", head, "the wide kernel's grid cap")
    assert cap[0] == cap[1]
    c["small_wide_blocks"] = int(cap[0])
    # mla_col_sum / mla_col_sum_bf16: rows per chunk and the chunk cap
    f = _one(r"const int chunks = int\(rows / (\d+) < 1 \? 1 : \(rows / (\d+) > (\d+) \? (\d+) : rows / (\d+)\)\);\s+// <= 64: the workspace", train, "mla_col_sum's chunks")
    b = _one(r"const int chunks = int\(rows / (\d+) < 1 \? 1 : \(rows / (\d+) > (\d+) \? (\d+) : rows / (\d+)\)\);\n", train, "mla_col_sum_bf16's chunks")
    for g in (f, b):
        assert g[0] == g[1] == g[4] and g[2] == g[3], g
    assert f[2] == b[2]
    c["colsum_rows"], c["colsum_chunks"] = {F32: int(f[0]), BF16: int(b[0])}, int(f[2])
    _one(r"if \(cols % 4 == 0 && ldx % 4 == 0 && mla::aligned\(x, 16\)\) \{          // 16-byte loads", train, "mla_col_sum's vector form")
    assert len(re.findall(r"const int64_t per = \(rows \+ gridDim\.y - 1\) / gridDim\.y;", train)) == 2, "the colsum kernels' rows per chunk"
    # the head's BatchNorm statistics up to 64 channels
    c["stat_blocks"] = int(_one(r"constexpr int kStatBlocks = (\d+);", head, "kStatBlocks"))
    c["max_channels"] = int(_one(r"constexpr int kMaxChannels = (\d+);", head, "kMaxChannels"))
    c["fused_channels"] = int(_one(r"if \(finish && channels <= (\d+)\) \{", head, "the one-launch finish"))
    _one(r"blocks = int\(groups < kStatBlocks \? groups : kStatBlocks\);", head, "sums_rows_kernel's grid")
    _one(r"const int64_t per_block = \(\(rows \+ gridDim\.x - 1\) / gridDim\.x \+ period - 1\) / period \* period;", head, "sums_rows_kernel's rows per block")
    _one(r"blocks = int\(\(rows \+ 63\) / 64 < kStatBlocks \? \(rows \+ 63\) / 64 : kStatBlocks\);", head, "sums_cols_kernel's grid")
    _one(r"\} else if \(cols <= kMaxChannels\) \{", head, "the narrow column mode")
    # the stem: normalisation constants, geometry, rows per block of the weight gradient
    n = _one(r"constexpr float kNormMean\[3\] = \{([\d.]+)f, ([\d.]+)f, ([\d.]+)f\}, kNormInv\[3\] = \{1\.f / ([\d.]+)f, 1\.f / ([\d.]+)f, 1\.f / ([\d.]+)f\};",
             core, "kNormMean / kNormInv")
    c["norm_mean"] = [float(np.float32(v)) for v in n[:3]]
    c["norm_inv"] = [float(np.float32(1.0) / np.float32(v)) for v in n[3:]]
    c["norm_std_text"] = [float(v) for v in n[3:]]
    c["img"], c["stem_out"] = int(_one(r"kImg = (\d+),", core, "kImg")), int(_one(r"kStemOut = (\d+),", core, "kStemOut"))
    _one(r"const int64_t n = blockIdx\.x / kStemOut;", fwd, "rn_stem_kernel's image index")
    _one(r"for \(int ox = pg; ox < kStemOut; ox \+= 4\) \{\n        float acc = poison;", fwd, "rn_stem_kernel's column loop")
    sadd, sdiv = _one(r"int64_t stem_rows_per_block\(int64_t rows\) \{ return \(rows \+ (\d+)\) / (\d+); \}", bwd, "stem_rows_per_block()")
    assert int(sadd) == int(sdiv) - 1
    c["stem_blocks"] = int(sdiv)
    return c


C = _constants()
NORM_MEAN, NORM_INV = C["norm_mean"], C["norm_inv"]
IMG, STEM_OUT = C["img"], C["stem_out"]


def name(dtype):
    return "f32" if dtype == F32 else "bf16"


# ---------------------------------------------------------------------------------------- 1. rn_stem forward ----

STEM_NS = (1, 3)
STEM_CONFS = ("repeat", "single")
STEM_P = 55


def stem_normalize(planes, conf):
    """tests/resnet50_restated.py normalize_input for (n, 224, 224) planes in float64, with the constants THE KERNEL uses: the f32
    kNormMean[c] and kNormInv[c] = f32(1.f / std_c) (a product where the restatement divides by the double std_c). 'repeat': every
    channel carries x; 'single': channel 0 carries x, channels 1 and 2 carry zeros. -> (n, 3, 224, 224)."""
    x = planes.double()
    zero = torch.zeros_like(x)
    return torch.stack([((x if c == 0 or conf == "repeat" else zero) - NORM_MEAN[c]) * NORM_INV[c] for c in range(3)], dim=1)


def stem_magnitudes(planes, conf):
    """The magnitudes of the two terms of every normalised channel, |x| inv_c [c carries x] + mean_c inv_c, inside the image."""
    x = planes.double().abs()
    zero = torch.zeros_like(x)
    return torch.stack([((x if c == 0 or conf == "repeat" else zero) + NORM_MEAN[c]) * NORM_INV[c] for c in range(3)], dim=1)


def stem_reference(planes, w, conf):
    """float64 conv1 (7 x 7, stride 2, zero padding 3 OF THE NORMALISED CHANNELS) NHWC, and sum|terms| per output:
    sum over the taps inside the image and the channels of |w_c| (|x| inv_c [c carries x] + mean_c inv_c). Where the three weights of a
    tap share their sign this is sum_k |a_k x_k| + |b_k| with the kernel's a_k = sum_c w_c inv_c, b_k = -sum_c w_c mean_c inv_c; where
    they do not, |a_k| and |b_k| are smaller than what their own three-term sums round against, and this is the sum that bounds."""
    dev = K.ref_device()
    w64 = w.double().to(dev)
    acc = F.conv2d(stem_normalize(planes, conf).to(dev), w64, stride=2, padding=3)
    terms = F.conv2d(stem_magnitudes(planes, conf).to(dev), w64.abs(), stride=2, padding=3)
    return acc.permute(0, 2, 3, 1).contiguous().cpu(), terms.permute(0, 2, 3, 1).contiguous().cpu()


def stem_literal_terms(planes, w, conf):
    """sum over the taps inside the image of |a_k x_k| + |b_k| with a_k, b_k formed in float64 as rn_stem_kernel forms them."""
    w64 = w.double()
    inv, mean = torch.tensor(NORM_INV, dtype=torch.float64).view(1, 3, 1, 1), torch.tensor(NORM_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    a = (w64[:, :1] * inv[:, :1]) if conf == "single" else (w64 * inv).sum(dim=1, keepdim=True)
    b = (w64 * mean * inv).sum(dim=1, keepdim=True)
    x = planes.double().abs().unsqueeze(1)
    t = F.conv2d(x, a.abs(), stride=2, padding=3) + F.conv2d(torch.ones_like(x), b.abs(), stride=2, padding=3)
    return t.permute(0, 2, 3, 1).contiguous()


def stem_bound(acc, terms, scale, shift, relu, dtype):
    """The expected output and its bound. P = STEM_P = 55 f32 roundings on sum|terms|, counted in rn_stem_kernel whichever way the
    compiler contracts multiply-adds:
       5  a[k] = w0 i0 + w1 i1 + w2 i2: three products, two additions, each against at most sum_c |w_c| inv_c (b[k]: two products
          per channel and two additions, at most 4 against sum_c |w_c| mean_c inv_c; 'single': one product for a[k]);
       2  a[k] * xs + b[k]: the product, and the addition of b[k];
      48  acc += term, 49 taps from acc = +0: every partial sum is at most sum|terms|.
    Epilogue acc * scale + shift: the bound of acc times |scale|, and 2 roundings on |acc scale| + |shift| (acc within its bound).
    ReLU is 1-Lipschitz. bf16: half an ulp of the stored value."""
    ref, b = acc, STEM_P * U * terms
    if scale is not None:
        s, h = scale.double(), shift.double()
        ref, b = acc * s + h, b * s.abs() + 2 * U * ((acc.abs() + b) * s.abs() + h.abs())
    if relu:
        ref = ref.clamp_min(0)
    if dtype == BF16:
        b = b + K.half_ulp_bf16(ref, b)
    return ref, b


@functools.lru_cache(maxsize=None)
def stem_case(conf, n):
    """n different planes in [0, 1); rows and columns 0..2 and 221..223 carry planted values of a few units (so the taps that fall
    outside the image would matter if they counted), which raise sum|terms| of the outputs that see them and of no other. The three
    channel weights of a tap share a random sign (magnitudes 0.01 .. 0.11 differ per channel): sum|terms| is then exactly the
    sum_k |a_k x_k| + |b_k| of the kernel's coefficients. Scales of both signs, shifts ~ N(0, 1)."""
    gen = torch.Generator().manual_seed(300 + n)
    planes = torch.rand(n, IMG, IMG, generator=gen)
    planes[:, :3, :] += 2.0
    planes[:, -3:, :] -= 1.5
    planes[:, :, :3] += 1.25
    planes[:, :, -3:] += 3.0
    sign = torch.randint(0, 2, (64, 1, 7, 7), generator=gen).float() * 2 - 1
    w = sign * (torch.rand(64, 3, 7, 7, generator=gen) * 0.1 + 0.01)
    scale, shift = torch.rand(64, generator=gen) + 0.5, torch.randn(64, generator=gen)
    scale[::5] *= -1.0
    acc, terms = stem_reference(planes, w, conf)
    return dict(planes=planes, w=w, scale=scale, shift=shift, acc=acc, terms=terms)


# ------------------------------------------------------------------------------------------ 2. rn_stem_wgrad ----

WGRAD_NS = (1, 10, 19)


def wgrad_rows_per_block(n):
    return -(-n * STEM_OUT // C["stem_blocks"])


def wgrad_p(n):
    """f32 roundings of one dw element against sum|terms| = inv_c ([c carries x] sum |dy x| + mean_c sum |dy|), counted in
    rn_stem_wgrad_partial_kernel and rn_stem_wgrad_finish_kernel. A thread adds the 28 columns ox = pg, pg + 4, ... of each of the
    block's rpb = stem_rows_per_block(112 n) output rows into s1[k] (a product and an addition per term; fused or not, the chain is
    28 rpb long and the product is one more) and s0[k]; the four column groups are added in LDS (3). The blocks' partials are added
    in double and inv_c (S1 - mean_c S0) is formed in double (2^-53 per operation: far below one unit here) and rounded once (1).
    The reference divides by the double std_c and subtracts the double mean_c where the kernel multiplies by the f32 kNormInv[c] and
    kNormMean[c]: 2^-24 relative each, 2 more units. P = 28 rpb + 1 + 3 + 1 + 2."""
    return 28 * wgrad_rows_per_block(n) + 7


@functools.lru_cache(maxsize=None)
def wgrad_case(conf, n):
    """test_resnet_kernels_gpu.stem_case (planes in [0, 1), dy ~ N(0, 1) rounded to bf16, float64 conv2d_weight of the normalised
    input) with sum|terms| per dw element: conv2d_weight of the magnitudes. The bf16 kernel rounds nothing else: dy is loaded as
    stored, x and the sums stay f32."""
    planes, dy, ref = RK.stem_case(conf, n)
    dev = K.ref_device()
    terms = conv2d_weight(stem_magnitudes(planes, conf).to(dev), (64, 3, 7, 7), RK.nchw(dy).abs().to(dev), stride=2, padding=3).cpu()
    return dict(planes=planes, dy=dy, ref=ref, terms=terms, bound=wgrad_p(n) * U * terms)


# -------------------------------------------------------------------------------------- 3. mla_linear_narrow ----

NARROW_NS = tuple(range(1, 17))
NARROW_KS = (4, 8, 64, 68, 600)                  # k4 = 1: lane 0 alone; 2; 16: one piece per lane; 17: lane 0's second trip; 150: ragged
NARROW_MS = (1, 17)                              # one group; a second block with a single row
NARROW_BIG = (C["narrow_blocks"] * C["narrow_rows"] + 5, 10, 600)      # rows of a second grid-stride trip, the last group partial


def narrow_grid(M):
    return min(-(-M // C["narrow_rows"]), C["narrow_blocks"])


def linear_case(M, N, Kk, device="cpu"):
    """Dyadic a (M, K), w (N, K), bias (N), the float64 a w^T with and without the bias; asserts the 2^24 condition."""
    a, w, b = K.gemm_operands(7000 + 31 * M + 17 * N + Kk, M, N, Kk, device=device)
    y, y_abs = K.gemm_reference(a, w, b)
    K.assert_exact_arithmetic(y_abs)
    return dict(a=a, w=w, b=b, y=y, y_nobias=K.gemm_reference(a, w, None)[0])


# --------------------------------------------------------------------------------------- 4. mla_linear_small ----

def small_form(M, N, Kk, ldo, out_offset):
    """Which kernel mla_linear_small launches; out_offset: floats between a 16-byte boundary and out."""
    wide = (N % 4 == 0 and N >= C["small_min_n"] and Kk <= C["small_max_k"] and N * Kk * 4 <= C["small_lds"] and ldo % 4 == 0
            and out_offset % 4 == 0 and M * N >= C["small_min_out"])
    return "wide" if wide else "plain"


# id -> (M, N, K, ldo - N, floats `out` is offset by, the form entered). Each term of the switch stands on either side of a pair.
SMALL_CASES = {
    "wide-66000-outputs": (110, 600, 10, 0, 0, "wide"),
    "plain-65400-outputs": (109, 600, 10, 0, 0, "plain"),           # M N < 65536
    "plain-n602": (110, 602, 10, 2, 0, "plain"),                    # N % 4 != 0 (ldo = 604)
    "plain-n60": (1100, 60, 10, 0, 0, "plain"),                     # N < 64
    "wide-n64-k64": (1024, 64, 64, 0, 0, "wide"),                   # N = 64, K = 64, M N = 65536: every bound met with equality
    "plain-n64-k65": (1024, 64, 65, 0, 0, "plain"),                 # K > 64
    "plain-n64-65472-outputs": (1023, 64, 64, 0, 0, "plain"),
    "wide-n192-k64": (342, 192, 64, 0, 0, "wide"),                  # N K 4 = 48 KiB exactly
    "plain-n192-k65": (342, 192, 65, 0, 0, "plain"),
    "plain-n196-k64": (342, 196, 64, 0, 0, "plain"),                # N K 4 > 48 KiB with K <= 64
    "plain-ldo-n+2": (110, 600, 10, 2, 0, "plain"),                 # ldo % 4 != 0
    "wide-ldo-n+4": (110, 600, 10, 4, 0, "wide"),                   # a pitched out the wide form accepts
    "plain-out-offset": (110, 600, 10, 4, 1, "plain"),              # out four bytes past a 16-byte boundary
    "wide-second-trip": (1750, 600, 10, 0, 0, "wide"),              # M 150 quads > 1024 x 256 threads
    "tiny-1x1x1": (1, 1, 1, 0, 0, "plain"),
    "tiny-3x7x5": (3, 7, 5, 3, 1, "plain"),
}


# ----------------------------------------------------------------------- 5. mla_col_sum, mla_col_sum_bf16 ----

COLSUM_ROWS = {F32: (1, 63, 64, 127, 129, 4096, 4097, 5120), BF16: (1, 255, 256, 513, 16384, 16385)}
COLSUM_COLS = (1, 10, 64, 65, 256, 260, 600, 601)
COLSUM_FORMS = {F32: ("dense", "pitched", "offset"), BF16: ("dense", "pitched")}


def colsum_chunks(rows, dtype):
    """(chunks, rows per chunk, rows of the last chunk) of mla_col_sum (f32) / mla_col_sum_bf16."""
    chunks = min(max(rows // C["colsum_rows"][dtype], 1), C["colsum_chunks"])
    per = -(-rows // chunks)
    return chunks, per, rows - (chunks - 1) * per


def colsum_layout(form, cols):
    """(floats in front of the matrix, floats behind each row) of a form. dense: none. pitched: the base stays 16-byte aligned and
    the pitch is no multiple of 4 floats. offset: the base is one float past a 16-byte boundary and the pitch is a multiple of 4."""
    if form == "dense":
        return 0, 0
    if form == "pitched":
        return 0, 1 if (cols + 1) % 4 else 2
    return 1, 3 - cols % 4


def colsum_vector_form(form, cols):
    """Whether mla_col_sum takes colsum_partial4_kernel (16-byte loads)."""
    left, right = colsum_layout(form, cols)
    return cols % 4 == 0 and (cols + left + right) % 4 == 0 and left % 4 == 0


@functools.lru_cache(maxsize=None)
def colsum_case(rows, cols):
    """Dyadic values (exact in bf16) and their float64 column sums; |sum| <= rows in units of 2^-3: an f32 value."""
    x = dyadic(torch.Generator().manual_seed(5000 + 7 * rows + cols), (rows, cols))
    K.assert_exact_arithmetic(x.double().abs().sum(dim=0), unit=2.0 ** -3)
    return x, x.double().sum(dim=0)


# -------------------------------------------------- 6. mla_bn_stats / mla_bn_stats_fused, 1..64 channels ----

STATS_PERIODS = (1, 10, 16, 17, 64)
STATS_GROUPS = (1, 3, C["stat_blocks"], 2 * C["stat_blocks"] + 1)
STATS_COLS0 = (1, 4, 600, 601)
STATS_COLS1 = (1, 10, 16, 17, 64)
STATS_ROWS1 = (1, 63, 65, 64 * C["stat_blocks"] + 1)
STATS_MAX_BYTES = 32 << 20                       # the eight largest mode-0 combinations (39 .. 158 MB) are left out
MOMENTUM = 0.1
CONSTANT = 0.375                                 # the constant channel's value: sums, mean and mean^2 are exact in double


def stats_mode0_cases(period):
    return [(period * g, c) for g in STATS_GROUPS for c in STATS_COLS0 if period * g * c * 4 <= STATS_MAX_BYTES]


def stats_blocks(mode, rows, period):
    """(blocks launched, rows per block, blocks that own at least one row) of sums_rows_kernel / sums_cols_kernel."""
    if mode == 0:
        blocks = min(rows // period, C["stat_blocks"])
        per = -(-(-(-rows // blocks)) // period) * period
    else:
        blocks = min(-(-rows // 64), C["stat_blocks"])
        per = -(-rows // blocks)
    return blocks, per, -(-rows // per)


def stats_layouts(cols):
    """(left, right) floats around each row: dense; one float in front and two behind (misaligned base and pitch: never 16-byte
    loads); for a multiple of 4 columns also four floats behind an aligned base (a pitch that keeps the 16-byte loads)."""
    return [(0, 0), (1, 2)] + ([(0, 4)] if cols % 4 == 0 else [])


def stats_vec_ok(cols, left, right):
    return cols % 4 == 0 and (cols + left + right) % 4 == 0 and left % 4 == 0


def stats_channels(mode, period, cols):
    return period if mode == 0 else cols


def stats_columns(x, mode, period):
    """(rows, cols) -> (count, channels): the elements of every channel down a column."""
    rows, cols = x.shape
    return x.reshape(rows // period, period, cols).permute(0, 2, 1).reshape(-1, period) if mode == 0 else x


def stats_input(rows, cols, mode, period):
    """Uniform values in [-1, 3); with more than one channel, channel channels // 2 is the constant 0.375. Running statistics away
    from their initial values."""
    ch = stats_channels(mode, period, cols)
    gen = torch.Generator().manual_seed(9000 + 13 * rows + 7 * cols + mode)
    x = torch.rand(rows, cols, generator=gen) * 4 - 1
    const = ch // 2 if ch > 1 else None
    if const is not None:
        if mode == 0:
            x[const::period] = CONSTANT
        else:
            x[:, const] = CONSTANT
    return x, torch.rand(ch, generator=gen) - 0.5, torch.rand(ch, generator=gen) * 1.5 + 0.5, const


def stats_reference(x, rm0, rv0, mode, period):
    """test_wide_head_gpu._stats_reference on the channels as columns (one f32 rounding of the double mean, of the double variance
    and of the double running update), plus what the double sums themselves may be off by at this count. Every summation chain of
    sums_rows_kernel / sums_cols_kernel / the partial reduction is shorter than `count` elements (a single element: no addition), so
    sum x is within count 2^-53 sum|x| and sum x^2 within count 2^-53 sum x^2; m = s / count adds one rounding, m m one, ss / count
    one, the subtraction one, and the error of m enters m^2 as 2 |m| (|m| <= mean|x|, and mean|x|^2 <= mean x^2 = mean^2 + var):
       mean  (count + 1) 2^-53 mean|x|
       var   (3 count + 5) 2^-53 (mean^2 + var).
    The running statistics take momentum x that (x count / (count - 1) for the unbiased variance)."""
    dev = K.ref_device()
    xc = stats_columns(x, mode, period).to(dev)
    count = xc.shape[0]
    ref = WH._stats_reference(xc, rm0.to(dev), rv0.to(dev), MOMENTUM)
    x64 = xc.double()
    e_mean = (count + 1) * D * x64.abs().mean(0)
    e_var = (3 * count + 5) * D * (ref["mean"] ** 2 + ref["var"])
    unb = count / (count - 1) if count > 1 else 1.0
    ref["b_mean"], ref["b_var"] = ref["b_mean"] + e_mean, ref["b_var"] + e_var
    ref["b_run_mean"], ref["b_run_var"] = ref["b_run_mean"] + MOMENTUM * e_mean, ref["b_run_var"] + MOMENTUM * unb * e_var
    ref = {k: v.cpu() for k, v in ref.items()}
    ref["count"] = count
    return ref
