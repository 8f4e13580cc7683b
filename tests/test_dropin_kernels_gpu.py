"""GPU tests of the stand-alone kernels of csrc/stft_generic.hip, which only whole-pipeline or norm-wise figures at one or two
configurations held: stft_kernel, mel_log_kernel, dataset_frames_kernel, postprocess_kernel, mono_mix_kernel and resample_kernel. ONE
KERNEL per check, through the wrapper the drop-in modules use and through the C entry into a buffer with a sentinel block behind it
(the wrappers allocate their own result, so the two calls must give the same bits), against float64 numpy computed from the same
stored operands; every output element is compared.

Kinds of checks (cases, references, bounds, restatements and the constants READ FROM THE SOURCE: tests/dropin_kernel_cases.py, evaluated
without a device by tests/test_dropin_kernel_cases_cpu.py):
  exact     a gather (dataset_frames), a double-precision mean rounded once (mono_mix), dyadic operands whose every partial sum is an f32
            value (mel_log's v, postprocess): equality of the bits;
  derived   |got - ref| <= P 2^-24 sum|terms| per element (stft: P = 5 log2(fft) + 4, counted in dropin_kernel_cases.stft_p; mel_log on
            uniform data; resample: the one rounding of a double accumulator); each prints its worst error / bound before asserting;
  yardstick stft on noise: per frame ||got - ref|| / ||ref|| <= 2 R, R the same figure of the plain f32 restatement fft_f32();
  measured  the device's logf alone: table MEASURED, by the rule of tests/test_train_kernels_gpu.py."""

import ctypes
import importlib

import numpy as np
import pytest
import torch

import dropin_kernel_cases as P
from conftest import PKG

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
SENTINEL = -7.0                          # fills whatever a kernel must not write
GUARD = 64                               # floats of it behind every output
NAN = float("nan")

# The accuracy of the device's logf is stated nowhere this test can read, so it is measured: name -> (worst relative error against
# float64 log on the MI355X over the test's whole parametrization, bound). The rule is bound = 4 x the measured value, never above
# 4 . 2^-24 (two f32 units in the last place at the low end of a binade). The worst figure, 1.78e-7 at (5, 257, 65), is 1.5 such
# units -- a result one unit from the correctly rounded one --, so 4 x it is 7.1e-7 and the cap, 2.38e-7, is the bound in force.
MEASURED = {
    "logf": (1.78e-7, min(4 * 1.78e-7, P.LOGF_CAP)),
}
assert all(b <= P.LOGF_CAP for _, b in MEASURED.values())


@pytest.fixture(scope="module")
def L():
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def fe():
    return importlib.import_module(PKG + ".frontend")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded(shape):
    """A contiguous view of `shape` in front of GUARD sentinels, all of it filled with the sentinel; (flat, view)."""
    n = int(np.prod(shape))
    flat = torch.full((n + GUARD,), SENTINEL, device="cuda")
    return flat, flat[:n].view(*shape)


def assert_guard(flat, n, what):
    assert bool((flat[n:] == SENTINEL).all()), what + ": wrote behind its output"


def fenced(a, fill=NAN):
    """The array on the device between two blocks of `fill`."""
    t = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    buf = torch.full((t.numel() + 2 * GUARD,), fill, dtype=t.dtype).cuda()
    buf[GUARD:GUARD + t.numel()] = t.cuda()
    return buf, buf[GUARD:GUARD + t.numel()].view(*a.shape)


def assert_fence(buf, n, what):
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), what + ": an input's fence changed"


def within(got, ref, bound, what):
    """Per-element bound on numpy arrays; an element whose bound is 0 must be equal. Prints the worst ratio before asserting."""
    err = np.abs(got.astype(np.float64) - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    print("%s: worst |error| / bound = %.3g" % (what, worst))
    assert worst <= 1.0, (what, worst)


# -------------------------------------------------------------------------------------------- 1. stft_kernel ----

def stft_direct(L, cfg, x, frames):
    """mla_stft_magnitude into a guarded buffer, the signal between NaN fences, with the operands the wrapper uploads."""
    fft, win, hop = cfg
    bins = fft // 2 + 1
    buf, sig = fenced(x)
    flat, out = guarded((frames, bins))
    window, tw = dev(P.stft_window(win)), dev(P.stft_twiddle(fft))
    L.check(L.lib().mla_stft_magnitude(vp(sig.data_ptr()), x.shape[0], vp(window.data_ptr()), vp(tw.data_ptr()), win, hop, fft,
                                       vp(out.data_ptr()), L.stream_ptr()))
    torch.cuda.synchronize()
    assert_guard(flat, frames * bins, "stft")
    assert_fence(buf, x.shape[0], "stft")
    return flat, out


@pytest.mark.parametrize("cfg", P.STFT_CONFIGS, ids=P.stft_id)
def test_stft_every_bin_within_its_derived_bound(L, fe, cfg):
    """frontend.stft_magnitude at one configuration: lengths of one frame (n == win and n == win + hop - 1), two frames and 3..5;
    noise, two impulses per frame (one at sample 0 of the first frame, one at win - 1 of the last), a constant and a cosine on bin
    fft / 4. Every bin of every input within P 2^-24 S of abs(rfft) in float64 on the stored operands, S = sum |x w| of its frame and
    P = 5 log2(fft) + 4 (dropin_kernel_cases.stft_p) -- for an impulse that is a few 1e-6 of the bin, where a wrong bit reversal,
    twiddle index or bin costs O(1). Noise, where S is about win / 4: per frame ||got - ref|| / ||ref|| <= 2 R with R the largest such
    figure of the plain f32 restatement over the configuration's noise signals (the factor 2 for the roundings fma contraction moves).
    The C entry into a sentinel-guarded buffer, the signal between NaN fences, gives the wrapper's bits."""
    fft, win, hop = cfg
    case = P.stft_case(cfg)
    worst, worst_e = 0.0, 0.0
    for (n, kind), it in case["items"].items():
        frames = P.stft_frames(n, win, hop)
        got_t = fe.stft_magnitude(it["x"], fft, hop, win)
        assert got_t.dtype == torch.float32 and tuple(got_t.shape) == (frames, fft // 2 + 1)
        got = got_t.cpu().numpy()
        assert torch.equal(stft_direct(L, cfg, it["x"], frames)[1], got_t), (n, kind)
        r = P.stft_worst_ratio(got, it["ref"], it["s"], fft)
        if r > 1.0:
            print("stft %s n %d %s: worst |error| / (P 2^-24 S) = %.3g" % (P.stft_id(cfg), n, kind, r))
        worst = max(worst, r)
        if kind == "noise":
            e = P.stft_frame_errors(got, it["ref"])
            worst_e = max(worst_e, float(e.max()))
    print("stft %s: worst |error| / (P 2^-24 S) = %.3g (P = %d); noise: worst e = %.3g, R = %.3g, e / 2R = %.3g"
          % (P.stft_id(cfg), worst, P.stft_p(fft), worst_e, case["R"], worst_e / (2 * case["R"]) if case["R"] else 0.0))
    assert worst <= 1.0
    assert worst_e <= 2 * case["R"]


@pytest.mark.parametrize("cfg", [(2, 1, 1), (64, 10, 37), (512, 400, 160), (4096, 4096, 4096)], ids=P.stft_id)
def test_stft_without_a_whole_frame_writes_nothing(L, fe, cfg):
    """n == win - 1: the wrapper returns shape (0, bins), and the C entry returns OK and leaves `out` untouched."""
    fft, win, hop = cfg
    x = np.full(max(win - 1, 0), 0.5, dtype=np.float32)
    got = fe.stft_magnitude(x, fft, hop, win)
    assert tuple(got.shape) == (0, fft // 2 + 1)
    flat, out = guarded((1, fft // 2 + 1))
    sig, window, tw = dev(np.full(max(win - 1, 1), 0.5, dtype=np.float32)), dev(P.stft_window(win)), dev(P.stft_twiddle(fft))
    L.check(L.lib().mla_stft_magnitude(vp(sig.data_ptr()), win - 1, vp(window.data_ptr()), vp(tw.data_ptr()), win, hop, fft, vp(out.data_ptr()),
                                       L.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((flat == SENTINEL).all())


# ----------------------------------------------------------------------------------------- 2. mel_log_kernel ----

def mel_log(L, spec, mel, offset):
    """mla_mel_log on its own operands between NaN fences, into a guarded buffer."""
    frames, bins = spec.shape
    bands = mel.shape[1]
    sbuf, s = fenced(spec)
    mbuf, m = fenced(mel)
    flat, out = guarded((frames, bands))
    L.check(L.lib().mla_mel_log(vp(s.data_ptr()), vp(m.data_ptr()), frames, bins, bands, float(offset), vp(out.data_ptr()), L.stream_ptr()))
    torch.cuda.synchronize()
    assert_guard(flat, frames * bands, "mel_log")
    assert_fence(sbuf, spec.size, "mel_log spec")
    assert_fence(mbuf, mel.size, "mel_log mel")
    return out.cpu().numpy()


def logf_error(got, ref):
    """Worst relative error of the finite results, the exact zeros excluded (they are asserted exactly)."""
    m = np.isfinite(ref) & (ref != 0.0)
    return float((np.abs(got[m].astype(np.float64) - ref[m]) / np.abs(ref[m])).max()) if m.any() else 0.0


@pytest.mark.parametrize("offset", P.MEL_OFFSETS)
@pytest.mark.parametrize("shape", P.MEL_SHAPES, ids=P.mel_id)
def test_mel_log_on_the_grid(L, shape, offset):
    """mla_mel_log on grid data (spec multiples of 2^-3 in [0, 4], mel multiples of 2^-3 in [0, 1], offset 0, 2^-6 or 1): acc + offset
    is an exact f32 value in any order (asserted by the case from its reference), so the kernel's logf argument IS the reference's v.
    -inf at exactly the reference's positions (the silent frame and the empty band at offset 0), exactly 0.0 where v == 1, and the
    finite rest within MEASURED["logf"] relative of float64 log(v) (every |log v| there is at least 2^-6)."""
    c = P.mel_grid_case(shape, offset)
    got = mel_log(L, c["spec"], c["mel"], offset)
    ref = c["ref"]
    finite = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), finite) and bool((got[~finite] == -np.inf).all()), "-inf is not where the reference has it"
    assert np.array_equal(got == 0.0, c["v"] == 1.0) and got[c["one"]] == 0.0, "log(1) is not exactly 0"
    err = logf_error(got, ref)
    print("logf %s offset %g: worst relative error %.3g (recorded %s, bound %.3g)" % (P.mel_id(shape), offset, err, MEASURED["logf"][0], MEASURED["logf"][1]))
    assert err <= MEASURED["logf"][1]


def test_mel_log_without_frames_writes_nothing(L):
    flat, out = guarded((1, 20))
    spec, mel = dev(np.ones((1, 129), dtype=np.float32)), dev(np.ones((129, 20), dtype=np.float32))
    L.check(L.lib().mla_mel_log(vp(spec.data_ptr()), vp(mel.data_ptr()), 0, 129, 20, 0.01, vp(out.data_ptr()), L.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((flat == SENTINEL).all())


@pytest.mark.parametrize("cid", list(P.MEL_UNIFORM))
def test_mel_log_on_uniform_data(L, cid):
    """spec uniform in [0, 30) against the real 16 kHz (257 x 64) and 8 kHz (129 x 20) matrices, offsets 0.01 and 0: the log within
    (bins + 1) 2^-24 sum|terms| / (acc + offset) plus the logf term MEASURED["logf"] |ref|; -inf where the reference has it."""
    c = P.mel_uniform_case(cid)
    got = mel_log(L, c["spec"], c["mel"], c["offset"])
    finite = np.isfinite(c["ref"])
    assert np.array_equal(np.isfinite(got), finite) and bool((got[~finite] == -np.inf).all())
    bound = c["bound"] + MEASURED["logf"][1] * np.abs(np.where(finite, c["ref"], 0.0))
    within(got[finite], c["ref"][finite], bound[finite], "mel_log uniform " + cid)


# ---------------------------------------------------------------------------------- 3. dataset_frames_kernel ----

@pytest.mark.parametrize("case", P.frames_cases(), ids=P.frames_id)
def test_dataset_frames_is_the_gather(L, case):
    """mla_dataset_frames against the numpy restatement of the index rule, torch.equal: distinct example values 1, 2, 3, ..., exactly
    0.0 in the slots at or above ex_per_clip (ex_per_clip == 0: a null `examples` and all zeros), NaN fences around `examples`,
    sentinels behind `out`. 35 clips at (10, 96, 32) are 2 150 400 outputs, past the 8192 x 256 lanes of one trip."""
    clips, ex, geo = case
    n_frames, frame_len, stride = geo
    e = P.frames_examples(clips, ex)
    want = P.frames_restated(e, clips, ex, geo)
    buf, src = fenced(e) if ex else (None, None)
    flat, out = guarded(want.shape)
    L.check(L.lib().mla_dataset_frames(vp(src.data_ptr()) if ex else None, clips, ex, n_frames, frame_len, stride, vp(out.data_ptr()), L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), torch.from_numpy(want)), P.frames_id(case)
    assert_guard(flat, want.size, "dataset_frames")
    if ex:
        assert_fence(buf, e.size, "dataset_frames")
    else:
        assert not bool(out.any())


# ------------------------------------------------------------------------------------- 4. postprocess_kernel ----

@pytest.fixture(scope="module")
def vggish():
    return importlib.import_module(PKG + ".torchvggish.vggish")


def postprocessor(vggish, E, mu):
    pp = vggish.Postprocessor().cuda()
    with torch.no_grad():
        pp.pca_eigen_vectors.copy_(torch.from_numpy(E))
        pp.pca_means.copy_(torch.from_numpy(mu).reshape(128, 1))
    return pp


def post_direct(L, x, E, mu):
    """mla_postprocess with every input between NaN fences, into a guarded buffer."""
    xb, xd = fenced(x)
    eb, ed = fenced(E)
    mb, md = fenced(mu)
    flat, out = guarded(x.shape)
    L.check(L.lib().mla_postprocess(vp(xd.data_ptr()), vp(ed.data_ptr()), vp(md.data_ptr()), x.shape[0], vp(out.data_ptr()), L.stream_ptr()))
    torch.cuda.synchronize()
    assert_guard(flat, x.size, "postprocess")
    for b, n in ((xb, x.size), (eb, E.size), (mb, mu.size)):
        assert_fence(b, n, "postprocess")
    return out


@pytest.mark.parametrize("rows", P.POST_ROWS)
def test_postprocess_on_the_grid_is_rint_of_float64(L, vggish, rows):
    """vggish.Postprocessor on grid data (E integers -8..8 over 64, x and mu multiples of 2^-4, x - mu in [-2, 2]): every step is an
    exact f32 value (units of 2^-10, 20 bits after the scaling; asserted on the CPU, where an f32 emulation is bit-equal to float64),
    so the output must EQUAL rint of the float64 value. 1000 rows: over 90 % of the outputs strictly inside 1..254 and all 256 levels
    (asserted on the reference on the CPU), x == mu (all 128), acc exactly -2 and +2 and beyond them (the clamp), one-hot x - mu
    (E read column by column: the transposed matrix fails). One row: torch.squeeze returns a vector of 128. The grid's only exact
    ties are acc == 0, 127.5 -> 128 under round-half-even and round-half-up alike: it does not tell the two rules apart."""
    c = P.post_grid_case()
    x = P.post_rows(c, rows)
    want = c["q"][500:501] if rows == 1 else c["q"][:rows]
    got = postprocessor(vggish, c["E"], c["mu"])(dev(x))
    assert tuple(got.shape) == ((128,) if rows == 1 else (rows, 128)) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().reshape(rows, 128).astype(np.float64), want)
    assert torch.equal(post_direct(L, x, c["E"], c["mu"]).reshape(got.shape), got)


def test_postprocess_on_uniform_data_rounds_as_float64_away_from_ties(L, vggish):
    """Uniform E, x, mu scaled so that most outputs stay interior (asserted on the CPU): got == rint(v64) wherever v64 is farther from
    a rounding tie than the derived 63.75 . 130 . 2^-24 . sum|terms| of its element; nearer, either neighbour is accepted."""
    c = P.post_uniform_case()
    got = postprocessor(vggish, c["E"], c["mu"])(dev(c["x"])).cpu().numpy()
    ok = P.post_uniform_ok(got, c)
    print("postprocess uniform: %d of %d outputs differ from rint(v64), %d of them outside the tie window"
          % (int((got != c["q"]).sum()), got.size, int((~ok).sum())))
    assert bool(ok.all())
    assert torch.equal(post_direct(L, c["x"], c["E"], c["mu"]).cpu(), torch.from_numpy(got))


# --------------------------------------------------------------------------------------- 5. mono_mix_kernel ----

@pytest.mark.parametrize("pcm16", [True, False], ids=["int16", "float32"])
@pytest.mark.parametrize("channels", P.MIX_CHANNELS)
def test_mono_mix_is_the_double_mean_rounded_once(L, fe, channels, pcm16):
    """frontend.as_device_mono at 2, 3, 5, 8 channels and 1, 255, 256, 257, 70 001 frames, int16 (pcm16=True; -32768 and 32767
    planted) and float32: BIT-EQUAL to the float64 statement of resample_core.h -- the channels added one by one in double, divided
    by their count, times 2^-15 for int16, cast once. The C entry with NaN (int16: -1) fences around the frames and sentinels behind
    `out` gives the same bits."""
    for n in P.MIX_NS:
        a = P.mix_input(n, channels, pcm16)
        want = torch.from_numpy(P.mix_reference(a))
        got = fe.as_device_mono(a, pcm16=pcm16)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n,)
        assert torch.equal(got.cpu(), want), "mono_mix %d channels n %d" % (channels, n)
        t = torch.from_numpy(a).reshape(-1)
        buf = torch.full((t.numel() + 2 * GUARD,), -1 if pcm16 else NAN, dtype=t.dtype).cuda()
        buf[GUARD:GUARD + t.numel()] = t.cuda()
        flat, out = guarded((n,))
        L.check(L.lib().mla_mono_mix(vp(buf[GUARD:].data_ptr()), L.I16 if pcm16 else L.F32, n, channels, vp(out.data_ptr()), L.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want)
        assert_guard(flat, n, "mono_mix")


# ---------------------------------------------------------------------------------------- 6. resample_kernel ----

@pytest.mark.parametrize("case", P.RESAMPLE_CASES, ids=P.resample_id)
def test_resample_is_the_oracle_rounded_once(L, fe, case):
    """frontend.resample to 16 kHz against oracle/resample.py on the f32-rounded input: |got - ref| <= 2^-24 |ref| + 1e-10 max|x| --
    the one f32 rounding of the double accumulator, and the double-precision difference between the kernel's fused position and the
    oracle's t (1 / ratio) (a numpy restatement of the kernel differs from the oracle by at most 3.5e-13 at these lengths: CPU
    test). Noise, an impulse at sample 0 and one at n - 1; 256 kHz has table step 32 and 1024 taps per wing, (44100, 3) a single
    output, (48000, 63) both wings clipped by the signal for every output. The C entry with NaN fences around x and sentinels behind
    y gives the same bits."""
    sr, n = case
    for kind in P.RESAMPLE_KINDS:
        c = P.resample_case(case, kind)
        got = fe.resample(dev(c["x"]), sr, P.SR_OUT)
        assert got.dtype == torch.float32 and tuple(got.shape) == c["ref"].shape
        within(got.cpu().numpy(), c["ref"], c["bound"], "resample %s %s" % (P.resample_id(case), kind))
        win, delta, num_table = fe._resample_filter(float(P.SR_OUT) / float(sr))
        xb, xd = fenced(c["x"])
        flat, y = guarded(c["ref"].shape)
        wd, dd = dev(win), dev(delta)
        L.check(L.lib().mla_resample(vp(xd.data_ptr()), n, float(sr), float(P.SR_OUT), vp(wd.data_ptr()), vp(dd.data_ptr()), win.shape[0], num_table,
                                     vp(y.data_ptr()), c["ref"].shape[0], L.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(y, got)
        assert_guard(flat, c["ref"].shape[0], "resample")
        assert_fence(xb, n, "resample")


def test_resample_of_too_short_a_signal_raises_on_both_sides(fe):
    from oracle import resample as ors
    sr, n = P.RESAMPLE_SHORT
    with pytest.raises(ValueError):
        fe.resample(torch.zeros(n).cuda(), sr, P.SR_OUT)
    with pytest.raises(ValueError):
        ors.resample(np.zeros(n), sr, P.SR_OUT)
