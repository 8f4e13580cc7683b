"""CPU side of tests/test_dropin_kernels_gpu.py: the constants read from csrc/stft_generic.hip are the ones the shapes were chosen for,
every case evaluates without a device, the grids are exact, the share conditions hold on the references, and the numpy restatements of
the kernels' arithmetic stay within the bounds the GPU file asserts."""

import numpy as np
import pytest

import dropin_kernel_cases as P
from infer_kernel_cases import U
from oracle import dataset_frames as odf
from oracle import resample as ors

F32 = np.float32


def test_constants_read_from_the_source():
    C = P.C
    assert C["max_fft"] == 4096 and C["stft_lanes"] == C["mel_lanes"] == C["frames_lanes"] == 256
    assert (C["frames_blocks"], C["frames_columns"], C["frames_slots"]) == (8192, 384, 4)


# ------------------------------------------------------------------------------------------------------ stft ----

def test_stft_configurations_cover_the_branches():
    ffts = {c[0] for c in P.STFT_CONFIGS}
    assert ffts == {1 << p for p in range(1, 13)} and max(ffts) == P.C["max_fft"]
    for p in range(1, 13):
        assert any(c[0] == 1 << p and c[1] < c[0] for c in P.STFT_CONFIGS)
    for named in ((2, 2, 1), (2, 1, 1), (4, 3, 2), (8, 8, 3), (256, 200, 80), (512, 400, 160), (1024, 1000, 999), (4096, 4096, 4096), (4096, 2500, 1000),
                  (64, 10, 37)):
        assert named in P.STFT_CONFIGS
    # the lane loops take one trip below 256 butterflies / points and several above; both sides occur
    assert any(c[0] // 2 < P.C["stft_lanes"] for c in P.STFT_CONFIGS) and any(c[0] // 2 > P.C["stft_lanes"] for c in P.STFT_CONFIGS)
    assert any(c[1] == 1 for c in P.STFT_CONFIGS) and any(c[2] > c[1] for c in P.STFT_CONFIGS) and any(c[1] == c[0] for c in P.STFT_CONFIGS)
    for cfg in P.STFT_CONFIGS:
        fft, win, hop = cfg
        assert 1 <= win <= fft and hop >= 1
        a, b, c, d = P.stft_lengths(cfg)
        assert [P.stft_frames(n, win, hop) for n in (a, b, c)] == [1, 1, 2] and 3 <= P.stft_frames(d, win, hop) <= 5
        assert P.stft_frames(win - 1, win, hop) == 0
        assert P.stft_p(fft) == 5 * int(np.log2(fft)) + 4


def test_stft_operands_are_the_wrappers():
    """The window and the twiddles the reference is built on are the arrays frontend.stft_magnitude uploads (same expressions)."""
    w = P.stft_window(400)
    assert w.dtype == F32 and w[0] == 0.0 and w.shape == (400,)
    t = P.stft_twiddle(8)
    assert t.dtype == F32 and t.shape == (4, 2) and t[0, 0] == 1.0 and t[0, 1] == 0.0 and t[2, 1] == -1.0


@pytest.mark.parametrize("cfg", P.STFT_CONFIGS, ids=P.stft_id)
def test_stft_case_and_restatement(cfg):
    """Every signal has the planted structure; fft_f32() stays inside P 2^-24 S per element on every input, and its broadband figure R
    meets the condition R <= 5e-7."""
    fft, win, hop = cfg
    case = P.stft_case(cfg)
    worst = 0.0
    for (n, kind), it in case["items"].items():
        x, ref, s = it["x"], it["ref"], it["s"]
        frames = P.stft_frames(n, win, hop)
        assert x.dtype == F32 and x.shape == (n,) and ref.shape == (frames, fft // 2 + 1) and s.shape == (frames,)
        if kind == "impulses":
            assert x[0] == 1.0 and (win == 1 or float(x[(frames - 1) * hop + win - 1]) in (1.0, -0.75))
            assert set(np.unique(x)) <= {0.0, 1.0, -0.75} and (win == 1 or (x == -0.75).any())
            if frames == 1 and win > 1:
                # one impulse alone in reach of the window: every bin equals |w32[p] x_p| summed coherently -- here the bound is tight
                assert bool((s <= 1.75).all())
        if kind == "cosine" and fft >= 4 and win == fft:
            # the cosine on bin fft / 4 under a full window: that bin carries half the window's sum
            assert abs(ref[0, fft // 4] - 0.5 * P.stft_window(win).astype(np.float64).sum()) <= 1e-3
        worst = max(worst, P.stft_worst_ratio(P.fft_f32(cfg, x), ref, s, fft))
    print("stft %s: restatement worst |error| / (P 2^-24 S) = %.3g (P = %d), R = %.3g" % (P.stft_id(cfg), worst, P.stft_p(fft), case["R"]))
    assert worst <= 1.0
    assert case["R"] <= P.STFT_R_MAX


def test_stft_bound_catches_what_it_is_for():
    """On the impulse input a bin index off by one, a twiddle off by 1e-5 and a window index off by one all leave the bound."""
    cfg = (256, 200, 80)
    n = P.stft_lengths(cfg)[3]
    it = P.stft_case(cfg)["items"][(n, "impulses")]
    good = P.fft_f32(cfg, it["x"])
    assert P.stft_worst_ratio(good, it["ref"], it["s"], 256) <= 1.0
    assert P.stft_worst_ratio(np.roll(good, 1, axis=1), it["ref"], it["s"], 256) > 1.0
    tw = P.stft_twiddle
    try:
        def off(fft):
            t = tw(fft)
            t[5, 0] += F32(1e-5)
            return t
        P.stft_twiddle = off
        bad = P.fft_f32(cfg, it["x"])
    finally:
        P.stft_twiddle = tw
    assert P.stft_worst_ratio(bad, it["ref"], it["s"], 256) > 1.0
    noise = P.stft_case(cfg)["items"][(n, "noise")]
    try:
        P.stft_twiddle = off
        e = P.stft_frame_errors(P.fft_f32(cfg, noise["x"]), noise["ref"])
    finally:
        P.stft_twiddle = tw
    assert float(e.max()) > 2 * P.stft_case(cfg)["R"]


# --------------------------------------------------------------------------------------------------- mel_log ----

def test_mel_shapes_cover_the_block_edges():
    lanes = P.C["mel_lanes"]
    outs = [f * b for f, _, b in P.MEL_SHAPES]
    assert any(o % lanes for o in outs) and any(o > lanes for o in outs) and any(o > lanes and o % lanes for o in outs)
    assert max(bins for _, bins, _ in P.MEL_SHAPES) * 4 * 64 < 2 ** 24          # the worst case of sum|terms| / 2^-6


@pytest.mark.parametrize("offset", P.MEL_OFFSETS)
@pytest.mark.parametrize("shape", P.MEL_SHAPES, ids=P.mel_id)
def test_mel_grid_case(shape, offset):
    """The grid is exact (asserted inside the case from the reference): the plain f32 chain reproduces v bit for bit. The planted
    -inf, the planted exact 0 and the |log v| >= 2^-6 condition hold on the reference."""
    frames, bins, bands = shape
    c = P.mel_grid_case(shape, offset)
    spec, mel, v, ref = c["spec"], c["mel"], c["v"], c["ref"]
    assert spec.shape == (frames, bins) and mel.shape == (bins, bands)
    assert np.array_equal(spec * 8, np.rint(spec * 8)) and 0 <= spec.min() and spec.max() <= 4
    assert np.array_equal(mel * 8, np.rint(mel * 8)) and 0 <= mel.min() and mel.max() <= 1
    assert np.array_equal(P.mel_f32_chain(spec, mel, offset).astype(np.float64), v)
    assert ref[c["one"]] == 0.0 and v[c["one"]] == 1.0
    finite = np.isfinite(ref)
    rest = finite & (v != 1.0)
    assert bool((np.abs(ref[rest]) >= P.MEL_MIN_LOG).all())
    if offset == 0.0:
        assert np.array_equal(~finite, v == 0.0) and bool((ref[~finite] == -np.inf).all())
        if frames >= 2:
            assert bool((~finite[frames - 1]).all())
        if bands >= 3:
            assert bool((~finite[:, bands - 1]).all())
        assert bool(finite.any())
    else:
        assert bool(finite.all())


@pytest.mark.parametrize("cid", list(P.MEL_UNIFORM))
def test_mel_uniform_case(cid):
    c = P.mel_uniform_case(cid)
    frames, bins, _, _ = P.MEL_UNIFORM[cid]
    assert c["spec"].shape == (frames, bins) and 0 <= c["spec"].min() and c["spec"].max() < 30 and not c["mel"][0].any()
    finite = np.isfinite(c["ref"])
    assert bool(finite.any()) and (c["offset"] == 0.0 or bool(finite.all()))
    assert float(c["bound"].max()) <= (bins + 1) * U
    with np.errstate(divide="ignore"):
        got = np.log(P.mel_f32_chain(c["spec"], c["mel"], c["offset"]).astype(np.float64))
    assert np.array_equal(np.isfinite(got), finite)
    ratio = float((np.abs(got - c["ref"])[finite] / c["bound"][finite]).max())
    print("mel_log uniform %s: f32 chain worst |error| / bound = %.3g" % (cid, ratio))
    assert ratio <= 1.0


# -------------------------------------------------------------------------------------------- dataset_frames ----

def test_frames_cases_cover_the_argument_space():
    cases = P.frames_cases()
    assert {c[1] for c in cases} == {0, 1, 2, 3, 4} and {c[0] for c in cases} == {1, 3, 35} and {c[2] for c in cases} == set(P.FRAMES_GEOMETRIES)
    for clips, ex, geo in cases:
        n_frames, frame_len, stride = geo
        assert (n_frames - 1) * stride + frame_len <= P.C["frames_columns"] and ex <= P.C["frames_slots"]
    total, trip = P.frames_trips(*P.FRAMES_BIG[::2])
    assert (total, trip) == (2150400, 2097152) and trip < total < 2 * trip            # a partial second grid-stride trip
    assert all(P.frames_trips(c[0], c[2])[0] <= trip for c in cases if c[0] != 35)
    assert total * 4 <= 9 << 20


@pytest.mark.parametrize("case", P.frames_cases(), ids=P.frames_id)
def test_frames_restatement(case):
    """The restatement against the index rule written element by element (sampled), the zeros of the missing slots, and -- at the
    two geometries the reference uses -- against oracle/dataset_frames.py's split of the same spectrogram."""
    clips, ex, geo = case
    n_frames, frame_len, stride = geo
    e = P.frames_examples(clips, ex)
    out = P.frames_restated(e, clips, ex, geo)
    assert out.shape == (clips, n_frames, 64, frame_len) and out.dtype == F32
    assert len(np.unique(e)) == e.size and (e.size == 0 or e.min() == 1.0)
    rng = np.random.default_rng(clips + ex + n_frames)
    for c, t, band, x in zip(rng.integers(0, clips, 200), rng.integers(0, n_frames, 200), rng.integers(0, 64, 200), rng.integers(0, frame_len, 200)):
        col = t * stride + x
        want = e[c * ex + col // 96, col % 96, band] if col // 96 < ex else 0.0
        assert out[c, t, band, x] == want
    cols = np.arange(n_frames)[:, None] * stride + np.arange(frame_len)[None, :]
    assert np.array_equal(out == 0.0, np.broadcast_to((cols >= 96 * ex)[None, :, None, :], out.shape))
    if geo in ((10, 96, 32), (4, 96, 96)) and ex:
        for c in range(min(clips, 2)):
            padded = np.zeros((4, 96, 64))
            padded[:ex] = e[c * ex:(c + 1) * ex]
            spec = np.concatenate(np.swapaxes(padded, 1, 2)[:4], axis=1)
            assert np.array_equal(out[c], odf.split(spec, n_frames, 96, 64, overlap=geo == (10, 96, 32)))


# ----------------------------------------------------------------------------------------------- postprocess ----

def test_post_grid_is_exact_and_meets_its_conditions():
    c = P.post_grid_case()
    E, mu, x, acc, v, q = (c[k] for k in ("E", "mu", "x", "acc", "v", "q"))
    assert np.array_equal(E * 64, np.rint(E * 64)) and np.abs(E).max() <= 0.125
    d = x.astype(np.float64) - mu.astype(np.float64)
    assert np.array_equal(x * 16, np.rint(x * 16)) and np.array_equal(mu * 16, np.rint(mu * 16)) and np.abs(d).max() <= 2.0
    assert np.array_equal(acc * 1024, np.rint(acc * 1024)) and float(c["terms"].max()) <= 32.0            # units of 2^-10, 2^15 of them
    assert np.array_equal(v * 4096, np.rint(v * 4096)) and v.max() <= 255.0                                # 20 bits
    # an f32 emulation of the kernel's chain is bit-equal to float64
    assert np.array_equal(P.post_f32_emulation(x, E, mu).astype(np.float64), q)
    # the only exact ties are acc == 0 (127.5 -> 128 under both rounding rules): the grid does not separate the rules
    tie = (v - np.floor(v)) == 0.5
    assert np.array_equal(tie, acc == 0.0) and bool((q[tie] == 128.0).all()) and bool(tie.any())
    # shares
    inside = float(((q >= 1) & (q <= 254)).mean())
    print("postprocess grid: %.1f %% of the outputs strictly inside 1..254" % (100 * inside))
    assert inside >= 0.90
    assert set(np.unique(q)) == set(float(i) for i in range(256))
    # planted rows
    assert bool((q[0] == 128.0).all())
    assert [acc[1, j] for j in (5, 6, 7, 8)] == [2.0, -2.0, 2.25, -2.25] and [q[1, j] for j in (5, 6, 7, 8)] == [255.0, 0.0, 255.0, 0.0]
    assert [acc[2, j] for j in (7, 8)] == [1.75, -1.75]
    for k in (0, 1, 77, 127):
        sign = 2.0 if k % 2 == 0 else -2.0
        assert np.array_equal(acc[3 + k], sign * E[:, k].astype(np.float64))
    # the one-hot rows tell E from its transpose
    assert not np.array_equal(P.post_reference(x[3:131], E.T.copy(), mu)["q"], q[3:131])
    for rows in P.POST_ROWS:
        assert P.post_rows(c, rows).shape == (rows, 128)


def test_post_uniform_case_meets_its_conditions():
    c = P.post_uniform_case()
    inside = float(((c["q"] >= 1) & (c["q"] <= 254)).mean())
    sure = float((c["tie"] > c["bound"]).mean())
    print("postprocess uniform: %.1f %% interior, %.3f %% of the outputs decided by the bound" % (100 * inside, 100 * sure))
    assert inside >= 0.50 and sure >= 0.99
    got = P.post_f32_emulation(c["x"], c["E"], c["mu"])
    assert bool(P.post_uniform_ok(got, c).all())
    # the criterion is not vacuous: the transposed matrix fails it
    assert not bool(P.post_uniform_ok(P.post_reference(c["x"], c["E"].T.copy(), c["mu"])["q"], c).all())


# -------------------------------------------------------------------------------------------------- mono_mix ----

@pytest.mark.parametrize("channels", P.MIX_CHANNELS)
def test_mix_reference(channels):
    for n in P.MIX_NS:
        a = P.mix_input(n, channels, True)
        assert a.dtype == np.int16 and a.shape == (n, channels) and a.min() == -32768 and a.max() == 32767
        ref = P.mix_reference(a)
        assert ref.dtype == F32 and ref.shape == (n,)
        exact = a.astype(np.int64).sum(axis=1) / (channels * 32768.0)
        assert np.array_equal(ref, exact.astype(F32)) or channels in (3, 5)          # a division by 3 or 5 rounds in double first
        assert float(np.abs(ref.astype(np.float64) - exact).max()) <= U
        if n >= 2:
            assert ref[0] == -1.0 and ref[1] == F32(32767.0 / 32768.0)
        f = P.mix_input(n, channels, False)
        assert f.dtype == F32
        rf = P.mix_reference(f)
        assert float(np.abs(rf.astype(np.float64) - f.astype(np.float64).mean(axis=1)).max()) <= U
        # a divisor off by one or a stride off by one channel is far outside equality
        assert not np.array_equal(rf, (f.astype(np.float64).sum(axis=1) / (channels + 1)).astype(F32))


# -------------------------------------------------------------------------------------------------- resample ----

def test_resample_cases_cover_the_edges():
    geo = {c: P.resample_geometry(c) for c in P.RESAMPLE_CASES}
    assert geo[(256000, 9000)][1:] == (32, 1024) and geo[(44100, 3)][0] == 1
    n_out, step, taps = geo[(48000, 63)]
    assert taps > 63 and n_out == 21                                        # both wings are clipped by the signal for every output
    assert all(c[1] <= 10000 for c in P.RESAMPLE_CASES)
    assert P.resample_geometry(P.RESAMPLE_SHORT)[0] == 0
    with pytest.raises(ValueError):
        ors.resample(np.zeros(1), P.RESAMPLE_SHORT[0], P.SR_OUT)


@pytest.mark.parametrize("case", P.RESAMPLE_CASES, ids=P.resample_id)
def test_resample_restatement_within_the_double_term(case):
    """The kernel's arithmetic restated (the position's fraction by one fused rounding) differs from the oracle by far less than the
    1e-10 max|x| the bound grants for it; the impulses land where the filter's centre is."""
    for kind in P.RESAMPLE_KINDS:
        c = P.resample_case(case, kind)
        assert c["ref"].shape == (P.resample_geometry(case)[0],) and c["x"].dtype == F32
        got = P.resample_restated(c["x"], case[0])
        diff = float(np.abs(got - c["ref"]).max())
        print("resample %s %s: restated kernel vs oracle %.3g" % (P.resample_id(case), kind, diff))
        assert diff <= 0.01 * P.RESAMPLE_DOUBLE * float(np.abs(c["x"]).max())
        if kind == "impulse-first":
            assert abs(c["ref"][0]) == np.abs(c["ref"]).max() > 0
        if kind == "impulse-last" and c["ref"].shape[0] > 1:
            assert np.abs(c["ref"][-1]) > 0.1 * np.abs(c["ref"]).max()
