"""CPU side of tests/test_pin_leftovers_gpu.py: the constants read from csrc/ are the ones the shapes were chosen for, the case
tables enter the branches they name, and every operand builder, float64 reference, bound and exactness assertion of the GPU file
evaluates without a device."""

import numpy as np
import pytest
import torch

import pin_leftover_cases as P
import resnet50_restated as R
from infer_kernel_cases import BF16, F32


def test_constants_read_from_the_sources():
    C = P.C
    assert (C["narrow_blocks"], C["narrow_rows"]) == (2048, 16)
    assert (C["small_min_n"], C["small_max_k"], C["small_lds"], C["small_min_out"], C["small_wide_blocks"]) == (64, 64, 48 * 1024, 65536, 1024)
    assert C["colsum_rows"] == {F32: 64, BF16: 256} and C["colsum_chunks"] == 64
    assert (C["stat_blocks"], C["max_channels"], C["fused_channels"]) == (512, 64, 16)
    assert (C["img"], C["stem_out"], C["stem_blocks"]) == (224, 112, 1024)
    # kNormMean is the f32 of the restatement's mean, kNormInv the f32 quotient 1.f / std
    assert C["norm_std_text"] == list(R.STD)
    for c in range(3):
        assert C["norm_mean"][c] == float(np.float32(R.MEAN[c]))
        assert C["norm_inv"][c] == float(np.float32(1.0) / np.float32(R.STD[c]))
        assert abs(C["norm_inv"][c] * R.STD[c] - 1.0) <= 2.0 ** -23


# ------------------------------------------------------------------------------------------------------ stem ----

@pytest.mark.parametrize("conf", P.STEM_CONFS)
@pytest.mark.parametrize("n", P.STEM_NS)
def test_stem_forward_case(conf, n):
    c = P.stem_case(conf, n)
    planes, w, acc, terms = c["planes"], c["w"], c["acc"], c["terms"]
    assert tuple(acc.shape) == (n, 112, 112, 64) and bool((terms > 0).all())
    # planes in [0, 1) inside, a few units on the planted border, every image different
    inner = planes[:, 3:-3, 3:-3]
    assert float(inner.min()) >= 0.0 and float(inner.max()) < 1.0 and 2.0 <= float(planes.abs().max()) < 8.0
    assert all(not torch.equal(planes[i], planes[j]) for i in range(n) for j in range(i))
    # the normalisation is the restatement's up to the f32 rounding of its constants
    mine, theirs = P.stem_normalize(planes, conf), R.normalize_input(planes.double().reshape(n, 1, 1, 224, 224), conf)
    assert float(((mine - theirs).abs() / P.stem_magnitudes(planes, conf)).max()) <= 2.0 ** -23
    # sign-coherent taps: sum|terms| is the sum of |a_k x_k| + |b_k| of the kernel's coefficients
    lit = P.stem_literal_terms(planes, w, conf)
    assert float(((lit - terms).abs() / terms).max()) < 1e-12
    # the planted border does not set the scale elsewhere: an output whose window lies inside rows / columns 3..220 is bounded by
    # 49 taps of the largest coefficient magnitudes on values below 1
    assert float(terms[:, 3:109, 3:109].max()) < 0.6 * float(terms.max())
    # a tap outside the image contributes nothing: an all-mean plane has the value 0 in channel-0-only form
    flat = torch.full((1, 224, 224), P.NORM_MEAN[0])
    w0 = torch.zeros(64, 3, 7, 7)
    w0[:, 0] = w[:, 0]
    assert float(P.stem_reference(flat, w0, "repeat")[0].abs().max()) == 0.0
    for dtype in (F32, BF16):
        for scale, shift, relu in ((None, None, False), (c["scale"], c["shift"], True)):
            ref, b = P.stem_bound(acc, terms, scale, shift, relu, dtype)
            assert bool(torch.isfinite(ref).all()) and bool((b > 0).all())
            if relu:
                pre = acc * scale.double() + shift.double()
                assert bool((pre < 0).any()) and bool((pre > 0).any()) and float(ref.min()) == 0.0
            # the bound is far below what the norm-wise test allows an interior element
            assert float(b.max()) < (1e-4 if dtype == F32 else 1e-2) * float(ref.abs().max())


@pytest.mark.parametrize("conf", P.STEM_CONFS)
@pytest.mark.parametrize("n", P.WGRAD_NS)
def test_stem_wgrad_case(conf, n):
    c = P.wgrad_case(conf, n)
    assert P.wgrad_rows_per_block(n) == {1: 1, 10: 2, 19: 3}[n] and P.wgrad_p(n) == {1: 35, 10: 63, 19: 91}[n]
    assert tuple(c["ref"].shape) == tuple(c["terms"].shape) == (64, 3, 7, 7)
    assert torch.equal(c["dy"].float().to(BF16), c["dy"])
    assert bool((c["ref"].abs() <= c["terms"] * (1 + 1e-6)).all()) and bool((c["bound"] > 0).all())
    # a worst-case bound over 12544 n terms of random sign: the same order as the norm-wise f32 figure (1e-4 of the largest value),
    # far below the bf16 one (1e-2), and per element
    assert float(c["bound"].max()) < 2e-3 * float(c["ref"].abs().max())


# ---------------------------------------------------------------------------------------------------- linear ----

def test_linear_narrow_cases():
    assert P.NARROW_NS == tuple(range(1, 17)) and [k // 4 for k in P.NARROW_KS] == [1, 2, 16, 17, 150]
    assert [P.narrow_grid(m) for m in P.NARROW_MS] == [1, 2]
    M, N, Kk = P.NARROW_BIG
    assert M == 2048 * 16 + 5 and P.narrow_grid(M) == 2048 and M % 16 == 5 and M * Kk * 4 < 79e6
    for N_ in P.NARROW_NS:
        for Kk_ in P.NARROW_KS:
            for M_ in P.NARROW_MS:
                c = P.linear_case(M_, N_, Kk_)
                assert tuple(c["y"].shape) == (M_, N_) and torch.equal(c["y"].float().double(), c["y"])
                assert Kk_ * N_ * 4 <= 64 * 1024
    c = P.linear_case(M, N, Kk)
    assert torch.equal(c["y"].float().double(), c["y"]) and torch.equal(c["y_nobias"] + c["b"].double(), c["y"])


def test_linear_small_cases_stand_on_both_sides_of_every_term():
    for cid, (M, N, Kk, pad, off, form) in P.SMALL_CASES.items():
        assert P.small_form(M, N, Kk, N + pad, off) == form, cid
        c = P.linear_case(M, N, Kk)
        assert torch.equal(c["y"].float().double(), c["y"]), cid
    S = P.SMALL_CASES
    base = S["wide-66000-outputs"]
    assert base[0] * base[1] == 66000 and S["plain-65400-outputs"][0] * 600 == 65400
    # each plain neighbour fails exactly one term of the switch
    C = P.C
    for cid, (M, N, Kk, pad, off, form) in S.items():
        if form == "plain" and not cid.startswith("tiny"):
            failed = [N % 4 != 0, N < C["small_min_n"], Kk > C["small_max_k"], N * Kk * 4 > C["small_lds"] and Kk <= C["small_max_k"],
                      (N + pad) % 4 != 0, off % 4 != 0, M * N < C["small_min_out"]]
            assert sum(failed) == 1, (cid, failed)
    M, N, Kk = S["wide-second-trip"][:3]
    assert M * (N // 4) > C["small_wide_blocks"] * 256
    assert S["wide-n192-k64"][1] * 64 * 4 == C["small_lds"] and S["wide-n64-k64"][0] * 64 == C["small_min_out"]


# --------------------------------------------------------------------------------------------------- col_sum ----

def test_col_sum_cases():
    assert [P.colsum_chunks(r, F32) for r in P.COLSUM_ROWS[F32]] == [
        (1, 1, 1), (1, 63, 63), (1, 64, 64), (1, 127, 127), (2, 65, 64), (64, 64, 64), (64, 65, 2), (64, 80, 80)]
    assert [P.colsum_chunks(r, BF16) for r in P.COLSUM_ROWS[BF16]] == [
        (1, 1, 1), (1, 255, 255), (1, 256, 256), (2, 257, 256), (64, 256, 256), (64, 257, 194)]
    for cols in P.COLSUM_COLS:
        assert P.colsum_vector_form("dense", cols) == (cols % 4 == 0)
        assert not P.colsum_vector_form("pitched", cols) and not P.colsum_vector_form("offset", cols)
        left, right = P.colsum_layout("pitched", cols)
        assert left == 0 and (cols + right) % 4 != 0
        left, right = P.colsum_layout("offset", cols)
        assert left == 1 and (cols + left + right) % 4 == 0
    assert {c % 64 for c in P.COLSUM_COLS} >= {0, 1} and {c % 256 for c in P.COLSUM_COLS} >= {0, 4}
    for dtype in (F32, BF16):
        for rows in P.COLSUM_ROWS[dtype]:
            for cols in P.COLSUM_COLS:
                x, ref = P.colsum_case(rows, cols)
                assert torch.equal(x.to(dtype).float(), x) and torch.equal(ref.float().double(), ref)


# ------------------------------------------------------------------------------------------------ statistics ----

def test_stats_case_tables():
    assert P.STATS_GROUPS == (1, 3, 512, 1025) and P.STATS_ROWS1 == (1, 63, 65, 64 * 512 + 1)
    seen = set()
    for period in P.STATS_PERIODS:
        cases = P.stats_mode0_cases(period)
        seen |= {(rows // period, cols) for rows, cols in cases}
        assert {rows // period for rows, _ in cases} == set(P.STATS_GROUPS) and {cols for _, cols in cases} == set(P.STATS_COLS0)
        # past kStatBlocks: blocks own three groups each, and the last third of them owns none
        assert P.stats_blocks(0, 1025 * period, period) == (512, 3 * period, 342)
        assert P.stats_blocks(0, 512 * period, period) == (512, period, 512) and P.stats_blocks(0, 3 * period, period) == (3, period, 3)
    assert len(seen) == 16
    left_out = [(p, g, c) for p in P.STATS_PERIODS for g in P.STATS_GROUPS for c in P.STATS_COLS0 if (p * g, c) not in P.stats_mode0_cases(p)]
    assert len(left_out) == 8 and all(p >= 16 and c >= 600 and g >= 512 for p, g, c in left_out)
    assert [P.stats_blocks(1, r, 0) for r in P.STATS_ROWS1] == [(1, 1, 1), (1, 63, 1), (2, 33, 2), (512, 65, 505)]
    for cols in P.STATS_COLS0:
        outcomes = {P.stats_vec_ok(cols, *lay) for lay in P.stats_layouts(cols)}
        assert outcomes == ({True, False} if cols % 4 == 0 else {False})
    F_ = P.C["fused_channels"]
    assert F_ in P.STATS_PERIODS and F_ + 1 in P.STATS_PERIODS and F_ in P.STATS_COLS1 and F_ + 1 in P.STATS_COLS1
    assert max(P.STATS_PERIODS) == max(P.STATS_COLS1) == P.C["max_channels"]


def _check_stats_reference(rows, cols, mode, period):
    x, rm0, rv0, const = P.stats_input(rows, cols, mode, period)
    ref = P.stats_reference(x, rm0, rv0, mode, period)
    ch = P.stats_channels(mode, period, cols)
    assert ref["count"] == (rows // period * cols if mode == 0 else rows)
    for k in ("mean", "var", "run_mean", "run_var"):
        assert tuple(ref[k].shape) == (ch,) and bool(torch.isfinite(ref[k]).all()) and bool((ref["b_" + k] >= 0).all()), k
    if const is not None:       # up to the reference's own double rounding (a device mean may multiply by 1 / count); the KERNEL's
        #                         value is compared with (0.375, 0) exactly by the GPU test
        assert abs(float(ref["mean"][const]) - P.CONSTANT) <= 4 * P.D and 0.0 <= float(ref["var"][const]) <= 4 * P.D
    if ref["count"] == 1:                       # one element: the unbiased variance is the biased one, 0
        assert float(ref["var"].abs().max()) == 0.0 and torch.equal(ref["run_var"], (1 - P.MOMENTUM) * rv0.double())
    else:
        other = [c for c in range(ch) if c != const]
        assert float(ref["var"][other].min()) > 0.0
        # the double sums' share of the bound stays below the one f32 rounding of the result
        assert bool((ref["b_var"][other] < 2 * P.U * ref["var"][other]).all())


@pytest.mark.parametrize("period", P.STATS_PERIODS)
def test_stats_row_mode_references(period):
    for rows, cols in P.stats_mode0_cases(period):
        _check_stats_reference(rows, cols, 0, period)


def test_stats_column_mode_references():
    for cols in P.STATS_COLS1:
        for rows in P.STATS_ROWS1:
            _check_stats_reference(rows, cols, 1, 0)


def test_stats_columns_orders_the_channels():
    x = torch.arange(6 * 2, dtype=torch.float32).reshape(6, 2)          # period 3: channel = row % 3
    cols = P.stats_columns(x, 0, 3)
    assert cols.shape == (4, 3) and cols[:, 1].tolist() == [2.0, 3.0, 8.0, 9.0]
    assert P.stats_columns(x, 1, 0) is x
