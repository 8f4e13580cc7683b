"""The log-mel backward (csrc/logmel_bwd.hip) without a GPU: the float64 reference's own properties (conditioning of the cases, the
explicit loop form of the formulas); the kernel's work items simulated on the host (csrc/logmel_bwd_hostsim.cpp: every stage and
all index arithmetic of csrc/logmel_bwd_core.h for every workgroup of a launch) against that reference under a bound taken from a
float32 restatement that is not the code under test; one store per element, zero tail, zeros for silence and for G = 0,
independence of batch, stride and grid, reads inside the inputs, the grid-cap crossing; the C entry's argument errors, reported
before any launch."""

import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import logmel_bwd_cases as D
from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def L():
    build = importlib.import_module(PKG + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def hostsim(tmp_path_factory, L):
    so = str(tmp_path_factory.mktemp("logmel_bwd_hostsim") / "logmel_bwd_hostsim.so")
    src = os.path.join(ROOT, PKG, "csrc", "logmel_bwd_hostsim.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.hostsim_logmel_bwd.argtypes = [vp, ci, i64, i64, i64, vp, ci, vp, i64, vp, vp]
    lib.hostsim_logmel_bwd_grid.argtypes = [i64]
    lib.hostsim_logmel_bwd_items.argtypes = [i64, i64]
    lib.hostsim_logmel_bwd_items.restype = i64
    lib.hostsim_logmel_bwd_build_tables.argtypes = [vp]
    return lib


def run_hostsim(hostsim, pcm, g, pad=0, d_pad=0, grid=0):
    """pcm (W, n) and g tensors -> (d_wave float32 tensor (W, n), max_read[2]); the rows of pcm lie n + pad elements apart, those of
    d_wave n + d_pad. d_wave comes in NaN-filled; asserts one store per valid element and none into the padding."""
    W, n = pcm.shape
    a = np.zeros((W, n + pad), dtype=pcm.numpy().dtype)
    a[:, :n] = pcm.numpy()
    gn = np.ascontiguousarray(g.numpy(), dtype=np.float32)
    out = np.full((W, n + d_pad), np.nan, dtype=np.float32)
    writes = np.zeros((W, n + d_pad), dtype=np.int32)
    max_read = np.zeros(2, dtype=np.int64)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)                                            # noqa: E731
    rc = hostsim.hostsim_logmel_bwd(p(a), int(a.dtype == np.int16), W, n, n + pad, p(gn), grid, p(out), n + d_pad, p(writes), p(max_read))
    assert rc == 0, rc
    assert (writes[:, :n] == 1).all() and not writes[:, n:].any(), "every element of d_wave is written exactly once"
    return torch.from_numpy(out[:, :n].copy()), max_read


def last_used(pcm, g, pad=0):
    """The highest element a launch may read of pcm (the last sample of the last used frame of the last row) and of G."""
    W, n = pcm.shape
    used = D.counts(n)[1] * D.EX
    return [(W - 1) * (n + pad) + D.HOP * (used - 1) + D.WIN - 1, g.numel() - 1]


@pytest.mark.parametrize("name", D.CONDITIONED)
def test_reference_cases_are_well_conditioned(name):
    assert D.least_relative_magnitude(name) >= 1e-5


def test_explicit_loop_equals_autograd():
    pcm, g = D.case("a")
    assert D.err(D.loop_form(pcm, g), D.reference("a")) <= 1e-12


def test_launcher_constants_and_cap(hostsim):
    W, n = D.cap_crossing_shape()
    assert hostsim.hostsim_logmel_bwd_max_wg() == D.MAX_WG and (W, n) == (8, 160000)
    for shape in ((1, 15600), (3, 30960), (W - 1, n), (W, n)):
        items = hostsim.hostsim_logmel_bwd_items(*shape)
        assert items == shape[0] * D.items_per_row(shape[1])
        assert hostsim.hostsim_logmel_bwd_grid(items) == min(items, D.MAX_WG)
    assert (W - 1) * D.items_per_row(n) <= D.MAX_WG < W * D.items_per_row(n)


def test_backward_tables_transpose_the_mel_matrix(hostsim, L):
    """The bin -> (b0, w0, w1) table rebuilds the dense float64 mel matrix (halved, rounded to float32) and the library's entry
    gives the host simulation's table."""
    n = hostsim.hostsim_logmel_bwd_table_floats()
    tab, tab2 = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    assert hostsim.hostsim_logmel_bwd_build_tables(tab.ctypes.data_as(ctypes.c_void_p)) == 0
    assert L.lib().mla_logmel_bwd_table_floats() == n
    assert L.lib().mla_logmel_bwd_build_tables(tab2.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(tab, tab2)
    mel = D.tables()[1].numpy()
    dense = np.zeros((256, D.BANDS), dtype=np.float32)
    b0 = tab[:1024].view(np.int32)[0::4]
    assert b0.min() >= 0 and b0.max() <= D.BANDS - 2
    for k in range(256):
        dense[k, b0[k]] = tab[4 * k + 1]
        dense[k, b0[k] + 1] = tab[4 * k + 2]
    assert np.array_equal(dense, (0.5 * mel[:256]).astype(np.float32)) and not mel[256].any()
    k = np.arange(256)
    assert np.array_equal(tab[1024::2], np.cos(2 * np.pi * k / 512).astype(np.float32))
    assert np.array_equal(tab[1025::2], (-np.sin(2 * np.pi * k / 512)).astype(np.float32))


@pytest.mark.parametrize("name", D.CASES)
def test_hostsim_against_the_float64_reference(hostsim, name):
    pcm, g = D.case(name)
    pad = D.STRIDE_PAD.get(name, 0)
    got, max_read = run_hostsim(hostsim, pcm, g, pad=pad)
    e, bound = D.err(got, D.reference(name)), D.bound(name)
    print("case %s: err %.3e, float32 restatement %.3e, bound %.3e" % (name, e, D.yardstick(name), bound))
    assert e <= bound
    assert max_read.tolist() == last_used(pcm, g, pad)
    assert bool(torch.isfinite(got).all())


def test_hostsim_zero_tail_and_silence(hostsim):
    pcm, g = D.case("b")
    got, _ = run_hostsim(hostsim, pcm, g)
    assert bool((got[:, 15600:] == 0).all()) and bool((got[:, :15600] != 0).float().mean() > 0.99)
    pcm, g = D.case("g")
    got, _ = run_hostsim(hostsim, pcm, g, pad=37)
    assert bool((got[2] == 0).all()), "silence: A_k = 0 passes nothing, no NaN"
    assert bool((got[1, 15600 + D.WIN:] == 0).all()), "frames of zeros behind the zero-extended signal"


@pytest.mark.parametrize("n", (240, 399, 400, 15599))
def test_hostsim_no_example_writes_zeros_and_reads_nothing(hostsim, n):
    pcm = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (2, n)).astype(np.float32))
    got, max_read = run_hostsim(hostsim, pcm, torch.zeros(0, 96, 64))
    assert bool((got == 0).all()) and max_read.tolist() == [-1, -1]


def test_hostsim_zero_gradient_gives_zeros(hostsim):
    pcm, g = D.case("c")
    got, _ = run_hostsim(hostsim, pcm, torch.zeros_like(g))
    assert bool((got == 0).all())


def test_hostsim_rows_do_not_depend_on_batch_stride_or_grid(hostsim):
    pcm, g = D.case("g")
    ref, _ = run_hostsim(hostsim, pcm, g, pad=37)
    for pad, d_pad, grid in ((0, 0, 0), (5, 11, 0), (37, 0, 1), (37, 0, 2), (37, 0, 5), (0, 3, 1000)):
        assert torch.equal(run_hostsim(hostsim, pcm, g, pad=pad, d_pad=d_pad, grid=grid)[0], ref)
    per = g.shape[0] // 3
    for r in range(3):
        alone, _ = run_hostsim(hostsim, pcm[r:r + 1], g[r * per:(r + 1) * per])
        assert torch.equal(alone[0], ref[r])


def test_hostsim_beyond_the_grid_cap(hostsim):
    """The smallest batch of 10 s rows at which workgroups take a second trip through the item loop."""
    pcm, g = D.case("cap")
    got, max_read = run_hostsim(hostsim, pcm, g)
    e, bound = D.err(got, D.reference("cap")), D.bound("cap")
    print("cap: err %.3e, bound %.3e" % (e, bound))
    assert e <= bound and max_read.tolist() == last_used(pcm, g)
    assert torch.equal(run_hostsim(hostsim, pcm[-1:], g[-10:])[0][0], got[-1]), "a row computed on a second trip equals the row alone"


def test_argument_errors_are_reported_before_any_launch(L):
    lib = L.lib()
    for sym in ("mla_logmel_examples_bwd", "mla_logmel_bwd_table_floats", "mla_logmel_bwd_build_tables"):
        assert sym in L.declared_symbols()
    vp = ctypes.c_void_p
    fake = vp(0x1000)                                    # device pointers: never dereferenced, every call below fails validation first
    E_ARG, E_SHORT, E_DTYPE = -1, -3, -5

    def bwd(pcm=fake, dtype=L.F32, n_wave=2, n=15600, stride=15600, tab=fake, btab=fake, g=fake, dw=fake, d_stride=15600):
        return lib.mla_logmel_examples_bwd(pcm, dtype, n_wave, n, stride, tab, btab, g, dw, d_stride, None)

    def expect(code, rc, needle):
        assert rc == code, (rc, lib.mla_last_error())
        assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    for null in ("pcm", "tab", "btab", "g", "dw"):
        expect(E_ARG, bwd(**{null: None}), "null")
    expect(E_ARG, bwd(n_wave=-1), "n_wave -1")
    expect(E_ARG, bwd(n=-1, stride=0, d_stride=0), "n_samples -1")
    expect(E_ARG, bwd(stride=15599), "strides")
    expect(E_ARG, bwd(d_stride=15599), "strides")
    expect(E_SHORT, bwd(n=239, stride=239, d_stride=239), "239 samples")
    for code in (L.BF16, L.BF16X3, L.F64, 9):
        expect(E_DTYPE, bwd(dtype=code), "pcm_dtype")
    expect(E_ARG, bwd(pcm=vp(0x1002)), "misaligned")
    assert bwd(pcm=vp(0x1002), dtype=L.I16, n_wave=0) == 0
    expect(E_ARG, bwd(dw=vp(0x1002)), "4-byte aligned")
    assert bwd(n_wave=0) == 0
    assert bwd(n_wave=0, pcm=None, tab=None, btab=None, g=None, dw=None) == 0
    assert lib.mla_logmel_bwd_build_tables(None) == E_ARG
