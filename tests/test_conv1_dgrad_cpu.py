"""conv1's input gradient (csrc/conv1_dgrad.hip) without a GPU: the float64 reference's own properties; the kernel's work items
simulated on the host (csrc/conv1_dgrad_hostsim.cpp: the tile / halo / code / gather arithmetic of csrc/conv1_dgrad_core.h for every
workgroup of a launch) against that reference, bit for bit; one store per dx element; reads inside every input; independence of
the clips and of the grid; the C entry's argument errors, reported before any launch."""

import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import conv1_dgrad_cases as D
from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def L():
    build = importlib.import_module(PKG + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def hostsim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("conv1_dgrad_hostsim") / "conv1_dgrad_hostsim.so")
    src = os.path.join(ROOT, PKG, "csrc", "conv1_dgrad_hostsim.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.hostsim_conv1_dgrad.argtypes = [vp, vp, vp, vp, ci, i64, ci, vp, vp, vp]
    lib.hostsim_conv1_dgrad_grid.argtypes = [i64]
    return lib


def run_hostsim(hostsim, x, w, b, d, bf16, grid=0):
    """-> (dx float32 tensor (n, 96, 64), max_read[4]); asserts one store per element. dx comes in NaN-filled."""
    n = x.shape[0]
    xs, ws, bs, ds = (np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (x, w, b, d))
    dx = np.full((n, 96, 64), np.nan, dtype=np.float32)
    writes = np.zeros((n, 96, 64), dtype=np.int32)
    max_read = np.zeros(4, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                            # noqa: E731
    rc = hostsim.hostsim_conv1_dgrad(p(xs), p(ws), p(bs), p(ds), int(bf16), n, grid, p(dx), p(writes), p(max_read))
    assert rc == 0, rc
    assert (writes == 1).all(), "every element of dx is written exactly once"
    return torch.from_numpy(dx), max_read


@pytest.mark.parametrize("n", D.NS)
def test_reference_properties(n):
    """What the issue states of the float64 reference: the 2^-7 grid and the 2^24 bound (asserted in reference()), gradient on nearly
    every pixel and on all four image borders."""
    dx, dabs = D.reference(n)
    assert float(dabs.max()) / D.UNIT <= 3425
    assert float((dx != 0).double().mean()) > 0.99
    for border in (dx[:, 0], dx[:, -1], dx[:, :, 0], dx[:, :, -1]):
        assert float((border != 0).double().mean()) > 0.9


def test_launcher_constants_and_cap(hostsim):
    n = D.cap_crossing_n()
    assert hostsim.hostsim_conv1_dgrad_max_wg() == D.C["max_wg"]
    for k in (1, 3, 65, n - 1, n, 1000):
        assert hostsim.hostsim_conv1_dgrad_grid(k) == D.grid_of(k)
    assert D.grid_of(n - 1) == (n - 1) * D.TILES and D.grid_of(n) == D.C["max_wg"] < n * D.TILES


@pytest.mark.parametrize("bf16", (False, True))
@pytest.mark.parametrize("n", (1, 3))
def test_hostsim_equals_the_float64_reference(hostsim, n, bf16):
    x, w, b, d = D.T.conv1_bwd_operands(n)
    dx, max_read = run_hostsim(hostsim, x, w, b, d, bf16)
    assert torch.equal(dx.double(), D.reference(n)[0])
    # the largest index read is the last element of each input, and no more
    assert max_read.tolist() == [x.numel() - 1, w.numel() - 1, b.numel() - 1, d.numel() - 1]


def test_hostsim_beyond_the_grid_cap(hostsim):
    """The smallest n at which workgroups take a second trip through the item loop."""
    n = D.cap_crossing_n()
    x, w, b, d = D.T.conv1_bwd_operands(n)
    dx, max_read = run_hostsim(hostsim, x, w, b, d, False)
    assert torch.equal(dx.double(), D.reference(n)[0])
    assert max_read.tolist() == [x.numel() - 1, w.numel() - 1, b.numel() - 1, d.numel() - 1]


def test_hostsim_does_not_depend_on_the_grid(hostsim):
    x, w, b, d = D.T.conv1_bwd_operands(3)
    ref = run_hostsim(hostsim, x, w, b, d, False)[0]
    for grid in (1, 5, 24, 1000):
        assert torch.equal(run_hostsim(hostsim, x, w, b, d, False, grid)[0], ref)


@pytest.mark.parametrize("bf16", (False, True))
def test_hostsim_clips_are_independent(hostsim, bf16):
    x2, w, b, d2 = D.two_clip_case()
    dx = run_hostsim(hostsim, x2, w, b, d2, bf16)[0]
    assert torch.equal(dx[0].double(), D.reference(1)[0][0])
    assert not bool(dx[1].any())


def test_bf16_recompute_rounds_x_and_w(hostsim):
    """Off the bf16 grid the two modes route differently: x = 1 + 2^-9 rounds to 1 in bf16, so a filter that prefers the larger of two
    neighbours sees a tie in bf16 mode (first position wins) and a strict maximum in f32 mode."""
    x = torch.ones(1, 96, 64)
    x[0, 1::2, 1::2] = 1.0 + 2.0 ** -9                       # position (1, 1) of every window is the largest input
    w = torch.zeros(64, 1, 3, 3)
    w[:, 0, 1, 1] = 1.0
    b = torch.zeros(64)
    d = torch.ones(1, 48, 32, 64)
    f32 = run_hostsim(hostsim, x, w, b, d, False)[0]
    lp = run_hostsim(hostsim, x, w, b, d, True)[0]
    assert torch.equal(f32[0, 1::2, 1::2], torch.full((48, 32), 64.0)) and not bool(f32[0, ::2].any())
    assert torch.equal(lp[0, ::2, ::2], torch.full((48, 32), 64.0)) and not bool(lp[0, 1::2].any())


def test_argument_errors_are_reported_before_any_launch(L):
    lib = L.lib()
    assert "mla_conv1_dgrad" in L.declared_symbols()
    vp = ctypes.c_void_p
    fake = vp(0x1000)                                    # device pointers: never dereferenced, every call below fails validation first
    E_ARG, E_SHAPE, E_DTYPE = -1, -2, -5

    def dgrad(x=fake, w=fake, bias=fake, d=fake, dtype=L.F32, n=2, dx=fake):
        return lib.mla_conv1_dgrad(x, w, bias, d, dtype, n, dx, None)

    def expect(code, rc, needle):
        assert rc == code, (rc, lib.mla_last_error())
        assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    for null in ("x", "w", "bias", "d", "dx"):
        expect(E_ARG, dgrad(**{null: None}), "null")
    expect(E_ARG, dgrad(n=-1), "n = -1")
    for code in (L.I16, L.BF16X3, L.F64, 9):
        expect(E_DTYPE, dgrad(dtype=code), "d_pooled dtype")
    expect(E_ARG, dgrad(d=vp(0x1008)), "16-byte aligned")
    expect(E_ARG, dgrad(d=vp(0x1008), dtype=L.BF16), "16-byte aligned")
    expect(E_SHAPE, dgrad(n=2 ** 41), "too many")
    assert dgrad(n=0) == 0
    assert dgrad(n=0, x=None, w=None, bias=None, d=None, dx=None, dtype=L.BF16) == 0
