"""The mel-dB backward (csrc/melspec_bwd.hip) without a GPU: the float64 reference's own properties (conditioning of the floor
cases, the explicit loop form of DESIGN.md 3.17); every workgroup of the three kernels simulated on the host
(csrc/melspec_bwd_hostsim.cpp: every stage and all index arithmetic of csrc/melspec_bwd_core.h) against that reference under a
bound taken from a float32 restatement that is not the code under test; one store per element, nothing behind n, reads inside the
rows, exact zeros for silence / G = 0 / floor_only without the floor's gradient, independence of batch, position, strides and
workgroup order; the C entries' argument errors, reported before any launch."""

import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import melspec_bwd_cases as D
from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def L():
    build = importlib.import_module(PKG + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def hostsim(tmp_path_factory, L):
    so = str(tmp_path_factory.mktemp("melspec_bwd_hostsim") / "melspec_bwd_hostsim.so")
    src = os.path.join(ROOT, PKG, "csrc", "melspec_bwd_hostsim.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, ci, cf, cd = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_double
    lib.hostsim_melspec_bwd_run_frames.argtypes = [i64]
    lib.hostsim_melspec_bwd_runs.argtypes = [i64, i64]
    lib.hostsim_melspec_bwd_runs.restype = i64
    lib.hostsim_melspec_bwd_span.argtypes = [i64]
    lib.hostsim_melspec_fwd_runs.argtypes = [i64, i64]
    lib.hostsim_melspec_fwd_runs.restype = i64
    lib.hostsim_melspec_fwd.argtypes = [vp, i64, i64, i64, i64, cd, i64, cf, vp, vp]
    lib.hostsim_melspec_fwd.restype = i64
    lib.hostsim_melspec_images_bwd.argtypes = [vp, vp, vp, i64, i64, i64, i64, cf, i64, i64, i64, ci, ci, vp, vp, vp]
    lib.hostsim_melspec_db_bwd.argtypes = [vp, i64, i64, i64, i64, cd, i64, cf, vp, ci, ci, vp, vp, i64, vp, vp]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_hostsim(hostsim, c, pad=0, d_pad=0, order=0, fold_threads=0, g=None):
    """Forward, images backward and db backward of the host simulation on case c -> (d_db, d_pcm) float32 tensors and the highest
    elements read [g, D, pcm, d_db]. The rows of pcm lie n + pad elements apart (the padding holds 1e30), those of d_pcm n + d_pad;
    outputs and workspace come in NaN-filled. Asserts one store per valid element and none behind n."""
    clips, n = c.pcm.shape
    frames = D.frames_of(n, c.hop)
    pcm = np.full((clips, n + pad), 1e30, dtype=np.float32)
    pcm[:, :n] = c.pcm.numpy()
    gn = np.ascontiguousarray((c.g if g is None else g).numpy(), dtype=np.float32)
    db = np.full((clips, c.n_mels, frames), np.nan, dtype=np.float32)
    partial = np.full((clips, int(hostsim.hostsim_melspec_fwd_runs(n, c.hop))), np.nan, dtype=np.float32)
    assert hostsim.hostsim_melspec_fwd(_p(pcm), clips, n, n + pad, c.hop, float(D.SR), c.n_mels, D.AMIN, _p(db), _p(partial)) == frames
    d_db = np.full_like(db, np.nan)
    w_db = np.zeros(db.shape, dtype=np.int32)
    read_img, read_db = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
    rc = hostsim.hostsim_melspec_images_bwd(_p(gn), _p(db), _p(partial), clips, n, c.hop, c.n_mels, D.TOP_DB, c.n_images, c.image_w, c.stride,
                                            int(c.floor_grad), order, _p(d_db), _p(w_db), _p(read_img))
    assert rc == 0, rc
    assert (w_db == 1).all(), "every element of d_db is stored exactly once"
    ws = np.full(clips * int(hostsim.hostsim_melspec_bwd_runs(n, c.hop)) * hostsim.hostsim_melspec_bwd_span(c.hop), np.nan, dtype=np.float32)
    d_pcm = np.full((clips, n + d_pad), np.nan, dtype=np.float32)
    w_pcm = np.zeros(d_pcm.shape, dtype=np.int32)
    rc = hostsim.hostsim_melspec_db_bwd(_p(pcm), clips, n, n + pad, c.hop, float(D.SR), c.n_mels, D.AMIN, _p(d_db), order, fold_threads, _p(ws),
                                        _p(d_pcm), n + d_pad, _p(w_pcm), _p(read_db))
    assert rc == 0, rc
    assert (w_pcm[:, :n] == 1).all() and not w_pcm[:, n:].any(), "every d_pcm[c][s], s < n, is stored exactly once and nothing behind n"
    assert np.isnan(d_pcm[:, n:]).all()
    return torch.from_numpy(d_db), torch.from_numpy(d_pcm[:, :n].copy()), read_img.tolist() + read_db.tolist()


@pytest.mark.parametrize("name", D.FLOOR_CASES)
def test_floor_cases_are_well_conditioned(name):
    gap, margin, near_err = D.conditioning(name)
    print("case %s: maximum unique by %.3g dB, margin to the floor %.3g dB, float32 dB error near the floor %.3g" % (name, gap, margin, near_err))
    assert gap >= D.MIN_MAX_GAP_DB
    assert margin >= D.MARGIN_FACTOR * near_err and margin > 0
    d_db = D.reference(name)[0]
    assert bool((d_db == 0).float().mean() > 0.02), "the case has clipped cells"


@pytest.mark.parametrize("name", [n for n in D.CASES if n not in D.FLOOR_CASES and n != "silence"])
def test_other_cases_have_a_unique_maximum_and_clip_nothing(name):
    gap, margin, _ = D.conditioning(name)
    c = D.case(name)
    with torch.no_grad():
        rel = D.spectrogram(c.pcm.double(), c, torch.float64)[1]
    assert gap > 0 and bool((rel > 0).all()) and margin > 1.0, "nothing is clipped: the floor term is 0 wherever the maximum lies"


@pytest.mark.parametrize("name,floor_grad", (("min", True), ("step", True), ("step", False), ("hop39", True)))
def test_explicit_loop_equals_autograd(name, floor_grad):
    c = D.case(name, floor_grad)
    d_db, d_pcm = D.loop_form(c)
    ref_db, ref_pcm = D.reference(name, floor_grad)
    assert D.err(d_db, ref_db) <= 1e-12 and D.err(d_pcm, ref_pcm) <= 1e-12


def test_run_geometry(hostsim):
    assert hostsim.hostsim_melspec_bwd_run_frames(98) == D.RUN_FRAMES == hostsim.hostsim_melspec_bwd_run_frames(39)
    assert hostsim.hostsim_melspec_bwd_span(98) == 2048 + 31 * 98 and hostsim.hostsim_melspec_bwd_span(39) == 2048 + 31 * 39
    assert hostsim.hostsim_melspec_bwd_runs(14000, 98) == 5, "case `runs`: more than two runs per clip"
    assert hostsim.hostsim_melspec_bwd_runs(88200, 98) == 29 and hostsim.hostsim_melspec_bwd_runs(1025, 98) == 1
    assert hostsim.hostsim_melspec_bwd_run_frames(3073) == 1 and hostsim.hostsim_melspec_bwd_span(3073) == 2048
    assert 2 * hostsim.hostsim_melspec_bwd_lds_bytes() <= 160 * 1024, "two workgroups per CU"


@pytest.mark.parametrize("name", D.CASES)
def test_hostsim_against_the_float64_reference(hostsim, name):
    c = D.case(name)
    pad = D.STRIDE_PAD.get(name, 0)
    d_db, d_pcm, reads = run_hostsim(hostsim, c, pad=pad)
    clips, n = c.pcm.shape
    for which, got in ((0, d_db), (1, d_pcm)):
        e, y = D.err(got, D.reference(name)[which]), D.yardstick(name, which)
        print("case %s %s: err %.3e, float32 restatement %.3e, ratio %.2f" % (name, ("d_db", "d_pcm")[which], e, y, e / y if y else 0.0))
        assert e <= D.YARDSTICK_FACTOR * y
        assert bool(torch.isfinite(got).all())
    assert reads[0] <= c.g.numel() - 1 and reads[1] == d_db.numel() - 1 and reads[3] == d_db.numel() - 1
    assert reads[2] == (clips - 1) * (n + pad) + n - 1, "the last sample of the last row is the highest element read of pcm"


def test_hostsim_large_hop_one_frame_per_run(hostsim):
    """hop > 3072: runs of a single frame whose spans do not touch."""
    base = D.case("runs")
    c = base._replace(hop=4000, n_images=1, image_w=4, stride=0, g=base.g[:, :1, :, :, :4].contiguous())
    d_db, d_pcm, _ = run_hostsim(hostsim, c)
    ref_db, ref_pcm = D.autograd_grads(c, torch.float64)
    y = D.err(D.autograd_grads(c, torch.float32)[1], ref_pcm)
    assert D.err(d_pcm, ref_pcm) <= D.YARDSTICK_FACTOR * y and D.err(d_db, ref_db) == 0.0


def test_hostsim_floor_only_and_silence_are_exact(hostsim):
    c = D.case("floor_only")
    d_db, d_pcm, _ = run_hostsim(hostsim, c)
    assert int((d_db != 0).sum()) == 1, "the gradient is the floor term alone: one cell of d_db"
    flat = int(d_db.abs().argmax())
    clipped = c.g != 0
    assert bool(clipped.any()) and d_db.flatten()[flat] != 0 and bool((d_pcm != 0).any())
    d_db, d_pcm, _ = run_hostsim(hostsim, D.case("floor_only", False))
    assert bool((d_db == 0).all()) and bool((d_pcm == 0).all()), "floor_grad=False: exactly 0"
    d_db, d_pcm, _ = run_hostsim(hostsim, D.case("silence"))
    assert bool((d_pcm == 0).all()), "silence: S = 0 < amin passes nothing, no NaN"
    assert bool((d_db != 0).any()), "nothing is clipped: d_db is the images' gradient"


def test_hostsim_zero_gradient_gives_zeros(hostsim):
    c = D.case("step")
    d_db, d_pcm, _ = run_hostsim(hostsim, c, g=torch.zeros_like(c.g))
    assert bool((d_db == 0).all()) and bool((d_pcm == 0).all())


def test_hostsim_rows_do_not_depend_on_batch_position_strides_or_order(hostsim):
    a, b = D.case("noise"), D.case("step")
    both = a._replace(pcm=torch.cat([a.pcm, b.pcm]), g=torch.cat([a.g, b.g]))
    ref_db, ref_pcm, _ = run_hostsim(hostsim, both, pad=37)
    for pad, d_pad, order, fold_threads in ((0, 0, 0, 0), (5, 11, 0, 0), (37, 0, 1, 0), (0, 3, 1, 64), (37, 0, 0, 1000)):
        d_db, d_pcm, _ = run_hostsim(hostsim, both, pad=pad, d_pad=d_pad, order=order, fold_threads=fold_threads)
        assert torch.equal(d_db, ref_db) and torch.equal(d_pcm, ref_pcm)
    for r in range(3):
        alone = both._replace(pcm=both.pcm[r:r + 1], g=both.g[r:r + 1])
        d_db, d_pcm, _ = run_hostsim(hostsim, alone)
        assert torch.equal(d_db[0], ref_db[r]) and torch.equal(d_pcm[0], ref_pcm[r]), "a row alone"
    swapped = both._replace(pcm=both.pcm.flip(0).contiguous(), g=both.g.flip(0).contiguous())
    d_db, d_pcm, _ = run_hostsim(hostsim, swapped, d_pad=2)
    assert torch.equal(d_db.flip(0), ref_db) and torch.equal(d_pcm.flip(0), ref_pcm), "a row at another position"


def test_argument_errors_are_reported_before_any_launch(L):
    lib = L.lib()
    for sym in ("mla_melspec_bwd_workspace_bytes", "mla_melspec_images_bwd", "mla_melspec_db_bwd"):
        assert sym in L.declared_symbols()
    vp = ctypes.c_void_p
    fake = vp(0x1000)                                    # device pointers: never dereferenced, every call below fails validation first
    E_ARG, E_SHAPE, E_SHORT = -1, -2, -3

    def images(g=fake, db=fake, ws=fake, clips=2, n=4096, hop=98, mels=224, top_db=80.0, n_images=3, w=20, stride=11, out=fake):
        return lib.mla_melspec_images_bwd(g, db, ws, clips, n, hop, mels, top_db, n_images, w, stride, 1, out, None)

    def db_bwd(pcm=fake, clips=2, n=4096, stride=4096, hop=98, mels=224, amin=1e-10, tab=fake, dd=fake, ws=fake, out=fake, d_stride=4096):
        return lib.mla_melspec_db_bwd(pcm, clips, n, stride, hop, mels, amin, tab, dd, ws, out, d_stride, None)

    def expect(code, rc, needle):
        assert rc == code, (rc, lib.mla_last_error())
        assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    for null in ("g", "db", "ws", "out"):
        expect(E_ARG, images(**{null: None}), "null melspec argument")
        expect(E_ARG, images(**{null: vp(0x1002)}), "4-byte aligned")
    for null in ("pcm", "tab", "dd", "ws", "out"):
        expect(E_ARG, db_bwd(**{null: None}), "null melspec argument")
        expect(E_ARG, db_bwd(**{null: vp(0x1002)}), "4-byte aligned")
    for call in (images, db_bwd):
        expect(E_ARG, call(hop=0), "melspec hop 0 < 1")
        expect(E_ARG, call(clips=-1), "melspec clips -1 < 0")
        expect(E_ARG, call(mels=0), "n_mels 0 outside")
        expect(E_SHORT, call(n=1024), "at least 1025 samples")
        assert call(clips=0) == 0
    expect(E_SHORT, db_bwd(n=1024, stride=1024, d_stride=1024), "at least 1025 samples")
    expect(E_SHAPE, images(n_images=4), "images leave the 42-column spectrogram")
    expect(E_SHAPE, images(w=43, n_images=1), "images leave the 42-column spectrogram")
    expect(E_ARG, images(top_db=-1.0), "top_db must be non-negative")
    expect(E_ARG, images(n_images=0), "bad melspec image arguments")
    expect(E_ARG, db_bwd(stride=4095), "clip stride 4095 < n_samples 4096")
    expect(E_ARG, db_bwd(d_stride=4095), "gradient stride 4095 < n_samples 4096")
    expect(E_ARG, db_bwd(amin=0.0), "amin must be positive")
    assert images(clips=0, g=None, db=None, ws=None, out=None) == 0
    assert db_bwd(clips=0, pcm=None, tab=None, dd=None, ws=None, out=None) == 0
    assert lib.mla_melspec_bwd_workspace_bytes(2, 88200, 98, 224) == 2 * 29 * (2048 + 31 * 98) * 4
    assert lib.mla_melspec_bwd_workspace_bytes(2, 88200, 0, 224) == -1 and lib.mla_melspec_bwd_workspace_bytes(-1, 88200, 98, 224) == -1
