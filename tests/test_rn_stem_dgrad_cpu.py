"""The ResNet stem's data gradient (rn_stem_dgrad_kernel, csrc/resnet_bwd.hip) and the saliency entries of the ResNet branch without
a GPU: the kernel's work items simulated on the host (csrc/rn_stem_dgrad_hostsim.cpp: the tile / halo / tap-map / gather arithmetic
of csrc/rn_stem_dgrad_core.h for every workgroup of a launch) against torch's conv2d_input in float64 with Input's fold applied; one
store per dx element; reads inside every input; independence of the images and of the grid; the tap map at the image borders; the C
entries' argument errors, reported before any launch; the new methods, and the refusals that stay."""

import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

import rn_saliency_cases as C
from conftest import PKG, ROOT

TOL = 1e-4


@pytest.fixture(scope="module")
def L():
    build = importlib.import_module(PKG + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG + "._lib")


@pytest.fixture(scope="module")
def hostsim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rn_stem_dgrad_hostsim") / "rn_stem_dgrad_hostsim.so")
    src = os.path.join(ROOT, PKG, "csrc", "rn_stem_dgrad_hostsim.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, src], check=True)
    lib = ctypes.CDLL(so)
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.hostsim_rn_stem_dgrad.argtypes = [vp, vp, vp, vp, ci, i64, ci, vp, vp, vp]
    lib.hostsim_rn_stem_dgrad_grid.argtypes = [i64]
    return lib


def run_hostsim(hostsim, dy, w, single, y=None, scale=None, grid=0):
    """-> (dx float32 tensor (n, 224, 224), max_read[4] of dy, y, scale, w); asserts one store per element. dx comes in NaN-filled."""
    n = dy.shape[0]
    arrs = [None if t is None else np.ascontiguousarray(t.numpy(), dtype=np.float32) for t in (dy, y, scale, w)]
    dx = np.full((n, 224, 224), np.nan, dtype=np.float32)
    writes = np.zeros((n, 224, 224), dtype=np.int32)
    max_read = np.zeros(4, dtype=np.int64)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)                     # noqa: E731
    rc = hostsim.hostsim_rn_stem_dgrad(p(arrs[0]), p(arrs[1]), p(arrs[2]), p(arrs[3]), int(single), n, grid, p(dx), p(writes), p(max_read))
    assert rc == 0, rc
    assert (writes == 1).all(), "every element of dx is written exactly once"
    return torch.from_numpy(dx), max_read.tolist()


def test_launcher_constants_and_cap(hostsim):
    cap, tiles = hostsim.hostsim_rn_stem_dgrad_max_wg(), hostsim.hostsim_rn_stem_dgrad_tiles()
    assert tiles == 28 and cap >= tiles
    n = cap // tiles + 1                                  # the smallest n at which workgroups take a second trip
    for k in (1, 3, n - 1, n, 1000):
        assert hostsim.hostsim_rn_stem_dgrad_grid(k) == min(k * tiles, cap)
    assert hostsim.hostsim_rn_stem_dgrad_grid(n) == cap < n * tiles


@pytest.mark.parametrize("epilogue", (False, True))
@pytest.mark.parametrize("single", (False, True))
@pytest.mark.parametrize("n", (1, 3))
def test_hostsim_against_conv2d_input_in_float64(hostsim, n, single, epilogue):
    dy, y, scale = C.stem_operands(n)
    w = C.stem_weight()
    if not epilogue:
        y = scale = None
    dx, max_read = run_hostsim(hostsim, dy, w, single, y, scale)
    e = C.rel_max(dx, C.stem_reference(dy, w, single, y, scale))
    print("hostsim n %d single %s epilogue %s: rel_max %.3g" % (n, single, epilogue, e))
    assert e <= TOL
    # the largest index read is the last element of each input, and no more
    assert max_read == [dy.numel() - 1, dy.numel() - 1 if epilogue else -1, 63 if epilogue else -1, w.numel() - 1]


def test_single_differs_from_repeat(hostsim):
    dy, _, _ = C.stem_operands(1)
    w = C.stem_weight()
    assert not torch.equal(run_hostsim(hostsim, dy, w, False)[0], run_hostsim(hostsim, dy, w, True)[0])


def test_hostsim_bf16_values(hostsim):
    dy, y, scale = C.stem_operands(1, bf16=True)
    w = C.stem_weight()
    assert C.rel_max(run_hostsim(hostsim, dy, w, False, y, scale)[0], C.stem_reference(dy, w, False, y, scale)) <= TOL


def test_hostsim_beyond_the_grid_cap(hostsim):
    n = hostsim.hostsim_rn_stem_dgrad_max_wg() // hostsim.hostsim_rn_stem_dgrad_tiles() + 1
    dy = C.stem_operands(1)[0].repeat(n, 1, 1, 1)
    dy[n - 1] = dy[n - 1].flip(0)
    w = C.stem_weight()
    dx, max_read = run_hostsim(hostsim, dy, w, False)
    assert max_read == [dy.numel() - 1, -1, -1, w.numel() - 1]
    assert C.rel_max(dx, C.stem_reference(dy, w, False)) <= TOL
    assert torch.equal(dx[0], run_hostsim(hostsim, dy[:1], w, False)[0][0])


def test_hostsim_does_not_depend_on_the_grid_or_on_n(hostsim):
    dy, y, scale = C.stem_operands(3)
    w = C.stem_weight()
    ref = run_hostsim(hostsim, dy, w, False, y, scale)[0]
    for grid in (1, 5, 28, 1000):
        assert torch.equal(run_hostsim(hostsim, dy, w, False, y, scale, grid)[0], ref)
    assert torch.equal(run_hostsim(hostsim, dy[1:2], w, False, y[1:2], scale)[0][0], ref[1])


@pytest.mark.parametrize("single", (False, True))
def test_one_hot_dy_pins_the_tap_map_at_the_borders(hostsim, single):
    """dy = 1 at output (oy, ox) of channel o paints a[o] into dx rows 2 oy - 3 .. 2 oy + 3: at the four corner outputs the taps that
    fall outside the image are lost (rows / columns 0, 1, 222, 223 keep 4 of 7), in the interior all 49 land."""
    dy = C.one_hot_dy()
    w = C.stem_weight()
    dx = run_hostsim(hostsim, dy, w, single)[0][0]
    a = C.folded_weight(w, single)[:, 0]
    expect = torch.zeros(224, 224, dtype=torch.float64)
    for k, (oy, ox) in enumerate(((0, 0), (0, 111), (111, 0), (111, 111), (57, 30))):
        for ky in range(7):
            for kx in range(7):
                iy, ix = 2 * oy - 3 + ky, 2 * ox - 3 + kx
                if 0 <= iy < 224 and 0 <= ix < 224:
                    expect[iy, ix] += a[7 * k + 3, ky, kx]
    assert int((expect != 0).sum()) == 16 + 20 + 20 + 25 + 49
    assert torch.equal(dx != 0, expect != 0)
    assert C.rel_max(dx, expect) <= 1e-6
    assert C.rel_max(dx, C.stem_reference(dy, w, single)[0]) <= 1e-6


def test_images_are_independent(hostsim):
    dy, y, scale = C.stem_operands(3)
    w = C.stem_weight()
    dy[1] = 0.0
    dx = run_hostsim(hostsim, dy, w, False, y, scale)[0]
    assert not bool(dx[1].any()) and bool(dx[0].any()) and bool(dx[2].any())


def test_argument_errors_are_reported_before_any_launch(L):
    lib = L.lib()
    assert {"mla_rn_stem_dgrad", "mla_rn_act_bwd"} <= set(L.declared_symbols())
    vp = ctypes.c_void_p
    fake = vp(0x1000)                                    # device pointers: never dereferenced, every call below fails validation first
    E_ARG, E_SHAPE, E_DTYPE = -1, -2, -5

    def expect(code, rc, needle):
        assert rc == code, (rc, lib.mla_last_error())
        assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    def stem(dy=fake, n=2, y=fake, scale=fake, w=fake, single=0, dx=fake, dtype=L.F32):
        return lib.mla_rn_stem_dgrad(dy, n, y, scale, w, single, dx, dtype, None)

    for null in ("dy", "w", "dx"):
        expect(E_ARG, stem(**{null: None}), "null")
    expect(E_ARG, stem(y=None), "come together")
    expect(E_ARG, stem(scale=None), "come together")
    expect(E_ARG, stem(n=-1), "n = -1")
    expect(E_ARG, stem(single=2), "single = 2")
    for code in (L.I16, L.BF16X3, L.F64, 9):
        expect(E_DTYPE, stem(dtype=code), "rn_stem_dgrad dtype")
    expect(E_ARG, stem(dy=vp(0x1008)), "16-byte aligned")
    expect(E_ARG, stem(y=vp(0x1008), dtype=L.BF16), "16-byte aligned")
    expect(E_SHAPE, stem(n=2 ** 33), "too many")
    assert stem(n=0) == 0
    assert stem(n=0, dy=None, y=None, scale=None, w=None, dx=None, dtype=L.BF16) == 0

    def act(dy=fake, y=fake, scale=fake, rows=4, channels=64, dpre=fake, dres=fake, dtype=L.F32):
        return lib.mla_rn_act_bwd(dy, y, scale, rows, channels, dpre, dres, dtype, None)

    for null in ("dy", "scale", "dpre"):
        expect(E_ARG, act(**{null: None}), "null")
    for bad in (dict(channels=60), dict(channels=0), dict(rows=-1)):
        expect(E_SHAPE, act(**bad), "multiple of 8")
    expect(E_DTYPE, act(dtype=L.I16), "rn_act_bwd dtype")
    for misaligned in ("dy", "y", "dpre", "dres"):
        expect(E_ARG, act(**{misaligned: vp(0x1008)}), "16-byte aligned")
    expect(E_SHAPE, act(rows=2 ** 40), "too many")
    assert act(rows=0, dy=None, dpre=None, scale=None) == 0


def test_the_new_entries_exist_and_the_old_refusals_stay():
    M = importlib.import_module(PKG + ".model")
    RN = importlib.import_module(PKG + ".resnet")
    ops = importlib.import_module(PKG + ".ops")
    assert callable(RN.trunk_input_backward) and callable(ops.rn_stem_dgrad) and callable(ops.rn_act_bwd)
    conf = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)
    rn = M.Ensemble("repeat", conf, [2, 1], "cpu", slots=2)
    x = torch.zeros(1, 2, 1, 224, 224)
    # refusals that come before the device is touched
    with pytest.raises(RuntimeError, match="saliency_images runs in eval mode only"):
        rn.saliency_images(x)
    rn.eval()
    for bad in (10, -1, True, 2.0, "3", torch.tensor([10]), torch.tensor([0, 1]), torch.tensor([0.0])):
        with pytest.raises(ValueError, match="target"):
            rn.saliency_images(x, target=bad)
    for shape in ((1, 2, 224, 224), (1, 3, 1, 224, 224), (2, 1, 224, 224), (1, 2, 1, 96, 64)):
        with pytest.raises(ValueError, match=r"saliency_images takes \(B, 2, 1, 224, 224\) images"):
            rn.saliency_images(torch.zeros(shape))
    with pytest.raises(ValueError, match="saliency_clips builds the dataset's bags of 10 windows"):
        rn.saliency_clips(torch.zeros(1, 88200))
    vgg = M.Ensemble("repeat", dict(conf, cnn_type="vggish", in_channels=1, just_bottlenecks=False), [2, 1], "cpu").eval()
    with pytest.raises(NotImplementedError, match=r"saliency\(\).*saliency_waveforms\(\)"):
        vgg.saliency_images(torch.zeros(1, 10, 1, 224, 224))
    with pytest.raises(NotImplementedError, match=r"saliency\(\).*saliency_waveforms\(\)"):
        vgg.saliency_clips(torch.zeros(1, 88200))
    # the autograd path stays train-mode only and still ends at the stem's weight gradient: the four refusals keep their text
    for call in (lambda: rn.set_input_grad(True), lambda: rn.cnn.set_input_grad(True), lambda: rn.saliency(torch.zeros(1, 2, 1, 224, 224)),
                 lambda: M.Ensemble("repeat", conf, [2, 1], "cpu", input_grad=True)):
        with pytest.raises(NotImplementedError, match="train-mode BatchNorm only.*stem has no backward-data"):
            call()
