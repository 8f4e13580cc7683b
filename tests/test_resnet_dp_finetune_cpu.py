"""CPU side of data-parallel ResNet-50 trunk finetuning: the two stages of the SyncBN backward (mla_rn_bn_bwd_sums /
mla_rn_bn_bwd_apply) are declared by the header, bound by _lib.py and validate their arguments on the host before any launch;
the Python layers carry the new keywords without touching the defaults."""

import ctypes
import importlib
import inspect

import pytest

from conftest import PKG

NEW = ["mla_rn_bn_bwd_sums", "mla_rn_bn_bwd_apply"]
E_ARG, E_SHAPE, E_DTYPE = -1, -2, -5


@pytest.fixture(scope="module")
def L():
    importlib.import_module(PKG + ".build").build(verbose=False)
    return importlib.import_module(PKG + "._lib")


def test_header_declares_and_lib_binds_both_stages(L):
    declared = L.declared_symbols()
    lib = L.lib()
    for name in NEW:
        assert name in declared, name
        assert getattr(lib, name).argtypes is not None, name
    # x dy y rows channels mean var eps workspace sums dgamma dbeta dtype stream
    assert len(lib.mla_rn_bn_bwd_sums.argtypes) == 14
    # x dy y rows channels mean var gamma eps sums workspace dx dres dtype stream
    assert len(lib.mla_rn_bn_bwd_apply.argtypes) == 15
    # the fused call and its workspace are what they were
    assert len(lib.mla_rn_bn_bwd.argtypes) == 16
    assert lib.mla_rn_bn_bwd_workspace_bytes(256) == 2 * 512 * 256 * 8 + 4 * 256 * 4


def test_argument_errors_are_reported_before_any_launch(L):
    """As tests/test_abi_cpu.py: fake aligned pointers that are never dereferenced, every call fails validation first. The row
    count of stage 2 is the last element of the sums message in DEVICE memory, so a zero count there is out of a host check's
    reach (include/mla_hip.h states it as a precondition); what the host can refuse is a stage 1 with no rows, which is the only
    way a zero count could enter the message."""
    lib = L.lib()
    lib.mla_last_error.restype = ctypes.c_char_p
    vp = ctypes.c_void_p
    fake, odd8, odd4 = vp(0x1000), vp(0x1008), vp(0x1004)

    def expect(code, rc, needle=None):
        assert rc == code, (rc, lib.mla_last_error())
        if needle:
            assert needle in lib.mla_last_error().decode(), lib.mla_last_error()

    def sums(x=fake, dy=fake, y=None, rows=98, ch=256, mean=fake, var=fake, ws=fake, s=fake, dg=None, db=None, dt=None):
        return lib.mla_rn_bn_bwd_sums(x, dy, y, rows, ch, mean, var, 1e-5, ws, s, dg, db, L.F32 if dt is None else dt, None)

    def apply(x=fake, dy=fake, y=None, rows=98, ch=256, mean=fake, var=fake, gamma=fake, s=fake, ws=fake, dx=fake, dres=None, dt=None):
        return lib.mla_rn_bn_bwd_apply(x, dy, y, rows, ch, mean, var, gamma, 1e-5, s, ws, dx, dres, L.F32 if dt is None else dt, None)

    for fn, who in ((sums, "rn_bn_bwd_sums"), (apply, "rn_bn_bwd_apply")):
        expect(E_ARG, fn(s=None), "null " + who)                   # NULL sums
        expect(E_ARG, fn(s=odd4), "aligned")                       # doubles
        expect(E_SHAPE, fn(rows=0), who)                           # no rows: no contribution to the count
        expect(E_SHAPE, fn(rows=-3))
        expect(E_SHAPE, fn(ch=100), "multiple of 64")
        expect(E_ARG, fn(x=None), "null")
        expect(E_ARG, fn(dy=None))
        expect(E_ARG, fn(mean=None))
        expect(E_ARG, fn(var=None))
        expect(E_ARG, fn(ws=None))
        expect(E_ARG, fn(x=odd8), "aligned")
        expect(E_ARG, fn(y=odd8), "aligned")
        expect(E_DTYPE, fn(dt=L.I16))
    expect(E_ARG, apply(gamma=None), "null")
    expect(E_ARG, apply(dx=None), "null")
    expect(E_ARG, apply(dx=odd8), "aligned")
    expect(E_ARG, apply(dres=odd8), "aligned")


def test_keyword_plumbing_keeps_the_defaults():
    TR = importlib.import_module(PKG + ".train")
    RN = importlib.import_module(PKG + ".resnet")
    ops = importlib.import_module(PKG + ".ops")
    p = inspect.signature(TR.TrainStep.__init__).parameters
    assert list(p)[-1] == "trunk_data_parallel" and p["trunk_data_parallel"].default is False
    p = inspect.signature(RN.trunk_backward).parameters
    assert list(p) == ["cnn_model", "tape", "d_feats", "grads", "dist"] and p["dist"].default is None
    assert list(inspect.signature(ops.rn_bn_bwd_sync).parameters) == \
        ["x", "dy", "mean", "var", "bn", "dist", "y", "want_dres", "dgamma", "dbeta"]
    assert not ops._local().bn_active                              # no group: rn_bn_bwd_sync is rn_bn_bwd
