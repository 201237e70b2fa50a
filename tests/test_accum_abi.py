"""rti_fit_accumulate / rti_fit_accum_solve / rti_fit_accum_state_doubles without a GPU: the symbols and their
signatures, the state size, and every argument check, which answers before any HIP call (the pointers below are
never dereferenced)."""
import ctypes

import pytest

import rti
from rti import _lib as L

P_ = ctypes.c_void_p(4096)
I64, INT, VP = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p


def test_symbols_and_signatures():
    lib = rti.load()
    want = {
        "rti_fit_accum_state_doubles": (I64, [INT, I64, INT]),
        "rti_fit_accumulate": (INT, [VP, INT, INT, VP, INT, I64, INT, I64, I64, VP, I64, INT, VP]),
        "rti_fit_accum_solve": (INT, [VP, INT, INT, I64, VP, I64, INT, I64, VP, INT, I64, VP, VP]),
    }
    for name, (res, args) in want.items():
        assert L.SIGNATURES[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.rti_version() == 100


def test_state_doubles():
    f = rti.load().rti_fit_accum_state_doubles
    assert f(6, 549, 3) == 3 * 7 * 549
    assert f(9, 1, 1) == 10 and f(16, 1 << 33, 2) == 2 * 17 * (1 << 33)
    assert f(7, 549, 3) == -1 and f(6, 0, 3) == -1 and f(6, 549, 0) == -1 and f(6, 549, 65536) == -1


def accumulate(R=P_, k=6, B=4, I=P_, dt=L.RTI_F32, P=64, C=1, ls=0, cs=0, state=P_, scs=0, init=1):
    return rti.load().rti_fit_accumulate(R, k, B, I, dt, P, C, ls, cs, state, scs, init, None)


def solve(M=P_, k=6, orth=0, n=20, state=P_, P=64, C=1, scs=0, coef=P_, layout=0, ocs=0, res=None):
    return rti.load().rti_fit_accum_solve(M, k, orth, n, state, P, C, scs, coef, layout, ocs, res, None)


ACC_BAD = {
    "null R": dict(R=None), "null I": dict(I=None), "null state": dict(state=None),
    "B = 0": dict(B=0), "B < 0": dict(B=-3), "P = 0": dict(P=0), "C = 0": dict(C=0), "C > 65535": dict(C=65536),
    "light_stride < P": dict(ls=63),
    "channel_stride < B*light_stride": dict(C=2, cs=4 * 64 - 1),
    "channel_stride < B*light_stride (padded planes)": dict(C=2, ls=70, cs=4 * 64),
    "state_channel_stride < (k+1)*P": dict(C=2, scs=7 * 64 - 1),
}
SOLVE_BAD = {
    "null M": dict(M=None), "null state": dict(state=None), "null coef": dict(coef=None),
    "n_lights = 0": dict(n=0), "n_lights < 0": dict(n=-1), "P = 0": dict(P=0), "C = 0": dict(C=0),
    "C > 65535": dict(C=65536),
    "state_channel_stride < (k+1)*P": dict(C=2, scs=7 * 64 - 1),
    "coef_channel_stride < P*k": dict(C=2, ocs=6 * 64 - 1),
    "layout": dict(layout=2),
}


@pytest.mark.parametrize("case", sorted(ACC_BAD))
def test_accumulate_bad_arguments(case):
    assert accumulate(**ACC_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_fit_accumulate" in rti.load().rti_last_error()


@pytest.mark.parametrize("case", sorted(SOLVE_BAD))
def test_solve_bad_arguments(case):
    assert solve(**SOLVE_BAD[case]) == L.RTI_ERR_BAD_ARG, case
    assert b"rti_fit_accum_solve" in rti.load().rti_last_error()


def test_unsupported():
    lib = rti.load()
    for k in (7, 0, 17):
        assert accumulate(k=k) == L.RTI_ERR_UNSUPPORTED
        assert b"rti_fit_accumulate" in lib.rti_last_error() and b"k=%d" % k in lib.rti_last_error()
        assert solve(k=k) == L.RTI_ERR_UNSUPPORTED
        assert b"rti_fit_accum_solve" in lib.rti_last_error() and b"k=%d" % k in lib.rti_last_error()
    assert accumulate(dt=L.RTI_F64) == L.RTI_ERR_UNSUPPORTED
    assert b"rti_fit_accumulate" in lib.rti_last_error() and b"dtype" in lib.rti_last_error()
    assert accumulate(dt=7) == L.RTI_ERR_UNSUPPORTED


def test_python_names_exist():
    for name in ("FitAccumulator", "fit_chunked", "fit_accumulate_into", "fit_accum_solve_into"):
        assert hasattr(rti, name) and name in rti.__all__
