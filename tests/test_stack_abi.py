"""The light-major stack / coefficient argument contract of every entry point that takes one, without a GPU: each
argument list below has exactly one fault and is refused before any HIP call (the pointers are never dereferenced)
with the status listed and a message that names the entry.  What tests/test_accum_abi.py and
tests/test_robust_abi.py already drive (all of rti_fit_accumulate / rti_fit_accum_solve; rti_fit_shared_robust's
null pointers, N < k, RTI_F64 and layout) is not repeated here.  The apply_operator entries check no channel
stride and write no coefficients, rti_fit_shared_pm has pixel strides of its own, the q8 / h16 entries take u8
only: they get the cases that apply to them."""
import ctypes

import pytest

import rti
from rti import _lib as L

PTR = ctypes.c_void_p(4096)
BAD, UNSUP = L.RTI_ERR_BAD_ARG, L.RTI_ERR_UNSUPPORTED
K, N, P = 6, 20, 64

# entry -> its argument names in ABI order, and the values of a call with no fault (stream None, strides 0 = dense)
STACK = ["I", "dt", "P", "C", "ls", "cs"]
COEF = ["coef", "layout", "ocs"]
ENTRIES = {
    "rti_fit_shared": ["pinv", "k", "N"] + STACK + COEF + ["kernel"],
    "rti_fit_shared_pm": ["pinv", "k", "N"] + STACK + COEF + ["kernel"],
    "rti_fit_residual": ["A", "k", "N"] + STACK + COEF + ["res", "partial"],
    "rti_fit_shared_residual": ["A", "ginv", "k", "N"] + STACK + COEF + ["res", "partial", "kernel"],
    "rti_fit_shared_residual_svd": ["A", "ginv", "k", "N"] + STACK + COEF + ["res", "partial", "kernel"],
    "rti_fit_shared_q8": ["op", "k", "N", "I", "P", "C", "ls", "cs"] + COEF + ["kernel"],
    "rti_fit_shared_h16": ["op", "k", "N", "I", "P", "C", "ls", "cs"] + COEF + ["kernel"],
    "rti_fit_shared_robust": ["A", "k", "N"] + STACK + ["lo", "hi", "min_lights", "iters", "delta"] + COEF
                             + ["res", "kept", "fallback", "kernel"],
    "rti_apply_operator": ["opT", "E", "N", "os"] + STACK + ["out", "odt", "orow", "ocs"],
    "rti_apply_operator_f16": ["op_hi", "op_lo", "Kp", "inv_scale", "E", "N"] + STACK + ["out", "odt", "orow", "ocs"],
}
DEFAULTS = dict(k=K, N=N, P=P, C=1, dt=L.RTI_F32, ls=0, cs=0, layout=0, ocs=0, kernel=0, partial=None, kept=None,
                fallback=None, lo=float("-inf"), hi=float("inf"), min_lights=K, iters=0, delta=0.0, E=8, os=0, Kp=32,
                inv_scale=1.0, odt=L.RTI_F32, orow=0)  # every other argument: the dummy pointer
POINTERS = {
    "rti_fit_shared": ["pinv", "I", "coef"], "rti_fit_shared_pm": ["pinv", "I", "coef"],
    "rti_fit_residual": ["A", "I", "coef", "res"],
    "rti_fit_shared_residual": ["A", "ginv", "I", "coef"], "rti_fit_shared_residual_svd": ["A", "ginv", "I", "coef"],
    "rti_fit_shared_q8": ["op", "I", "coef"], "rti_fit_shared_h16": ["op", "I", "coef"],
    "rti_fit_shared_robust": [],  # tests/test_robust_abi.py
    "rti_apply_operator": ["opT", "I", "out"], "rti_apply_operator_f16": ["op_hi", "op_lo", "I", "out"],
}
OPERATORS = ("rti_apply_operator", "rti_apply_operator_f16")


def cases(entry):
    """{case name: (overrides, status)}"""
    names = ENTRIES[entry]
    out = {f"null {p}": ({p: None}, BAD) for p in POINTERS[entry]}
    out.update({"N = 0": (dict(N=0, min_lights=0), BAD), "P = 0": (dict(P=0), BAD), "C = 0": (dict(C=0), BAD),
                "C = 65536": (dict(C=65536), BAD)})
    if entry not in OPERATORS + ("rti_fit_shared_robust",):
        out["N = k - 1"] = (dict(N=K - 1), BAD)
    if "dt" in names:
        out["dtype 7"] = (dict(dt=7), UNSUP)
        if entry != "rti_fit_shared_robust":
            out["dtype RTI_F64"] = (dict(dt=L.RTI_F64), UNSUP)
    if "layout" in names and entry != "rti_fit_shared_robust":
        out["layout 2"] = (dict(layout=2), BAD)
    if entry != "rti_fit_shared_pm":  # ls / cs are its pixel strides
        out["light_stride = P - 1"] = (dict(ls=P - 1), BAD)
        if entry not in OPERATORS:
            out["channel_stride one short, dense planes"] = (dict(C=2, cs=N * P - 1), BAD)
            out["channel_stride one short, padded planes"] = (dict(C=2, ls=P + 16, cs=N * (P + 16) - 1), BAD)
    if "layout" in names:
        out["coef_channel_stride = P*k - 1"] = (dict(C=2, ocs=P * K - 1), BAD)
    return out


ALL = [(e, c) for e in ENTRIES for c in cases(e)]


@pytest.mark.parametrize("entry,case", ALL, ids=[f"{e}-{c}" for e, c in ALL])
def test_one_fault_is_refused(entry, case):
    lib = rti.load()
    over, status = cases(entry)[case]
    values = {**DEFAULTS, **over}
    args = [values.get(n, PTR) for n in ENTRIES[entry]]  # an overridden pointer is None
    assert len(args) + 1 == len(L.SIGNATURES[entry][1])
    assert getattr(lib, entry)(*args, None) == status, (entry, case, lib.rti_last_error())
    msg = lib.rti_last_error()
    # the two fit + residual entries share one implementation, which reports as rti_fit_shared_residual
    assert (b"rti_fit_shared_residual" if entry == "rti_fit_shared_residual_svd" else entry.encode()) in msg, msg
