"""The safe-net Krylov entries (fasp_solver_d{csr,bsr,str}_sp*, fasp_solver_dcsr_itsolver_s / _krylov_s) on a machine without a GPU:
they are exported and declared, refuse to run without a device (ERROR_MISC, x untouched: there is no CPU fallback), refuse the solver
types that have no safe text before any work, and the recorded fixture covers what tests/test_gpu_safe_krylov.py relies on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _safe_krylov_cases as K
from _libs import ROOT, T

ENTRIES = [f"fasp_solver_d{fmt}_{m}" for fmt, ms in K.FORMATS.items() for m in ms] + ["fasp_solver_dcsr_itsolver_s", "fasp_solver_dcsr_krylov_s"]


def test_every_safe_entry_is_exported_and_declared(fa):
    assert len(ENTRIES) == 15
    L = fa.lib()
    hdr = open(os.path.join(ROOT, "include", "fasp_hip.h")).read()
    dev = open(os.path.join(ROOT, "include", "fasp_hip_dev.h")).read()
    for sym in ENTRIES:
        assert hasattr(L, sym) and sym in fa.EXPORTS and re.search(r"\b%s\s*\(" % sym, hdr), sym
    assert hasattr(L, "fasp_hip_safe_update_selftest") and re.search(r"\bfasp_hip_safe_update_selftest\s*\(", dev)
    assert fa.SAFE_FORMATS == {k: tuple(v) for k, v in K.FORMATS.items()}


def test_without_a_device_every_entry_returns_error_misc_and_leaves_x(fa):
    if fa.available():
        pytest.skip("a GPU is present")
    L = fa.lib()
    for fmt, methods in K.FORMATS.items():
        for m in methods:
            case = K._case(fmt, m, "p7_5", "diag", 1, "conv")
            st, x, calls = K.run(L, case, print_level=0)
            assert st == T.ERROR_MISC and np.all(x == 0.0) and calls == 0, (fmt, m)
    case = K._case("csr", "spcg", "p7_5", None, 1, "conv")
    st, x, _ = K.run(L, case, print_level=0, via_itsolver=True)
    assert st == T.ERROR_MISC and np.all(x == 0.0)
    S = K.system("csr", "p7_5")
    it = fa.param_solver_init(); it.print_level = 0; it.itsolver_type = T.SOLVER_GMRES
    x = np.zeros(S["n"])
    assert fa.solver_dcsr_krylov_s(S["ia"], S["ja"], S["val"], np.array(S["b"]), x, it) == T.ERROR_MISC and np.all(x == 0.0)


@pytest.mark.parametrize("typ", K.UNKNOWN_TYPES)
def test_itsolver_s_refuses_a_type_without_a_safe_text(fa, typ):
    S = K.system("csr", "p7_5")
    it = fa.param_solver_init(); it.print_level = 0; it.itsolver_type = typ
    x = np.zeros(S["n"])
    with K.Captured() as cap:
        st = fa.solver_dcsr_itsolver_s(S["ia"], S["ja"], S["val"], np.array(S["b"]), x, it)
        st2 = fa.solver_dcsr_krylov_s(S["ia"], S["ja"], S["val"], np.array(S["b"]), x, it)
    assert st == T.ERROR_SOLVER_TYPE and st2 == T.ERROR_SOLVER_TYPE and np.all(x == 0.0)
    assert cap.text.count(f"### ERROR: Unknown iterative solver type {typ}! [fasp_solver_dcsr_itsolver_s]") == 2


def test_the_fixture_covers_every_method_and_format():
    G = np.load(K.GOLDEN)
    keys = [str(k) for k in G["keys"]]
    cases = {c["key"]: c for c in K.cases()}
    assert len(keys) == len(set(keys)) and set(keys) <= set(cases)
    assert np.all(G["sens"] <= K.SENS_MAX) and np.all(G["sens"] >= 0.0)
    rec = {k: (int(G["code"][j]), int(G["restore"][j]), G[f"x_{j}"]) for j, k in enumerate(keys)}
    for k, (code, restore, x) in rec.items():
        assert len(x) == K.system(cases[k]["fmt"], cases[k]["matrix"])["n"] and np.all(np.isfinite(x)), k
    for fmt, methods in K.FORMATS.items():
        for m in methods:
            mine = {k: v for k, v in rec.items() if cases[k]["fmt"] == fmt and cases[k]["method"] == m}
            for pc in (None, "diag"):
                for stop in (1, 2, 3):   # (a) converged solves
                    assert any(cases[k]["kind"] == "conv" and cases[k]["pc"] == pc and cases[k]["stop"] == stop and v[0] > 0 for k, v in mine.items()), (fmt, m, pc, stop)
            nan = [v for k, v in mine.items() if cases[k]["kind"] == "nan"]   # (c)
            assert nan, (fmt, m)
            if m in ("spgmres", "spvgmres"):
                assert all(v[1] == 0 and np.all(v[2] == 0.0) for v in nan), (fmt, m)
            else:   # (b) a MaxIt exit that restores an earlier iterate
                mx = [(cases[k], v) for k, v in mine.items() if cases[k]["kind"] == "maxit"]
                assert mx and all(v[0] == T.ERROR_SOLVER_MAXIT and 0 < v[1] < c["maxit"] for c, v in mx), (fmt, m)
    for k, it in K.PINNED_RESTORES.items():
        assert rec[k][1] == it, k
    assert os.path.getsize(K.GOLDEN) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "amg_swz.npz"))
