#!/usr/bin/env python3
"""Writes tests/golden/safe_krylov.npz from the compiled reference (oracle/_ref/libfasp_ref.so) through ctypes: the recorded side of the
tests of the safe-net Krylov solvers.  The reference's fasp_solver_d{csr,bsr,str}_sp* and fasp_solver_dcsr_itsolver_s are called as they
are, on the cases of tests/_safe_krylov_cases.py.

    python tools/gen_golden_safe_krylov.py

Contents:
  keys                 the keys of the cases that qualify, in the order of the arrays below
  code, restore, sens  per case: the reference's return code; the iteration of its "Restore iteration" line (-1: none printed); the
                       max-norm distance, relative to max|x|, between its x and its x for perturbed(b) (1 + 1e-14 xi per entry)
  x_<j>                the reference's x of case j
A case qualifies only when both runs give the same code and the same restore line and sens <= SENS_MAX.  A structured case with nc = 3 goes
through the reference as the scalar CSR matrix of the same entries (reference_case).  While recording, the coverage the tests rely on is
asserted per method and format, the CSR cases are repeated through fasp_solver_dcsr_itsolver_s (the same bits), the unknown solver types
are checked to be refused, and the pinned restore iterations are checked.  Only data is written."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _libs  # noqa: E402
import _safe_krylov_cases as K  # noqa: E402
from faspsolver_amd import _types as T  # noqa: E402


def record(R, case):
    rc = K.reference_case(case)
    S = K.system(rc["fmt"], rc["matrix"])
    with K.Captured() as c1:
        st1, x1, _ = K.run(R, rc)
    with K.Captured() as c2:
        st2, x2, _ = K.run(R, rc, b=K.perturbed(S["b"], case["key"]))
    r1, r2 = K.restore_iteration(c1.text), K.restore_iteration(c2.text)
    mx = float(np.max(np.abs(x1)))
    sens = float(np.max(np.abs(x1 - x2))) / mx if mx > 0 else float(np.max(np.abs(x2)))
    ok = st1 == st2 and r1 == r2 and np.isfinite(sens) and sens <= K.SENS_MAX
    if ok and rc["fmt"] == "csr":   # the dispatcher reaches the same text
        with K.Captured():
            st3, x3, _ = K.run(R, rc, via_itsolver=True)
        assert st3 == st1 and np.array_equal(x3.view(np.uint64), x1.view(np.uint64)), case["key"]
    return ok, st1, r1, sens, x1


def check_coverage(cases, kept):
    """Per method and format: converged solves with and without the preconditioner under every stop type, the NaN case with a finite x,
    and, for the three methods with an iteration-wise safety net, a MaxIt exit that restores an earlier iterate."""
    have = {c["key"]: (c, v) for c, v in zip(cases, kept) if v is not None}
    for fmt, methods in K.FORMATS.items():
        for m in methods:
            mine = [(c, v) for c, v in have.values() if c["fmt"] == fmt and c["method"] == m]
            for pc in (None, "diag"):
                for stop in (1, 2, 3):
                    assert any(c["kind"] == "conv" and c["pc"] == pc and c["stop"] == stop and v[0] > 0 for c, v in mine), (fmt, m, pc, stop)
            nan = [v for c, v in mine if c["kind"] == "nan"]
            assert nan and all(np.all(np.isfinite(v[3])) for v in nan), (fmt, m)
            if m in ("spgmres", "spvgmres"):
                assert all(v[1] == 0 for v in nan), (fmt, m)          # restores iteration 0
            else:
                mx = [v for c, v in mine if c["kind"] == "maxit"]
                assert mx and all(v[0] == T.ERROR_SOLVER_MAXIT and 0 < v[1] < c["maxit"] for c, v in mine if c["kind"] == "maxit"), (fmt, m)
    for key, it in K.PINNED_RESTORES.items():
        assert have[key][1][1] == it, (key, have[key][1][1])
    for name in ("p7_5", "p7_11"):
        assert sum(c["matrix"] == name for c, _ in have.values()) == len(K.METHODS), name


def check_unknown_types(R):
    S = K.system("csr", "p7_5")
    A, keep = K.as_matrix(S)
    for typ in K.UNKNOWN_TYPES:
        x = np.zeros(S["n"])
        bv, _ = T.as_vec(np.array(S["b"]))
        xv = T.dvector(len(x), T.dp(x))
        it = T.ITS_param()
        it.print_level = 0; it.itsolver_type = typ; it.stop_type = 1; it.restart = 20; it.maxit = 100; it.tol = K.TOL
        with K.Captured() as cap:
            st = R.fasp_solver_dcsr_itsolver_s(C.byref(A), C.byref(bv), C.byref(xv), None, C.byref(it))
        assert st == T.ERROR_SOLVER_TYPE and np.all(x == 0.0) and "Unknown iterative solver type" in cap.text, typ


def main():
    R = _libs.ref()
    assert R is not None, "oracle/_ref/libfasp_ref.so is missing (make -C oracle all)"
    K.set_protos(R)
    cases = K.cases()
    kept = []
    for c in cases:
        ok, st, rest, sens, x = record(R, c)
        kept.append((st, rest, sens, x) if ok else None)
        print(f"{c['key']:50s} code {st:4d} restore {rest:3d} sens {sens:.2e}{'' if ok else '   -- does not qualify'}")
    check_coverage(cases, kept)
    check_unknown_types(R)
    sel = [(c, v) for c, v in zip(cases, kept) if v is not None]
    out = dict(keys=np.array([c["key"] for c, _ in sel]), code=np.array([v[0] for _, v in sel], dtype=np.int32),
               restore=np.array([v[1] for _, v in sel], dtype=np.int32), sens=np.array([v[2] for _, v in sel]))
    for j, (_, v) in enumerate(sel):
        out[f"x_{j}"] = v[3]
    np.savez_compressed(K.GOLDEN, **out)
    print(f"wrote {K.GOLDEN}: {len(sel)} of {len(cases)} cases, {os.path.getsize(K.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
