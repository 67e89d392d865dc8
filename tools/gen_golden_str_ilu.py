#!/usr/bin/env python3
"""Writes tests/golden/str_ilu.npz from the compiled reference (oracle/_ref/libfasp_ref.so): the recorded side of the structured-ILU
tests.

    python tools/gen_golden_str_ilu.py

Contents, for the seeded cases of tests/_str_ilu_cases.py:
  fact_keys / fact_sha   "<case>/<lfil>" and the SHA-256 of diag | bands of the reference's fasp_ilu_dstr_setup0 / _setup1
  fact_<case>_<lfil>     the factor itself (diag | bands) where it has at most 2000 doubles
  apply_<case>_<lfil>    z of fasp_precond_dstr_ilu0 / _ilu1 on the case's right-hand side: the reference's for nc = 1, 2, 4, 6, the numpy
                         restatement's (tests/_str_ilu_cases.model_apply) for nc = 3, 5, 7, whose reference texts run out of their arrays
  solve_<key>_<lfil>_it / _x     the reference's fasp_solver_dstr_krylov_ilu, nc = 1
  block_<nc>_<key>_it            the reference's fasp_solver_dbsr_krylov_ilu, ILU(0), on fasp_format_dstr_dbsr(A), nc = 2, 3 (nc = 5: the
                                 structured factor is another one -- fasp_ilu_dstr_setup0 inverts with fasp_smat_inv_nc5 -- nothing recorded)
While recording, the restatement is held to the reference at nc = 1, 2, 4, 6; every scalar solve must keep its true relative residual a
factor MARGIN away from the tolerance at the reference's last step and at the one before (so that a rounding-level difference in a
reduction cannot move the count); the block factor of the BSR path must agree with the structured one to rounding (one application)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _libs  # noqa: E402
import _str_cases as S  # noqa: E402
import _str_ilu_cases as I  # noqa: E402
from _libs import T  # noqa: E402

P = C.POINTER


def bsr_protos(R):
    R.fasp_format_dstr_dbsr.argtypes = [P(T.dSTRmat)]
    R.fasp_format_dstr_dbsr.restype = T.dBSRmat
    R.fasp_solver_dbsr_krylov_ilu.argtypes = [P(T.dBSRmat), P(T.dvector), P(T.dvector), P(T.ITS_param), P(T.ILU_param)]
    R.fasp_solver_dbsr_krylov_ilu.restype = C.c_int
    R.fasp_ilu_dbsr_setup.argtypes = [P(T.dBSRmat), P(T.ILU_data), P(T.ILU_param)]
    R.fasp_ilu_dbsr_setup.restype = C.c_short
    R.fasp_precond_dbsr_ilu.argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
    R.fasp_precond_dbsr_ilu.restype = None
    return R


def main():
    R = _libs.ref()
    if R is None:
        sys.exit("needs oracle/_ref/libfasp_ref.so (make -C oracle)")
    I.protos(R)
    bsr_protos(R)
    out = {}
    keys, shas = [], []
    for key, c, lfils in I.host_cases():
        for lfil in lfils:
            snap = I.factor(R, c, lfil)
            assert snap is not None, (key, lfil)
            raw = I.factor_bytes(snap)
            keys.append(f"{key}/{lfil}")
            shas.append(I.digest(raw))
            if len(raw) // 8 <= I.WHOLE:
                out[f"fact_{key}_{lfil}"] = np.frombuffer(raw, dtype=np.float64).copy()
            if (c["nx"], c["ny"], c["nz"]) in I.APPLY_GRIDS and not key.endswith("_swap"):
                r = I.rhs(c)
                zm = I.model_apply(snap, lfil, r)
                if c["nc"] in I.REF_APPLY_OK:
                    z = I.host_apply(R, snap, lfil, r)
                    assert np.array_equal(z.view(np.uint64), zm.view(np.uint64)), (key, lfil)
                out[f"apply_{key}_{lfil}"] = zm
    out.update(fact_keys=np.array(keys), fact_sha=np.array(shas))

    for key, sym, method, restart in I.SCALAR_SOLVES:
        c, b = I.scalar_system(sym)
        for lfil in (0, 1):
            it, x = I.solve_ilu(R, c, b, method, restart, lfil)
            rr = I.true_relres(c, b, x)
            st1, x1 = I.solve_ilu(R, c, b, method, restart, lfil, maxit=it - 1)   # the iterate before the last one
            rr1 = I.true_relres(c, b, x1)
            print(f"{key} ILU({lfil}): {it} iterations, true relative residual {rr:.3e}, one step earlier {rr1:.3e}")
            assert it > 3 and rr * I.MARGIN <= I.TOL and rr1 >= I.TOL * I.MARGIN, (key, lfil, it, rr, rr1)
            out[f"solve_{key}_{lfil}_it"], out[f"solve_{key}_{lfil}_x"] = np.int32(it), x

    for nc in I.BLOCK_NC:
        for key, sym, method, restart in I.BLOCK_SOLVES:
            c, b = I.block_system(nc, sym)
            A, keep = I.as_str(c)
            B = R.fasp_format_dstr_dbsr(C.byref(A))
            # the BSR path's ILU(0) of the converted matrix is mathematically the structured ILU(0): one application agrees to rounding
            d = T.ILU_data()
            assert R.fasp_ilu_dbsr_setup(C.byref(B), C.byref(d), C.byref(I.ilu_param(0))) == 0
            r = I.rhs(c)
            zb = np.zeros_like(r)
            R.fasp_precond_dbsr_ilu(T.dp(r.copy()), T.dp(zb), C.cast(C.byref(d), C.c_void_p))
            zs = I.model_apply(I.factor(R, c, 0), 0, r)
            agree = np.max(np.abs(zb - zs)) <= 1e-12 * np.max(np.abs(zs))
            assert agree == (nc in I.BLOCK_COUNT_NC), (nc, key, np.max(np.abs(zb - zs)))
            if not agree:   # nc = 5: fasp_ilu_dstr_setup0 inverts with the 5 x 5 closed form, whose result is not the inverse
                print(f"nc {nc} {key}: the structured and the BSR factor differ (max |dz| {np.max(np.abs(zb - zs)):.2e}): no count recorded")
                continue
            x = np.zeros_like(b)
            bv, kb = T.as_vec(b)
            xv = T.dvector(x.size, T.dp(x))
            it = R.fasp_solver_dbsr_krylov_ilu(C.byref(B), C.byref(bv), C.byref(xv), C.byref(S.its_param(method, restart)), C.byref(I.ilu_param(0)))
            rr = I.true_relres(c, b, x)
            print(f"nc {nc} {key}: reference BSR ILU(0) {it} iterations, true relative residual {rr:.3e}")
            assert it > 2 and rr <= 1.01 * I.TOL, (nc, key, it, rr)
            out[f"block_{nc}_{key}_it"] = np.int32(it)

    np.savez_compressed(I.GOLDEN, **out)
    print("wrote", I.GOLDEN, os.path.getsize(I.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
