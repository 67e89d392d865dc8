#!/usr/bin/env python3
"""Writes tests/golden/str_cases.npz and tests/golden/data/str_5x4x3_nc2.dat from the compiled reference
(oracle/_ref/libfasp_ref.so): the recorded side of the structured-matrix (dSTRmat) tests.

    python tools/gen_golden_str.py

Contents, for the seeded cases of tests/_str_cases.py:
  layout            sizeof and member offsets of dSTRmat and precond_diag_str, from a C program compiled against the reference's headers
  op_keys / op_sha  "<case>/<alpha>" and the SHA-256 of the reference's fasp_blas_dstr_aAxpy result (alpha "mxv": onto a cleared y)
  op_small_*        the results themselves for the cases of at most 420 rows
  csr_sha           SHA-256 of IA | JA | val of the reference's fasp_format_dstr_dcsr
  dinv_*            fasp_precond_dstr_diag results (inverse blocks by fasp_smat_inv)
  solve_*           iteration counts and solutions of the reference's STR solvers (nc = 1) and counts of its BSR solver (nc > 1)
Every product is also held to the numpy restatement of its form (tests/_str_cases.model_aAxpy) while it is recorded.  On a 2D grid with
nx == 1 the reference's block texts (nc > 1) start their middle loop at nx instead of nline (BlaSpmvSTR.c:701, :906, :1062), visit rows
1 .. nline-1 twice and read before the start of the band and of x: nothing is recorded from those calls, the restated form is."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _libs  # noqa: E402
import _str_cases as S  # noqa: E402
from _libs import T  # noqa: E402

LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "fasp.h"
#define O(t, m) (int)offsetof(t, m)
int main(void) {
    printf("%d %d %d %d %d %d %d %d %d %d %d\n", (int)sizeof(dSTRmat), O(dSTRmat, nx), O(dSTRmat, ny), O(dSTRmat, nz), O(dSTRmat, nxy),
           O(dSTRmat, nc), O(dSTRmat, ngrid), O(dSTRmat, diag), O(dSTRmat, nband), O(dSTRmat, offsets), O(dSTRmat, offdiag));
    printf("%d %d %d %d\n", (int)sizeof(precond_diag_str), O(precond_diag_str, nc), O(precond_diag_str, diag), MAT_STR);
    return 0;
}
"""


def layout():
    inc = os.path.join(_libs.REF_TREE, "base", "include")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write(LAYOUT_C)
        subprocess.run(["gcc", "-I", inc, src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    return np.array([int(v) for v in out], dtype=np.int32)


def main():
    R = _libs.ref()
    if R is None:
        sys.exit("needs oracle/_ref/libfasp_ref.so (make -C oracle)")
    S.ref_protos(R)
    out = {"layout": layout()}

    keys, shas, small, small_off, csr = [], [], [], [0], []
    for c in S.op_cases():
        diag, bands = S.build(c)
        x, y0 = S.vectors(c)
        for alpha in S.ALPHAS:
            ym = S.model_aAxpy(c, diag, bands, alpha, x, y0)
            if c["ref_ok"]:
                y = S.ref_aAxpy(R, c, diag, bands, alpha, x, y0)
                assert np.array_equal(y.view(np.uint64), ym.view(np.uint64)), (c["name"], alpha)
            keys.append(f"{c['name']}/{alpha}")
            shas.append(S.digest(ym))
            if ym.size <= 420:
                small.append(ym)
                small_off.append(small_off[-1] + ym.size)
            else:
                small_off.append(small_off[-1])
        A, keep = S.as_str(c, diag, bands)
        B = T.dCSRmat()
        assert R.fasp_format_dstr_dcsr(C.byref(A), C.byref(B)) == 0
        ia, ja, val = T.csr_arrays(B)
        csr.append(np.frombuffer(hashlib.sha256(ia.tobytes() + ja.tobytes() + val.tobytes()).digest(), dtype=np.uint8))
        if c["name"] == "c3d_5x4x3_nc2":
            os.makedirs(os.path.dirname(S.DATA_FILE), exist_ok=True)
            R.fasp_dstr_write(S.DATA_FILE.encode(), C.byref(A))
    out.update(op_keys=np.array(keys), op_sha=np.array(shas), op_small=np.concatenate(small), op_small_off=np.array(small_off),
               csr_names=np.array([c["name"] for c in S.op_cases()]), csr_sha=np.array(csr))

    for nc in S.DINV_NC:
        diag, r = S.dinv_inputs(nc)
        dinv = S.ref_dinv(R, nc, diag)
        z = np.zeros_like(r)
        dd = T.precond_diag_str(nc, T.dvector(dinv.size, T.dp(dinv)))
        R.fasp_precond_dstr_diag(T.dp(r), T.dp(z), C.byref(dd))
        assert np.array_equal(z.view(np.uint64), S.model_dinv_apply(nc, dinv, r).view(np.uint64)), nc
        out[f"dinv_{nc}"], out[f"dinv_z_{nc}"] = dinv, z

    for key, sym, method, restart in S.SCALAR_SOLVES:
        c, diag, bands, b = S.scalar_system(sym)
        for entry in ("krylov", "krylov_diag"):
            it, x = S.solve_with(R, "fasp_solver_dstr_" + entry, c, diag, bands, b, method, restart)
            assert it > 10 and S.true_relres(c, diag, bands, b, x) <= 1.01 * S.TOL, (key, entry, it)
            out[f"solve_{key}_{entry}_it"], out[f"solve_{key}_{entry}_x"] = np.int32(it), x
    c, diag, bands, b = S.scalar_system(True)
    assert np.array_equal(S.ref_dinv(R, 1, diag), 1.0 / diag)   # what the tests hand to fasp_precond_dstr_diag for nc = 1
    for entry, dinv in (("krylov", None), ("krylov_diag", S.ref_dinv(R, 1, diag))):
        it, x = S.minres_with(R, c, diag, bands, b, dinv)
        assert it > 10, it
        out[f"solve_minres_{entry}_it"], out[f"solve_minres_{entry}_x"] = np.int32(it), x
    for nc in S.BLOCK_NC:
        for key, sym, method, restart in S.BLOCK_SOLVES:
            c, diag, bands, b = S.block_system(nc, sym)
            it, x = S.ref_bsr_krylov_diag(R, c, diag, bands, b, method, restart)
            assert 10 <= it <= 30 and S.true_relres(c, diag, bands, b, x) <= 1.01 * S.TOL, (nc, key, it)
            out[f"block_{nc}_{key}_it"] = np.int32(it)

    np.savez_compressed(S.GOLDEN, **out)
    print("wrote", S.GOLDEN, os.path.getsize(S.GOLDEN), "bytes;", S.DATA_FILE, os.path.getsize(S.DATA_FILE), "bytes")


if __name__ == "__main__":
    main()
