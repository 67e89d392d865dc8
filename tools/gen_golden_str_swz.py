#!/usr/bin/env python3
"""Writes tests/golden/str_swz.npz from the compiled reference (oracle/_ref/libfasp_ref.so): the recorded side of the structured block
Gauss-Seidel (Schwarz) tests.

    python tools/gen_golden_str_swz.py

Contents, for the seeded cases of tests/_str_swz_cases.py (dominant and weak matrices, nc 1, 2, 3, 5, 7 on 5 x 4 x 3, 9 x 7 x 1 and 1 x 8 x 6,
the neighbour sets geometric / NULL / all absent / far with a point named twice and a self entry, the orders natural / reversed / random /
12-colour / a sequence naming points twice):
  layout            sizeof and member offsets of precond_data_str, from a C program compiled against the reference's headers
  keys              "<matrix>/<neighbours>/<order>"
  sha_u / head      SHA-256 and first 8 doubles of u after one fasp_smoother_dstr_swz sweep
  sha_d / sha_p     SHA-256 of the block of all factors / all pivots fasp_generate_diaginv_block carves its results from
  d_<k>, p_<k>, u_<k>  factors, pivots and u whole for the cases of WHOLE_KEYS, k the index into keys
  stop_d / stop_p   the factors and pivots of the case with one patch that stops
  it_keys / it      "<method>/<neighbours>/<order>" and the iteration count of the reference's fasp_solver_dstr_krylov_blockgs on the upwind
                    9 x 8 x 7 system; it_x_<j>: its solution
Nothing else of the reference is recorded.  While recording, the numpy restatement (factor_all, model_sweep sequential and batched) is held
to the reference bit for bit, and the weak matrices are asserted to interchange rows in at least 90 % of their nc = 1 patches with geometric
neighbours (every patch for nc >= 2 is not asserted, only printed).  On 1 x 8 x 6 with nc > 1 the reference's fasp_blas_dstr_aAxpy leaves its
arrays (BlaSpmvSTR.c:701, :906, :1062), so its sweep is never called there: the factors are the reference's, u is the
restatement's."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _libs  # noqa: E402
import _str_swz_cases as W  # noqa: E402

FIELDS = ("AMG_type", "print_level", "maxit", "max_levels", "tol", "cycle_type", "smoother", "presmooth_iter", "postsmooth_iter",
          "coarsening_type", "relaxation", "coarse_scaling", "mgl_data", "LU", "scaled", "A", "A_str", "SS_str", "diaginv", "pivot", "diaginvS",
          "pivotS", "order", "neigh", "r", "w")


def layout():
    src_text = '#include <stdio.h>\n#include <stddef.h>\n#include "fasp.h"\nint main(void) {\n    printf("%d", (int)sizeof(precond_data_str));\n'
    src_text += "".join(f'    printf(" %d", (int)offsetof(precond_data_str, {f}));\n' for f in FIELDS) + "    return 0;\n}\n"
    inc = os.path.join(_libs.REF_TREE, "base", "include")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write(src_text)
        subprocess.run(["gcc", "-I", inc, src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    return np.array([int(v) for v in out], dtype=np.int32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def main():
    R = _libs.ref()
    if R is None:
        sys.exit("needs oracle/_ref/libfasp_ref.so (make -C oracle)")
    W.protos(R)
    out = {"layout": layout()}
    keys, sha_u, sha_d, sha_p, heads = [], [], [], [], []
    for key, c, grid, nk, ok in W.host_cases():
        neigh, order = W.neigh_of(grid, nk), W.order_of(grid, ok)
        f = W.generate(R, c, neigh)
        fac = W.factor_all(c, neigh)
        d, p = W.packed(fac, c, neigh)
        assert np.array_equal(bits(d), bits(f.d)) and np.array_equal(p, f.p), key
        assert not any(s for _, _, _, s in fac), key
        if key.startswith("weak") and c["nc"] == 1 and nk == "geo":
            assert W.interchanges(fac) >= 0.9 * len(fac), (key, W.interchanges(fac), len(fac))
        if key.startswith("dom"):
            assert W.interchanges(fac) == 0, key
        b, u0 = W.vectors(c)
        us = W.model_sweep(c, neigh, order, fac, b, u0, sequential=True)
        assert np.array_equal(bits(us), bits(W.model_sweep(c, neigh, order, fac, b, u0))), key
        if not (c["nx"] == 1 and c["nc"] > 1):
            u = W.call_swz(R, c, neigh, order, f, b, u0)
            assert np.array_equal(bits(u), bits(us)), key
        assert np.all(np.isfinite(us)), key
        if key in W.WHOLE_KEYS:
            assert d.size <= 40 * W.WHOLE, (key, d.size)
            out[f"d_{len(keys)}"], out[f"p_{len(keys)}"], out[f"u_{len(keys)}"] = f.d, f.p, us
        keys.append(key); sha_u.append(W.digest(us)); sha_d.append(W.digest(f.d)); sha_p.append(W.digest(f.p)); heads.append(us[:W.HEAD].copy())
        print(key, "interchanges", W.interchanges(fac), "of", len(fac))
    # one patch that stops: what the reference leaves
    c = W.stopped_case()
    f = W.generate(R, c, None)
    fac = W.factor_all(c, None)
    d, p = W.packed(fac, c, None)
    assert np.array_equal(bits(d), bits(f.d)) and np.array_equal(p, f.p) and sum(s for _, _, _, s in fac) == 1
    out["stop_d"], out["stop_p"] = f.d, f.p
    # the reference's iteration counts
    c, b = W.scalar_system()
    it_keys, its = [], []
    for mkey, method, restart in W.KRYLOV:
        for nk, ok in W.KRYLOV_SETS:
            grid = (c["nx"], c["ny"], c["nz"])
            st, x = W.solve_blockgs(R, c, b, W.neigh_of(grid, nk), W.order_of(grid, ok), method, restart)
            assert st > 0, (mkey, nk, ok, st)
            out[f"it_x_{len(its)}"] = x
            it_keys.append(f"{mkey}/{nk}/{ok}"); its.append(st)
            print(it_keys[-1], st)
    out.update(keys=np.array(keys), sha_u=np.array(sha_u), sha_d=np.array(sha_d), sha_p=np.array(sha_p), head=np.array(heads),
               it_keys=np.array(it_keys), it=np.array(its, dtype=np.int32))
    np.savez_compressed(W.GOLDEN, **out)
    print("wrote", W.GOLDEN, os.path.getsize(W.GOLDEN), "bytes,", len(keys), "cases")


if __name__ == "__main__":
    main()
