#!/usr/bin/env python3
"""Writes tests/golden/bsr_smoothers.npz from the compiled reference (oracle/_ref/libfasp_ref.so) through ctypes: the recorded side of the
tests of the block smoother entries.  The reference's own fasp_smoother_dbsr_* are called as they are on every case of
tests/_bsr_smoother_cases.py; recorded are the inputs b and u of every matrix and the output u of every case.

    python tools/gen_golden_bsr_smoothers.py

While recording, the numpy restatement of the cases module is asserted equal to the reference bit for bit on every case, the inverse
diagonal blocks of the library's host code are asserted equal to the reference's fasp_smoother_dbsr_jacobi_setup on every matrix whose
rows all hold a diagonal block, and the identity / reversed marks are asserted to give the ascending / descending results.  Only data is
written."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _libs  # noqa: E402
import _bsr_smoother_cases as S  # noqa: E402
from faspsolver_amd import _types as T  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def main():
    R = _libs.ref()
    if R is None:
        sys.exit("needs oracle/_ref/libfasp_ref.so (make -C oracle)")
    S.protos(R)
    out = {}
    for name in S.MATRICES:
        ia, ja, val, nb = S.matrix(name)
        if not name.startswith("scaled:"):
            b, u0 = S.inputs(name)
            out[f"{name}/b"], out[f"{name}/u0"] = b, u0
        rows = np.repeat(np.arange(len(ia) - 1), np.diff(ia))
        if len(np.unique(rows[ja == rows])) == len(ia) - 1:
            A, keep = T.as_bsr(ia.copy(), ja.copy(), val.copy(), nb)
            d = np.zeros((len(ia) - 1) * nb * nb)
            R.fasp_smoother_dbsr_jacobi_setup(C.byref(A), T.dp(d))
            assert np.array_equal(bits(d), bits(S.diaginv(name))), name
    for case in S.CASES:
        u = S.call_entry(R, case)
        assert np.array_equal(bits(u), bits(S.restated(case))), case["id"]
        out[case["id"] + "/out"] = u
    for case in S.CASES:
        twin = {"ident": "asc", "rev": "desc"}.get(case["order"])
        if twin:
            other = S._case(case["mat"], case["entry"], twin, case["w"], case["u0"])["id"]
            assert np.array_equal(bits(out[case["id"] + "/out"]), bits(out[other + "/out"])), case["id"]
    np.savez_compressed(S.GOLDEN, **out)
    print("wrote", S.GOLDEN, os.path.getsize(S.GOLDEN), "bytes,", len(S.CASES), "cases on", len(S.MATRICES), "matrices")


if __name__ == "__main__":
    main()
