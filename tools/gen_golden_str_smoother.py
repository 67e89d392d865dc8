#!/usr/bin/env python3
"""Writes tests/golden/str_smoother.npz from the compiled reference (oracle/_ref/libfasp_ref.so): the recorded side of the
structured-smoother tests.

    python tools/gen_golden_str_smoother.py

Contents, for the seeded cases of tests/_str_smoother_cases.py (every variant and order of ItrSmootherSTR.c, nc 1 .. 7, on 5 x 4 x 3,
9 x 7 x 1 and 1 x 8 x 6):
  keys / sha      "<case>/<variant>" and the SHA-256 of the reference's u after one sweep
  head            the first 8 doubles of each u
  u_<k>           u itself (at most 2000 doubles) for the variants of WHOLE_KEYS, k the index into keys
Nothing else of the reference is recorded.  While recording, the numpy restatement (model_sweep, sequential and batched) is held to the
reference bit for bit; a case at which the reference's text would leave its arrays is to be dropped here and said so (none was found:
the smoothers index bands, vectors and diaginv with the bounds of their own loops at every nc)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _libs  # noqa: E402
import _str_smoother_cases as M  # noqa: E402


def main():
    R = _libs.ref()
    if R is None:
        sys.exit("needs oracle/_ref/libfasp_ref.so (make -C oracle)")
    M.protos(R)
    keys, shas, heads, out = [], [], [], {}
    for key, c, (vkey, entry, kind, order, mark, w, cf) in M.host_cases():
        b, u0 = M.vectors(c)
        dinv = M.dinv_of(R, c)
        u = M.call(R, entry, c, b, u0, order=order, mark=mark, w=w, dinv=dinv)
        for seq in (True, False):
            um = M.model_sweep(c, kind, order, mark, w, dinv, b, u0, cf_entry=cf, sequential=seq)
            assert np.array_equal(u.view(np.uint64), um.view(np.uint64)), (key, seq)
        assert np.all(np.isfinite(u)), key
        if vkey in M.WHOLE_KEYS and u.size <= M.WHOLE:
            out[f"u_{len(keys)}"] = u
        keys.append(key); shas.append(M.digest(u)); heads.append(u[:M.HEAD].copy())
    # the public entries that dispatch (_gs, _gs1, _sor, _sor1) and invert for themselves: the same bits as the order-specific ones
    c = M.grid_case((5, 4, 3), 3)
    b, u0 = M.vectors(c)
    dinv = M.dinv_of(R, c)
    rb = M.red_black((5, 4, 3))
    for name, kw in (("gs", dict(order=M.ASCEND)), ("gs1", dict(order=M.DESCEND, dinv=dinv)), ("sor", dict(order=M.CPFIRST, mark=rb, w=1.1)),
                     ("sor1", dict(order=M.USERDEFINED, mark=M.permutation((5, 4, 3), "random"), w=1.1, dinv=dinv)),
                     ("jacobi1", dict(dinv=dinv)), ("gs", dict(order=7))):
        u = M.call(R, name, c, b, u0, **kw)
        kind = M.JACOBI if name.startswith("jacobi") else M.GS if name.startswith("gs") else M.SOR
        um = M.model_sweep(c, kind, kw.get("order"), kw.get("mark"), kw.get("w"), dinv, b, u0)
        assert np.array_equal(u.view(np.uint64), um.view(np.uint64)), name
    out.update(keys=np.array(keys), sha=np.array(shas), head=np.array(heads))
    np.savez_compressed(M.GOLDEN, **out)
    print("wrote", M.GOLDEN, os.path.getsize(M.GOLDEN), "bytes,", len(keys), "cases")


if __name__ == "__main__":
    main()
