"""Host: how many entries of R consecutive rows share an x operand, per level of the P7(n) hierarchy -- entries / distinct columns of
every group of R rows (the whole level, through fasp_hip_rgroup_selftest), in the brick numbering an upload gives the level
(fasp_hip_cluster_order, chunk 262 144) and in the natural order; and what the row-group coding (csrc/kernels5.hip.h) makes of the level:
coded or the rule that refuses it, bytes per entry.   python tools/lab/rgroup_reuse.py [n]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import faspsolver_amd as fa
from faspsolver_amd import _types as T
import _rgroup_cases as RG

n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
L = fa.lib()
P = C.POINTER
ia, ja, a, f, ue = fa.poisson7pt(n)
amgp = fa.param_amg_init(); amgp.smoother = T.SMOOTHER_JACOBI; amgp.relaxation = 0.6667
H = fa.AMG(ia, ja, a, amgp, host_only=True)
L.fasp_hip_cluster_order.argtypes = [P(T.dCSRmat), C.c_int, P(C.c_int)]
L.fasp_hip_permute_csr.argtypes = [P(T.dCSRmat), P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_double)]
ip = lambda q: q.ctypes.data_as(P(C.c_int))
print(f"P7({n}): level, rows, entries per row | reuse R=8, R=16 brick | R=16 natural | coding at R=16 in the brick numbering")
for l in range(H.num_levels - 1):
    nr, nc, lia, lja, lval = H.matrix(l, 0)
    lia = np.array(lia, dtype=np.int32); lja = np.array(lja, dtype=np.int32); lval = np.array(lval, dtype=np.float64)
    if len(lja) < 48 * nr:
        continue
    A, keep = T.as_csr(lia, lja, lval)
    order = np.zeros(nr, np.int32)
    assert L.fasp_hip_cluster_order(C.byref(A), 262144, ip(order)) == 0
    inv = np.zeros(nr, np.int32); inv[order] = np.arange(nr, dtype=np.int32)
    bia = np.zeros(nr + 1, np.int32); bja = np.zeros(len(lja), np.int32); bv = np.zeros(len(lja))
    assert L.fasp_hip_permute_csr(C.byref(A), ip(order), ip(inv), ip(bia), ip(bja), T.dp(bv)) == 0
    reuse = []
    for (xa, xj, xv, rows) in ((bia, bja, bv, 8), (bia, bja, bv, 16), (lia, lja, lval, 16)):
        # (the mean-row rule is not lifted: shorter rows print the rule)
        d, nb, _, _ = RG.selftest(xa, xj, xv, rows=rows, min_reuse=1e-9)
        reuse.append(len(xj) / d["ucols"] if d["coded"] else float("nan"))
    d, nb, _, _ = RG.selftest(bia, bja, bv, rows=16)
    what = f"coded, {nb / len(lja):.2f} bytes per entry" if d["coded"] else f"refused by rule {d['why']}"
    print(f"level {l}: {nr:8d} rows {len(lja) / nr:7.1f} | {reuse[0]:5.2f} {reuse[1]:5.2f} | {reuse[2]:5.2f} | {what}", flush=True)
H.close()
