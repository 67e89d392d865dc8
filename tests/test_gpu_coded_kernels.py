"""The lossless coded CSR kernels -- k_csr_rowpat4, k_csr_rowpat5 (csrc/kernels2.hip.h), the six k_csr_rowpat<OP, LDS_TAB, RPL> and
k_csr_dict8<OP, 8 | 16 | 24> (csrc/kernels.hip.h) -- on the irregular matrices of tests/_csr_cases.py, every row operation, one by one
through fasp_hip_matrix_op, against the CPU oracle's restatement of the reference on the same inputs.

These kernels sum every row left to right, one lane per row, from the exact stored values (the comments in the kernels say so), so the
row results must be BIT-EQUAL to the oracle's -- compared as int64, so that a wrong signed zero shows.  The fused sums (op 7, and op 5
where the kernel forms it) are summed over the kernel's own block layout and are held to the a-priori bound of _libs.sum_bound_ratio
with m = the number of rows, against the np.longdouble sum of the oracle's terms.  *kind_out must be the family the matrix was built
for: a matrix that misses its kernel fails.  Every call is made twice and must repeat itself bit for bit.

What a stencil never reaches and these do is listed with each generator (tests/_csr_cases.py); tests/test_csr_cases.py checks the
generators, the library's coder and the oracle itself without a GPU."""
import ctypes as C

import numpy as np
import pytest

from faspsolver_amd import _types as T

import _csr_cases as cc
from _libs import default_params, oracle, poisson7pt, sum_bound_ratio

pytestmark = pytest.mark.gpu

OPNAME = {v: k for k, v in cc.OPS.items()}


def _protos(L):
    P = C.POINTER
    D = P(C.c_double)
    L.fasp_hip_level_op.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, D, D, D, D, C.c_double, D]
    L.fasp_hip_matrix_op.argtypes = [P(T.dCSRmat), C.c_int, D, D, D, D, C.c_double, D, P(C.c_int)]


def _once(call, nrow, op, x, b, y0, scalar):
    y = y0.copy(); y2 = np.zeros(nrow); red = C.c_double(0)
    st = call(op, T.dp(x), T.dp(b), T.dp(y), T.dp(y2), scalar, C.byref(red) if op in (5, 7) else None)
    assert st == 0, st
    return y, y2, red.value


def _bits(v):
    return np.ascontiguousarray(v).view(np.int64)


def _check(call, c, op, seed, label):
    """One row operation of case c through `call`, twice, against the oracle."""
    nrow, ncol = c["nrow"], c["ncol"]
    scalar = cc.SCALAR.get(op, 0.0)
    x, b, y0 = cc.inputs(nrow, ncol, op, seed, c["inf_rows"])
    want, want2 = cc.reference(oracle(), c, op, x, b, y0, scalar)
    y, y2, red = _once(call, nrow, op, x, b, y0, scalar)
    ya, y2a, reda = _once(call, nrow, op, x, b, y0, scalar)
    assert np.all(np.isfinite(want))
    bad = np.flatnonzero(_bits(y) != _bits(want))
    assert len(bad) == 0, (label, OPNAME[op], len(bad), bad[:8], y[bad[:8]], want[bad[:8]])
    if op == 8:
        bad = np.flatnonzero(_bits(y2) != _bits(want2))
        assert len(bad) == 0, (label, "y2", len(bad), bad[:8], y2[bad[:8]], want2[bad[:8]])
        assert np.array_equal(_bits(y2), _bits(y2a))
    assert np.array_equal(_bits(y), _bits(ya)), (label, OPNAME[op], "the second call differs")
    if op == 7 or (op == 5 and not np.isnan(red)):
        ld = np.longdouble
        terms = want.astype(ld) * b.astype(ld)
        ratio = sum_bound_ratio(np.array([red]), np.array([terms.sum()]), np.array([np.abs(terms).sum()]), np.array([nrow]))
        print(f"{label} {OPNAME[op]}: fused sum {red!r}, error / bound {ratio:.3e}")
        assert ratio <= 1.0, (label, OPNAME[op], red, float(terms.sum()), ratio)
        assert red == reda or (np.isnan(red) and np.isnan(reda))
    if op == 7:
        assert not np.isnan(red)


RUN_OPS = [(run, op) for run in cc.RUNS for op in (run["ops"] or cc.build(run)[0]["ops"])]


@pytest.mark.parametrize("run,op", RUN_OPS, ids=[f"{r['id']}-{OPNAME[o]}" for r, o in RUN_OPS])
def test_coded_kernel_equals_oracle(gpu, run, op):
    L = gpu.lib()
    _protos(L)
    c, kind = cc.build(run)
    A, keep = T.as_csr(c["ia"], c["ja"], c["val"], c["ncol"])
    kinds = []

    def call(op_, *rest):
        k = C.c_int(-1)
        st = L.fasp_hip_matrix_op(C.byref(A), op_, *rest, C.byref(k))
        kinds.append(k.value)
        return st
    try:
        for key, value, _ in run["tune"]:
            assert L.fasp_hip_tune(key.encode(), value) == 0
        _check(call, c, op, 7 * cc.RUNS.index(run) + op, run["id"])
    finally:
        for key, _, default in run["tune"]:
            L.fasp_hip_tune(key.encode(), default)
    assert kinds == [kind, kind], (run["id"], kinds, kind)     # the matrix ran on the kernel it was built for


def test_rectangular_matrix_has_no_smoother(gpu):
    """fasp_hip_matrix_op takes a rectangular matrix as a transfer operator: no diagonal tables, ops 5 and 6 are refused."""
    L = gpu.lib()
    _protos(L)
    c = cc.p5(0)
    A, keep = T.as_csr(c["ia"], c["ja"], c["val"], c["ncol"])
    x, b, y0 = cc.inputs(c["nrow"], c["ncol"], 0, 5)
    for op in (5, 6):
        y = y0.copy(); y2 = np.zeros(c["nrow"])
        assert L.fasp_hip_matrix_op(C.byref(A), op, T.dp(x), T.dp(b), T.dp(y), T.dp(y2), 1.0, None, None) < 0
        assert np.array_equal(y, y0)


def test_coded_operators_of_a_hierarchy_equal_oracle(gpu):
    """P7(20): every operator of every level that runs on a coded kernel (fasp_hip_amg_kernel_info 4, 5, 6, 9), every applicable op
    through fasp_hip_level_op, against the oracle on the host copy of that operator (H.matrix)."""
    L = gpu.lib()
    _protos(L)
    ia, ja, a, f, ue = poisson7pt(20)
    itp, amgp = default_params()
    amgp.smoother = T.SMOOTHER_JACOBI; amgp.relaxation = 0.6667
    H = gpu.AMG(ia, ja, a, amgp)
    try:
        seen = {}
        for level in range(H.num_levels):
            for which in (0, 1, 2):
                if which and level == H.num_levels - 1:
                    continue
                kind, _ = H.kernel_info(level, which)
                if kind not in (4, 5, 6, 9):
                    continue
                nr, nc, mia, mja, mval = H.matrix(level, which)
                c = dict(name=f"P7(20) level {level} operator {which}", nrow=nr, ncol=nc, ia=mia, ja=mja, val=mval, inf_rows=None)
                call = lambda op, *rest: L.fasp_hip_level_op(H.h, level, which, op, *rest)
                for op in (cc.OPS_SQUARE if which == 0 else cc.OPS_RECT):
                    _check(call, c, op, 1000 + 100 * level + 10 * which + op, c["name"])
                assert H.kernel_info(level, which)[0] == kind
                seen[(level, which)] = kind
        print("coded operators of P7(20):", seen)
        assert seen.get((0, 0)) in (5, 6) and len(seen) >= 2
    finally:
        H.close()
