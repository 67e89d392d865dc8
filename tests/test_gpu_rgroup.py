"""k_csr_rgroup (csrc/kernels5.hip.h): groups of 16 (or 8) consecutive rows walked over the union of their columns, one gather of x per
union column -- through fasp_hip_matrix_op with fasp_hip_tune("rgroup", 2) against the kernel the plan picks without it ("rgroup", 0)
and against a numpy left-to-right row sum, for every row operation the kernel serves and weighted Jacobi with two weights.

The matrices (tests/_rgroup_cases.py) hold the shapes that can go wrong: a row count that is no multiple of the group; unions of exactly
64, 65 and 1 columns; a union of fewer chunks than the group has waves; empty rows inside a group; a row whose entries all lie in the last
chunk; a column all rows of a group hold and one a single row holds; signed zeros; a group that spans exactly 65 535 columns.

Tolerance: a row sum in any fixed order agrees with the left-to-right sum to 1e-13 of the row's absolute sum (the bar of
tests/test_gpu_estream.py); an operation that adds b_i or the old y_i rounds that sum once more, a sweep divides it by the diagonal.
The numpy reference alone meets the bar against exactly rounded sums: tests/test_rgroup_coding.py."""
import ctypes as C

import numpy as np
import pytest

import _rgroup_cases as RG
from _libs import T

pytestmark = pytest.mark.gpu

CK_RGROUP = {(16, 4): 29, (16, 8): 30, (8, 4): 31, (8, 8): 32, (16, 2): 33, (8, 2): 34}   # kernel codes of fasp_hip_csr_plan2
OPS = ("y = A x", "y = b - A x", "y += A x", "y -= A x", "y += s A x", "Jacobi", "L1", None, "y = A x with the next level's first sweep")


def _setup(L):
    P = C.POINTER
    L.fasp_hip_matrix_op.argtypes = [P(T.dCSRmat), C.c_int, T.c_double_p, T.c_double_p, T.c_double_p, T.c_double_p, C.c_double, T.c_double_p, P(C.c_int)]
    L.fasp_hip_matrix_traits2.argtypes = [P(T.dCSRmat), P(C.c_int)]
    L.fasp_hip_csr_plan2.argtypes = [P(C.c_int), C.c_int, C.c_int, C.c_int, P(C.c_int), P(C.c_double)]


def _op(L, A, op, x, b, y0, scalar):
    y = y0.copy(); y2 = np.full(len(y0), np.nan)
    kind = C.c_int(-1)
    assert L.fasp_hip_matrix_op(C.byref(A), op, T.dp(x), T.dp(b), T.dp(y), T.dp(y2), scalar, None, C.byref(kind)) == 0
    assert kind.value == 0       # the family stays that of k_csr_rows / k_csr_estream
    return y, y2


def _kernel(L, A, op):
    t = (C.c_int * 32)(); out = (C.c_int * 11)(); nb = C.c_double(0)
    assert L.fasp_hip_matrix_traits2(C.byref(A), t) == 0
    assert L.fasp_hip_csr_plan2(t, op, 0, 0, out, C.byref(nb)) == 0
    return out[0], t[28], nb.value


def _reference(ia, ja, val, x, b, y0, l1):
    """-> per op (expected, tolerance) from the left-to-right sums"""
    n = len(ia) - 1
    s, rowabs = RG.row_sums_left_to_right(ia, ja, val, x)
    so, _ = RG.row_sums_left_to_right(ia, ja, val, x, skip_diag=True)
    rows = np.repeat(np.arange(n), np.diff(ia))
    d = np.zeros(n)
    hit = ja == rows
    d[rows[hit]] = val[hit]
    ok = np.abs(d) > 1e-20
    dd = np.where(ok, d, 1.0)
    ref = {0: (s, 1e-13 * rowabs), 1: (b - s, 1e-13 * (rowabs + np.abs(b))), 2: (y0 + s, 1e-13 * (rowabs + np.abs(y0))),
           3: (y0 - s, 1e-13 * (rowabs + np.abs(y0))), 4: (y0 + s * 0.7, 1e-13 * (rowabs + np.abs(y0)))}
    for w in (0.6667, 1.3):
        xn = np.where(ok, (1 - w) * x + w * (b - so) / dd, x)
        ref[(5, w)] = (xn, 1e-13 * (w * (rowabs + np.abs(b)) / np.abs(dd) + np.abs(xn)))
    okl = np.abs(l1) > 1e-20
    ll = np.where(okl, l1, 1.0)
    xl = np.where(okl, x + (b - s) / ll, x)
    ref[6] = (xl, 1e-13 * ((rowabs + np.abs(b)) / ll + np.abs(xl)))
    return ref, rowabs


def _run_all(L, ia, ja, val, ops, rows, waves, expect_coded=True):
    n = len(ia) - 1
    A, keep = T.as_csr(ia, ja, val)
    rng = np.random.default_rng(17)
    x = rng.standard_normal(n); b = rng.standard_normal(n); y0 = rng.standard_normal(n)
    l1 = np.add.reduceat(np.abs(val), ia[:-1].astype(np.int64)) * (np.diff(ia) > 0) if len(val) else np.zeros(n)
    l1 = np.where(np.diff(ia) > 0, l1, 0.0)
    ref, rowabs = _reference(ia, ja, val, x, b, y0, l1)
    got = {}
    try:
        L.fasp_hip_tune(b"rgroup_rows", rows); L.fasp_hip_tune(b"rgroup_waves", waves)
        for rg in (2, 0):
            L.fasp_hip_tune(b"rgroup", rg)
            kernel, has_copy, nbytes = _kernel(L, A, 0)
            if rg == 2 and expect_coded:
                assert has_copy == 1 and kernel == CK_RGROUP[(rows, waves)] and nbytes < 10.0 * len(ja)
            else:
                assert has_copy == 0 and kernel < 29
            for op in ops:
                for w in ((0.6667, 1.3) if op == 5 else (0.7,)):
                    key = (5, w) if op == 5 else op
                    y, y2 = _op(L, A, op, x, b, y0, w)
                    got[(rg, key)] = y
                    if op == 8:
                        want, tol = ref[0]
                        # y2_i = scalar y_i / b_i: the fused first Jacobi sweep of the next level, from the stored result
                        assert np.array_equal(y2, np.where(np.abs(b) > 1e-20, (1 - w) * 0.0 + w * y / b, 0.0)), (rg, op)
                    else:
                        want, tol = ref[key]
                    err = np.abs(y - want)
                    print(f"rgroup {rg} R {rows} W {waves} {OPS[op]} {w if op == 5 else ''}: max err / tolerance {np.max(err / np.maximum(tol, 1e-300)):.3f}")
                    assert np.all(err <= tol + 1e-300), (rg, key)
                    if op == 0:
                        assert np.all(y[np.diff(ia) == 0] == 0.0)
                        y_again, _ = _op(L, A, op, x, b, y0, w)
                        assert np.array_equal(y, y_again), rg        # bit-reproducible from run to run
    finally:
        L.fasp_hip_tune(b"rgroup", 1); L.fasp_hip_tune(b"rgroup_rows", 0); L.fasp_hip_tune(b"rgroup_waves", 0)
    return got, ref


@pytest.mark.parametrize("rows,waves", [(16, 4), (16, 8), (8, 4), (8, 8), (16, 2), (8, 2)])
def test_every_operation_on_the_banded_matrix(gpu, rows, waves):
    L = gpu.lib()
    _setup(L)
    ia, ja, val = RG.banded()
    got, ref = _run_all(L, ia, ja, val, (0, 1, 2, 3, 4, 5, 6, 8), rows, waves)
    for (rg, key), y in got.items():     # new kernel against the old one: two fixed orders of the same sums
        if rg == 2:
            tol = ref[0 if key == 8 else key][1]
            assert np.all(np.abs(y - got[(0, key)]) <= 2 * tol + 1e-300), key


def test_group_spanning_65535_columns(gpu):
    L = gpu.lib()
    _setup(L)
    ia, ja, val = RG.wide(65535)
    _run_all(L, ia, ja, val, (0, 5), 16, 4)


def test_refused_matrix_runs_the_old_kernel_with_identical_output(gpu):
    L = gpu.lib()
    _setup(L)
    ia, ja, val = RG.scattered()
    got, ref = _run_all(L, ia, ja, val, (0, 1, 2, 3, 4, 5, 6, 8), 16, 4, expect_coded=False)
    for (rg, key), y in got.items():
        if rg == 2:
            assert np.array_equal(y, got[(0, key)]), key


def test_p7_64_solve_with_and_without_row_groups(gpu):
    """The whole solve: level 4 of P7(64) (1 980 rows of 166 entries) takes the row-group kernel for its residuals and sweeps.  Equal
    iteration counts, final relative residuals within the project's bar (1e-10 absolute, 1e-6 relative), one cycle to 1e-13."""
    from _libs import default_params
    ia, ja, a, f, ue = gpu.poisson7pt(64)
    itp, amgp = default_params()
    itp.tol = 1e-8
    amgp.smoother = T.SMOOTHER_JACOBI; amgp.relaxation = 0.6667
    L = gpu.lib()
    r = np.random.default_rng(7).standard_normal(len(f))
    try:
        # (16 rows per group: level 4 is too small to be renumbered, and groups of 8 of its rows in the natural order share too little)
        L.fasp_hip_tune(b"rgroup", 2); L.fasp_hip_tune(b"rgroup_rows", 16)
        H = gpu.AMG(ia, ja, a, amgp)          # (the copy is built at upload, the key is read again at every launch)
        z2 = H.precond(r)
        st2, x2, h2, s2 = H.solve(f, itp)
        L.fasp_hip_tune(b"rgroup", 0)
        z0 = H.precond(r)
        st0, x0, h0, s0 = H.solve(f, itp)
    finally:
        L.fasp_hip_tune(b"rgroup", 1); L.fasp_hip_tune(b"rgroup_rows", 0)
    H.close()
    print(f"rgroup 2: {st2} iterations, relres {s2.relres:.10e}; rgroup 0: {st0} iterations, relres {s0.relres:.10e}; cycle differs by {np.abs(z2 - z0).max() / np.abs(z0).max():.2e}")
    assert not np.array_equal(z2, z0)           # another kernel did run
    assert st2 == st0 and st0 > 0
    assert abs(s2.relres - s0.relres) <= 1e-10 and abs(s2.relres - s0.relres) <= 1e-6 * s0.relres
    assert np.abs(z2 - z0).max() <= 1e-13 * np.abs(z0).max()
    assert np.abs(x2 - x0).max() <= 1e-10 * np.abs(x0).max()
