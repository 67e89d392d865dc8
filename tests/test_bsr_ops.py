"""Block (BSR) operators of config 3: dBSRmat SpMV / aAxpy / inverse diagonal blocks / block
Jacobi.  CPU: oracle vs the reference build (bit-exact).  GPU: HIP kernels vs the oracle --
bit-exact too, the kernel evaluates every block row in the reference's order."""
import ctypes as C

import numpy as np
import pytest

from _libs import (DATA, RAGGED_SHAPES, SOR_WEIGHTS, T, bsr_mxv_bound_ratio, bsr_tile, orc_bsr_ops, orc_diaginv,
                   poisson7pt_bsr, ragged_bsr, ragged_case, read_bsr, read_vec, ref, wide_bsr)


def _cases():
    return {"spe01": lambda: read_bsr(DATA + "/bsrmat_SPE01.dat"),
            "p7x3_8": lambda: poisson7pt_bsr(8),
            "p7x2_6": lambda: poisson7pt_bsr(6, np.array([[2.0, -1.0], [0.5, 3.0]])),
            "p7x1_7": lambda: poisson7pt_bsr(7, np.array([[1.5]])),
            "p7x5_5": lambda: poisson7pt_bsr(5, np.arange(25, dtype=float).reshape(5, 5) / 7 + np.eye(5) * 9)}


_orc_setup = orc_bsr_ops


@pytest.mark.ref
@pytest.mark.parametrize("case", ["spe01", "p7x3_8", "p7x2_6", "p7x1_7", "p7x5_5"])
def test_oracle_bsr_ops_vs_reference(case):
    R = ref()
    if R is None:
        pytest.skip("oracle/_ref not available")
    o = _orc_setup()
    ia, ja, val, nb = _cases()[case]()
    A, keep = T.as_bsr(ia, ja, val, nb)
    n = A.ROW * nb
    rng = np.random.default_rng(5)
    x = rng.standard_normal(n); y0 = rng.standard_normal(n)
    R.fasp_blas_dbsr_mxv.argtypes = [C.POINTER(T.dBSRmat), T.c_double_p, T.c_double_p]
    R.fasp_blas_dbsr_aAxpy.argtypes = [C.c_double, C.POINTER(T.dBSRmat), T.c_double_p, T.c_double_p]
    y1 = np.zeros(n); y2 = np.ones(n)
    o.orc_bsr_mxv(C.byref(A), T.dp(x), T.dp(y1)); R.fasp_blas_dbsr_mxv(C.byref(A), T.dp(x), T.dp(y2))
    assert np.array_equal(y1, y2)
    for alpha in (1.0, -1.0, 0.3):
        y1 = y0.copy(); y2 = y0.copy()
        o.orc_bsr_aAxpy(alpha, C.byref(A), T.dp(x), T.dp(y1)); R.fasp_blas_dbsr_aAxpy(alpha, C.byref(A), T.dp(x), T.dp(y2))
        assert np.array_equal(y1, y2)
    if nb <= 3:
        R.fasp_dbsr_getdiaginv.argtypes = [C.POINTER(T.dBSRmat)]
        R.fasp_dbsr_getdiaginv.restype = T.dvector
        dr = R.fasp_dbsr_getdiaginv(C.byref(A))
        d_ref = np.ctypeslib.as_array(dr.val, (dr.row,)).copy()
        dp_ = o.orc_bsr_getdiaginv(C.byref(A))
        d_orc = np.ctypeslib.as_array(dp_, (A.ROW * nb * nb,)).copy()
        o.orc_free(dp_)
        assert np.array_equal(d_ref, d_orc)
        R.fasp_smoother_dbsr_jacobi1.argtypes = [C.POINTER(T.dBSRmat), C.POINTER(T.dvector), C.POINTER(T.dvector), T.c_double_p]
        b = rng.standard_normal(n)
        u1 = x.copy(); u2 = x.copy()
        o.orc_bsr_jacobi1(C.byref(A), T.dp(b), T.dp(u1), T.dp(d_orc))
        bv = T.dvector(n, T.dp(b)); uv = T.dvector(n, T.dp(u2))
        R.fasp_smoother_dbsr_jacobi1(C.byref(A), C.byref(bv), C.byref(uv), T.dp(d_ref))
        assert np.array_equal(u1, u2)


@pytest.mark.ref
@pytest.mark.parametrize("shape", list(RAGGED_SHAPES))
@pytest.mark.parametrize("nb", range(1, 8))
def test_oracle_ragged_bsr_vs_reference(nb, shape):
    """The reference's fasp_blas_dbsr_mxv / _aAxpy are unrolled per nb and per row length, its sweeps per nb: on ragged_bsr
    (rows of 0 .. 2 CAPB + 3 blocks, unsorted columns, COL != ROW) the oracle must give the same bits, also for block Jacobi
    at every nb and for the four Gauss-Seidel / SOR sweeps."""
    R = ref()
    if R is None:
        pytest.skip("oracle/_ref not available")
    o = _orc_setup()
    c = ragged_case(nb, shape)
    A, keep = T.as_bsr(c["ia"], c["ja"], c["val"], nb, ncol=c["COL"])
    n = c["ROW"] * nb
    x = c["x"].copy()
    R.fasp_blas_dbsr_mxv.argtypes = [C.POINTER(T.dBSRmat), T.c_double_p, T.c_double_p]
    R.fasp_blas_dbsr_aAxpy.argtypes = [C.c_double, C.POINTER(T.dBSRmat), T.c_double_p, T.c_double_p]
    y1 = np.full(n, np.nan); y2 = np.full(n, np.nan)
    o.orc_bsr_mxv(C.byref(A), T.dp(x), T.dp(y1)); R.fasp_blas_dbsr_mxv(C.byref(A), T.dp(x), T.dp(y2))
    assert np.array_equal(y1, y2)
    for alpha in (1.0, -1.0, 0.3):
        y1 = c["y0"].copy(); y2 = c["y0"].copy()
        o.orc_bsr_aAxpy(alpha, C.byref(A), T.dp(x), T.dp(y1)); R.fasp_blas_dbsr_aAxpy(alpha, C.byref(A), T.dp(x), T.dp(y2))
        assert np.array_equal(y1, y2), alpha
    if shape != "square":
        return
    d = orc_diaginv(o, A)
    b = c["b"].copy()
    vec = [C.POINTER(T.dBSRmat), C.POINTER(T.dvector), C.POINTER(T.dvector), T.c_double_p]
    R.fasp_smoother_dbsr_jacobi1.argtypes = vec
    u1 = c["u0"].copy(); u2 = c["u0"].copy()
    bv = T.dvector(n, T.dp(b)); uv = T.dvector(n, T.dp(u2))
    o.orc_bsr_jacobi1(C.byref(A), T.dp(b), T.dp(u1), T.dp(d))
    R.fasp_smoother_dbsr_jacobi1(C.byref(A), C.byref(bv), C.byref(uv), T.dp(d))
    assert np.array_equal(u1, u2)
    for descend, gs, sor in ((0, R.fasp_smoother_dbsr_gs_ascend, R.fasp_smoother_dbsr_sor_ascend),
                             (1, R.fasp_smoother_dbsr_gs_descend, R.fasp_smoother_dbsr_sor_descend)):
        gs.argtypes = vec; sor.argtypes = vec + [C.c_double]
        gs.restype = None; sor.restype = None
        u1 = c["u0"].copy(); u2 = c["u0"].copy(); uv = T.dvector(n, T.dp(u2))
        o.orc_bsr_gs_sor(C.byref(A), T.dp(b), T.dp(u1), T.dp(d), descend, 0, 0.0)
        gs(C.byref(A), C.byref(bv), C.byref(uv), T.dp(d))
        assert np.array_equal(u1, u2), ("gs", descend)
        assert np.abs(u1).max() < 1e3   # (ragged_bsr's diagonal keeps a sweep bounded)
        for w in SOR_WEIGHTS:
            u1 = c["u0"].copy(); u2 = c["u0"].copy(); uv = T.dvector(n, T.dp(u2))
            o.orc_bsr_gs_sor(C.byref(A), T.dp(b), T.dp(u1), T.dp(d), descend, 1, w)
            sor(C.byref(A), C.byref(bv), C.byref(uv), T.dp(d), w)
            assert np.array_equal(u1, u2), ("sor", descend, w)
            assert np.abs(u1).max() < 1e3


@pytest.mark.parametrize("nb", range(1, 8))
def test_oracle_ragged_mxv_within_rounding_bound(nb):
    """The oracle's block SpMV against an 80-bit evaluation that shares no code with it: within the a-priori bound of a
    double-precision sum of m products (_libs.bsr_mxv_bound_ratio), on rows of up to 2 CAPB + 3 blocks."""
    o = _orc_setup()
    worst = 0.0
    for shape in RAGGED_SHAPES:
        c = ragged_case(nb, shape)
        A, keep = T.as_bsr(c["ia"], c["ja"], c["val"], nb, ncol=c["COL"])
        x = c["x"].copy(); y = np.full(c["ROW"] * nb, np.nan)
        o.orc_bsr_mxv(C.byref(A), T.dp(x), T.dp(y))
        worst = max(worst, bsr_mxv_bound_ratio(c["ROW"], nb, c["ia"], c["ja"], c["val"], x, y))
    print(f"nb = {nb}: worst |y - Ax| / bound = {worst:.3e}")
    assert worst <= 1.0


def test_ragged_bsr_reaches_the_kernel_edges():
    """The generators are deterministic and hold what the device tests rely on (ragged_bsr asserts the rest itself)."""
    for nb in range(1, 8):
        RW, CAPB, U = bsr_tile(nb)
        a = ragged_bsr(nb, 3); b = ragged_bsr(nb, 3)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
        ROW, COL, ia, ja, val, lens = a
        assert ROW == (3139, 835, 407, 259, 189, 151, 129)[nb - 1] and COL == ROW
        rows = np.repeat(np.arange(ROW), lens)
        assert ((ja == rows).reshape(-1).astype(int).sum() == ROW) and lens[RW] == 1 and lens[0] == 2 * CAPB + 3
        # unsymmetric pattern: entries (i, j) whose transpose (j, i) is not stored -- the sweeps' schedule needs A^T for them
        stored = set(zip(rows.tolist(), ja.tolist()))
        assert sum((j, i) not in stored for i, j in stored) > ROW
        assert set(np.unique(lens[3 * RW + 2:ROW - 1])) >= set(range(1, U + 2))   # row lengths 1 .. U + 1 and beyond
        for extra in (37, -50):
            ROW, COL, ia, ja, val, lens = ragged_bsr(nb, 3, False, extra)
            assert COL == ROW + extra and ja.max() < COL and lens[RW - 1] == 0 and not lens[2 * RW:3 * RW].any()
    ROW, COL, ia, ja, val, lens = wide_bsr(7)
    assert ROW == 2048 * 4 * 9 + 5 and (lens == 1).sum() == np.sum((7 * np.arange(ROW) + 3) % ROW == np.arange(ROW))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["spe01", "p7x3_8", "p7x2_6", "p7x1_7", "p7x5_5"])
def test_gpu_bsr_ops_bit_exact(gpu, case):
    o = _orc_setup()
    L = gpu.lib()
    ia, ja, val, nb = _cases()[case]()
    A, keep = T.as_bsr(ia, ja, val, nb)
    n = A.ROW * nb
    rng = np.random.default_rng(7)
    x = rng.standard_normal(n); y0 = rng.standard_normal(n)
    y1 = np.zeros(n); y2 = np.ones(n)
    o.orc_bsr_mxv(C.byref(A), T.dp(x), T.dp(y1)); L.fasp_blas_dbsr_mxv(C.byref(A), T.dp(x), T.dp(y2))
    assert np.array_equal(y1, y2)
    for alpha in (1.0, -1.0, 0.3):
        y1 = y0.copy(); y2 = y0.copy()
        o.orc_bsr_aAxpy(alpha, C.byref(A), T.dp(x), T.dp(y1)); L.fasp_blas_dbsr_aAxpy(alpha, C.byref(A), T.dp(x), T.dp(y2))
        assert np.array_equal(y1, y2)
    if nb <= 3:
        dv = L.fasp_dbsr_getdiaginv(C.byref(A))
        d = np.ctypeslib.as_array(dv.val, (dv.row,)).copy()
        dp_ = o.orc_bsr_getdiaginv(C.byref(A))
        assert np.array_equal(d, np.ctypeslib.as_array(dp_, (A.ROW * nb * nb,)))
        o.orc_free(dp_)
        b = rng.standard_normal(n)
        u1 = x.copy(); u2 = x.copy()
        o.orc_bsr_jacobi1(C.byref(A), T.dp(b), T.dp(u1), T.dp(d))
        bv = T.dvector(n, T.dp(b)); uv = T.dvector(n, T.dp(u2))
        L.fasp_smoother_dbsr_jacobi1(C.byref(A), C.byref(bv), C.byref(uv), T.dp(d))
        assert np.array_equal(u1, u2)


def test_spe01_shape():
    ia, ja, val, nb = read_bsr(DATA + "/bsrmat_SPE01.dat")
    assert (len(ia) - 1, len(ja), nb) == (302, 1788, 3)
    assert len(read_vec(DATA + "/rhs_SPE01.dat")) == 906
