"""The block (BSR) device kernels away from the 7-point stencil: k_bsr_wstream<NB, OP> (fasp_blas_dbsr_mxv / _aAxpy /
fasp_smoother_dbsr_jacobi1) and the level-scheduled block sweeps k_bsr_seq_level<NB> (fasp_hip_bsr_sweep) at every block
width 1 .. 7, against the oracle BIT FOR BIT -- the kernels claim the reference's order of operations -- on matrices
built to reach the kernel's edges (_libs.ragged_bsr): tiles of several LDS chunks, one block row longer than a chunk,
chunks of an odd number of doubles, empty block rows at a tile's end and start, a tile without blocks, NNZ = 0, row
lengths 1 .. 2U + 2 (the clamped column loads), unsorted columns, the diagonal block anywhere in its row, partial tiles,
COL != ROW, the grid-stride loop (_libs.wide_bsr), and an unsymmetric pattern under the sweeps' schedule.  Every output
buffer starts as NaN: a row that is never written shows."""
import ctypes as C

import numpy as np
import pytest

from _libs import (RAGGED_SHAPES, SOR_WEIGHTS, T, OrcBSR, bsr_mxv_bound_ratio, bsr_params, bsr_tile, orc_bsr_ops,
                   orc_diaginv, poisson7pt, ragged_case, wide_bsr)

pytestmark = pytest.mark.gpu

NBS = list(range(1, 8))


@pytest.fixture(scope="module")
def libs(gpu):
    return orc_bsr_ops(), gpu.lib()


def _nan(n):
    return np.full(n, np.nan)


def _mxv(lib_fn, A, x, nrow):
    y = _nan(nrow)
    lib_fn(C.byref(A), T.dp(x), T.dp(y))
    return y


def _aAxpy(lib_fn, alpha, A, x, y0):
    y = y0.copy()
    lib_fn(alpha, C.byref(A), T.dp(x), T.dp(y))
    return y


def _jacobi(o, L, A, b, u0, d):
    n = len(u0)
    u1 = u0.copy(); u2 = u0.copy()
    o.orc_bsr_jacobi1(C.byref(A), T.dp(b), T.dp(u1), T.dp(d))
    bv = T.dvector(n, T.dp(b)); uv = T.dvector(n, T.dp(u2))
    L.fasp_smoother_dbsr_jacobi1(C.byref(A), C.byref(bv), C.byref(uv), T.dp(d))
    return u1, u2


def _check_mxv_aAxpy(o, L, A, x, y0, alphas):
    """mxv and aAxpy of the device against the oracle, bit for bit; returns the device's y = A x."""
    n = len(y0)
    y = _mxv(L.fasp_blas_dbsr_mxv, A, x, n)
    assert np.array_equal(_mxv(o.orc_bsr_mxv, A, x, n), y)
    for alpha in alphas:
        assert np.array_equal(_aAxpy(o.orc_bsr_aAxpy, alpha, A, x, y0), _aAxpy(L.fasp_blas_dbsr_aAxpy, alpha, A, x, y0)), alpha
    return y


@pytest.mark.parametrize("shape", list(RAGGED_SHAPES))
@pytest.mark.parametrize("nb", NBS)
def test_ragged_ops_bit_exact(libs, nb, shape):
    o, L = libs
    c = ragged_case(nb, shape)
    A, keep = T.as_bsr(c["ia"], c["ja"], c["val"], nb, ncol=c["COL"])
    x = c["x"].copy(); y0 = c["y0"].copy()
    y = _check_mxv_aAxpy(o, L, A, x, y0, (1.0, -1.0, 0.3))
    assert np.array_equal(_aAxpy(L.fasp_blas_dbsr_aAxpy, 0.0, A, x, y0), y0)   # alpha = 0 leaves y untouched
    ratio = bsr_mxv_bound_ratio(c["ROW"], nb, c["ia"], c["ja"], c["val"], x, y)
    print(f"nb = {nb} {shape}: worst |y - Ax| / bound = {ratio:.3e}")
    assert ratio <= 1.0
    if shape == "square":
        u1, u2 = _jacobi(o, L, A, c["b"].copy(), c["u0"], orc_diaginv(o, A))
        assert np.array_equal(u1, u2)


def _random_rows(rng, ROW, COL, k, nb):
    """ROW block rows of k blocks each in distinct random columns, standard normal values."""
    ja = np.concatenate([rng.choice(COL, size=k, replace=False) for _ in range(ROW)]).astype(np.int32)
    ia = (np.arange(ROW + 1) * k).astype(np.int32)
    return ia, ja, rng.standard_normal(len(ja) * nb * nb)


@pytest.mark.parametrize("nb", NBS)
def test_small_shapes(libs, nb):
    """ROW = 1 (one block; U + 1 blocks), the sizes around one wave tile and one 4-wave workgroup tile, and NNZ = 0."""
    o, L = libs
    RW, CAPB, U = bsr_tile(nb)
    rng = np.random.default_rng(40 + nb)
    shapes = [(1, 1, 1), (1, U + 3, U + 1)] + [(R, max(R, 3) + 2, 3) for R in (RW - 1, RW, RW + 1, 4 * RW - 1, 4 * RW + 1)]
    for ROW, COL, k in shapes:
        ia, ja, val = _random_rows(rng, ROW, COL, k, nb)
        A, keep = T.as_bsr(ia, ja, val, nb, ncol=COL)
        _check_mxv_aAxpy(o, L, A, rng.standard_normal(COL * nb), rng.standard_normal(ROW * nb), (0.3,))
    ia = np.zeros(6, dtype=np.int32); ja = np.zeros(0, dtype=np.int32); val = np.zeros(0)
    A, keep = T.as_bsr(ia, ja, val, nb, ncol=4)
    x = rng.standard_normal(4 * nb); y0 = rng.standard_normal(5 * nb)
    y = _check_mxv_aAxpy(o, L, A, x, y0, (0.3,))   # (the oracle's aAxpy of an empty matrix is y (1 / alpha) alpha)
    assert np.array_equal(y, np.zeros(5 * nb))


@pytest.mark.parametrize("nb", NBS)
def test_grid_stride(libs, nb):
    """More 4-wave tiles than the largest grid: every workgroup's `t += gridDim.x` loop runs at least twice."""
    o, L = libs
    ROW, COL, ia, ja, val, lens = wide_bsr(nb)
    A, keep = T.as_bsr(ia, ja, val, nb)
    rng = np.random.default_rng(60 + nb)
    x = rng.standard_normal(ROW * nb); y0 = rng.standard_normal(ROW * nb)
    _check_mxv_aAxpy(o, L, A, x, y0, (0.3,))
    u1, u2 = _jacobi(o, L, A, rng.standard_normal(ROW * nb), x, orc_diaginv(o, A))
    assert np.array_equal(u1, u2)


@pytest.mark.parametrize("agg", [2, 1], ids=["vmb", "pairwise"])
@pytest.mark.parametrize("nb", [2, 3, 5, 7])
def test_hierarchy_operators(libs, nb, agg):
    """A, P and R of every level of the oracle's UA hierarchy of P7(8) (x) B_nb: one block per row of P, long rows of R,
    COL != ROW."""
    o, L = libs
    rng = np.random.default_rng(80 + nb)
    ia, ja, a, f, ue = poisson7pt(8)
    Bk = rng.standard_normal((nb, nb)) + np.diag(nb + rng.random(nb))
    itp, amgp = bsr_params(agg=agg)
    H = OrcBSR(ia, ja, (a[:, None, None] * Bk[None, :, :]).reshape(-1), nb, amgp)
    assert H.status >= 0 and H.num_levels >= 2
    seen = 0
    for lvl in H.levels:
        for which in "APR":
            if lvl[which] is None:
                continue
            ROW, COL, NNZ, mia, mja, mval = lvl[which]
            A, keep = T.as_bsr(mia, mja, mval, nb, ncol=COL)
            _check_mxv_aAxpy(o, L, A, rng.standard_normal(COL * nb), rng.standard_normal(ROW * nb), (-1.0,))
            seen += ROW != COL
    assert seen >= 2


def _sweep(L, A, b, u, d, descend, sor, w):
    nlev = C.c_int(-1)
    st = L.fasp_hip_bsr_sweep(C.byref(A), T.dp(b), T.dp(u), T.dp(d), descend, sor, w, C.byref(nlev))
    return st, nlev.value


@pytest.mark.parametrize("nb", NBS)
def test_block_sweeps_bit_exact(libs, nb):
    """One block Gauss-Seidel / SOR sweep on the UNSYMMETRIC square pattern: the schedule needs the transpose pattern for
    the rows a later row reads without being read by it.  Then an ascending and a descending sweep in a row."""
    o, L = libs
    c = ragged_case(nb, "square")
    A, keep = T.as_bsr(c["ia"], c["ja"], c["val"], nb)
    d = orc_diaginv(o, A)
    b = c["b"].copy()
    for descend in (0, 1):
        for sor, w in [(0, 0.0)] + [(1, w) for w in SOR_WEIGHTS]:
            u1 = c["u0"].copy(); u2 = c["u0"].copy()
            o.orc_bsr_gs_sor(C.byref(A), T.dp(b), T.dp(u1), T.dp(d), descend, sor, w)
            st, nlev = _sweep(L, A, b, u2, d, descend, sor, w)
            assert st == 0 and 1 < nlev < c["ROW"], (st, nlev)
            assert np.array_equal(u1, u2), (descend, sor, w)
    u1 = c["u0"].copy(); u2 = c["u0"].copy()
    for descend in (0, 1):
        o.orc_bsr_gs_sor(C.byref(A), T.dp(b), T.dp(u1), T.dp(d), descend, 1, 1.1)
        assert _sweep(L, A, b, u2, d, descend, 1, 1.1)[0] == 0
    assert np.array_equal(u1, u2)


def test_block_sweep_refuses_bad_arguments(libs):
    o, L = libs
    c = ragged_case(7, "square")
    n = c["ROW"] * 7
    b = c["b"].copy(); d = np.ones(n * 7)
    nlev = C.c_int(-1)
    null = C.POINTER(C.c_double)()

    def call(A, bp=None, up=None, dp=None, nl=C.byref(nlev)):
        u = c["u0"].copy()
        st = L.fasp_hip_bsr_sweep(A, T.dp(b) if bp is None else bp, T.dp(u) if up is None else up,
                                  T.dp(d) if dp is None else dp, 0, 0, 1.0, nl)
        assert np.array_equal(u, c["u0"])   # a refused call touches nothing
        return st

    def mat(**kw):
        A, keep = T.as_bsr(c["ia"], c["ja"], c["val"], 7)
        for k, v in kw.items():
            setattr(A, k, v)
        return A, keep

    A, keep = mat()
    assert call(None) == T.ERROR_INPUT_PAR
    assert call(C.byref(A), bp=null) == T.ERROR_INPUT_PAR
    assert call(C.byref(A), up=null) == T.ERROR_INPUT_PAR
    assert call(C.byref(A), dp=null) == T.ERROR_INPUT_PAR
    assert call(C.byref(A), nl=None) == T.ERROR_INPUT_PAR
    for bad in (dict(nb=0), dict(nb=8), dict(storage_manner=1), dict(COL=c["ROW"] + 1)):
        A, keep = mat(**bad)
        assert call(C.byref(A)) == T.ERROR_INPUT_PAR, bad
    assert nlev.value == -1
