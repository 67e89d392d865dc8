"""Structured matrices (dSTRmat) on the device: k_str_band against the reference's fasp_blas_dstr_aAxpy bit for bit in each of its four
arithmetic forms, and the STR Krylov entries against the reference's solvers.

Operator cases (tests/_str_cases.py): the device result is compared with the recorded reference result (tests/golden/str_cases.npz: SHA-256
of every result, the result itself up to 420 rows) and, where oracle/_ref is built, with the live reference.  The reference's
fasp_blas_dstr_mxv is never called (it clears ngrid*nc*nc doubles): "mxv" is its aAxpy(1.0) onto a cleared y.  The two cases
c2d_1x6x5_nc3 / _nc2 are held to the restated form and never handed to the reference: with nx == 1 its block texts of the 2D product loop
from nx where they mean nline (BlaSpmvSTR.c:701, :906, :1062), visit rows 1 .. nline-1 twice and read in front of the band and of x.
The launch does not cap its grid (one thread per scalar row), so there is no case beyond a cap.

Solves, tol 1e-8 from a zero guess: nc = 1 on 9 x 8 x 7 against the reference's own STR solvers -- equal iteration counts and
max|x - x_ref| <= 1e-9 max|x_ref|; nc = 2, 3, 5 on 6 x 5 x 4 against the reference's BSR solver of the converted matrix (the two products sum
in different orders): iteration count within one of the reference's, true relative residual in np.longdouble at most 1.01 tol."""
import ctypes as C

import numpy as np
import pytest

import _libs
import _str_cases as S
from _libs import T

pytestmark = pytest.mark.gpu


class MF(C.Structure):
    _fields_ = [("data", C.c_void_p), ("fct", C.c_void_p)]


@pytest.fixture(scope="module")
def G():
    return np.load(S.GOLDEN)


@pytest.fixture(scope="module")
def R():
    lib = _libs.ref()
    return S.ref_protos(lib) if lib is not None else None


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def dev_aAxpy(L, case, diag, bands, alpha, x, y0):
    A, keep = S.as_str(case, diag, bands)
    if alpha == "mxv":
        y = np.full_like(y0, np.nan)
        L.fasp_blas_dstr_mxv(C.byref(A), T.dp(x), T.dp(y))
    else:
        y = y0.copy()
        L.fasp_blas_dstr_aAxpy(alpha, C.byref(A), T.dp(x), T.dp(y))
    return y


@pytest.mark.parametrize("case", S.op_cases(), ids=lambda c: c["name"])
def test_band_product_bit_for_bit(gpu, G, R, case):
    L = gpu.lib()
    diag, bands = S.build(case)
    x, y0 = S.vectors(case)
    keys = list(G["op_keys"])
    for alpha in S.ALPHAS:
        y = dev_aAxpy(L, case, diag, bands, alpha, x, y0)
        k = keys.index(f"{case['name']}/{alpha}")
        lo, hi = G["op_small_off"][k], G["op_small_off"][k + 1]
        if hi > lo:
            want = G["op_small"][lo:hi]
            bad = np.flatnonzero(_bits(y) != _bits(want))
            assert bad.size == 0, (alpha, bad[:8], y[bad[:8]], want[bad[:8]])
        if R is not None and case["ref_ok"]:
            want = S.ref_aAxpy(R, case, diag, bands, alpha, x, y0)
            bad = np.flatnonzero(_bits(y) != _bits(want))
            assert bad.size == 0, (alpha, bad[:8], y[bad[:8]], want[bad[:8]])
        assert np.array_equal(S.digest(y), G["op_sha"][k]), alpha


def test_one_grid_point_and_no_grid_point(gpu):
    """An empty matrix (ngrid = 0) and a matrix of one grid point are legal."""
    L = gpu.lib()
    one = dict(name="one", nx=1, ny=1, nz=1, nc=3, offsets=[1, -1])   # both bands are empty
    diag, bands = S.build(one)
    x, y0 = S.vectors(one)
    y = dev_aAxpy(L, one, diag, bands, 0.37, x, y0)
    assert np.array_equal(_bits(y), _bits(S.model_aAxpy(dict(one, form=S.FORM_G), diag, bands, 0.37, x, y0)))
    A, keep = T.as_str(0, 0, 0, 2, [], np.zeros(0), [])
    L.fasp_blas_dstr_mxv(C.byref(A), T.dp(np.zeros(1)), T.dp(np.zeros(1)))


@pytest.mark.parametrize("key,sym,method,restart", S.SCALAR_SOLVES, ids=[s[0] for s in S.SCALAR_SOLVES])
@pytest.mark.parametrize("entry", ["krylov", "krylov_diag"])
def test_scalar_solves_match_the_reference(gpu, G, R, entry, key, sym, method, restart):
    L = gpu.lib()
    c, diag, bands, b = S.scalar_system(sym)
    it, x = S.solve_with(L, "fasp_solver_dstr_" + entry, c, diag, bands, b, method, restart)
    it_g, x_g = int(G[f"solve_{key}_{entry}_it"]), G[f"solve_{key}_{entry}_x"]
    print(f"{key} {entry}: {it} iterations (recorded {it_g}), max|dx| / max|x| = {np.max(np.abs(x - x_g)) / np.max(np.abs(x_g)):.3e}")
    assert it == it_g
    assert np.max(np.abs(x - x_g)) <= 1e-9 * np.max(np.abs(x_g))
    if R is not None:
        it_r, x_r = S.solve_with(R, "fasp_solver_dstr_" + entry, c, diag, bands, b, method, restart)
        assert it == it_r and np.max(np.abs(x - x_r)) <= 1e-9 * np.max(np.abs(x_r))


@pytest.mark.parametrize("entry", ["krylov", "krylov_diag"])
def test_scalar_minres_matches_the_reference(gpu, G, R, entry):
    """MinRes is not among the methods fasp_solver_dstr_itsolver dispatches (SolSTR.c:76): fasp_solver_dstr_pminres, without a
    preconditioner and with the block-diagonal one built by hand."""
    L = gpu.lib()
    c, diag, bands, b = S.scalar_system(True)
    dinv = None if entry == "krylov" else 1.0 / diag
    it, x = S.minres_with(L, c, diag, bands, b, dinv)
    it_g, x_g = int(G[f"solve_minres_{entry}_it"]), G[f"solve_minres_{entry}_x"]
    print(f"minres {entry}: {it} iterations (recorded {it_g}), max|dx| / max|x| = {np.max(np.abs(x - x_g)) / np.max(np.abs(x_g)):.3e}")
    assert it == it_g
    assert np.max(np.abs(x - x_g)) <= 1e-9 * np.max(np.abs(x_g))
    if R is not None:
        it_r, x_r = S.minres_with(R, c, diag, bands, b, dinv)
        assert it == it_r and np.max(np.abs(x - x_r)) <= 1e-9 * np.max(np.abs(x_r))


@pytest.mark.parametrize("key,sym,method,restart", S.BLOCK_SOLVES, ids=[s[0] for s in S.BLOCK_SOLVES])
@pytest.mark.parametrize("nc", S.BLOCK_NC)
def test_block_solves_against_the_reference_bsr_solver(gpu, G, R, nc, key, sym, method, restart):
    L = gpu.lib()
    c, diag, bands, b = S.block_system(nc, sym)
    it, x = S.solve_with(L, "fasp_solver_dstr_krylov_diag", c, diag, bands, b, method, restart)
    it_g = int(G[f"block_{nc}_{key}_it"])
    rr = S.true_relres(c, diag, bands, b, x)
    print(f"nc {nc} {key}: {it} iterations (reference BSR {it_g}), true relative residual {rr:.3e}")
    assert abs(it - it_g) <= 1
    assert rr <= 1.01 * S.TOL
    if R is not None:
        it_r, x_r = S.ref_bsr_krylov_diag(R, c, diag, bands, b, method, restart)
        assert it_r == it_g and abs(it - it_r) <= 1


def _matfree_krylov(L, A, b, method, restart):
    mf = MF()
    L.fasp_solver_matfree_init.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.fasp_solver_matfree_init.restype = None
    L.fasp_solver_matfree_init(T.MAT_STR, C.addressof(mf), C.addressof(A))
    assert mf.fct == C.cast(L.fasp_hip_mxv_str, C.c_void_p).value and mf.data == C.addressof(A)
    L.fasp_solver_krylov.argtypes = [C.c_void_p, C.POINTER(T.dvector), C.POINTER(T.dvector), C.POINTER(T.ITS_param)]
    x = np.zeros_like(b)
    bv, kb = T.as_vec(b)
    xv = T.dvector(x.size, T.dp(x))
    p = S.its_param(method, restart)
    return L.fasp_solver_krylov(C.addressof(mf), C.byref(bv), C.byref(xv), C.byref(p)), x


@pytest.mark.parametrize("nc", [1, 3])
def test_matfree_str_operator_stays_on_the_device(gpu, nc):
    """fasp_solver_matfree_init(MAT_STR) + fasp_solver_krylov: the same count and bit for bit the same x as fasp_solver_dstr_krylov.
    BiCGstab: the method whose matrix-free text is the text of the format families (krylov_run, csrc/pcg.hip.h); for CG, MinRes and
    the GMRES variants the reference keeps older texts for mxv_matfree, which the next test holds to their own stopping test."""
    method, restart = T.SOLVER_BiCGstab, 25
    L = gpu.lib()
    c, diag, bands, b = S.scalar_system(False) if nc == 1 else S.block_system(nc, False)
    A, keep = S.as_str(c, diag, bands)
    it, x = S.solve_with(L, "fasp_solver_dstr_krylov", c, diag, bands, b, method, restart)
    it_mf, x_mf = _matfree_krylov(L, A, b, method, restart)
    assert it > 5 and it_mf == it
    assert np.array_equal(_bits(x_mf), _bits(x))


@pytest.mark.parametrize("method,restart", [(T.SOLVER_CG, 25), (T.SOLVER_VGMRES, 10)], ids=["cg", "vgmres"])
def test_matfree_str_older_texts(gpu, method, restart):
    L = gpu.lib()
    c, diag, bands, b = S.scalar_system(True)
    A, keep = S.as_str(c, diag, bands)
    it_mf, x_mf = _matfree_krylov(L, A, b, method, restart)
    rr = S.true_relres(c, diag, bands, b, x_mf)
    print(f"matrix-free text of method {method}: {it_mf} iterations, true relative residual {rr:.3e}")
    assert it_mf > 5 and rr <= 1.01 * S.TOL
    x = x_mf
    y = np.full_like(b, np.nan)
    L.fasp_hip_mxv_str(C.addressof(A), T.dp(x), T.dp(y))       # the installed function itself, on host vectors
    assert np.array_equal(_bits(y), _bits(S.model_aAxpy(c, diag, bands, "mxv", x, y)))


@pytest.mark.parametrize("nc", [1, 3])
def test_pcg_with_hand_built_diag_precond_is_krylov_diag(gpu, G, nc):
    L = gpu.lib()
    c, diag, bands, b = S.scalar_system(True) if nc == 1 else S.block_system(nc, True)
    it, x = S.solve_with(L, "fasp_solver_dstr_krylov_diag", c, diag, bands, b, T.SOLVER_CG, 25)
    if nc == 1:
        dinv = 1.0 / diag
    else:   # the library's own inverse blocks (fasp_smat_inv restated), through the BSR entry that hands them out
        ngrid = diag.size // (nc * nc)
        D, keepd = T.as_bsr(np.arange(ngrid + 1), np.arange(ngrid), diag, nc)
        v = L.fasp_dbsr_getdiaginv(C.byref(D))
        dinv = np.ctypeslib.as_array(v.val, shape=(v.row,)).copy()
    A, keep = S.as_str(c, diag, bands)
    dd = T.precond_diag_str(nc, T.dvector(dinv.size, T.dp(dinv)))
    pc = T.precond(C.cast(C.pointer(dd), C.c_void_p), C.cast(L.fasp_precond_dstr_diag, T.PRECOND_FCT))
    x2 = np.zeros_like(b)
    bv, kb = T.as_vec(b)
    xv = T.dvector(x2.size, T.dp(x2))
    it2 = L.fasp_solver_dstr_pcg(C.byref(A), C.byref(bv), C.byref(xv), C.byref(pc), S.TOL, 1e-18, 500, T.STOP_REL_RES, 0)
    assert it > 5 and it2 == it
    assert np.array_equal(_bits(x2), _bits(x))
    # a foreign preconditioner (a Python callback doing the same arithmetic) is staged through the host: same iterates
    def fct(r, z, data):
        rr = np.ctypeslib.as_array(r, shape=(b.size,))
        np.ctypeslib.as_array(z, shape=(b.size,))[:] = S.model_dinv_apply(nc, dinv, rr)
    cb = T.PRECOND_FCT(fct)
    pc3 = T.precond(None, cb)
    x3 = np.zeros_like(b)
    xv3 = T.dvector(x3.size, T.dp(x3))
    it3 = L.fasp_solver_dstr_pcg(C.byref(A), C.byref(bv), C.byref(xv3), C.byref(pc3), S.TOL, 1e-18, 500, T.STOP_REL_RES, 0)
    assert it3 == it and np.array_equal(_bits(x3), _bits(x))


def test_itsolver_dispatch_and_refusals(gpu):
    L = gpu.lib()
    c, diag, bands, b = S.scalar_system(True)
    A, keep = S.as_str(c, diag, bands)
    n = b.size
    bv, kb = T.as_vec(b)
    x = np.full(n, 0.25)
    xv = T.dvector(n, T.dp(x))
    for method in (T.SOLVER_MinRes, T.SOLVER_VFGMRES, T.SOLVER_GCG, T.SOLVER_GCR, 13):   # SolSTR.c:76: CG, BiCGstab, GMRES, VGMRES only
        p = S.its_param(method, 25)
        assert L.fasp_solver_dstr_itsolver(C.byref(A), C.byref(bv), C.byref(xv), None, C.byref(p)) == T.ERROR_SOLVER_TYPE
        assert L.fasp_solver_dstr_krylov(C.byref(A), C.byref(bv), C.byref(xv), C.byref(p)) == T.ERROR_SOLVER_TYPE
        assert L.fasp_solver_dstr_krylov_diag(C.byref(A), C.byref(bv), C.byref(xv), C.byref(p)) == T.ERROR_SOLVER_TYPE
        assert np.all(x == 0.25)
    p = S.its_param(T.SOLVER_CG, 25)
    args = (S.TOL, 1e-18, 500, T.STOP_REL_RES, 0)

    def refused(Am, bvm, xvm):
        ok = L.fasp_solver_dstr_pcg(C.byref(Am) if Am is not None else None, C.byref(bvm) if bvm is not None else None,
                                    C.byref(xvm) if xvm is not None else None, None, *args) == T.ERROR_INPUT_PAR
        if Am is not None and bvm is not None and xvm is not None:
            ok = ok and L.fasp_solver_dstr_krylov_diag(C.byref(Am), C.byref(bvm), C.byref(xvm), C.byref(p)) == T.ERROR_INPUT_PAR
        return ok and bool(np.all(x == 0.25))

    assert refused(None, bv, xv) and refused(A, None, xv) and refused(A, bv, None)
    assert L.fasp_solver_dstr_krylov(C.byref(A), C.byref(bv), C.byref(xv), None) == T.ERROR_INPUT_PAR
    for field, value in (("nc", 0), ("nc", 8), ("nband", -1)):
        Am, km = S.as_str(c, diag, bands)
        setattr(Am, field, value)
        assert refused(Am, bv, xv), (field, value)
    for k, value in ((0, 0), (1, c["offsets"][0])):   # an offset of 0, a repeated offset
        c2 = dict(c, offsets=list(c["offsets"]))
        c2["offsets"][k] = value
        b2 = [np.zeros(n - abs(o)) for o in c2["offsets"]]
        Am, km = S.as_str(c2, diag, b2)
        assert refused(Am, bv, xv), (k, value)
    assert refused(A, T.dvector(n - 1, T.dp(b)), xv) and refused(A, bv, T.dvector(n + 1, T.dp(x)))
    far = dict(c, offsets=[1, -1, n + 3])             # |offset| >= ngrid: legal and empty
    Am, km = S.as_str(far, diag, [np.zeros(n - 1), np.zeros(n - 1), np.zeros(0)])
    x[:] = 0.0
    assert L.fasp_solver_dstr_pcg(C.byref(Am), C.byref(bv), C.byref(xv), None, *args) > 0
    assert L.fasp_hip_time_str_mxv(C.byref(Am), 2) > 0.0 and L.fasp_hip_time_str_mxv(C.byref(Am), 0) == -1.0
