"""Block ILU on the device (csrc/ilu.hip.h, the NB-templated triangular solves) against the compiled reference:
  1. fasp_precond_dbsr_ilu gives the reference's z byte for byte, nb 1..7 x ILU(0..2), both forms of the solves, with a
     registered (resident) factor and with a caller-built copy of it; fasp_smoother_dbsr_ilu likewise;
  2. SPE01 with fasp_solver_dbsr_krylov_ilu, every BSR Krylov method x ILU(0) / ILU(1): the reference's iteration counts
     (the tutorial case pinned: GMRES, tol 1e-6, ILU(0): 18); CG + ILU(0) on SPD P7(n) (x) B3;
  3. the Fortran wrapper, residency of factors (block and scalar ones side by side), and the scale P7(64 / 128) (x) B3.
Schedule edges and hand-built factors: see test_gpu_ilu_kernels.py."""
import ctypes as C

import numpy as np
import pytest

import _libs
from _libs import DATA, T, poisson7pt_bsr, read_bsr, read_csr, read_vec
from test_bilu_setup import Bsr, bilu_protos, ilu_param, matrix
from test_ilu_setup import Csr, ilu_protos

pytestmark = [pytest.mark.gpu, pytest.mark.ref]
P = C.POINTER


@pytest.fixture(scope="module")
def libs(gpu):
    ref = _libs.ref()
    if ref is None:
        pytest.fail("the reference build (oracle/_ref/libfasp_ref.so) is missing")
    ours = ilu_protos(bilu_protos(gpu.lib()))
    ours.fasp_hip_ilu_resident_count.restype = C.c_int
    ref = ilu_protos(bilu_protos(ref))
    yield ours, ref
    ours.fasp_hip_tune(b"ilu_form", -1)


def _ptr(v):
    return v.ctypes.data_as(T.c_double_p)


def _vec(v):
    return T.dvector(len(v), _ptr(v))


def _vp(d):
    return C.cast(C.byref(d), C.c_void_p)


@pytest.mark.parametrize("lfil", [0, 1, 2])
@pytest.mark.parametrize("nb", range(1, 8))
@pytest.mark.parametrize("mname", ["P7_6", "nonsym"])
def test_apply_bitwise(libs, mname, nb, lfil):
    ours, ref = libs
    arrays = matrix(mname, nb)
    n = (len(arrays[0]) - 1) * nb
    r = np.random.default_rng(21 + nb).uniform(-1.0, 1.0, n)
    A1, d1 = Bsr(*arrays, nb), T.ILU_data()
    A2, d2 = Bsr(*arrays, nb), T.ILU_data()
    assert ours.fasp_ilu_dbsr_setup(C.byref(A1.M), C.byref(d1), C.byref(ilu_param(ours, T.ILUk, lfil))) == 0
    assert ref.fasp_ilu_dbsr_setup(C.byref(A2.M), C.byref(d2), C.byref(ilu_param(ref, T.ILUk, lfil))) == 0
    try:
        zr = np.zeros(n)
        ref.fasp_precond_dbsr_ilu(_ptr(r.copy()), _ptr(zr), _vp(d2))
        copy = T.ILU_data.from_buffer_copy(d1)   # a caller-built ILU_data over the same arrays: not registered
        for form in (0, 1):
            ours.fasp_hip_tune(b"ilu_form", form)
            for d in (d1, copy):
                z = np.full(n, np.nan)
                ours.fasp_precond_dbsr_ilu(_ptr(r.copy()), _ptr(z), _vp(d))
                assert z.tobytes() == zr.tobytes(), (form, d is d1, np.max(np.abs(z - zr)))
        ours.fasp_hip_tune(b"ilu_form", -1)
        assert ours.fasp_hip_ilu_resident_count() == 1
        # the smoother: x += (LU)^-1 (b - A x); the residual comes from the BSR residual kernel, which reproduces the
        # reference's aAxpy rounding (test_bsr_ops.py), so x is compared byte for byte
        b = np.random.default_rng(22).uniform(-1.0, 1.0, n)
        x0 = np.random.default_rng(23).uniform(-1.0, 1.0, n)
        x1, x2 = x0.copy(), x0.copy()
        ours.fasp_smoother_dbsr_ilu(C.byref(A1.M), C.byref(_vec(b)), C.byref(_vec(x1)), _vp(d1))
        ref.fasp_smoother_dbsr_ilu(C.byref(A2.M), C.byref(_vec(b)), C.byref(_vec(x2)), _vp(d2))
        assert x1.tobytes() == x2.tobytes(), np.max(np.abs(x1 - x2))
    finally:
        ours.fasp_ilu_data_free(C.byref(d1)); ref.fasp_ilu_data_free(C.byref(d2))
    assert ours.fasp_hip_ilu_resident_count() == 0


def spe01():
    ia, ja, val, nb = read_bsr(DATA + "/bsrmat_SPE01.dat")
    return ia, ja, val, nb, read_vec(DATA + "/rhs_SPE01.dat")


def _krylov(L, ia, ja, val, nb, b, solver, lfil, tol, maxit=500, restart=None):
    A = Bsr(ia, ja, val, nb)
    x = np.zeros(len(b)); bb = np.array(b)
    it = T.ITS_param()
    L.fasp_param_solver_init(C.byref(it))
    it.itsolver_type, it.tol, it.maxit, it.print_level = solver, tol, maxit, 0
    if restart is not None:
        it.restart = restart
    st = L.fasp_solver_dbsr_krylov_ilu(C.byref(A.M), C.byref(_vec(bb)), C.byref(_vec(x)), C.byref(it),
                                       C.byref(ilu_param(L, T.ILUk, lfil)))
    return st, x


def _relres(ia, ja, val, nb, b, x):
    A, keep = T.as_bsr(ia, ja, val, nb)
    y = np.zeros(len(b)); xx = np.array(x)
    _libs.oracle().orc_bsr_mxv(C.byref(A), _ptr(xx), _ptr(y))
    return np.linalg.norm(b - y) / np.linalg.norm(b)


SOLVERS = [T.SOLVER_CG, T.SOLVER_BiCGstab, T.SOLVER_GMRES, T.SOLVER_VGMRES, T.SOLVER_VFGMRES]


@pytest.mark.parametrize("lfil", [0, 1])
@pytest.mark.parametrize("solver", SOLVERS)
def test_spe01_every_krylov_method(libs, solver, lfil):
    ours, ref = libs
    ia, ja, val, nb, b = spe01()
    it1, x1 = _krylov(ours, ia, ja, val, nb, b, solver, lfil, 1e-8)
    it2, x2 = _krylov(ref, ia, ja, val, nb, b, solver, lfil, 1e-8)
    assert it1 == it2, (it1, it2)
    if it2 > 0:
        r1, r2 = _relres(ia, ja, val, nb, b, x1), _relres(ia, ja, val, nb, b, x2)
        # SPE01 is badly conditioned: the rounding of the device's reductions (the preconditioner itself is bitwise, see
        # test_apply_bitwise) moves the last digits of the final residual (BiCGstab 3.4e-9 against 1.9e-9, the GMRES
        # variants alike).  Same count; the residuals agree to 1e-6 relative or both meet the tolerance.
        assert abs(r1 - r2) <= 1e-10 + 1e-6 * abs(r2) or max(r1, r2) <= 1e-8, (r1, r2)


def test_spe01_tutorial_case(libs):
    """tutorial/main/spe01-its.c: GMRES, tol 1e-6, ILU(0) -- 18 iterations (tutorial/out/spe01-its-c.out)"""
    ours, ref = libs
    ia, ja, val, nb, b = spe01()
    it1, x1 = _krylov(ours, ia, ja, val, nb, b, T.SOLVER_GMRES, 0, 1e-6)
    it2, _ = _krylov(ref, ia, ja, val, nb, b, T.SOLVER_GMRES, 0, 1e-6)
    assert it1 == 18 == it2
    assert _relres(ia, ja, val, nb, b, x1) < 1e-6


@pytest.mark.parametrize("n", [16, 32])
def test_cg_spd_p7_b3(libs, n):
    ours, ref = libs
    ia, ja, val, nb = poisson7pt_bsr(n)
    b = np.random.default_rng(n).uniform(-1.0, 1.0, (len(ia) - 1) * nb)
    it1, x1 = _krylov(ours, ia, ja, val, nb, b, T.SOLVER_CG, 0, 1e-8)
    it2, x2 = _krylov(ref, ia, ja, val, nb, b, T.SOLVER_CG, 0, 1e-8)
    assert it1 == it2 > 0
    assert np.max(np.abs(x1 - x2)) <= 1e-6 * np.max(np.abs(x2))


def test_fortran_wrapper(libs):
    ours, _ = libs
    ours.fasp_fwrapper_dbsr_krylov_ilu_.argtypes = [P(C.c_int), P(C.c_int), P(C.c_int), T.c_int_p, T.c_int_p, T.c_double_p,
                                                    T.c_double_p, T.c_double_p, P(C.c_double), P(C.c_int), P(C.c_int)]
    ours.fasp_fwrapper_dbsr_krylov_ilu_.restype = None
    ia, ja, val, nb, b = spe01()
    A = Bsr(ia, ja, val, nb)
    bb, x = np.array(b), np.zeros(len(b))
    ours.fasp_fwrapper_dbsr_krylov_ilu_(C.byref(C.c_int(len(ia) - 1)), C.byref(C.c_int(len(ja))), C.byref(C.c_int(nb)),
                                        A.ia.ctypes.data_as(T.c_int_p), A.ja.ctypes.data_as(T.c_int_p), _ptr(A.val),
                                        _ptr(bb), _ptr(x), C.byref(C.c_double(1e-8)), C.byref(C.c_int(300)),
                                        C.byref(C.c_int(0)))
    _, x2 = _krylov(ours, ia, ja, val, nb, b, T.SOLVER_VFGMRES, 0, 1e-8, maxit=300)
    assert x.tobytes() == x2.tobytes()
    assert _relres(ia, ja, val, nb, b, x) < 1e-8


def test_residency(libs):
    ours, ref = libs
    ia, ja, val, nb, b = spe01()
    n = len(b)
    for _ in range(20):
        A, d = Bsr(ia, ja, val, nb), T.ILU_data()
        assert ours.fasp_ilu_dbsr_setup(C.byref(A.M), C.byref(d), C.byref(ilu_param(ours, T.ILUk, 0))) == 0
        assert ours.fasp_hip_ilu_resident_count() == 0
        z = np.zeros(n)
        ours.fasp_precond_dbsr_ilu(_ptr(np.array(b)), _ptr(z), _vp(d))
        assert ours.fasp_hip_ilu_resident_count() == 1
        ours.fasp_ilu_data_free(C.byref(d))
        assert ours.fasp_hip_ilu_resident_count() == 0
        st, _ = _krylov(ours, ia, ja, val, nb, b, T.SOLVER_BiCGstab, 0, 1e-8)
        assert st > 0 and ours.fasp_hip_ilu_resident_count() == 0
    # a scalar factor and a block factor resident at once: each gives its own reference z (the kind record decides;
    # the scalar setup leaves ILU_data.nb as the caller's struct held it, here 3)
    csr = read_csr(DATA + "/csrmat_FE.dat")
    Ac1, Ac2, dc1, dc2 = Csr(*csr), Csr(*csr), T.ILU_data(), T.ILU_data()
    dc1.nb = dc2.nb = 3
    Ab1, Ab2, db1, db2 = Bsr(ia, ja, val, nb), Bsr(ia, ja, val, nb), T.ILU_data(), T.ILU_data()
    assert ours.fasp_ilu_dcsr_setup(C.byref(Ac1.M), C.byref(dc1), C.byref(ilu_param(ours, T.ILUk, 1))) == 0
    assert ref.fasp_ilu_dcsr_setup(C.byref(Ac2.M), C.byref(dc2), C.byref(ilu_param(ref, T.ILUk, 1))) == 0
    assert ours.fasp_ilu_dbsr_setup(C.byref(Ab1.M), C.byref(db1), C.byref(ilu_param(ours, T.ILUk, 1))) == 0
    assert ref.fasp_ilu_dbsr_setup(C.byref(Ab2.M), C.byref(db2), C.byref(ilu_param(ref, T.ILUk, 1))) == 0
    try:
        nc = len(csr[0]) - 1
        rc, rb = np.random.default_rng(1).uniform(-1, 1, nc), np.random.default_rng(2).uniform(-1, 1, n)
        for _ in range(2):
            zc, zc_ref, zb, zb_ref = np.zeros(nc), np.zeros(nc), np.zeros(n), np.zeros(n)
            ours.fasp_precond_ilu(_ptr(rc.copy()), _ptr(zc), _vp(dc1))
            ours.fasp_precond_dbsr_ilu(_ptr(rb.copy()), _ptr(zb), _vp(db1))
            ref.fasp_precond_ilu(_ptr(rc.copy()), _ptr(zc_ref), _vp(dc2))
            ref.fasp_precond_dbsr_ilu(_ptr(rb.copy()), _ptr(zb_ref), _vp(db2))
            assert zc.tobytes() == zc_ref.tobytes() and zb.tobytes() == zb_ref.tobytes()
            assert ours.fasp_hip_ilu_resident_count() == 2
    finally:
        for L, d in ((ours, dc1), (ref, dc2), (ours, db1), (ref, db2)):
            L.fasp_ilu_data_free(C.byref(d))
    assert ours.fasp_hip_ilu_resident_count() == 0


def test_scale_p7_64_bicgstab(libs):
    ours, ref = libs
    ia, ja, val, nb = poisson7pt_bsr(64)
    b = np.random.default_rng(64).uniform(-1.0, 1.0, (len(ia) - 1) * nb)
    it1, x1 = _krylov(ours, ia, ja, val, nb, b, T.SOLVER_BiCGstab, 0, 1e-8)
    it2, x2 = _krylov(ref, ia, ja, val, nb, b, T.SOLVER_BiCGstab, 0, 1e-8)
    # BiCGstab on 786k unknowns from a random right-hand side: the device's reduction order shifts the count by a few
    # (54 against 51 measured); CG on the same operator matches exactly (test_cg_spd_p7_b3)
    assert it2 > 0 and abs(it1 - it2) <= max(3, it2 // 10), (it1, it2)
    assert _relres(ia, ja, val, nb, b, x1) <= 1e-8


def test_scale_p7_128(libs):
    ours, ref = libs
    ia, ja, val, nb = poisson7pt_bsr(128)
    n = (len(ia) - 1) * nb
    r = np.random.default_rng(128).uniform(-1.0, 1.0, n)
    A1, d1, A2, d2 = Bsr(ia, ja, val, nb), T.ILU_data(), Bsr(ia, ja, val, nb), T.ILU_data()
    assert ours.fasp_ilu_dbsr_setup(C.byref(A1.M), C.byref(d1), C.byref(ilu_param(ours, T.ILUk, 0))) == 0
    assert ref.fasp_ilu_dbsr_setup(C.byref(A2.M), C.byref(d2), C.byref(ilu_param(ref, T.ILUk, 0))) == 0
    try:
        z, zr = np.zeros(n), np.zeros(n)
        ours.fasp_precond_dbsr_ilu(_ptr(r.copy()), _ptr(z), _vp(d1))
        ref.fasp_precond_dbsr_ilu(_ptr(r.copy()), _ptr(zr), _vp(d2))
        assert z.tobytes() == zr.tobytes()
    finally:
        ours.fasp_ilu_data_free(C.byref(d1)); ref.fasp_ilu_data_free(C.byref(d2))
    st, x = _krylov(ours, ia, ja, val, nb, r, T.SOLVER_BiCGstab, 0, 1e-8)
    assert st > 0
    assert _relres(ia, ja, val, nb, r, x) < 1e-7
