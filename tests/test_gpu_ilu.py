"""ILU preconditioner on the device (csrc/ilu.hip.h) against the compiled reference:
  1. fasp_precond_ilu / _forward / _backward give the reference's z byte for byte, with both forms of the triangular
     solves (fasp_hip_tune("ilu_form", 0 / 1)); fasp_smoother_dcsr_ilu to 1e-14 relative (its residual b - A x comes from
     this library's SpMV kernels, whose sums may be ordered differently from the reference's aAxpy);
  2. the ILU cases of the reference's regression test (test/main/regression.c:798-848, reg.out iteration counts);
  3. every Krylov method of fasp_solver_dcsr_itsolver with ILU(0) and ILUt on FE and P7(24): the reference's iteration
     counts, final residuals to the usual rule (BiCGstab / MinRes on FE: to 1e-3, see the test);
  4. fasp_precond_setup(PREC_ILU) + fasp_solver_dcsr_pcg, twenty rounds, no device factor left behind;
  5. ILU-CG at P7(64) / P7(128).
Schedule edges and hand-built factors: see test_gpu_ilu_kernels.py."""
import ctypes as C

import numpy as np
import pytest

import _libs
from _libs import DATA, T, poisson7pt, read_csr, read_vec, read_vecind
from test_ilu_setup import Csr, PARAMS, ilu_param, ilu_protos, matrices, nos7

pytestmark = [pytest.mark.gpu, pytest.mark.ref]
P = C.POINTER


@pytest.fixture(scope="module")
def libs(gpu):
    ref = _libs.ref()
    if ref is None:
        pytest.fail("the reference build (oracle/_ref/libfasp_ref.so) is missing")
    ours = ilu_protos(gpu.lib())
    ours.fasp_hip_ilu_resident_count.restype = C.c_int
    ours.fasp_precond_setup.argtypes = [C.c_short, P(T.AMG_param), P(T.ILU_param), P(T.dCSRmat)]
    ours.fasp_precond_setup.restype = P(T.precond)
    ours.fasp_mem_free.argtypes = [C.c_void_p]
    ours.fasp_mem_free.restype = None
    for L in (ours, ref):
        L.fasp_solver_dcsr_pcg.argtypes = [P(T.dCSRmat), P(T.dvector), P(T.dvector), P(T.precond), C.c_double, C.c_double,
                                           C.c_int, C.c_short, C.c_short]
        L.fasp_solver_dcsr_pcg.restype = C.c_int
    yield ours, ilu_protos(ref)
    ours.fasp_hip_tune(b"ilu_form", -1)


@pytest.fixture(scope="module")
def mats():
    return matrices()


def _ptr(v):
    return v.ctypes.data_as(T.c_double_p)


def _vec(v):
    return T.dvector(len(v), _ptr(v))


@pytest.mark.parametrize("mname", ["FD", "FE", "NOS7", "P7_8", "P7_16", "nonsym"])
@pytest.mark.parametrize("pname,typ,lfil,droptol,permtol", PARAMS)
def test_apply_bitwise(libs, mats, mname, pname, typ, lfil, droptol, permtol):
    ours, ref = libs
    arrays = mats[mname]
    n = len(arrays[0]) - 1
    r = np.random.default_rng(11).uniform(-1.0, 1.0, n)
    A1, d1 = Csr(*arrays), T.ILU_data()
    A2, d2 = Csr(*arrays), T.ILU_data()
    assert ours.fasp_ilu_dcsr_setup(C.byref(A1.M), C.byref(d1), C.byref(ilu_param(ours, typ, lfil, droptol, permtol))) == 0
    assert ref.fasp_ilu_dcsr_setup(C.byref(A2.M), C.byref(d2), C.byref(ilu_param(ref, typ, lfil, droptol, permtol))) == 0
    try:
        for fn in ("fasp_precond_ilu", "fasp_precond_ilu_forward", "fasp_precond_ilu_backward"):
            zr = np.zeros(n)
            getattr(ref, fn)(_ptr(r.copy()), _ptr(zr), C.cast(C.byref(d2), C.c_void_p))
            for form in (0, 1):
                ours.fasp_hip_tune(b"ilu_form", form)
                z = np.full(n, np.nan)
                getattr(ours, fn)(_ptr(r.copy()), _ptr(z), C.cast(C.byref(d1), C.c_void_p))
                assert z.tobytes() == zr.tobytes(), (fn, form, np.max(np.abs(z - zr)))
        ours.fasp_hip_tune(b"ilu_form", -1)
        # the smoother: x += (LU)^-1 (b - A x) on the (ILUtp: renumbered) matrix
        b = np.random.default_rng(12).uniform(-1.0, 1.0, n)
        x0 = np.random.default_rng(13).uniform(-1.0, 1.0, n)
        x1, x2 = x0.copy(), x0.copy()
        ours.fasp_smoother_dcsr_ilu(C.byref(A1.M), C.byref(_vec(b)), C.byref(_vec(x1)), C.cast(C.byref(d1), C.c_void_p))
        ref.fasp_smoother_dcsr_ilu(C.byref(A2.M), C.byref(_vec(b)), C.byref(_vec(x2)), C.cast(C.byref(d2), C.c_void_p))
        assert np.max(np.abs(x1 - x2)) <= 1e-14 * np.max(np.abs(x2))
    finally:
        ours.fasp_ilu_data_free(C.byref(d1)); ref.fasp_ilu_data_free(C.byref(d2))
    assert ours.fasp_hip_ilu_resident_count() == 0


def _dvec_rand(n):
    """fasp_dvec_rand (AuxVector.c:192): glibc srand(1) / rand(), j = 1 + floor(n rand / (RAND_MAX + 1)), x_i = j / n"""
    libc = C.CDLL(None)
    libc.rand.restype = C.c_int
    libc.srand(1)
    return np.array([float(1 + int(float(n) * libc.rand() / (2147483647 + 1.0))) / n for _ in range(n)])


def _problem(name):
    if name == "FD":
        ia, ja, a = read_csr(DATA + "/csrmat_FD.dat")
        return ia, ja, a, read_vec(DATA + "/rhs_FD.dat"), read_vecind(DATA + "/sol_FD.dat")
    if name == "FE":
        ia, ja, a = read_csr(DATA + "/csrmat_FE.dat")
        return ia, ja, a, read_vec(DATA + "/rhs_FE.dat"), read_vecind(DATA + "/sol_FE.dat")
    ia, ja, a = nos7()
    sol = _dvec_rand(len(ia) - 1)
    b = np.zeros(len(sol))
    A = Csr(ia, ja, a)
    _libs.oracle().orc_mxv(C.byref(A.M), _ptr(sol), _ptr(b))
    return ia, ja, a, b, sol


def _krylov_ilu(L, arrays, b, typ, lfil, tol, maxit=500, solver=T.SOLVER_CG, droptol=1e-3):
    A = Csr(*arrays)
    x = np.zeros(len(b))
    it = T.ITS_param()
    L.fasp_param_solver_init(C.byref(it))
    it.maxit, it.tol, it.print_level, it.itsolver_type = maxit, tol, 0, solver
    prm = ilu_param(L, typ, lfil, droptol, 0.01)
    bb = np.array(b)   # (kept alive across the call)
    st = L.fasp_solver_dcsr_krylov_ilu(C.byref(A.M), C.byref(_vec(bb)), C.byref(_vec(x)), C.byref(it), C.byref(prm))
    assert A.ja.tobytes() == np.ascontiguousarray(arrays[1], np.int32).tobytes()   # ILUtp: numbered back by the free
    return st, x


def _relres(arrays, b, x):
    A = Csr(*arrays)
    y = np.zeros(len(b))
    xx = np.array(x)
    _libs.oracle().orc_mxv(C.byref(A.M), _ptr(xx), _ptr(y))
    return np.linalg.norm(b - y) / np.linalg.norm(b)


REG = [("FD", T.ILUk, 1e-8, 7), ("FD", T.ILUt, 1e-10, 5), ("FD", T.ILUtp, 1e-10, 5),
       ("FE", T.ILUk, 1e-8, 41), ("FE", T.ILUt, 1e-10, 15), ("FE", T.ILUtp, 1e-10, 15),
       ("NOS7", T.ILUk, 1e-8, None), ("NOS7", T.ILUt, 1e-10, None), ("NOS7", T.ILUtp, 1e-10, None)]


@pytest.mark.parametrize("prob,typ,tol,pinned", REG)
def test_regression_cases(libs, prob, typ, tol, pinned):
    ours, ref = libs
    ia, ja, a, b, sol = _problem(prob)
    it1, x1 = _krylov_ilu(ours, (ia, ja, a), b, typ, 2, tol)
    it2, x2 = _krylov_ilu(ref, (ia, ja, a), b, typ, 2, tol)
    if pinned is not None:
        assert it1 == pinned, (it1, it2)   # reg.out
    # The reference build run in this process is the yardstick wherever it reproduces reg.out itself (on one GPU machine its
    # CG took 42 iterations for FE / ILUk where reg.out and the same build on a CPU-only machine take 41).
    if pinned is None or it2 == pinned:
        assert it1 == it2 > 0, (it1, it2)
        # (ILUtp: the solve ran on A with renumbered columns, x comes out in that numbering -- the reference's behaviour)
        r1, r2 = _relres((ia, ja, a), b, x1), _relres((ia, ja, a), b, x2)
        assert abs(r1 - r2) <= 1e-10 + 1e-6 * abs(r2), (r1, r2)
        assert np.max(np.abs(x1 - x2)) <= 1e-6 * np.max(np.abs(x2))
    if typ != T.ILUtp or np.max(np.abs(x2 - sol)) < 1e-4:
        assert np.max(np.abs(x1 - sol)) < 1e-4   # check_solu's tolerance (regression.c:56), where the reference passes it


SOLVERS = [T.SOLVER_CG, T.SOLVER_BiCGstab, T.SOLVER_MinRes, T.SOLVER_GMRES, T.SOLVER_VGMRES, T.SOLVER_VFGMRES,
           T.SOLVER_GCG, T.SOLVER_GCR]


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("typ,lfil", [(T.ILUk, 0), (T.ILUt, 2)])
@pytest.mark.parametrize("prob", ["FE", "P7_24"])
def test_every_krylov_method(libs, solver, typ, lfil, prob):
    ours, ref = libs
    if prob == "FE":
        ia, ja, a = read_csr(DATA + "/csrmat_FE.dat"); b = read_vec(DATA + "/rhs_FE.dat")
    else:
        ia, ja, a, b, _ = poisson7pt(24)
    it1, x1 = _krylov_ilu(ours, (ia, ja, a), b, typ, lfil, 1e-8, maxit=300, solver=solver)
    it2, x2 = _krylov_ilu(ref, (ia, ja, a), b, typ, lfil, 1e-8, maxit=300, solver=solver)
    assert it1 == it2, (it1, it2)
    r1, r2 = _relres((ia, ja, a), b, x1), _relres((ia, ja, a), b, x2)
    if solver in (T.SOLVER_BiCGstab, T.SOLVER_MinRes) and prob == "FE":
        # BiCGstab / MinRes amplify the rounding of the device's reductions on FE: same count, final residuals agree to
        # 1e-3 relative, or both are below the tolerance
        assert abs(r1 - r2) <= 1e-3 * abs(r2) or max(r1, r2) <= 1e-8, (r1, r2)
    else:
        assert abs(r1 - r2) <= 1e-10 + 1e-6 * abs(r2), (r1, r2)


def test_precond_object_rounds(libs):
    ours, ref = libs
    ia, ja, a = read_csr(DATA + "/csrmat_FE.dat"); b = read_vec(DATA + "/rhs_FE.dat")
    it_ref, x_ref = _krylov_ilu(ours, (ia, ja, a), b, T.ILUk, 0, 1e-8)
    for _ in range(20):
        A = Csr(ia, ja, a)
        prm = ilu_param(ours, T.ILUk, 0, 1e-3, 0.01)
        pc = ours.fasp_precond_setup(T.PREC_ILU, None, C.byref(prm), C.byref(A.M))
        assert pc and pc.contents.data
        x = np.zeros(len(b))
        bb = np.array(b)
        it = ours.fasp_solver_dcsr_pcg(C.byref(A.M), C.byref(_vec(bb)), C.byref(_vec(x)), pc, 1e-8, 1e-20, 500, 1, 0)
        assert ours.fasp_hip_ilu_resident_count() == 1
        assert it == it_ref and x.tobytes() == x_ref.tobytes()
        d = C.cast(pc.contents.data, P(T.ILU_data))
        ours.fasp_ilu_data_free(d)
        ours.fasp_mem_free(pc.contents.data); ours.fasp_mem_free(C.cast(pc, C.c_void_p))
    assert ours.fasp_hip_ilu_resident_count() == 0


@pytest.mark.parametrize("n,lfil", [(64, 0), (128, 0), (64, 2)])
def test_scale_p7(libs, n, lfil):
    ours, ref = libs
    ia, ja, a, b, _ = poisson7pt(n)
    it1, x1 = _krylov_ilu(ours, (ia, ja, a), b, T.ILUk, lfil, 1e-8)
    it2, x2 = _krylov_ilu(ref, (ia, ja, a), b, T.ILUk, lfil, 1e-8)
    assert it1 == it2 > 0
    assert np.max(np.abs(x1 - x2)) <= 1e-6 * np.max(np.abs(x2))
