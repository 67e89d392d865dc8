"""ILU smoothing on the top levels of the block AMG cycle (AMG_param.ILU_levels > 0; csrc/ilu.hip.h bsr_ilu_smooth, csrc/bsr.hip.h
mgcycle_bsr) on the device against the compiled reference (fasp_solver_mgcycle_bsr, PreMGCycle.c:321-326 / :508-512):
  1. one application of the preconditioner, nb 1..7, both forms of the triangular solves, 0 / 1 / 2 Gauss-Seidel sweeps behind
     the ILU step;
  2. levels with a factor ignore AMG_param.smoother;
  3. whole solves: the reference's iteration counts (pinned from the compiled reference on a CPU machine), iterates, residuals;
  4. the shipped ini tests/golden/data/ini/bamg.dat (AMG_ILU_levels = 1) solves;
  5. twenty create -> solve -> destroy rounds leave no device memory and no registered factor behind.
Every test here needs ILU_levels > 0 to be accepted by the block path."""
import ctypes as C
import os

import numpy as np
import pytest

import _libs
from _libs import T, bsr_params, bsr_protos, poisson7pt_bsr, ref_bsr_solve

pytestmark = [pytest.mark.gpu, pytest.mark.ref]
P = C.POINTER
INI = os.path.join(_libs.DATA, "ini", "bamg.dat")


def block(nb):
    """B3 of the suite for nb = 3; else 3 I plus ones on the first off-diagonals"""
    if nb == 3:
        return _libs.B3
    return 3.0 * np.eye(nb) + np.eye(nb, k=1) + np.eye(nb, k=-1)


def system(n, nb):
    ia, ja, val, nb = poisson7pt_bsr(n, block(nb))
    f = np.sin(0.37 * np.arange((len(ia) - 1) * nb)) + 0.1
    return ia, ja, val, nb, f


def params(agg=2, ilu_levels=1, lfil=0, solver=T.SOLVER_VGMRES, cycle=T.V_CYCLE, steps=1, smoother=T.SMOOTHER_JACOBI):
    itp, amgp = bsr_params(solver, cycle, agg)
    amgp.coarse_dof = 50
    amgp.ILU_levels, amgp.ILU_lfil = ilu_levels, lfil
    amgp.presmooth_iter = amgp.postsmooth_iter = steps
    amgp.smoother = smoother
    amgp.relaxation = 1.1 if smoother == T.SMOOTHER_SOR else 1.0
    return itp, amgp


@pytest.fixture(scope="module")
def libs(gpu):
    _, R = bsr_protos()
    if R is None:
        pytest.fail("the reference build (oracle/_ref/libfasp_ref.so) is missing")
    ours = gpu.lib()
    ours.fasp_hip_ilu_resident_count.restype = C.c_int
    yield gpu, R
    ours.fasp_hip_tune(b"ilu_form", -1)


_ref_h = {}


def ref_precond(R, n, nb, amgp, r):
    """z = B r by the reference (ref_bsr_precond); its hierarchy is built once per (system, setup parameters)"""
    key = (n, nb, amgp.aggregation_type, amgp.ILU_levels, amgp.ILU_lfil)
    if key not in _ref_h:
        ia, ja, val, nb, _ = system(n, nb)
        A, keep = T.as_bsr(ia, ja, val, nb)
        _, p = params(amgp.aggregation_type, amgp.ILU_levels, amgp.ILU_lfil)
        h = R.ref_bsr_setup_ua(C.byref(A), C.byref(p))
        assert h
        _ref_h[key] = (h, A, keep)
    h, A, keep = _ref_h[key]
    fn = C.CFUNCTYPE(None, C.c_void_p, P(T.AMG_param), P(T.dBSRmat), T.c_double_p, T.c_double_p)(("ref_bsr_precond", R))
    z = np.zeros(len(r)); rr = r.copy()
    fn(h, C.byref(amgp), C.byref(A), T.dp(rr), T.dp(z))
    return z, R.ref_bsr_num_levels(h)


# (n, nb, form the schedule's depth selects: P7(6) has 16 dependency levels -- level launches --, P7(10) 28 -- the single launch)
APPLY = [(6, 1, 0), (6, 2, 0), (6, 3, 0), (6, 5, 0), (6, 7, 0), (10, 3, 1)]


@pytest.mark.parametrize("steps", [0, 1, 2])
@pytest.mark.parametrize("n,nb,auto_form", APPLY)
def test_one_application_equals_reference(libs, n, nb, auto_form, steps):
    gpu, R = libs
    ia, ja, val, nb, _ = system(n, nb)
    r = np.random.default_rng(100 * n + nb).uniform(-1.0, 1.0, (len(ia) - 1) * nb)
    _, p_ref = params(steps=steps)
    z_ref, nl_ref = ref_precond(R, n, nb, p_ref, r)
    _, p = params(steps=steps)
    G = gpu.BSRAMG(ia, ja, val, nb, p)
    try:
        nl = G.num_levels
        assert nl == nl_ref >= 2
        info = G.ilu_info(0)
        assert info is not None and G.ilu_info(nl - 1) is None
        assert info[0] == info[1] == 3 * n - 2 and info[2] == info[3] == auto_form
        assert info[4] >= (n ** 3 + 63) // 64 and info[5] >= (n ** 3 + 63) // 64
        for form in (0, 1):
            gpu.lib().fasp_hip_tune(b"ilu_form", form)
            assert G.ilu_info(0)[2:4] == (form, form)
            z = G.precond(r)
            err = np.max(np.abs(z - z_ref)) / np.max(np.abs(z_ref))
            print("P7(%d) (x) B%d, %d sweeps, form %d: max|z - z_ref| / max|z_ref| = %.3e" % (n, nb, steps, form, err))
            assert err <= 1e-9, (form, err)
    finally:
        gpu.lib().fasp_hip_tune(b"ilu_form", -1)
        G.free()


def test_ilu_levels_ignore_the_callers_smoother(libs):
    gpu, _ = libs
    ia, ja, val, nb, _ = system(6, 3)
    r = np.random.default_rng(5).uniform(-1.0, 1.0, (len(ia) - 1) * nb)
    out = []
    for sm in (T.SMOOTHER_JACOBI, T.SMOOTHER_SOR):
        _, p = params(smoother=sm)
        G = gpu.BSRAMG(ia, ja, val, nb, p)
        assert G.num_levels == 2   # level 0 is the only smoothed level
        out.append(G.precond(r))
        G.free()
    assert np.any(out[0] != 0.0) and out[0].tobytes() == out[1].tobytes()


def _relres(ia, ja, val, nb, b, x):
    A, keep = T.as_bsr(ia, ja, val, nb)
    y = np.zeros(len(b)); xx = np.array(x)
    _libs.oracle().orc_bsr_mxv(C.byref(A), T.dp(xx), T.dp(y))
    return np.linalg.norm(b - y) / np.linalg.norm(b)


# (n, nb, aggregation, ILU_levels, solver, cycle, lfil, the compiled reference's count on a CPU machine or None)
VG, CG, BCGS = T.SOLVER_VGMRES, T.SOLVER_CG, T.SOLVER_BiCGstab
SOLVES = [(6, 3, 2, 1, VG, 1, 0, 5), (6, 3, 2, 2, VG, 1, 0, 5),
          (10, 3, 1, 1, VG, 1, 0, 7), (10, 3, 1, 2, VG, 1, 0, 6),
          (12, 3, 2, 1, VG, 1, 0, 8), (12, 3, 2, 2, VG, 1, 0, 7),
          (10, 2, 1, 1, VG, 1, 0, 7), (10, 2, 1, 2, VG, 1, 0, 6),
          (10, 5, 1, 1, VG, 1, 0, 7), (10, 5, 1, 2, VG, 1, 0, 6),
          (12, 3, 2, 1, CG, 1, 0, None), (12, 3, 2, 2, CG, 1, 0, None),
          (12, 3, 2, 1, BCGS, 1, 0, None), (12, 3, 2, 2, BCGS, 1, 0, None),
          (12, 3, 2, 2, VG, T.W_CYCLE, 0, None),
          (10, 3, 1, 1, VG, 1, 1, None)]


@pytest.mark.parametrize("n,nb,agg,ilu_levels,solver,cycle,lfil,pinned", SOLVES)
def test_solve_equals_reference(libs, n, nb, agg, ilu_levels, solver, cycle, lfil, pinned):
    gpu, R = libs
    ia, ja, val, nb, f = system(n, nb)
    i1, a1 = params(agg, ilu_levels, lfil, solver, cycle)
    i2, a2 = params(agg, ilu_levels, lfil, solver, cycle)
    x1 = np.zeros(len(f))
    it1 = gpu.solver_dbsr_krylov_amg(ia, ja, val, nb, f, x1, i1, a1)
    it2, x2 = ref_bsr_solve(ia, ja, val, nb, f, i2, a2)
    print("P7(%d) (x) B%d agg %d ILU_levels %d solver %d cycle %d lfil %d: %d iterations, reference %d, pinned %s"
          % (n, nb, agg, ilu_levels, solver, cycle, lfil, it1, it2, pinned))
    assert a1.ILU_levels == a2.ILU_levels == ilu_levels
    if pinned is not None:
        assert it1 == pinned, (it1, it2)
    # the reference run in this process is the yardstick wherever it reproduces the pinned count itself
    if pinned is None or it2 == pinned:
        assert it1 == it2 > 0, (it1, it2)
        assert np.max(np.abs(x1 - x2)) <= 1e-8 * np.max(np.abs(x2))
        r1, r2 = _relres(ia, ja, val, nb, f, x1), _relres(ia, ja, val, nb, f, x2)
        assert abs(r1 - r2) <= 1e-10, (r1, r2)
    assert _relres(ia, ja, val, nb, f, x1) <= 1e-8


def test_handle_api_equals_dropin(libs):
    """fasp_hip_bsr_amg_create + fasp_hip_bsr_solve give the bytes of fasp_solver_dbsr_krylov_amg"""
    gpu, _ = libs
    ia, ja, val, nb, f = system(10, 3)
    i1, a1 = params(1, 2); i2, a2 = params(1, 2)
    x1 = np.zeros(len(f))
    it1 = gpu.solver_dbsr_krylov_amg(ia, ja, val, nb, f, x1, i1, a1)
    G = gpu.BSRAMG(ia, ja, val, nb, a2)
    assert G.num_levels == 3 and G.ilu_info(0) is not None and G.ilu_info(1) is not None and G.ilu_info(2) is None
    it2, x2, hist, stats = G.solve(f, i2)
    G.free()
    assert it1 == it2 == 6 and x1.tobytes() == x2.tobytes()


def test_shipped_ini_solves(libs):
    gpu, R = libs
    L = gpu.lib()
    pairs = []
    for _ in range(2):
        itp, amgp = T.ITS_param(), T.AMG_param()
        assert L.fasp_hip_param_input(INI.encode(), C.byref(itp), C.byref(amgp)) >= 0
        assert amgp.ILU_levels == 1 and amgp.SWZ_levels == 0 and amgp.AMG_type == T.UA_AMG
        pairs.append((itp, amgp))
    ia, ja, val, nb, f = system(10, 3)
    x1 = np.zeros(len(f))
    it1 = gpu.solver_dbsr_krylov_amg(ia, ja, val, nb, f, x1, *pairs[0])
    it2, x2 = ref_bsr_solve(ia, ja, val, nb, f, *pairs[1])
    assert it1 == it2 > 0, (it1, it2)
    assert np.max(np.abs(x1 - x2)) <= 1e-8 * np.max(np.abs(x2))
    assert _relres(ia, ja, val, nb, f, x1) <= pairs[0][0].tol


def _hip_runtime():
    """the HIP runtime this process has loaded (libfasp_hip.so links it)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    pytest.fail("libamdhip64 is not loaded")


def _free_bytes(hip):
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_lifetime(libs):
    gpu, _ = libs
    L = gpu.lib()
    ia, ja, val, nb, f = system(10, 3)

    def one_round():
        itp, amgp = params(1, 2)
        G = gpu.BSRAMG(ia, ja, val, nb, amgp)
        assert L.fasp_hip_ilu_resident_count() == 0
        st, x, hist, stats = G.solve(f, itp)
        assert st == 6 and L.fasp_hip_ilu_resident_count() == 0
        G.free()
        assert L.fasp_hip_ilu_resident_count() == 0
        return x.tobytes()

    hip = _hip_runtime()
    first = one_round()   # (work space the library keeps for the process is allocated by now)
    start = _free_bytes(hip)
    for _ in range(20):
        assert one_round() == first
    assert _free_bytes(hip) == start
