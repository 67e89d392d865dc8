"""The solver-level entry points next to the AMG drop-in: fasp_solver_dcsr_itsolver / _krylov / _krylov_diag
(SolCSR.c:56/:245/:333) and their block twins (SolBSR.c:64/:145/:186) -- what test/main/regression.c drives for its
"CG solver", "Diagonal preconditioned CG solver", "... in BSR format" problems.  Checked on the GPU against the compiled
reference (same entry points, CPU) where it is available, else against the oracle's Krylov restatements."""
import ctypes as C

import numpy as np
import pytest

import faspsolver_amd as fa
from faspsolver_amd import _types as T

from _libs import default_params, have_ref, poisson7pt, poisson7pt_bsr, ref
from test_plugin_krylov import diag_pc, orc_krylov

pytestmark = pytest.mark.gpu
WHICH = {1: 0, 2: 3, 3: 5, 4: 4, 5: 1, 6: 2, 7: 6, 8: 7}   # itsolver_type -> oracle `which`


def _rhs(n):
    return np.random.default_rng(11).standard_normal(n)


def _call(lib_, name, A, f, itp):
    fn = getattr(lib_, name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(T.dvector), C.POINTER(T.dvector), C.POINTER(T.ITS_param)]
    x = np.zeros(len(f)); bv, fk = T.as_vec(f); xv = T.dvector(len(f), T.dp(x))
    st = fn(C.addressof(A), C.byref(bv), C.byref(xv), C.byref(itp))
    return st, x


@pytest.mark.parametrize("solver", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("entry", ["fasp_solver_dcsr_krylov", "fasp_solver_dcsr_krylov_diag"])
def test_csr_krylov_entry_points(entry, solver):
    ia, ja, a, f, ue = poisson7pt(12)
    f = _rhs(len(f))
    itp, _ = default_params(); itp.tol = 1e-8; itp.itsolver_type = solver; itp.restart = 20; itp.maxit = 400
    A, keep = T.as_csr(ia, ja, a)
    s2, x2 = _call(fa.lib(), entry, A, f, itp)
    fct = diag_pc(ia, ja, a) if entry.endswith("diag") else None
    s1, x1, rr = orc_krylov(WHICH[solver], ia, ja, a, f, fct, maxit=400, restart=20)
    if solver == 2:   # BiCGstab on a rough right-hand side: the iteration count moves with the last bits of the dots
        assert abs(s1 - s2) <= 4 and s2 > 0
        assert np.abs(x1 - x2).max() <= 1e-6 * np.abs(x1).max()
    else:
        assert s1 == s2 and s1 > 5
        assert np.abs(x1 - x2).max() <= 1e-9 * np.abs(x1).max()
    if have_ref():
        itp2, _ = default_params(); itp2.tol = 1e-8; itp2.itsolver_type = solver; itp2.restart = 20; itp2.maxit = 400
        s3, x3 = _call(ref(), entry, A, f, itp2)
        assert s3 == s1 and np.array_equal(x3, x1)   # the oracle's restatement IS the reference's entry point


@pytest.mark.parametrize("solver", [1, 4, 5, 6])
@pytest.mark.parametrize("entry", ["fasp_solver_dbsr_krylov", "fasp_solver_dbsr_krylov_diag"])
def test_bsr_krylov_entry_points(entry, solver):
    if not have_ref():
        pytest.skip("block Krylov entry points are checked against the compiled reference")
    ia, ja, val, nb = poisson7pt_bsr(8)
    n = (len(ia) - 1) * nb
    f = _rhs(n)
    A, keep = T.as_bsr(ia, ja, val, nb)
    itp, _ = default_params(); itp.tol = 1e-8; itp.itsolver_type = solver; itp.restart = 20; itp.maxit = 600
    itp2, _ = default_params(); itp2.tol = 1e-8; itp2.itsolver_type = solver; itp2.restart = 20; itp2.maxit = 600
    s1, x1 = _call(ref(), entry, A, f, itp2)
    s2, x2 = _call(fa.lib(), entry, A, f, itp)
    assert s1 == s2 and s1 > 5
    assert np.abs(x1 - x2).max() <= 1e-9 * np.abs(x1).max()


def test_unknown_solver_type_is_refused():
    ia, ja, a, f, ue = poisson7pt(6)
    A, keep = T.as_csr(ia, ja, a)
    itp, _ = default_params(); itp.itsolver_type = 13   # SOLVER_SMinRes belongs to fasp_solver_dcsr_itsolver_s
    st, x = _call(fa.lib(), "fasp_solver_dcsr_krylov", A, f, itp)
    assert st == T.ERROR_SOLVER_TYPE and not x.any()


# ---- resident handles: the Krylov workspace a handle owns ------------------------------------------------
def _jacobi_params(solver, restart):
    itp, amgp = default_params()
    itp.tol = 1e-8; itp.itsolver_type = solver; itp.restart = restart
    amgp.smoother = T.SMOOTHER_JACOBI; amgp.relaxation = 0.6667
    return itp, amgp


def _same(r1, r2):
    """status, solution and residual history of two solves, bit for bit"""
    return r1[0] == r2[0] and np.array_equal(r1[1], r2[1]) and np.array_equal(r1[2], r2[2])


def test_gpu_workspace_reuse_across_methods():
    """One handle, methods whose workspaces differ in the number of vectors, one after the other: every driver writes a
    workspace vector before it reads it, so a solve does not see what the solve before it left behind."""
    ia, ja, a, f, ue = poisson7pt(8)
    f = _rhs(len(f))
    order = [(T.SOLVER_VGMRES, 5), (T.SOLVER_BiCGstab, 5), (T.SOLVER_VFGMRES, 30), (T.SOLVER_MinRes, 30), (T.SOLVER_VGMRES, 5)]
    H = fa.AMG(ia, ja, a, _jacobi_params(1, 30)[1])
    got = [H.solve(f, _jacobi_params(solver, restart)[0])[:3] for solver, restart in order]
    H.close()
    assert all(g[0] > 0 for g in got)
    assert _same(got[0], got[4])
    for (solver, restart), g in zip(order, got):
        F = fa.AMG(ia, ja, a, _jacobi_params(1, 30)[1])
        fresh = F.solve(f, _jacobi_params(solver, restart)[0])[:3]
        F.close()
        assert _same(g, fresh), (solver, restart)


def test_gpu_two_handles_interleaved():
    """A CSR and a BSR handle alive together, solved in turn and destroyed in the opposite order of creation: each handle
    owns its Krylov workspace, the results are those of the handles alone."""
    from _libs import bsr_params
    ia, ja, a, f, ue = poisson7pt(8)
    f = _rhs(len(f))
    bia, bja, bval, nb = poisson7pt_bsr(6)
    bf = _rhs((len(bia) - 1) * nb)
    H = fa.AMG(ia, ja, a, _jacobi_params(1, 30)[1])
    G = fa.BSRAMG(bia, bja, bval, nb, bsr_params()[1])
    c1 = H.solve(f, _jacobi_params(T.SOLVER_VGMRES, 30)[0])[:3]
    b1 = G.solve(bf, bsr_params(T.SOLVER_VGMRES)[0])[:3]
    c2 = H.solve(f, _jacobi_params(T.SOLVER_VGMRES, 30)[0])[:3]
    G.free()
    H.close()
    assert c1[0] > 0 and b1[0] > 0
    assert _same(c1, c2)
    H = fa.AMG(ia, ja, a, _jacobi_params(1, 30)[1])
    c0 = H.solve(f, _jacobi_params(T.SOLVER_VGMRES, 30)[0])[:3]
    H.close()
    G = fa.BSRAMG(bia, bja, bval, nb, bsr_params()[1])
    b0 = G.solve(bf, bsr_params(T.SOLVER_VGMRES)[0])[:3]
    G.free()
    assert _same(c1, c0) and _same(b1, b0)
