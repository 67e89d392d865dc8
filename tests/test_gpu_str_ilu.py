"""Structured ILU(0) / ILU(1) on the device (csrc/str_ilu.hip.h): the triangular solves k_str_tri in both forms against the host
preconditioner functions, and the Krylov entries around them.

One application is compared with np.array_equal against fasp_precond_dstr_ilu0 / _ilu1 on host vectors, which tests/test_str_ilu_host.py
holds to the reference bit for bit: the device evaluates the reference's terms in the reference's order and skips only terms whose
coefficient the bind-time check has found to be exactly 0.0, so z can differ in the sign of a zero at most.  Every case generator asserts
that fasp_hip_str_ilu_form accepts the factor -- otherwise the test would silently exercise the staging path.

Solves, tol 1e-8 from a zero guess.  Device-bound against host-staged: the same z bit for bit, hence the same iterates -- equal counts and
array_equal x, no tolerance needed.  fasp_solver_dstr_krylov_ilu, nc = 1, against the reference's own: equal iteration counts and
max|x - x_ref| <= 1e-9 max|x_ref| (the rule of tests/test_gpu_str.py; the generator asserts that the reference's true residual is a factor
1.05 away from tol at its last step and at the one before).  CG runs on a symmetric 2-D system: on a 3-D grid the reference's scalar
ILU(0) is far from symmetric (BlaILUSetupSTR.c:144) and its own CG does not converge.  nc > 1 (the reference's STR solvers are not callable
there): true relative residual <= 1.01 tol, and for ILU(0) with nc = 2, 3 the count within one of the reference's BSR ILU(0) solve of the
converted matrix; for nc = 5 that factor is another one (fasp_ilu_dstr_setup0 inverts with fasp_smat_inv_nc5, whose closed form is not the
inverse; checked on the CPU by the generator), so only the residual bound is left, as for ILU(1)."""
import ctypes as C

import numpy as np
import pytest

import _libs
import _str_cases as S
import _str_ilu_cases as I
from _libs import T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(gpu):
    return I.protos(gpu.lib())


@pytest.fixture(scope="module")
def G():
    return np.load(I.GOLDEN)


@pytest.fixture(scope="module")
def R():
    lib = _libs.ref()
    return I.protos(lib) if lib is not None else None


@pytest.fixture(autouse=True)
def _tunes_back(gpu):
    yield
    lib = gpu.lib()
    lib.fasp_hip_tune(b"str_ilu_form", -1)
    lib.fasp_hip_tune(b"str_ilu_wgs", 0)


_FACTORS = {}


def factored(L, grid, nc, lfil):
    """(snapshot of the library's factor of the grid case, its right-hand side, z of the host function): computed once, read-only."""
    k = (grid, nc, lfil)
    if k not in _FACTORS:
        case = I.grid_case(grid, nc)
        snap = I.factor(L, case, lfil)
        r = I.rhs(case)
        z = I.host_apply(L, snap, lfil, r)
        for a in [snap["diag"], r, z] + snap["bands"]:
            a.setflags(write=False)
        _FACTORS[k] = (snap, r, z)
    return _FACTORS[k]


def dev_apply(L, snap, lfil, r, form, wgs=0):
    """One application on the device in `form` (0 level launches, 1 planes pipelined) -> (status, z)."""
    LU, keep = I.factor_struct(snap)
    L.fasp_hip_tune(b"str_ilu_form", form)
    L.fasp_hip_tune(b"str_ilu_wgs", wgs)
    assert L.fasp_hip_str_ilu_form(C.byref(LU), lfil) == form      # bindable, and the form the test is about
    z = np.full_like(r, np.nan)
    st = L.fasp_hip_str_ilu_apply(C.byref(LU), lfil, T.dp(np.array(r)), T.dp(z))
    return st, z


def check_apply(L, grid, nc, lfil, form, wgs=0):
    snap, r, want = factored(L, grid, nc, lfil)
    st, z = dev_apply(L, snap, lfil, r, form, wgs)
    assert st == 0                                               # the error word is clear
    bad = np.flatnonzero(z != want)
    assert bad.size == 0 and np.array_equal(z, want), (bad[:8], z[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("form", [0, 1], ids=["level", "pipe"])
@pytest.mark.parametrize("lfil", [0, 1])
@pytest.mark.parametrize("nc", [1, 2, 3, 5, 7])
@pytest.mark.parametrize("grid", [(5, 4, 3), (17, 9, 6)], ids=["5x4x3", "17x9x6"])
def test_one_application(L, grid, nc, lfil, form):
    check_apply(L, grid, nc, lfil, form)


# in-plane levels wider than a workgroup's 4 * (64 / nc) points, so that the sub-step loop of the pipelined form runs: 67 points against
# 36 (nc 7), 260 against 256 (nc 1); 70 x 67 x 3 with nc 1 and 3 fit in one step (256 and 84 points)
@pytest.mark.parametrize("form", [0, 1], ids=["level", "pipe"])
@pytest.mark.parametrize("lfil", [0, 1])
@pytest.mark.parametrize("grid,nc", [((70, 67, 3), 1), ((70, 67, 3), 3), ((70, 67, 3), 7), ((300, 260, 2), 1)],
                         ids=["70x67x3-nc1", "70x67x3-nc3", "70x67x3-nc7", "300x260x2-nc1"])
def test_wide_planes(L, grid, nc, lfil, form):
    check_apply(L, grid, nc, lfil, form)


@pytest.mark.parametrize("wgs", [1, 2])
@pytest.mark.parametrize("lfil", [0, 1])
@pytest.mark.parametrize("nc", [1, 3])
def test_ticket_loop_with_fewer_workgroups_than_planes(L, nc, lfil, wgs):
    """Nine planes on one and on two workgroups: a workgroup draws plane after plane; no residency is assumed."""
    check_apply(L, (6, 5, 9), nc, lfil, 1, wgs)


@pytest.mark.parametrize("lfil", [0, 1])
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("grid", [(9, 7, 1), (1, 8, 6)], ids=["9x7x1", "1x8x6"])
def test_2d_grids_run_the_level_form(L, grid, nc, lfil):
    snap, r, want = factored(L, grid, nc, lfil)
    LU, keep = I.factor_struct(snap)
    L.fasp_hip_tune(b"str_ilu_form", 1)
    assert L.fasp_hip_str_ilu_form(C.byref(LU), lfil) == 0       # nothing to pipeline, whatever is asked for
    z = np.full_like(r, np.nan)
    assert L.fasp_hip_str_ilu_apply(C.byref(LU), lfil, T.dp(np.array(r)), T.dp(z)) == 0
    assert np.array_equal(z, want)


def _pc(L, LU, lfil, foreign):
    """(precond, keepalive): the library's function -- recognised, device bound -- or the same function behind a ctypes trampoline, which
    is a foreign address and host staged."""
    f = getattr(L, f"fasp_precond_dstr_ilu{lfil}")
    if foreign:
        cb = T.PRECOND_FCT(lambda r, z, data: f(r, z, data))
    else:
        cb = C.cast(f, T.PRECOND_FCT)
    return T.precond(C.cast(C.pointer(LU), C.c_void_p), cb), cb


def _plugin_solve(L, entry, case, b, pc, restart=10, maxit=200):
    A, keep = I.as_str(case)
    x = np.zeros_like(b)
    bv, kb = T.as_vec(b)
    xv = T.dvector(x.size, T.dp(x))
    fn = getattr(L, "fasp_solver_dstr_" + entry)
    if entry in ("pgmres", "pvgmres"):
        it = fn(C.byref(A), C.byref(bv), C.byref(xv), C.byref(pc), I.TOL, 1e-18, maxit, restart, T.STOP_REL_RES, 0)
    else:
        it = fn(C.byref(A), C.byref(bv), C.byref(xv), C.byref(pc), I.TOL, 1e-18, maxit, T.STOP_REL_RES, 0)
    return it, x


def test_wrap_coefficient_is_not_bound_and_the_solve_still_converges(L):
    """One non-zero coefficient between grid points that are no geometric neighbours: the device skips such terms, so the factor is not
    bound; the solve goes through the host function, which evaluates it."""
    case, b = I.scalar_system(False)
    snap = I.factor(L, case, 0)
    LU, keep = I.factor_struct(snap)
    assert L.fasp_hip_str_ilu_form(C.byref(LU), 0) >= 0
    bands = [a.copy() for a in snap["bands"]]
    nx = case["nx"]
    assert bands[0][nx - 1] == 0.0               # row nx (x = 0) and column nx - 1 (x = nx - 1): the end of the first line
    bands[0][nx - 1] = 0.05
    snap2 = dict(snap, bands=bands)
    LU2, keep2 = I.factor_struct(snap2)
    assert L.fasp_hip_str_ilu_form(C.byref(LU2), 0) == -1
    assert L.fasp_hip_str_ilu_apply(C.byref(LU2), 0, T.dp(b.copy()), T.dp(np.zeros_like(b))) == T.ERROR_INPUT_PAR
    bands[0][nx - 1] = np.nan
    assert L.fasp_hip_str_ilu_form(C.byref(LU2), 0) == -1      # (LU2 views `bands`)
    bands[0][nx - 1] = 0.05
    pc, keep3 = _pc(L, LU2, 0, False)
    it, x = _plugin_solve(L, "pbcgs", case, b, pc)
    rr = I.true_relres(case, b, x)
    print(f"BiCGstab with the unbound factor: {it} iterations, true relative residual {rr:.3e}")
    assert it > 0 and rr <= 1.01 * I.TOL
    z_host = I.host_apply(L, snap2, 0, b)        # ... and the host function does use the coefficient
    assert not np.array_equal(z_host, I.host_apply(L, snap, 0, b))


@pytest.mark.parametrize("entry", ["pcg", "pbcgs", "pminres", "pgmres", "pvgmres"])
@pytest.mark.parametrize("lfil", [0, 1])
@pytest.mark.parametrize("nc", [1, 3])
def test_device_bound_and_host_staged_solves_are_the_same_solve(L, nc, lfil, entry):
    sym = entry in ("pcg", "pminres")
    case, b = I.scalar_system(sym) if nc == 1 else I.block_system(nc, sym)
    snap = I.factor(L, case, lfil)
    LU, keep = I.factor_struct(snap)
    assert L.fasp_hip_str_ilu_form(C.byref(LU), lfil) >= 0
    pc_dev, k1 = _pc(L, LU, lfil, False)
    pc_host, k2 = _pc(L, LU, lfil, True)
    it_dev, x_dev = _plugin_solve(L, entry, case, b, pc_dev)
    it_host, x_host = _plugin_solve(L, entry, case, b, pc_host)
    print(f"{entry} nc {nc} ILU({lfil}): {it_dev} iterations device bound, {it_host} host staged")
    assert it_dev == it_host and it_dev > 1
    assert np.array_equal(x_dev, x_host)


@pytest.mark.parametrize("lfil", [0, 1])
@pytest.mark.parametrize("key,sym,method,restart", I.SCALAR_SOLVES, ids=[s[0] for s in I.SCALAR_SOLVES])
def test_krylov_ilu_scalar_matches_the_reference(L, G, R, key, sym, method, restart, lfil):
    case, b = I.scalar_system(sym)
    it, x = I.solve_ilu(L, case, b, method, restart, lfil)
    it_g, x_g = int(G[f"solve_{key}_{lfil}_it"]), G[f"solve_{key}_{lfil}_x"]
    print(f"{key} ILU({lfil}): {it} iterations (recorded {it_g}), max|dx| / max|x| = {np.max(np.abs(x - x_g)) / np.max(np.abs(x_g)):.3e}")
    assert it == it_g
    assert np.max(np.abs(x - x_g)) <= 1e-9 * np.max(np.abs(x_g))
    if R is not None:
        it_r, x_r = I.solve_ilu(R, case, b, method, restart, lfil)
        assert it == it_r and np.max(np.abs(x - x_r)) <= 1e-9 * np.max(np.abs(x_r))


@pytest.mark.parametrize("lfil", [0, 1])
@pytest.mark.parametrize("key,sym,method,restart", I.BLOCK_SOLVES, ids=[s[0] for s in I.BLOCK_SOLVES])
@pytest.mark.parametrize("nc", I.BLOCK_NC)
def test_krylov_ilu_block(L, G, nc, key, sym, method, restart, lfil):
    case, b = I.block_system(nc, sym)
    it, x = I.solve_ilu(L, case, b, method, restart, lfil)
    rr = I.true_relres(case, b, x)
    rec = f"block_{nc}_{key}_it"
    it_g = int(G[rec]) if lfil == 0 and rec in G.files else None
    print(f"nc {nc} {key} ILU({lfil}): {it} iterations (reference BSR ILU(0): {it_g}), true relative residual {rr:.3e}")
    assert it > 0 and rr <= 1.01 * I.TOL
    assert (rec in G.files) == (nc in I.BLOCK_COUNT_NC)
    if it_g is not None:
        assert abs(it - it_g) <= 1


def test_krylov_ilu_refusals(L):
    case, b = I.scalar_system(False)
    A, keep = I.as_str(case)
    x = np.full_like(b, 0.25)
    bv, kb = T.as_vec(b)
    xv = T.dvector(x.size, T.dp(x))
    p = S.its_param(T.SOLVER_BiCGstab, 25)
    for lfil in (2, -1):
        assert L.fasp_solver_dstr_krylov_ilu(C.byref(A), C.byref(bv), C.byref(xv), C.byref(p), C.byref(I.ilu_param(lfil))) == T.ERROR_MISC
    four = dict(case, offsets=case["offsets"][:4], bands=case["bands"][:4])   # a 2-D stencil on a 3-D grid: the factorisation refuses it
    A4, keep4 = I.as_str(four)
    for lfil in (0, 1):
        assert L.fasp_solver_dstr_krylov_ilu(C.byref(A4), C.byref(bv), C.byref(xv), C.byref(p), C.byref(I.ilu_param(lfil))) == T.ERROR_INPUT_PAR
    assert L.fasp_solver_dstr_krylov_ilu(C.byref(A), C.byref(bv), C.byref(xv), None, C.byref(I.ilu_param(0))) == T.ERROR_INPUT_PAR
    assert np.all(x == 0.25)
    LU = T.dSTRmat()
    assert L.fasp_hip_str_ilu_form(C.byref(LU), 0) == -1 and L.fasp_hip_time_str_ilu(C.byref(LU), 0, 3) == -1.0
