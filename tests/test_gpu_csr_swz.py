"""The CSR overlapping Schwarz method on the device (csrc/csr_swz.hip.h): sweeps, factors, the preconditioner, the solves.

The numpy restatement of tests/_csr_swz_cases.py is the specification of the arithmetic: the device's x, factors and pivots are compared
with it on the bits, so any scheduling race or reordering shows.  Against the reference's own sweep (its block solve is GMRES to 1e-8) the
bound is 10 d, d the recorded distance between the reference's sweep and the float64 exact-block model; where d is below 1e-12 max|x| (the
reference's GMRES converged exactly) it is 1e-9 max|x|, the project's solution bar.  Recorded side: tests/golden/csr_swz.npz."""
import ctypes as C

import numpy as np
import pytest

import _csr_swz_cases as W
from _libs import T

pytestmark = pytest.mark.gpu
TOL = 1e-8
DIRS = {1: "f", 2: "b", 3: "fb"}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def L(gpu):
    return gpu.lib()


_restated_x = {}


def restated_x(key, d):
    """x after the restatement's sequential sweeps of direction d from the case's x0 (computed once)."""
    if (key, d) not in _restated_x:
        c = W.sweep_case(key)
        _restated_x[(key, d)] = c["R"].apply(d, c["x0"].copy(), c["b"])
    return _restated_x[(key, d)]


@pytest.mark.parametrize("key", list(W.SWEEP_CASES))
def test_sweeps_factors_and_info(gpu, key):
    g, c = W.golden(), W.sweep_case(key)
    R = c["R"]
    S = W.LibSwz(gpu, c["ia"], c["ja"], c["val"], c["maxlvl"])
    assert S.st == 0
    try:
        lev = [R.levels(False), R.levels(True)]
        nsw = sum(1 for f in R.factors if f[2])
        for d in (1, 2, 3):
            st, x, info, fac, piv = S.sweeps(d, c["b"], c["x0"], want_factors=(d == 1))
            assert st == 0
            want = restated_x(key, d)
            xr, dist = g[f"{key}/x_{DIRS[d]}"], float(g[f"{key}/d"][d - 1])
            scale = float(np.max(np.abs(xr)))
            bound = 10.0 * dist if dist >= 1e-12 * scale else 1e-9 * scale
            err = float(np.max(np.abs(x - xr)))
            print(f"{key} dir {d}: |x - restated| {np.max(np.abs(x - want)):.2e}  |x - x_ref| {err:.2e}  bound {bound:.2e}  info {info.tolist()}")
            assert np.array_equal(bits(x), bits(want))
            assert err <= bound
            launches = {1: lev[0].max() + 1, 2: lev[1].max() + 1, 3: lev[0].max() + lev[1].max() + 2}[d]
            assert info.tolist() == [lev[0].max() + 1, lev[1].max() + 1, launches, R.nblk, R.maxbs, nsw, 0, 1]
            if d == 1:
                wf, wp = R.packed_factors()
                assert np.array_equal(bits(fac), bits(wf)) and np.array_equal(piv, wp)
        if key in W.INTERCHANGING:
            assert nsw >= 0.9 * R.nblk
        if key in W.DOMINANT:
            assert nsw == 0
        # the public one-sweep entries on host vectors are the same sweeps
        x = c["x0"].copy(); xv = T.dvector(S.n, T.dp(x)); bv, _ = T.as_vec(c["b"])
        S.L.fasp_dcsr_swz_forward(C.byref(S.D), C.byref(S.prm), C.byref(xv), C.byref(bv))
        assert np.array_equal(bits(x), bits(restated_x(key, 1)))
        x = c["x0"].copy(); xv = T.dvector(S.n, T.dp(x))
        S.L.fasp_dcsr_swz_backward(C.byref(S.D), C.byref(S.prm), C.byref(xv), C.byref(bv))
        assert np.array_equal(bits(x), bits(restated_x(key, 2)))
    finally:
        S.free()


def test_three_sweeps_are_three_calls(gpu):
    c = W.sweep_case("p7_6x5x4_l2")
    S = W.LibSwz(gpu, c["ia"], c["ja"], c["val"], c["maxlvl"])
    try:
        st, x3, info, _, _ = S.sweeps(3, c["b"], c["x0"], nsweeps=3)
        x = c["x0"]
        for _ in range(3):
            st1, x, _, _, _ = S.sweeps(3, c["b"], x)
        assert st == 0 and st1 == 0 and np.array_equal(bits(x3), bits(x)) and info[2] == 3 * (info[0] + info[1]) and info[7] == 1
    finally:
        S.free()


@pytest.mark.parametrize("key", ["nonsym_9x7_l2", "weak_diag_l1", "hub128_l1"])
def test_precond_on_host_vectors(gpu, key):
    c = W.sweep_case(key)
    r, z0 = c["b"], np.zeros(len(c["b"]))
    for typ, d in ((1, 1), (2, 2), (3, 3), (7, 1)):   # an unknown type is a forward sweep
        S = W.LibSwz(gpu, c["ia"], c["ja"], c["val"], c["maxlvl"], typ=typ)
        try:
            z = np.full(S.n, 9.0)
            rr = np.array(r)
            S.L.fasp_precond_swz(T.dp(rr), T.dp(z), C.byref(S.D))
            st, want, _, _, _ = S.sweeps(d, r, z0)
            assert st == 0 and np.array_equal(bits(z), bits(want))
            assert np.array_equal(bits(z), bits(c["R"].apply(d, z0.copy(), r)))
        finally:
            S.free()


def _its(gpu, solver):
    it = gpu.param_solver_init()
    it.itsolver_type = solver; it.tol = TOL; it.maxit = 500; it.restart = 30; it.print_level = 0
    return it


_G = W.golden()
QUALIFIED = [(j, str(k)) for j, k in enumerate(_G["solve_keys"]) if _G["solve_ok"][j]]


@pytest.mark.parametrize("j,key", QUALIFIED, ids=[k for _, k in QUALIFIED])
def test_krylov_swz_matches_the_reference(gpu, capfd, j, key):
    g = W.golden()
    build, solver, typ, lvl = W.SOLVE_CASES[key]
    ia, ja, val = build()
    n = len(ia) - 1
    b = W.solve_rhs(n)
    A, keep = T.as_csr(ia, ja, val)
    x = np.zeros(n); xv = T.dvector(n, T.dp(x)); bv, _ = T.as_vec(b)
    it = _its(gpu, solver)
    prm = T.SWZ_param(); gpu.lib().fasp_param_swz_init(C.byref(prm)); prm.SWZ_maxlvl = lvl; prm.SWZ_type = typ
    st = gpu.lib().fasp_solver_dcsr_krylov_swz(C.byref(A), C.byref(bv), C.byref(xv), C.byref(it), C.byref(prm))
    out = capfd.readouterr().out
    rows = np.repeat(np.arange(n), np.diff(ia))
    relres = float(np.linalg.norm(b - np.bincount(rows, val * x[ja], minlength=n)) / np.linalg.norm(b))
    xr, dist = g[f"solve_x_{j}"], float(g["solve_dist"][j])
    err = float(np.max(np.abs(x - xr)))
    print(f"{key}: iterations {st} (reference {g['solve_it'][j]})  relres {relres:.3e}  |x - x_ref| {err:.2e}  10 dist {10 * dist:.2e}")
    assert "SWZ_Krylov method setup" in out
    assert st == g["solve_it"][j]
    assert relres <= 1.01 * TOL
    assert err <= 10.0 * dist
    assert gpu.lib().fasp_hip_csr_swz_resident_count() == 0


@pytest.mark.parametrize("key", ["cg_p5_17x15_t3_l2", "gmres_nonsym_17x15_t1_l2", "bicgstab_nonsym_17x15_t2_l3"])
def test_device_bound_and_host_staged_agree(gpu, key):
    """fasp_precond_swz recognised by its address against the same function behind a ctypes trampoline (a foreign address: staged)."""
    build, solver, typ, lvl = W.SOLVE_CASES[key]
    ia, ja, val = build()
    n = len(ia) - 1
    b = W.solve_rhs(n)
    A, keep = T.as_csr(ia, ja, val)
    bv, _ = T.as_vec(b)
    S = W.LibSwz(gpu, ia, ja, val, lvl, typ=typ)
    Lb = S.L
    f = Lb.fasp_precond_swz
    try:
        res = []
        cb = T.PRECOND_FCT(lambda r, z, data: f(r, z, data))
        for pc in (T.precond(C.addressof(S.D), C.cast(f, T.PRECOND_FCT)), T.precond(C.addressof(S.D), cb)):
            x = np.zeros(n); xv = T.dvector(n, T.dp(x))
            it = _its(gpu, solver)
            res.append((Lb.fasp_solver_dcsr_itsolver(C.byref(A), C.byref(bv), C.byref(xv), C.byref(pc), C.byref(it)), x))
        assert res[0][0] > 0 and res[0][0] == res[1][0] and np.array_equal(bits(res[0][1]), bits(res[1][1]))
    finally:
        S.free()


def test_one_setup_two_solves_one_factorisation(gpu):
    build, solver, typ, lvl = W.SOLVE_CASES["cg_p5_17x15_t3_l2"]
    ia, ja, val = build()
    n = len(ia) - 1
    A, keep = T.as_csr(ia, ja, val)
    S = W.LibSwz(gpu, ia, ja, val, lvl, typ=typ)
    Lb = S.L
    assert Lb.fasp_hip_csr_swz_resident_count() == 0
    pc = T.precond(C.addressof(S.D), C.cast(Lb.fasp_precond_swz, T.PRECOND_FCT))
    xs = []
    for seed in (1, 2):
        b = np.random.default_rng(seed).standard_normal(n)
        bv, _ = T.as_vec(b)
        x = np.zeros(n); xv = T.dvector(n, T.dp(x))
        it = _its(gpu, solver)
        assert Lb.fasp_solver_dcsr_itsolver(C.byref(A), C.byref(bv), C.byref(xv), C.byref(pc), C.byref(it)) > 0
        assert Lb.fasp_hip_csr_swz_resident_count() == 1
        xs.append(x)
    assert not np.array_equal(xs[0], xs[1])
    st, _, info, _, _ = S.sweeps(1, np.ones(n), np.zeros(n))
    assert st == 0 and info[7] == 1          # still the first factorisation
    S.free()
    assert Lb.fasp_hip_csr_swz_resident_count() == 0
