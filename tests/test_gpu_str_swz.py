"""The structured block Gauss-Seidel (Schwarz) smoother on the device (csrc/str_swz.hip.h): k_str_swz_factor (assembly and LU with row
interchanges of every patch) and k_str_swz_level (one launch per level of independent visits), and the entries around them.

Every comparison of factors, pivots and sweeps is np.array_equal on the bits against the numpy restatement (tests/_str_swz_cases.py), which
tests/test_str_swz_host.py holds to the reference bit for bit: no tolerance.  The dominant matrices never interchange a row, the weak ones do in
nearly every patch: only they reach the interchange path of both kernels.  Every sweep asserts the levels and launches that ran (info) and a
zero status.

Solves, tol 1e-8 from a zero guess.  nc = 1 (the upwind 9 x 8 x 7 system) against the reference's own fasp_solver_dstr_krylov_blockgs: equal
iteration counts and max|x - x_ref| <= 1e-9 max|x_ref|, the rule of tests/test_gpu_str.py.  nc = 3, 5 (the reference's STR solvers are not
callable there): the device-bound solve against the same solve with the preconditioner behind a ctypes trampoline (a foreign address: host
staged, one-shot per application) -- equal counts and array_equal x -- and the true relative residual <= 1.01 tol."""
import ctypes as C
import functools

import numpy as np
import pytest

import _str_cases as S
import _str_swz_cases as W
from _libs import T

pytestmark = pytest.mark.gpu

NCS = [1, 2, 3, 5, 7]


@pytest.fixture(scope="module")
def L(gpu):
    return W.protos(gpu.lib())


@pytest.fixture(scope="module")
def G():
    return np.load(W.GOLDEN)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def case_of(grid, nc, which):
    c = {"dom": lambda: W.grid_case(grid, nc), "weak": lambda: W.weak_case(grid, nc), "wrap": lambda: W.wrap_case(grid, nc),
         "noncanon": lambda: W.grid_case(grid, nc, order=W.NONCANON[len(W.grid_case(grid, nc)["offsets"])])}[which]()
    b, u0 = W.vectors(c)
    for a in [b, u0, c["diag"]] + list(c["bands"]):
        a.setflags(write=False)
    return c, b, u0


@functools.lru_cache(maxsize=None)
def fac_of(grid, nc, which, nk):
    """The restatement's factors, computed once: (factor_all, packed factors, packed pivots)."""
    c = case_of(grid, nc, which)[0]
    neigh = W.neigh_of(grid, nk)
    fac = W.factor_all(c, neigh)
    return (fac,) + W.packed(fac, c, neigh)


@functools.lru_cache(maxsize=None)
def want_of(grid, nc, which, nk, ok, nsweeps=1):
    c, b, u0 = case_of(grid, nc, which)
    u = u0
    for _ in range(nsweeps):
        u = W.model_sweep(c, W.neigh_of(grid, nk), W.order_of(grid, ok), fac_of(grid, nc, which, nk)[0], b, u)
    u.setflags(write=False)
    return u


def dev_sweep(L, c, neigh, order, b, u0, nsweeps=1):
    """nsweeps sweeps through fasp_hip_str_swz (factored on the device) -> (status, u, info)."""
    A, keep = W.as_str(c)
    nb = None if neigh is None else np.ascontiguousarray(neigh, dtype=np.int32)
    od = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    u = np.array(u0)
    info = (C.c_int * 8)()
    st = L.fasp_hip_str_swz(C.byref(A), None if nb is None else T.ip(nb), 0 if nb is None else nb.shape[1], None if od is None else T.ip(od),
                            T.dp(np.array(b)), T.dp(u), nsweeps, info)
    return st, u, list(info)


def check_sweep(L, grid, nc, which, nk, ok, nsweeps=1):
    c, b, u0 = case_of(grid, nc, which)
    neigh, order = W.neigh_of(grid, nk), W.order_of(grid, ok)
    fac = fac_of(grid, nc, which, nk)[0]
    want = want_of(grid, nc, which, nk, ok, nsweeps)
    st, u, info = dev_sweep(L, c, neigh, order, b, u0, nsweeps)
    lev = W.visit_levels(c, neigh, W.visits(c, order))
    assert st == 0, (st, info)
    assert info[0] == lev.max() + 1 and info[1] == info[0] and info[2] == lev.size and info[3] == np.bincount(lev).max(), info
    assert info[4] == max(f[1].shape[0] for f in fac) and info[6] == 0, info
    if ok == "natural":   # every patch is factored once: the interchanges are the restatement's
        assert info[5] == W.interchanges(fac), info
    bad = np.flatnonzero(_bits(u) != _bits(want))
    assert bad.size == 0, (bad[:8], u[bad[:8]], want[bad[:8]])
    return info


# ---- factorisation ----------------------------------------------------------------------------------------------------------------------
# 5 x 4 x 3: every patch has 4 .. 7 members, m varies inside a wavefront; 17 x 9 x 6: 918 points, no multiple of 64, interior patches
@pytest.mark.parametrize("which", ["dom", "weak"])
@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("grid", [(5, 4, 3), (17, 9, 6), (9, 7, 1)], ids=["5x4x3", "17x9x6", "9x7x1"])
def test_factors_and_pivots_are_the_references_bytes(L, grid, nc, which):
    c = case_of(grid, nc, which)[0]
    fac, d, p = fac_of(grid, nc, which, "geo")
    f = W.generate(L, c, W.geometric(grid))
    assert [f.dv[i].row for i in range(f.n)] == [x[1].size for x in fac] and [f.pv[i].row for i in range(f.n)] == [x[2].size for x in fac]
    assert f.doff == list(np.concatenate([[0], np.cumsum([x[1].size for x in fac])[:-1]]))     # carved in order from one block
    bad = np.flatnonzero(_bits(f.d) != _bits(d))
    assert bad.size == 0, (bad[:8], f.d[bad[:8]], d[bad[:8]])
    assert np.array_equal(f.p, p)
    if which == "weak":
        assert W.interchanges(fac) >= 0.9 * len(fac)


@pytest.mark.parametrize("nk", ["none", "absent", "far"])
def test_factors_of_the_other_neighbour_sets(L, nk):
    grid = (5, 4, 3)
    for nc in (1, 3):
        c = case_of(grid, nc, "weak")[0]
        fac, d, p = fac_of(grid, nc, "weak", nk)
        f = W.generate(L, c, W.neigh_of(grid, nk))
        assert np.array_equal(_bits(f.d), _bits(d)) and np.array_equal(f.p, p)


def test_a_patch_that_stops(L, G, capfd):
    c = W.stopped_case()
    f = W.generate(L, c, None)
    assert np.array_equal(_bits(f.d), _bits(G["stop_d"])) and np.array_equal(f.p, G["stop_p"])
    b, u0 = W.vectors(c)
    capfd.readouterr()
    st, u, info = dev_sweep(L, c, None, None, b, u0)
    assert st == T.ERROR_INPUT_PAR and info[6] == 1 and info[5] == 0 and np.array_equal(_bits(u), _bits(u0))
    assert "stopped" in capfd.readouterr().err
    assert W.solve_blockgs(L, c, b, None, None, T.SOLVER_GMRES, 10)[0] == T.ERROR_INPUT_PAR


# ---- sweeps -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ok", ["natural", "reversed", "random", "colour", "twice"])
@pytest.mark.parametrize("which", ["dom", "weak"])
@pytest.mark.parametrize("nc", NCS)
def test_sweep_in_every_order(L, nc, which, ok):
    info = check_sweep(L, (5, 4, 3), nc, which, "geo", ok)
    if ok in ("natural", "reversed"):
        assert info[0] == 28
    if ok == "colour":
        assert info[0] == 12


# (the restatement of 49-row patches level after level is slow in numpy: nc = 7 takes the 12-colour order only)
@pytest.mark.parametrize("grid,nc,ok", [((17, 9, 6), 1, "natural"), ((17, 9, 6), 1, "colour"), ((17, 9, 6), 3, "natural"), ((17, 9, 6), 3, "colour"),
                                        ((17, 9, 6), 7, "colour"), ((9, 7, 1), 1, "natural"), ((9, 7, 1), 3, "random"), ((9, 7, 1), 7, "natural")])
def test_sweep_on_grids_that_are_no_multiple_of_a_wavefront(L, grid, nc, ok):
    check_sweep(L, grid, nc, "weak", "geo", ok)


@pytest.mark.parametrize("nc", [1, 3])
def test_a_level_wider_than_a_workgroup(L, nc):
    info = check_sweep(L, (41, 20, 4), nc, "weak", "geo", "colour")
    assert info[0] == 12 and info[3] == 275


@pytest.mark.parametrize("ok", ["natural", "random"])
@pytest.mark.parametrize("nk", ["none", "absent", "far"])
@pytest.mark.parametrize("nc", [1, 3])
def test_sweep_with_the_other_neighbour_sets(L, nc, nk, ok):
    info = check_sweep(L, (5, 4, 3), nc, "weak", nk, ok)
    if ok == "natural":
        assert info[0] == {"none": 10, "absent": 10, "far": 60}[nk]


@pytest.mark.parametrize("which", ["noncanon", "wrap"])
@pytest.mark.parametrize("nc", [1, 3])
def test_another_storage_order_and_a_wrap_coefficient(L, nc, which):
    """noncanon: +1 stored before -1, planes first (the products are taken by ascending offset all the same); wrap: the matrix is no longer
    grid-like for the reference's product either -- the coefficient is a term and a dependency."""
    for ok in ("natural", "random"):
        check_sweep(L, (5, 4, 3), nc, which, "geo", ok)
    if which == "wrap":
        assert not np.array_equal(want_of((5, 4, 3), nc, "wrap", "geo", "natural"), want_of((5, 4, 3), nc, "dom", "geo", "natural"))


@pytest.mark.parametrize("nc", [1, 3])
def test_three_resident_sweeps_are_three_public_calls(L, nc):
    """On the dominant matrix: three sweeps of a weak one, which no sweep makes smaller, need not stay finite."""
    grid = (17, 9, 6)
    c, b, u0 = case_of(grid, nc, "dom")
    geo, order = W.geometric(grid), W.order_of(grid, "random")
    check_sweep(L, grid, nc, "dom", "geo", "random", nsweeps=3)
    f = W.generate(L, c, geo)                       # the public smoother with factors of our fasp_generate_diaginv_block
    v = u0
    for _ in range(3):
        v = W.call_swz(L, c, geo, order, f, b, v)
    assert np.array_equal(_bits(v), _bits(want_of(grid, nc, "dom", "geo", "random", 3)))


def test_the_public_smoother_with_the_references_recorded_factors(L, G):
    keys = list(G["keys"])
    for key in W.WHOLE_KEYS:
        k = keys.index(key)
        name, nk, ok = key.split("/")
        kind, g, ncs = name.split("_")
        grid, nc = tuple(int(v) for v in g.split("x")), int(ncs[2:])
        c, b, u0 = case_of(grid, nc, kind)
        neigh = W.neigh_of(grid, nk)
        msz = [len(W.members(i, neigh)) * nc for i in range(W.ngrid_of(c))]
        f = W.Factors.from_blocks(len(msz), ((0 if neigh is None else neigh.shape[1]) + 1) * nc, G[f"d_{k}"], G[f"p_{k}"], msz)
        u = W.call_swz(L, c, neigh, W.order_of(grid, ok), f, b, u0)
        assert np.array_equal(_bits(u), _bits(G[f"u_{k}"])), key


@pytest.mark.parametrize("nc", [1, 3])
def test_the_preconditioner_called_directly_is_a_sweep_from_zero(L, nc):
    grid = (5, 4, 3)
    c, b, u0 = case_of(grid, nc, "weak")
    geo, order = W.geometric(grid), W.order_of(grid, "random")
    pd = W.PcData(c, geo, order, W.generate(L, c, geo))
    z = np.full(b.size, 7.0)
    L.fasp_precond_dstr_blockgs(T.dp(np.array(b)), T.dp(z), pd.ptr())
    want = W.model_sweep(c, geo, order, fac_of(grid, nc, "weak", "geo")[0], b, np.zeros_like(b))
    assert np.array_equal(_bits(z), _bits(want))


# ---- solves -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk,ok", W.KRYLOV_SETS, ids=[f"{a}-{b}" for a, b in W.KRYLOV_SETS])
@pytest.mark.parametrize("mkey,method,restart", W.KRYLOV, ids=[k[0] for k in W.KRYLOV])
def test_krylov_blockgs_scalar_matches_the_reference(L, G, mkey, method, restart, nk, ok):
    c, b = W.scalar_system()
    grid = (c["nx"], c["ny"], c["nz"])
    j = list(G["it_keys"]).index(f"{mkey}/{nk}/{ok}")
    it_g, x_g = int(G["it"][j]), G[f"it_x_{j}"]
    it, x = W.solve_blockgs(L, c, b, W.neigh_of(grid, nk), W.order_of(grid, ok), method, restart)
    print(f"{mkey} {nk} {ok}: {it} iterations (recorded {it_g}), max|dx| / max|x| = {np.max(np.abs(x - x_g)) / np.max(np.abs(x_g)):.3e}")
    if (nk, ok) == ("geo", "natural"):
        assert it_g == {"bicgstab": 6, "gmres": 9, "vgmres": 9}[mkey]
    if nk == "none":
        assert it_g == {"bicgstab": 15, "gmres": 29, "vgmres": 29}[mkey]
    assert it == it_g
    assert np.max(np.abs(x - x_g)) <= 1e-9 * np.max(np.abs(x_g))


def _plugin_solve(L, entry, c, b, pc, restart):
    A, keep = W.as_str(c)
    x = np.zeros_like(b)
    bv, kb = T.as_vec(b)
    xv = T.dvector(x.size, T.dp(x))
    fn = getattr(L, "fasp_solver_dstr_" + entry)
    if entry == "pgmres":
        it = fn(C.byref(A), C.byref(bv), C.byref(xv), C.byref(pc), S.TOL, 1e-18, 500, restart, T.STOP_REL_RES, 0)
    else:
        it = fn(C.byref(A), C.byref(bv), C.byref(xv), C.byref(pc), S.TOL, 1e-18, 500, T.STOP_REL_RES, 0)
    return it, x


@pytest.mark.parametrize("mkey,method,restart,entry", [("bicgstab", T.SOLVER_BiCGstab, 25, "pbcgs"), ("gmres", T.SOLVER_GMRES, 10, "pgmres")], ids=["bicgstab", "gmres"])
@pytest.mark.parametrize("nc", [3, 5])
def test_krylov_blockgs_blocks_device_bound_and_host_staged(L, nc, mkey, method, restart, entry):
    c, b = W.block_system(nc)
    grid = (c["nx"], c["ny"], c["nz"])
    geo = W.geometric(grid)
    it_dev, x_dev = W.solve_blockgs(L, c, b, geo, None, method, restart)                  # factors on the device only, bound
    pd = W.PcData(c, geo, None, W.generate(L, c, geo))
    f = L.fasp_precond_dstr_blockgs
    cb = T.PRECOND_FCT(lambda r, z, data: f(r, z, data))                                    # a foreign address: host staged, one-shot
    it_host, x_host = _plugin_solve(L, entry, c, b, T.precond(pd.ptr(), cb), restart)
    it_up, x_up = _plugin_solve(L, entry, c, b, T.precond(pd.ptr(), C.cast(f, T.PRECOND_FCT)), restart)   # the caller's factors, uploaded and bound
    it_diag, _ = S.solve_with(L, "fasp_solver_dstr_krylov_diag", c, c["diag"], c["bands"], b, method, restart)
    rr = S.true_relres(c, c["diag"], c["bands"], b, x_dev)
    print(f"{mkey} nc {nc}: {it_dev} iterations device bound, {it_host} host staged, {it_diag} with _krylov_diag; true relative residual {rr:.3e}")
    assert it_dev == it_host == it_up and it_dev > 1
    assert np.array_equal(x_dev, x_host) and np.array_equal(x_dev, x_up)
    assert rr <= 1.01 * S.TOL
