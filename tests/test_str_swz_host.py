"""The structured block Gauss-Seidel (Schwarz) smoother without a GPU: the numpy restatement (tests/_str_swz_cases.py: patch matrix, LU with
row interchanges, solve, levels, the sweep point after point and in batches) against the recorded reference (tests/golden/str_swz.npz, written
by tools/gen_golden_str_swz.py) and, where oracle/_ref is built, against the live one, bit for bit; the level counts; and the host half of the
device path -- fasp_hip_str_swz_levels, the layout of precond_data_str, the refusals, all of which are decided before a device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _libs
import _str_ilu_cases as I
import _str_swz_cases as W
from _libs import ROOT, T

FIELDS = ("AMG_type", "print_level", "maxit", "max_levels", "tol", "cycle_type", "smoother", "presmooth_iter", "postsmooth_iter",
          "coarsening_type", "relaxation", "coarse_scaling", "mgl_data", "LU", "scaled", "A", "A_str", "SS_str", "diaginv", "pivot", "diaginvS",
          "pivotS", "order", "neigh", "r", "w")


@pytest.fixture(scope="module")
def L(fa):
    return W.protos(fa.lib())


@pytest.fixture(scope="module")
def G():
    return np.load(W.GOLDEN)


@pytest.fixture(scope="module")
def R():
    lib = _libs.ref()
    return W.protos(lib) if lib is not None else None


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


CASES = W.host_cases()


@pytest.mark.parametrize("grid", W.HOST_GRIDS, ids=["5x4x3", "9x7x1", "1x8x6"])
@pytest.mark.parametrize("kind", ["dom", "weak"])
def test_restatement_is_the_reference(G, R, grid, kind):
    keys = list(G["keys"])
    g = "x".join(str(v) for v in grid)
    mine = [c for c in CASES if c[0].startswith(f"{kind}_{g}_")]
    assert mine
    facs = {}
    for key, c, _, nk, ok in mine:
        k = keys.index(key)
        neigh, order = W.neigh_of(grid, nk), W.order_of(grid, ok)
        if (c["name"], nk) not in facs:
            facs[(c["name"], nk)] = W.factor_all(c, neigh)
        fac = facs[(c["name"], nk)]
        d, p = W.packed(fac, c, neigh)
        assert np.array_equal(W.digest(d), G["sha_d"][k]) and np.array_equal(W.digest(p), G["sha_p"][k]), key
        b, u0 = W.vectors(c)
        us = W.model_sweep(c, neigh, order, fac, b, u0, sequential=True)
        ub = W.model_sweep(c, neigh, order, fac, b, u0)
        assert np.array_equal(_bits(us), _bits(ub)), key
        assert np.array_equal(_bits(us[:W.HEAD]), _bits(G["head"][k])) and np.array_equal(W.digest(us), G["sha_u"][k]), key
        if f"u_{k}" in G.files:
            assert np.array_equal(_bits(d), _bits(G[f"d_{k}"])) and np.array_equal(p, G[f"p_{k}"]) and np.array_equal(_bits(us), _bits(G[f"u_{k}"])), key
        if R is not None and ok in ("natural", "random"):
            f = W.generate(R, c, neigh)
            assert np.array_equal(_bits(d), _bits(f.d)) and np.array_equal(p, f.p), key
            if not (c["nx"] == 1 and c["nc"] > 1):   # there the reference's product leaves its arrays (module docstring of the generator)
                assert np.array_equal(_bits(us), _bits(W.call_swz(R, c, neigh, order, f, b, u0))), key


def test_weak_matrices_interchange_rows_and_dominant_ones_do_not():
    for grid in W.HOST_GRIDS:
        geo = W.geometric(grid)
        assert W.interchanges(W.factor_all(W.grid_case(grid, 1), geo)) == 0
        fac = W.factor_all(W.weak_case(grid, 1), geo)
        assert W.interchanges(fac) >= 0.9 * len(fac) and not any(s for _, _, _, s in fac)
        fac = W.factor_all(W.weak_case(grid, 2), geo)
        assert W.interchanges(fac) == len(fac)


def test_the_stopped_patch_holds_what_the_reference_leaves(G):
    c = W.stopped_case()
    fac = W.factor_all(c, None)
    assert [i for i, f in enumerate(fac) if f[3]] == [7]
    d, p = W.packed(fac, c, None)
    assert np.array_equal(_bits(d), _bits(G["stop_d"])) and np.array_equal(p, G["stop_p"])


def _levels(L, case, neigh, order):
    A, keep = W.as_str(case)
    n = W.ngrid_of(case)
    nb = None if neigh is None else np.ascontiguousarray(neigh, dtype=np.int32)
    od = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    visit, level = np.full(n + 3, -1, dtype=np.int32), np.full(n + 3, -1, dtype=np.int32)
    nv = L.fasp_hip_str_swz_levels(C.byref(A), None if nb is None else T.ip(nb), 0 if nb is None else nb.shape[1], None if od is None else T.ip(od),
                                   T.ip(visit), T.ip(level), n + 3)
    return nv, visit[:max(nv, 0)], level[:max(nv, 0)]


@pytest.mark.parametrize("grid", [(5, 4, 3), (9, 7, 1), (1, 8, 6), (41, 20, 4)], ids=["5x4x3", "9x7x1", "1x8x6", "41x20x4"])
def test_level_counts(L, grid):
    gx, gy, gz = I.geometry(*grid)
    n = gx * gy * gz
    c = W.grid_case(grid, 1)
    geo = W.geometric(grid)
    want = (gx - 1) + 3 * (gy - 1) + 7 * (gz - 1) + 1
    assert want == {(5, 4, 3): 28, (9, 7, 1): 27, (1, 8, 6): 23, (41, 20, 4): 119}[grid]
    for okey in ("natural", "reversed"):
        nv, visit, level = _levels(L, c, geo, W.order_of(grid, okey))
        assert nv == n and level.max() + 1 == want, okey
    nv, visit, level = _levels(L, c, geo, W.colour12(grid))
    assert nv == n and level.max() + 1 == 12
    if grid == (41, 20, 4):
        assert np.bincount(level).max() == 275
    for nb in (None, W.neigh_of(grid, "absent")):
        nv, visit, level = _levels(L, c, nb, None)
        i = np.arange(n)
        assert nv == n and np.array_equal(level, i % gx + (i // gx) % gy + i // (gx * gy)) and level.max() + 1 == (gx - 1) + (gy - 1) + (gz - 1) + 1


@pytest.mark.parametrize("nk,ok", [("geo", "natural"), ("geo", "random"), ("geo", "twice"), ("far", "natural"), ("far", "random"), ("none", "reversed")])
def test_library_levels_are_the_restatements(L, nk, ok):
    grid = (5, 4, 3)
    for c in (W.grid_case(grid, 3), W.wrap_case(grid, 1)):
        neigh, order = W.neigh_of(grid, nk), W.order_of(grid, ok)
        pts = W.visits(c, order)
        nv, visit, level = _levels(L, c, neigh, order)
        assert nv == 60 and np.array_equal(visit, pts) and np.array_equal(level, W.visit_levels(c, neigh, pts))
        if (nk, ok) == ("far", "natural"):
            assert level.max() + 1 == 60       # every patch holds the next point: one chain
    lev = W.visit_levels(W.wrap_case(grid, 1), None, np.arange(60))
    assert lev[5] == lev[4] + 1                # a wrap coefficient is a dependency: row 5 (x = 0, y = 1) reads point 4 (x = 4, y = 0)


def test_struct_layout_matches_the_reference(G, tmp_path):
    lay = [int(v) for v in G["layout"]]
    D = T.precond_data_str
    assert [C.sizeof(D)] + [getattr(D, f).offset for f in FIELDS] == lay
    checks = [f'_Static_assert(sizeof(precond_data_str)=={lay[0]},"size");']
    checks += [f'_Static_assert(offsetof(precond_data_str,{m})=={o},"{m}");' for m, o in zip(FIELDS, lay[1:])]
    src = tmp_path / "l.c"
    src.write_text('#include <stddef.h>\n#include "fasp_hip.h"\n' + "\n".join(checks) + "\nint main(void){return 0;}\n")
    subprocess.run(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_exports(fa):
    for s in ("fasp_generate_diaginv_block", "fasp_smoother_dstr_swz", "fasp_precond_dstr_blockgs", "fasp_solver_dstr_krylov_blockgs",
              "fasp_hip_str_swz", "fasp_hip_str_swz_levels", "fasp_hip_time_str_swz"):
        assert s in fa.EXPORTS and hasattr(fa.lib(), s)


def _swz(L, case, neigh, order, b, u, nsweeps=1):
    A, keep = W.as_str(case)
    nb = None if neigh is None else np.ascontiguousarray(neigh, dtype=np.int32)
    od = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    info = (C.c_int * 8)()
    st = L.fasp_hip_str_swz(C.byref(A), None if nb is None else T.ip(nb), 0 if nb is None else nb.shape[1], None if od is None else T.ip(od),
                            T.dp(b), T.dp(u), nsweeps, info)
    return st, list(info)


def test_refusals(L, G, capfd):
    """Everything here is decided on the host, before any device work: no GPU is needed, and nothing is touched."""
    grid = (5, 4, 3)
    c = W.grid_case(grid, 2)
    n = 60
    b, u0 = W.vectors(c)
    geo = W.geometric(grid)
    fac = W.factor_all(c, geo)
    d, p = W.packed(fac, c, geo)
    msz = [f[1].shape[0] for f in fac]
    good = lambda: W.Factors.from_blocks(n, 14, d, p, msz)
    bad_neigh = geo.copy(); bad_neigh[17, 2] = n
    short_order = np.arange(n - 1, dtype=np.int32)
    bad_order = np.arange(n, dtype=np.int32); bad_order[9] = n
    neg_order = np.arange(n, dtype=np.int32); neg_order[9] = -1
    capfd.readouterr()
    # the dev entry and the level entry
    for neigh, order, word in ((bad_neigh, None, "outside 0 .. 59"), (geo, bad_order, "of the order"), (geo, neg_order, "of the order")):
        u = u0.copy()
        st, info = _swz(L, c, neigh, order, b, u)
        assert st == T.ERROR_INPUT_PAR and np.array_equal(_bits(u), _bits(u0))
        assert word in capfd.readouterr().err
        assert _levels(L, c, neigh, order)[0] == T.ERROR_INPUT_PAR
        capfd.readouterr()
    # the public smoother: neigh, order, and factors that do not fit
    ragged = T.ivector(n * 6 - 1, T.ip(np.ascontiguousarray(geo).reshape(-1)))
    A, keep = W.as_str(c)

    def public(f, nv=None, ov=None, neigh=geo):
        u = u0.copy()
        bb = b.copy()
        bv, uv = T.dvector(bb.size, T.dp(bb)), T.dvector(u.size, T.dp(u))
        nk = np.ascontiguousarray(neigh, dtype=np.int32).reshape(-1)
        nvv = nv if nv is not None else T.ivector(nk.size, T.ip(nk))
        L.fasp_smoother_dstr_swz(C.byref(A), C.byref(bv), C.byref(uv), f.dv, f.pv, C.byref(nvv), None if ov is None else C.byref(ov))
        assert np.array_equal(_bits(u), _bits(u0))
        return capfd.readouterr().err

    assert "multiple of ngrid" in public(good(), nv=ragged)
    assert "outside 0 .. 59" in public(good(), neigh=bad_neigh)
    assert "needs ngrid = 60 entries" in public(good(), ov=T.ivector(n - 1, T.ip(short_order)))
    assert "of the order" in public(good(), ov=T.ivector(n, T.ip(bad_order)))
    f = good(); f.dv[5].row -= 1
    assert "does not fit its patch" in public(f)
    f = good(); f.pv[5].row += 1
    assert "does not fit its patch" in public(f)
    f = good(); f.p[f.poff[11] + 1] = msz[11]
    assert "pivot 1 of grid point 11" in public(f)
    f = good(); f.p[f.poff[11] + 3] = 2                    # below the row: what a stopped factorisation leaves
    assert "pivot 3 of grid point 11" in public(f)
    f = good(); f.d[f.doff[20] + 2 * msz[20] + 2] = 0.0
    assert "0.0 on U's diagonal" in public(f)
    # the preconditioner called directly: z untouched
    for f, neigh, word in ((good(), bad_neigh, "outside 0 .. 59"), (None, geo, "diaginv or pivot is NULL")):
        pd = W.PcData(c, neigh, None, f)
        z = np.full(n * 2, 7.0)
        L.fasp_precond_dstr_blockgs(T.dp(b.copy()), T.dp(z), pd.ptr())
        assert np.all(z == 7.0) and word in capfd.readouterr().err
    f = good(); f.p[f.poff[11] + 3] = 2
    pd = W.PcData(c, geo, None, f)
    z = np.full(n * 2, 7.0)
    L.fasp_precond_dstr_blockgs(T.dp(b.copy()), T.dp(z), pd.ptr())
    assert np.all(z == 7.0) and "pivot 3 of grid point 11" in capfd.readouterr().err
    # the recorded stopped factor is refused the same way (its pivots behind the stop are zeros)
    cs = W.stopped_case()
    fs = W.Factors.from_blocks(n, 1, G["stop_d"], G["stop_p"], [1] * n)
    As, keeps = W.as_str(cs)
    bs, us0 = W.vectors(cs)
    u = us0.copy()
    bv, uv = T.dvector(bs.size, T.dp(bs.copy())), T.dvector(u.size, T.dp(u))
    L.fasp_smoother_dstr_swz(C.byref(As), C.byref(bv), C.byref(uv), fs.dv, fs.pv, None, None)
    assert np.array_equal(_bits(u), _bits(us0)) and "0.0 on U's diagonal" in capfd.readouterr().err
    # the solver entry returns ERROR_INPUT_PAR
    assert W.solve_blockgs(L, c, b, bad_neigh, None, T.SOLVER_GMRES, 10)[0] == T.ERROR_INPUT_PAR
    assert W.solve_blockgs(L, c, b, geo, bad_order, T.SOLVER_GMRES, 10)[0] == T.ERROR_INPUT_PAR
    # a patch of more than 64 rows
    wide = np.tile(np.arange(10, dtype=np.int32), (n, 1))
    c7 = W.grid_case(grid, 7)
    b7, u7 = W.vectors(c7)
    u = u7.copy()
    capfd.readouterr()
    assert _swz(L, c7, wide, None, b7, u)[0] == T.ERROR_INPUT_PAR and np.array_equal(_bits(u), _bits(u7))
    assert "more than the 64" in capfd.readouterr().err
    # nc < 1: the reference's message, nothing done
    A0, keep0 = W.as_str(c)
    A0.nc = 0
    u = u0.copy()
    f = good()
    bv, uv = T.dvector(b.size, T.dp(b.copy())), T.dvector(u.size, T.dp(u))
    L.fasp_smoother_dstr_swz(C.byref(A0), C.byref(bv), C.byref(uv), f.dv, f.pv, None, None)
    L.fasp_generate_diaginv_block(C.byref(A0), None, f.dv, f.pv)
    assert np.array_equal(_bits(u), _bits(u0)) and capfd.readouterr().out.count("nc is illegal") == 2
