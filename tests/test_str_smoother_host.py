"""The structured smoothers without a GPU: the numpy restatement of ItrSmootherSTR.c (tests/_str_smoother_cases.model_sweep) against the
recorded reference (tests/golden/str_smoother.npz, written by tools/gen_golden_str_smoother.py) and, where oracle/_ref is built, against
the live one -- every variant, order and nc 1 .. 7 on 5 x 4 x 3, 9 x 7 x 1 and 1 x 8 x 6, bit for bit, the sequential and the batched
evaluation alike --, and the host half of the device path: the form str_sweep_plan chooses (fasp_hip_str_sweep_form), the levels of the
ordered form (fasp_hip_str_sweep_levels) and the refusals, all of which are decided before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import _libs
import _str_ilu_cases as I
import _str_smoother_cases as M
from _libs import T


@pytest.fixture(scope="module")
def L(fa):
    lib = fa.lib()
    yield lib
    lib.fasp_hip_tune(b"str_sweep_form", -1)


@pytest.fixture(scope="module")
def G():
    return np.load(M.GOLDEN)


@pytest.fixture(scope="module")
def R():
    lib = _libs.ref()
    return M.protos(lib) if lib is not None else None


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("nc", M.HOST_NC)
@pytest.mark.parametrize("grid", M.HOST_GRIDS, ids=["5x4x3", "9x7x1", "1x8x6"])
def test_restatement_is_the_reference(G, R, fa, grid, nc):
    c = M.grid_case(grid, nc)
    b, u0 = M.vectors(c)
    dinv = M.dinv_of(fa.lib(), c)            # the library's own inverse blocks: the restated fasp_smat_inv
    if R is not None and nc > 1:
        assert np.array_equal(_bits(dinv), _bits(M.dinv_of(R, c)))
    keys = list(G["keys"])
    for vkey, entry, kind, order, mark, w, cf in M.variants(grid):
        k = keys.index(f"{c['name']}/{vkey}")
        us = M.model_sweep(c, kind, order, mark, w, dinv, b, u0, cf_entry=cf, sequential=True)
        ub = M.model_sweep(c, kind, order, mark, w, dinv, b, u0, cf_entry=cf)
        assert np.array_equal(_bits(us), _bits(ub)), vkey
        assert np.array_equal(_bits(us[:M.HEAD]), _bits(G["head"][k])), vkey
        assert np.array_equal(M.digest(us), G["sha"][k]), vkey
        if f"u_{k}" in G.files:
            bad = np.flatnonzero(_bits(us) != _bits(G[f"u_{k}"]))
            assert bad.size == 0, (vkey, bad[:8])
        if R is not None:
            assert np.array_equal(_bits(us), _bits(M.call(R, entry, c, b, u0, order=order, mark=mark, w=w, dinv=dinv))), vkey


def test_scalar_sor_cf_closes_its_second_pass_as_gauss_seidel():
    """ItrSmootherSTR.c:1443, kept because bits are the contract: the SECOND points of the scalar C/F SOR are the GS values."""
    grid = (5, 4, 3)
    c = M.grid_case(grid, 1)
    b, u0 = M.vectors(c)
    rb = M.red_black(grid)
    sor = M.model_sweep(c, M.SOR, M.CPFIRST, rb, 1.1, None, b, u0, cf_entry=True)
    first_only = M.model_sweep(c, M.SOR, M.CPFIRST, np.where(rb == 1, 1, 0), 1.1, None, b, u0, cf_entry=True)
    gs_second = M.model_sweep(c, M.GS, M.CPFIRST, np.where(rb == -1, 1, 0), None, None, b, first_only, cf_entry=True)
    assert np.array_equal(_bits(sor), _bits(gs_second)) and not np.array_equal(sor, first_only)


def _form(L, case, order, mark=None):
    A, keep = M.as_str(case)
    mk = None if mark is None else np.ascontiguousarray(mark, dtype=np.int32)
    return L.fasp_hip_str_sweep_form(C.byref(A), order, None if mk is None else mk.ctypes.data_as(T.c_int_p))


def test_plan(L, capfd):
    g3, g2 = M.grid_case((5, 4, 3), 2), M.grid_case((9, 7, 1), 3)
    for forced, want3 in ((0, M.FORM_LEVEL), (1, M.FORM_PIPE), (2, M.FORM_LIST)):
        L.fasp_hip_tune(b"str_sweep_form", forced)
        assert _form(L, g3, M.ASCEND) == want3 and _form(L, g3, M.DESCEND) == want3
        assert _form(L, g2, M.ASCEND) == (M.FORM_LIST if forced == 2 else M.FORM_LEVEL)      # 2-D: nothing to pipeline
        assert _form(L, M.grid_case((1, 8, 6), 1), M.DESCEND) == (M.FORM_LIST if forced == 2 else M.FORM_LEVEL)
        # a sequence, a C/F marking, a matrix that is not grid-like: the ordered form whatever is asked for
        assert _form(L, g3, M.USERDEFINED, M.permutation((5, 4, 3), "natural")) == M.FORM_LIST
        assert _form(L, g3, M.CPFIRST, M.red_black((5, 4, 3))) == M.FORM_LIST
        assert _form(L, M.wrap_case((5, 4, 3), 2), M.ASCEND) == M.FORM_LIST
        assert _form(L, M.extra_offset_case((5, 4, 3), 1), M.ASCEND) == M.FORM_LIST
        assert _form(L, M.grid_case((5, 4, 3), 3, order=M.NONCANON[6]), M.ASCEND) == want3   # storage order is free
    L.fasp_hip_tune(b"str_sweep_form", -1)
    assert _form(L, g3, M.ASCEND) in (M.FORM_LEVEL, M.FORM_PIPE)
    capfd.readouterr()
    assert _form(L, M.wrap_case((5, 4, 3), 1), M.ASCEND) == M.FORM_LIST
    assert "not geometric neighbours" in capfd.readouterr().out
    assert _form(L, M.extra_offset_case((5, 4, 3), 1), M.DESCEND) == M.FORM_LIST
    assert "an offset outside" in capfd.readouterr().out
    assert _form(L, g3, 7) == -1                                                              # mark NULL, neither ASCEND nor DESCEND
    # a 2-D stencil on a 3-D grid is grid-like; one line is not
    c = M.grid_case((5, 4, 3), 1)
    c2 = dict(c, offsets=c["offsets"][:4], bands=c["bands"][:4])
    L.fasp_hip_tune(b"str_sweep_form", 0)
    assert _form(L, c2, M.ASCEND) == M.FORM_LEVEL
    line = dict(name="line", nx=7, ny=1, nz=1, nc=1, offsets=[-1, 1], diag=np.ones(7), bands=[np.ones(6), np.ones(6)])
    assert _form(L, line, M.ASCEND) == M.FORM_LIST
    L.fasp_hip_tune(b"str_sweep_form", -1)


def _levels(L, case, order, mark=None):
    A, keep = M.as_str(case)
    n = M.ngrid_of(case)
    mk = None if mark is None else np.ascontiguousarray(mark, dtype=np.int32)
    visit, level = np.full(2 * n, -1, dtype=np.int32), np.full(2 * n, -1, dtype=np.int32)
    nv = L.fasp_hip_str_sweep_levels(C.byref(A), order, None if mk is None else mk.ctypes.data_as(T.c_int_p), visit.ctypes.data_as(T.c_int_p),
                                     level.ctypes.data_as(T.c_int_p), 2 * n)
    return nv, visit[:max(nv, 0)], level[:max(nv, 0)]


@pytest.mark.parametrize("grid", [(5, 4, 3), (9, 7, 1), (1, 8, 6)], ids=["5x4x3", "9x7x1", "1x8x6"])
def test_levels_of_the_ordered_form(L, grid):
    c = M.grid_case(grid, 1)
    n = M.ngrid_of(c)
    gx, gy, gz = I.geometry(*grid)
    i = np.arange(n)
    xyz = i % gx + (i // gx) % gy + i // (gx * gy)
    nv, visit, level = _levels(L, c, M.USERDEFINED, M.permutation(grid, "natural"))
    assert nv == n and np.array_equal(visit, i) and np.array_equal(level, xyz)               # the natural order: x + y + z again
    nv, visit, level = _levels(L, c, M.ASCEND)
    assert nv == n and np.array_equal(level, xyz)
    nv, visit, level = _levels(L, c, M.DESCEND)
    assert nv == n and np.array_equal(visit, i[::-1]) and np.array_equal(level, xyz.max() - xyz[::-1])
    rb = M.red_black(grid)
    for order in (M.CPFIRST, M.FPFIRST):
        nv, visit, level = _levels(L, c, order, rb)
        first = np.flatnonzero(rb == order)
        assert nv == n and np.array_equal(visit[:first.size], first) and np.array_equal(level, (np.arange(n) >= first.size).astype(np.int32))
    # a marking that leaves points out: only the marked points are visited; a level never holds two visits that depend on each other
    pm = M.partial_marks(grid)
    nv, visit, level = _levels(L, c, M.CPFIRST, pm)
    assert nv == int(np.sum(pm != 0)) and set(visit) == set(np.flatnonzero(pm != 0))
    # the library's levels against the restatement's rule with geometric neighbours only: on a grid-like matrix the wrap terms are not terms
    rnd = M.permutation(grid, "random")
    nv, visit, level = _levels(L, c, M.USERDEFINED, rnd)
    nbr = {int(p): [int(p + d) for d, ok in ((-1, p % gx > 0), (1, p % gx < gx - 1), (-gx, (p // gx) % gy > 0), (gx, (p // gx) % gy < gy - 1),
                                              (-gx * gy, p // (gx * gy) > 0), (gx * gy, p // (gx * gy) < gz - 1)) if ok] for p in range(n)}
    lw, mr, want = [-1] * n, [-1] * n, []
    for p in (int(q) for q in rnd):
        lv = max([lw[p], mr[p]] + [lw[j] for j in nbr[p]]) + 1
        want.append(lv); lw[p] = lv
        for j in nbr[p]:
            mr[j] = max(mr[j], lv)
    assert nv == n and np.array_equal(visit, rnd) and np.array_equal(level, want)


def test_levels_with_a_wrap_coefficient_follow_the_index_rule(L):
    grid = (5, 4, 3)
    c = M.wrap_case(grid, 1)
    nv, visit, level = _levels(L, c, M.ASCEND)
    assert nv == 60 and np.array_equal(level, M.visit_levels(c, np.arange(60)))
    assert level[5] == level[4] + 1            # row 5 (x = 0, y = 1) waits for point 4 (x = 4, y = 0)


def _sweep(L, case, kind, order, mark, w, b, u, nsweeps=1, dinv=None):
    A, keep = M.as_str(case)
    mk = None if mark is None else np.ascontiguousarray(mark, dtype=np.int32)
    info = (C.c_int * 8)()
    return L.fasp_hip_str_sweep(C.byref(A), kind, order, None if mk is None else mk.ctypes.data_as(T.c_int_p), w, None if dinv is None else T.dp(dinv),
                                T.dp(b), T.dp(u), nsweeps, info)


def test_refusals(L, fa, capfd):
    grid = (5, 4, 3)
    c = M.grid_case(grid, 2)
    b, u0 = M.vectors(c)
    M.protos(L)
    # a USERDEFINED sequence with an entry out of range, and with a point named twice: refused with a message, u untouched
    for bad in (np.r_[np.arange(59), 60], np.r_[np.arange(59), -1], np.r_[np.arange(59), 3]):
        u = u0.copy()
        assert _sweep(L, c, M.GS, M.USERDEFINED, bad, 1.0, b, u) == T.ERROR_INPUT_PAR and np.array_equal(_bits(u), _bits(u0))
        assert _form(L, c, M.USERDEFINED, bad) == T.ERROR_INPUT_PAR
        dinv = M.dinv_of(L, c)
        capfd.readouterr()
        for name, kw in (("gs_order", {}), ("sor_order", dict(w=1.1)), ("gs1", dict(order=M.USERDEFINED)), ("sor", dict(order=M.USERDEFINED, w=1.1))):
            got = M.call(L, name, c, b, u0, mark=bad, dinv=dinv, **kw)
            assert np.array_equal(_bits(got), _bits(u0)), name
            assert "user-defined order" in capfd.readouterr().err
    # NULL diaginv with nc > 1 in a *1 or order-specific entry
    rb = M.red_black(grid)
    for name, kw in (("jacobi1", {}), ("gs1", dict(order=M.ASCEND)), ("gs_ascend", {}), ("gs_descend", {}), ("gs_cf", dict(order=1, mark=rb)),
                     ("sor1", dict(order=M.DESCEND, w=1.1)), ("sor_ascend", dict(w=1.1)), ("sor_descend", dict(w=1.1)),
                     ("gs_order", dict(mark=M.permutation(grid, "natural"))), ("sor_order", dict(mark=M.permutation(grid, "natural"), w=1.1)),
                     ("sor_cf", dict(order=-1, mark=rb, w=1.1))):
        got = M.call(L, name, c, b, u0, dinv=None, **kw)
        assert np.array_equal(_bits(got), _bits(u0)), name
        assert "diaginv is NULL" in capfd.readouterr().err, name
    # mark == NULL and an order that is neither ASCEND nor DESCEND does nothing, as in the reference
    assert np.array_equal(_bits(M.call(L, "gs", c, b, u0, order=7)), _bits(u0))
    assert np.array_equal(_bits(M.call(L, "sor", c, b, u0, order=M.CPFIRST, w=1.1)), _bits(u0))
    u = u0.copy()
    assert _sweep(L, c, M.GS, 7, None, 1.0, b, u) == 0 and np.array_equal(_bits(u), _bits(u0))
    # nc < 1: the reference's message, nothing done; nc > 7 and a kind outside 0 .. 2 are refused
    capfd.readouterr()
    A, keep = M.as_str(c)
    A.nc = 0
    bb, u = b.copy(), u0.copy()
    bv, uv = T.dvector(bb.size, T.dp(bb)), T.dvector(u.size, T.dp(u))
    L.fasp_smoother_dstr_gs(C.byref(A), C.byref(bv), C.byref(uv), M.ASCEND, None)
    L.fasp_smoother_dstr_jacobi(C.byref(A), C.byref(bv), C.byref(uv))
    assert np.array_equal(_bits(u), _bits(u0))
    assert capfd.readouterr().out.count("nc is illegal") == 2
    c8 = dict(nx=2, ny=2, nz=1, nc=8, offsets=[-1, 1], diag=np.ones(4 * 64), bands=[np.zeros(3 * 64), np.zeros(3 * 64)])
    u = np.ones(32)
    assert _sweep(L, c8, M.GS, M.ASCEND, None, 1.0, np.ones(32), u) == T.ERROR_INPUT_PAR and np.all(u == 1.0)
    assert _form(L, c8, M.ASCEND) == T.ERROR_INPUT_PAR
    u = u0.copy()
    assert _sweep(L, c, 3, M.ASCEND, None, 1.0, b, u) == T.ERROR_INPUT_PAR and np.array_equal(_bits(u), _bits(u0))
    if not fa.available():   # no device: the sweep itself is refused, there is no CPU fallback
        u = u0.copy()
        assert _sweep(L, c, M.GS, M.ASCEND, None, 1.0, b, u) == T.ERROR_MISC and np.array_equal(_bits(u), _bits(u0))
