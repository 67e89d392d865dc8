"""The structured smoothers on the device (csrc/str_sweep.hip.h): k_str_jacobi, and the Gauss-Seidel / SOR sweeps in their three forms --
one launch per level x + y + z, planes pipelined over workgroups, the ordered form (level list) -- forced by the tune key str_sweep_form
on the same input.

Every comparison is np.array_equal on the bits against the numpy restatement of ItrSmootherSTR.c (tests/_str_smoother_cases.model_sweep),
which tests/test_str_smoother_host.py holds to the reference bit for bit: no tolerance.  The geometric forms skip only terms whose
coefficient the plan has found to be exactly 0.0; with the finite vectors and right-hand sides used here (no -0.0 among them) that changes
no bit.  Every run asserts the form that ran (info[0]) -- otherwise a test would silently exercise another kernel -- and a zero status: the
error word is clear."""
import ctypes as C
import functools

import numpy as np
import pytest

import _str_ilu_cases as I
import _str_smoother_cases as M
from _libs import T

pytestmark = pytest.mark.gpu

NCS = [1, 2, 3, 5, 7]
KINDS = [(M.GS, 1.0), (M.SOR, 1.1), (M.SOR, 0.0), (M.SOR, 1.0)]
FORMS = {"level": M.FORM_LEVEL, "pipe": M.FORM_PIPE, "list": M.FORM_LIST}


@pytest.fixture(scope="module")
def L(gpu):
    return M.protos(gpu.lib())


@pytest.fixture(autouse=True)
def _tunes_back(gpu):
    yield
    lib = gpu.lib()
    lib.fasp_hip_tune(b"str_sweep_form", -1)
    lib.fasp_hip_tune(b"str_sweep_wgs", 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def case_of(grid, nc, which="grid"):
    """(case, b, u0, dinv) built once, read-only.  dinv: the library's own inverse blocks (host code)."""
    import faspsolver_amd as fa
    c = {"grid": lambda: M.grid_case(grid, nc), "noncanon": lambda: M.grid_case(grid, nc, order=M.NONCANON[6 if I.geometry(*grid)[2] > 1 else 4], ),
         "wrap": lambda: M.wrap_case(grid, nc), "extra": lambda: M.extra_offset_case(grid, nc), "diffusion": lambda: M.diffusion_case(grid)}[which]()
    b, u0 = M.vectors(c)
    dinv = M.dinv_of(fa.lib(), c)
    for a in [b, u0, c["diag"]] + list(c["bands"]) + ([] if dinv is None else [dinv]):
        a.setflags(write=False)
    return c, b, u0, dinv


@functools.lru_cache(maxsize=None)
def want_of(grid, nc, which, kind, w, order, markkey=None, cf=False):
    c, b, u0, dinv = case_of(grid, nc, which)
    u = M.model_sweep(c, kind, order, mark_of(grid, markkey), w, dinv, b, u0, cf_entry=cf)
    u.setflags(write=False)
    return u


def mark_of(grid, key):
    return None if key is None else {"rb": M.red_black, "part": M.partial_marks}[key](grid) if key in ("rb", "part") else M.permutation(grid, key)


def dev_sweep(L, c, kind, order, mark, w, dinv, b, u0, form=-1, wgs=0, nsweeps=1):
    """nsweeps sweeps through fasp_hip_str_sweep under the forced form -> (status, u, info)."""
    A, keep = M.as_str(c)
    L.fasp_hip_tune(b"str_sweep_form", form)
    L.fasp_hip_tune(b"str_sweep_wgs", wgs)
    mk = None if mark is None else np.ascontiguousarray(mark, dtype=np.int32)
    u = np.array(u0)
    info = (C.c_int * 8)()
    st = L.fasp_hip_str_sweep(C.byref(A), kind, order, None if mk is None else mk.ctypes.data_as(T.c_int_p), w, None if dinv is None else T.dp(np.array(dinv)),
                              T.dp(np.array(b)), T.dp(u), nsweeps, info)
    return st, u, list(info)


def check(L, grid, nc, form, which="grid", wgs=0, kinds=KINDS, orders=(M.ASCEND, M.DESCEND)):
    c, b, u0, dinv = case_of(grid, nc, which)
    for kind, w in kinds:
        for order in orders:
            want = want_of(grid, nc, which, kind, w, order)
            st, u, info = dev_sweep(L, c, kind, order, None, w, dinv, b, u0, form, wgs)
            assert st == 0 and info[0] == form, (kind, w, order, st, info)      # the form the test is about; the error word is clear
            if form == M.FORM_PIPE:
                assert info[1] == 1 and 1 <= info[3] <= I.geometry(*grid)[2] and (not wgs or info[3] == wgs)   # one launch, at most a workgroup per plane
            bad = np.flatnonzero(_bits(u) != _bits(want))
            assert bad.size == 0, (kind, w, order, bad[:8], u[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("grid", [(5, 4, 3), (17, 9, 6)], ids=["5x4x3", "17x9x6"])
def test_jacobi(L, grid, nc):
    c, b, u0, dinv = case_of(grid, nc)
    want = want_of(grid, nc, "grid", M.JACOBI, 1.0, 0)
    st, u, info = dev_sweep(L, c, M.JACOBI, 0, None, 1.0, dinv, b, u0)
    assert st == 0 and info[0] == M.FORM_JACOBI and info[1] == 1
    assert np.array_equal(_bits(u), _bits(want))
    assert np.array_equal(_bits(M.call(L, "jacobi", c, b, u0)), _bits(want))          # inverts for itself


# 70 x 67 x 3: in-plane levels of up to 67 points against the 36 (nc 7) .. 256 (nc 1) of a workgroup step; 17 x 9 x 6: no multiple of 64
@pytest.mark.parametrize("form", list(FORMS), ids=list(FORMS))
@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("grid", [(5, 4, 3), (17, 9, 6), (70, 67, 3)], ids=["5x4x3", "17x9x6", "70x67x3"])
def test_gs_sor_ascend_descend_in_every_form(L, grid, nc, form):
    check(L, grid, nc, FORMS[form])


@pytest.mark.parametrize("wgs", [1, 2])
@pytest.mark.parametrize("nc", NCS)
def test_ticket_loop_with_fewer_workgroups_than_planes(L, nc, wgs):
    """Nine planes on one and on two workgroups: a workgroup draws plane after plane; no residency is assumed."""
    check(L, (6, 5, 9), nc, M.FORM_PIPE, wgs=wgs)


@pytest.mark.parametrize("form", ["level", "list"])
@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("grid", [(9, 7, 1), (1, 8, 6)], ids=["9x7x1", "1x8x6"])
def test_2d_grids(L, grid, nc, form):
    check(L, grid, nc, FORMS[form])
    if form == "level":   # nothing to pipeline, whatever is asked for
        c, b, u0, dinv = case_of(grid, nc)
        st, u, info = dev_sweep(L, c, M.GS, M.ASCEND, None, 1.0, dinv, b, u0, M.FORM_PIPE)
        assert st == 0 and info[0] == M.FORM_LEVEL and np.array_equal(_bits(u), _bits(want_of(grid, nc, "grid", M.GS, 1.0, M.ASCEND)))


@pytest.mark.parametrize("form", list(FORMS), ids=list(FORMS))
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("grid", [(5, 4, 3), (17, 9, 6), (9, 7, 1)], ids=["5x4x3", "17x9x6", "9x7x1"])
def test_bands_stored_in_another_order(L, grid, nc, form):
    """+1 before -1, planes first: the terms are taken in storage order in every form."""
    if grid[2] == 1 and form == "pipe":
        form = "level"
    check(L, grid, nc, FORMS[form], which="noncanon", kinds=[(M.GS, 1.0), (M.SOR, 1.1)])


@pytest.mark.parametrize("perm", ["reversed", "random"])
@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("grid", [(5, 4, 3), (17, 9, 6)], ids=["5x4x3", "17x9x6"])
def test_user_defined_order(L, grid, nc, perm):
    c, b, u0, dinv = case_of(grid, nc)
    mark = M.permutation(grid, perm)
    for kind, w in ((M.GS, 1.0), (M.SOR, 1.1)):
        want = want_of(grid, nc, "grid", kind, w, M.USERDEFINED, perm)
        st, u, info = dev_sweep(L, c, kind, M.USERDEFINED, mark, w, dinv, b, u0)
        assert st == 0 and info[0] == M.FORM_LIST and info[4] == mark.size
        assert np.array_equal(_bits(u), _bits(want)), (kind, w)
    # the reversed sequence is the descending sweep
    if perm == "reversed":
        assert np.array_equal(_bits(want_of(grid, nc, "grid", M.GS, 1.0, M.USERDEFINED, perm)), _bits(want_of(grid, nc, "grid", M.GS, 1.0, M.DESCEND)))


@pytest.mark.parametrize("marks", ["rb", "part"])
@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("grid", [(5, 4, 3), (17, 9, 6)], ids=["5x4x3", "17x9x6"])
def test_cf_orders(L, grid, nc, marks):
    c, b, u0, dinv = case_of(grid, nc)
    mark = mark_of(grid, marks)
    for order in (M.CPFIRST, M.FPFIRST):
        for kind, w in KINDS:
            want = want_of(grid, nc, "grid", kind, w, order, marks)
            st, u, info = dev_sweep(L, c, kind, order, mark, w, dinv, b, u0)
            assert st == 0 and info[0] == M.FORM_LIST and info[4] == int(np.sum(mark != 0))
            if marks == "rb":
                assert info[1] == 2 and info[2] == 2                  # a colouring: two levels, two launches
            assert np.array_equal(_bits(u), _bits(want)), (order, kind, w)
            keep = np.repeat(mark == 0, nc)
            assert np.array_equal(_bits(u[keep]), _bits(u0[keep]))    # points marked neither keep their bits


@pytest.mark.parametrize("which", ["wrap", "extra"])
@pytest.mark.parametrize("nc", [1, 3])
def test_matrices_that_are_not_grid_like_take_the_ordered_form(L, nc, which):
    grid = (17, 9, 6)
    c, b, u0, dinv = case_of(grid, nc, which)
    for forced in (-1, M.FORM_LEVEL, M.FORM_PIPE):
        for kind, w in ((M.GS, 1.0), (M.SOR, 1.1)):
            for order in (M.ASCEND, M.DESCEND):
                want = want_of(grid, nc, which, kind, w, order)
                st, u, info = dev_sweep(L, c, kind, order, None, w, dinv, b, u0, forced)
                assert st == 0 and info[0] == M.FORM_LIST and info[5] == 0
                assert np.array_equal(_bits(u), _bits(want)), (forced, kind, order)
    # ... and Jacobi takes every term of the reference
    st, u, info = dev_sweep(L, c, M.JACOBI, 0, None, 1.0, dinv, b, u0)
    assert st == 0 and np.array_equal(_bits(u), _bits(want_of(grid, nc, which, M.JACOBI, 1.0, 0)))
    if which == "wrap":   # the coefficient matters: the grid-like matrix gives another vector
        assert not np.array_equal(want_of(grid, nc, which, M.GS, 1.0, M.ASCEND), M.model_sweep(case_of(grid, nc)[0], M.GS, M.ASCEND, None, 1.0, dinv, b, u0))


@pytest.mark.parametrize("form", list(FORMS), ids=list(FORMS))
@pytest.mark.parametrize("nc", [1, 3])
def test_three_resident_sweeps_are_three_public_calls(L, nc, form):
    grid = (17, 9, 6)
    c, b, u0, dinv = case_of(grid, nc)
    for kind, w, name, kw in ((M.GS, 1.0, "gs", {}), (M.SOR, 1.1, "sor", dict(w=1.1))):
        st, u, info = dev_sweep(L, c, kind, M.DESCEND, None, w, dinv, b, u0, FORMS[form], nsweeps=3)
        assert st == 0 and info[0] == FORMS[form]
        v = u0
        for _ in range(3):
            v = M.call(L, name, c, b, v, order=M.DESCEND, **kw)
        assert np.array_equal(_bits(u), _bits(v))
    st, u, info = dev_sweep(L, c, M.JACOBI, 0, None, 1.0, dinv, b, u0, nsweeps=3)
    v = u0
    for _ in range(3):
        v = M.call(L, "jacobi1", c, b, v, dinv=None if dinv is None else np.array(dinv))
    assert st == 0 and np.array_equal(_bits(u), _bits(v))


def test_every_public_entry_once(L):
    """Each of the sixteen entries through the ctypes mirror, nc = 3 on 5 x 4 x 3, against the restatement."""
    import faspsolver_amd as fa
    assert fa.ASCEND == 12 and fa.DESCEND == 21 and fa.USERDEFINED == 0 and fa.CPFIRST == 1 and fa.FPFIRST == -1
    grid, nc = (5, 4, 3), 3
    c, b, u0, dinv = case_of(grid, nc)
    d = np.array(dinv)
    rb, rnd = M.red_black(grid), M.permutation(grid, "random")
    calls = [("jacobi", {}, (M.JACOBI, 1.0, 0, None, False)), ("jacobi1", dict(dinv=d), (M.JACOBI, 1.0, 0, None, False)),
             ("gs", dict(order=M.ASCEND), (M.GS, 1.0, M.ASCEND, None, False)), ("gs", dict(order=M.FPFIRST, mark=rb), (M.GS, 1.0, M.FPFIRST, "rb", False)),
             ("gs1", dict(order=M.USERDEFINED, mark=rnd, dinv=d), (M.GS, 1.0, M.USERDEFINED, "random", False)),
             ("gs_ascend", dict(dinv=d), (M.GS, 1.0, M.ASCEND, None, False)), ("gs_descend", dict(dinv=d), (M.GS, 1.0, M.DESCEND, None, False)),
             ("gs_order", dict(dinv=d, mark=rnd), (M.GS, 1.0, M.USERDEFINED, "random", False)),
             ("gs_cf", dict(dinv=d, mark=rb, order=M.CPFIRST), (M.GS, 1.0, M.CPFIRST, "rb", True)),
             ("sor", dict(order=M.DESCEND, w=1.1), (M.SOR, 1.1, M.DESCEND, None, False)),
             ("sor1", dict(order=M.CPFIRST, mark=rb, dinv=d, w=1.1), (M.SOR, 1.1, M.CPFIRST, "rb", False)),
             ("sor_ascend", dict(dinv=d, w=1.1), (M.SOR, 1.1, M.ASCEND, None, False)), ("sor_descend", dict(dinv=d, w=0.0), (M.SOR, 0.0, M.DESCEND, None, False)),
             ("sor_order", dict(dinv=d, mark=rnd, w=1.1), (M.SOR, 1.1, M.USERDEFINED, "random", False)),
             ("sor_cf", dict(dinv=d, mark=rb, order=M.FPFIRST, w=1.1), (M.SOR, 1.1, M.FPFIRST, "rb", True))]
    assert {n for n, _, _ in calls} == set(M.ENTRIES)
    for name, kw, (kind, w, order, markkey, cf) in calls:
        want = want_of(grid, nc, "grid", kind, w, order, markkey, cf)
        assert np.array_equal(_bits(M.call(L, name, c, b, u0, **kw)), _bits(want)), name
    # the scalar C/F SOR with its SECOND pass closed as Gauss-Seidel (ItrSmootherSTR.c:1443)
    c1, b1, u1, _ = case_of(grid, 1)
    assert np.array_equal(_bits(M.call(L, "sor_cf", c1, b1, u1, mark=rb, order=M.CPFIRST, w=1.1)), _bits(want_of(grid, 1, "grid", M.SOR, 1.1, M.CPFIRST, "rb", True)))


def test_ten_gs_sweeps_reduce_the_residual(L):
    grid = (17, 9, 6)
    c, b, u0, dinv = case_of(grid, 1, "diffusion")
    st, u, info = dev_sweep(L, c, M.GS, M.ASCEND, None, 1.0, None, b, u0, nsweeps=10)
    assert st == 0
    v = u0
    for _ in range(10):
        v = M.model_sweep(c, M.GS, M.ASCEND, None, 1.0, None, b, v)
    r0, r10, want = M.residual_norm(c, b, u0), M.residual_norm(c, b, u), M.residual_norm(c, b, v)
    print(f"residual norm {r0:.6e} -> {r10:.6e} after ten sweeps")
    assert np.array_equal(_bits(u), _bits(v)) and r10 == want and r10 < r0
