"""The ILU triangular solves of csrc/ilu.hip.h (k_ilu_level, k_ilu_flow, every block size, the L / U forms) on hand-built factors at
the edges of their schedule, against the restatements of tests/_ilu_cases.py -- plain Python floats in the reference's order, proven
against the compiled reference by test_ilu_cases.py on the CPU, so nothing here needs the reference library.

  every case x entry x form   z starts NaN-filled, the call is made twice: both results BIT-EQUAL to the restatement and to each other,
                              r / ijlu / luval untouched, no factor resident (caller-built factors are never registered).  Levels of
                              1, 63, 64, 65, 128, 129 rows, chains of 2 .. 129 levels, n = 1, empty rows, a 300-entry row beside short
                              ones, unsorted and stranded entries, 150 chunks per level, 4100 chunks in one launch (cap)
  schedule                    fasp_hip_ilu_schedule (uploads, reports, launches nothing) = the restated rule of ilu_build_tri: levels,
                              chunks, slab entries, entries, longest row, the form the depth selects, the workgroups of either form
  auto form                   24 levels: level launches; 25, 26: the single launch; the solve with ilu_form = -1 gives the restated bits
  special values              +0.0 / -0.0 right-hand sides bit for bit; one +inf, one quiet NaN at row 0, n // 2, n - 1: NaN in the same
                              places, the same bits elsewhere.  No input holds the all-ones pattern (the single launch's own mark)
  block smoother              fasp_smoother_dbsr_ilu, nb 1, 3, 6: x + restatement(b - A x) bit for bit, the residual in the order
                              test_bsr_ops.py pins for the block residual kernel (the oracle's aAxpy(-1)); no case needed the bound
  refusals                    a column outside [0, n) among the entries a triangle reads: ERROR_DATA_STRUCTURE from the schedule entry,
                              without a launch; nb = 8: ERROR_INPUT_PAR

The restatements hold their own a-priori bound (test_ilu_cases.py): largest error / bound 0.54 (scalar), 0.42 (blocks).  The kernels
are compared bit for bit, so no further ratio is measured here.  Measured on an MI355X: the 129 tests of this file take under 3 s (2.6 .. 2.9 over four runs),
the slowest 0.8 s (cap with level launches, its first use builds the factor of 262 400 rows)."""
import ctypes as C

import numpy as np
import pytest

import _ilu_cases as K
from _libs import T
from test_ilu_cases import call_smoother, smoother_case, special_rhs

pytestmark = pytest.mark.gpu

SCALAR_ENTRIES = ("fasp_precond_ilu", "fasp_precond_ilu_forward", "fasp_precond_ilu_backward")
INFO = ("levels", "chunks", "slab", "real", "longest", "auto", "level_wgs", "flow_wgs")


@pytest.fixture(scope="module")
def lib(gpu):
    L = gpu.lib()
    L.fasp_hip_ilu_resident_count.restype = C.c_int
    yield L
    L.fasp_hip_tune(b"ilu_form", -1)


def _vp(d):
    return C.cast(C.byref(d), C.c_void_p)


def apply(L, entry, F, r):
    """One application through a fresh caller-built ILU_data, z NaN-filled before; the inputs must come back untouched"""
    d, keep = F.ilu_data()
    rr, z = np.array(r), np.full(F.n * F.nb, np.nan)
    getattr(L, entry)(T.dp(rr), T.dp(z), _vp(d))
    assert rr.tobytes() == np.asarray(r).tobytes(), (entry, "r changed")
    assert keep[0].tobytes() == F.ijlu.tobytes() and keep[1].tobytes() == F.luval.tobytes(), (entry, "the factor changed")
    assert L.fasp_hip_ilu_resident_count() == 0
    return z


def assert_bits(label, got, want):
    ok, bad = K.same_values(got, want)
    assert ok, (label, len(bad), bad[:8], np.asarray(got)[bad[:8]], np.asarray(want)[bad[:8]])


def check(L, entry, F, r, want, forms=(0, 1), twice=True):
    """the entry in each form, twice: the restated bits both times (NaN in the same places), the two results equal in every byte"""
    try:
        for form in forms:
            L.fasp_hip_tune(b"ilu_form", form)
            z = apply(L, entry, F, r)
            assert_bits((entry, "form", form), z, want)
            if twice:
                assert apply(L, entry, F, r).tobytes() == z.tobytes(), (entry, "form", form, "two calls differ")
    finally:
        L.fasp_hip_tune(b"ilu_form", -1)


@pytest.mark.parametrize("entry", SCALAR_ENTRIES)
@pytest.mark.parametrize("case", [c for c in K.SCALAR_CASES if c != "cap"])
def test_scalar_solves_equal_the_restatement(lib, case, entry):
    F = K.factor(case)
    want = K.restated(case, 1, entry)
    assert np.all(np.isfinite(want))
    check(lib, entry, F, K.rhs(F), want)


@pytest.mark.parametrize("nb", range(1, 8))
@pytest.mark.parametrize("case", K.BLOCK_CASES)
def test_block_solve_equals_the_restatement(lib, case, nb):
    F = K.factor(case, nb)
    want = K.restated(case, nb, "fasp_precond_dbsr_ilu")
    assert np.all(np.isfinite(want))
    check(lib, "fasp_precond_dbsr_ilu", F, K.rhs(F), want)


@pytest.mark.parametrize("form", [0, 1])
def test_cap_more_chunks_than_wavefronts_in_the_single_launch(lib, form):
    F = K.factor("cap")
    check(lib, "fasp_precond_ilu", F, K.rhs(F), K.restated("cap", 1, "fasp_precond_ilu"), forms=(form,), twice=False)


def device_schedule(L, F, nb, which):
    d, keep = F.ilu_data()
    info = np.full(8, np.nan)
    st = L.fasp_hip_ilu_schedule(C.byref(d), nb, which, T.dp(info))
    assert L.fasp_hip_ilu_resident_count() == 0
    return st, info


@pytest.mark.parametrize("case,nb", [(c, 1) for c in K.SCALAR_CASES] + [(c, nb) for c in K.BLOCK_CASES for nb in range(2, 8)])
def test_schedule_equals_the_restated_rule(lib, case, nb):
    F = K.factor(case, nb)
    for which, upper in ((1, False), (2, True)):
        st, info = device_schedule(lib, F, nb, which)
        want = K.schedule(F, upper)
        assert st == 0 and dict(zip(INFO, info.tolist())) == {k: float(want[k]) for k in INFO}, (which, info)


@pytest.mark.parametrize("n,single", [(24, 0), (25, 1), (26, 1)])
def test_auto_form_switches_beyond_24_levels(lib, n, single):
    F = K.factor(f"chain:{n}")
    lib.fasp_hip_tune(b"ilu_form", -1)
    for which in (1, 2):
        st, info = device_schedule(lib, F, 1, which)
        assert st == 0 and (info[0], info[5]) == (n, single)
        d, keep = F.ilu_data()
        took = np.zeros(6)
        assert lib.fasp_hip_ilu_time(C.byref(d), which, 1, T.dp(took)) >= 0.0      # the form the solves take as the tune stands
        assert (took[0], took[1]) == (n, single)
    for entry in SCALAR_ENTRIES:
        check(lib, entry, F, K.rhs(F), K.restated(f"chain:{n}", 1, entry), forms=(-1,))


@pytest.mark.parametrize("case", ["bands:65", "chain:65"])
def test_special_values(lib, case):
    F = K.factor(case)
    for label, r in special_rhs(F):
        for entry in SCALAR_ENTRIES:
            want = K.ENTRIES[entry](F, r)
            if label in ("zeros", "all -0.0"):
                assert np.all(np.isfinite(want))
            else:
                assert not np.all(np.isfinite(want))
            check(lib, entry, F, r, want)


@pytest.mark.parametrize("nb", [1, 3, 6])
@pytest.mark.parametrize("case", K.BLOCK_CASES)
def test_block_smoother_equals_the_restatement(lib, case, nb):
    F = K.factor(case, nb)
    ia, ja, val, b, x0, want = smoother_case(F)
    try:
        for form in (0, 1):
            lib.fasp_hip_tune(b"ilu_form", form)
            assert_bits(("smoother", "form", form), call_smoother(lib, F, ia, ja, val, b, x0), want)
            assert lib.fasp_hip_ilu_resident_count() == 0
    finally:
        lib.fasp_hip_tune(b"ilu_form", -1)


def test_refusals(lib):
    for kind in ("u_high", "u_far", "l_neg"):
        for which in (1, 2):   # the copy holds both triangles: either one's fault refuses it
            st, info = device_schedule(lib, K.edge_factor(kind), 1, which)
            assert st == T.ERROR_DATA_STRUCTURE and not info.any(), (kind, which, st)
    F = K.edge_factor("stranded_out")   # out-of-range columns that nothing reads: a valid factor, the chain's schedule and bits
    for which in (1, 2):
        st, info = device_schedule(lib, F, 1, which)
        assert st == 0 and info[0] == F.n
    r = K.rhs(F)
    check(lib, "fasp_precond_ilu", F, r, K.precond_ilu(F, r))
    F = K.factor("chain:2")
    assert device_schedule(lib, F, 8, 1)[0] == T.ERROR_INPUT_PAR and device_schedule(lib, F, 0, 1)[0] == T.ERROR_INPUT_PAR
    assert device_schedule(lib, F, 1, 0)[0] == T.ERROR_INPUT_PAR and device_schedule(lib, F, 1, 3)[0] == T.ERROR_INPUT_PAR
    assert lib.fasp_hip_ilu_schedule(None, 1, 1, T.dp(np.zeros(8))) == T.ERROR_INPUT_PAR
