"""The hand-built factors of tests/_ilu_cases.py on the CPU: the restated solves equal the compiled reference's byte for byte
(so test_gpu_ilu_kernels.py needs no reference library), hold an a-priori rounding bound of their own in np.longdouble, and the
cases have the schedule properties the device tests rely on.

The a-priori check (|x_i - row i evaluated exactly on the computed x| <= gamma_m s_i, _ilu_cases.triangle_ratio) is a measurement
against a derived bound, not a tuned tolerance: the largest error / bound over all cases is 0.54 (scalar) and 0.42 (blocks)."""
import ctypes as C

import numpy as np
import pytest

import _ilu_cases as K
import _libs
from _libs import T

SCALAR = [c for c in K.SCALAR_CASES if c != "cap"]
BLOCK = [(c, nb) for c in K.BLOCK_CASES for nb in range(1, 8)]


@pytest.fixture(scope="module")
def ref():
    R = _libs.ref()
    if R is None:
        pytest.fail("the reference build (oracle/_ref/libfasp_ref.so) is missing")
    for f in K.ENTRIES:
        getattr(R, f).argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
        getattr(R, f).restype = None
    return R


def _call(lib, entry, F, r):
    """one application through a caller-built ILU_data -> (z, the arrays it ran on)"""
    d, keep = F.ilu_data()
    rr, z = np.array(r), np.full(F.n * F.nb, np.nan)
    getattr(lib, entry)(T.dp(rr), T.dp(z), C.cast(C.byref(d), C.c_void_p))
    assert rr.tobytes() == np.asarray(r).tobytes()
    assert keep[0].tobytes() == F.ijlu.tobytes() and keep[1].tobytes() == F.luval.tobytes()
    return z


@pytest.mark.ref
@pytest.mark.parametrize("entry", ["fasp_precond_ilu", "fasp_precond_ilu_forward", "fasp_precond_ilu_backward"])
@pytest.mark.parametrize("case", SCALAR)
def test_scalar_restatement_equals_the_reference(ref, case, entry):
    F = K.factor(case)
    assert K.restated(case, 1, entry).tobytes() == _call(ref, entry, F, K.rhs(F)).tobytes()


@pytest.mark.ref
@pytest.mark.parametrize("case,nb", BLOCK)
def test_block_restatement_equals_the_reference(ref, case, nb):
    F = K.factor(case, nb)
    r = K.rhs(F)
    z = K.restated(case, nb, "fasp_precond_dbsr_ilu")
    assert z.tobytes() == _call(ref, "fasp_precond_dbsr_ilu", F, r).tobytes()
    if nb == 1:   # the reference's case 1 is its scalar solve
        assert z.tobytes() == _call(ref, "fasp_precond_ilu", F, r).tobytes()


@pytest.mark.ref
@pytest.mark.parametrize("case", ["bands:65", "chain:65"])
def test_restatement_on_special_values_equals_the_reference(ref, case):
    """signed zeros bit for bit; Inf / NaN right-hand sides: NaN in the same places, the same bits elsewhere"""
    F = K.factor(case)
    for label, r in special_rhs(F):
        for entry in ("fasp_precond_ilu", "fasp_precond_ilu_forward", "fasp_precond_ilu_backward"):
            ok, bad = K.same_values(K.ENTRIES[entry](F, r), _call(ref, entry, F, r))
            assert ok, (label, entry, bad[:8])


def smoother_case(F):
    """fasp_smoother_dbsr_ilu on the factor: (ia, ja, val of A, b, x0, the restated result x0 + restatement(b - A x0)), the residual
    formed by the oracle's aAxpy(-1), the order test_bsr_ops.py pins for the reference and for the device's residual kernel"""
    n = F.n * F.nb
    ia, ja, val = K.smoother_matrix(F)
    A, keep = T.as_bsr(ia, ja, val, F.nb)
    rng = np.random.default_rng(50 + F.nb)
    b, x0 = rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n)
    res = b.copy()
    _libs.orc_bsr_ops().orc_bsr_aAxpy(-1.0, C.byref(A), T.dp(x0.copy()), T.dp(res))
    return ia, ja, val, b, x0, x0 + K.precond_dbsr_ilu(F, res)


def call_smoother(lib, F, ia, ja, val, b, x0):
    n = F.n * F.nb
    A, keep = T.as_bsr(ia, ja, val, F.nb)
    d, dkeep = F.ilu_data()
    bb, x = b.copy(), x0.copy()
    lib.fasp_smoother_dbsr_ilu(C.byref(A), C.byref(T.dvector(n, T.dp(bb))), C.byref(T.dvector(n, T.dp(x))), C.cast(C.byref(d), C.c_void_p))
    assert bb.tobytes() == b.tobytes() and dkeep[0].tobytes() == F.ijlu.tobytes() and dkeep[1].tobytes() == F.luval.tobytes()
    assert keep[1].tobytes() == np.asarray(ja, dtype=np.int32).tobytes() and keep[2].tobytes() == val.tobytes()
    return x


@pytest.mark.ref
@pytest.mark.parametrize("nb", [1, 3, 6])
@pytest.mark.parametrize("case", K.BLOCK_CASES)
def test_smoother_restatement_equals_the_reference(ref, case, nb):
    F = K.factor(case, nb)
    ia, ja, val, b, x0, want = smoother_case(F)
    ref.fasp_smoother_dbsr_ilu.argtypes = [C.POINTER(T.dBSRmat), C.POINTER(T.dvector), C.POINTER(T.dvector), C.c_void_p]
    ref.fasp_smoother_dbsr_ilu.restype = None
    assert call_smoother(ref, F, ia, ja, val, b, x0).tobytes() == want.tobytes()
    assert np.all(np.isfinite(want)) and np.any(want != x0)


def special_rhs(F):
    """right-hand sides with +0.0 / -0.0 entries, one +inf, one quiet NaN at row 0, n // 2, n - 1 -> [(label, r)]"""
    n = F.n
    out = []
    z = K.rhs(F, 9)
    z[::3] = 0.0
    z[1::3] = -0.0
    out.append(("zeros", z))
    out.append(("all -0.0", np.full(n, -0.0)))
    for at in (0, n // 2, n - 1):
        for name, v in (("inf", np.inf), ("nan", np.nan)):
            r = K.rhs(F, 10)
            r[at] = v
            out.append((f"{name}@{at}", r))
    for _, r in out:
        assert not np.any(K.bits(r) == np.uint64(0xFFFFFFFFFFFFFFFF))   # never the single launch's "not computed" mark
        r.setflags(write=False)
    return out


_worst = {}


def _apriori(F):
    r = K.rhs(F)
    if F.nb == 1:
        y, z = K.precond_ilu_forward(F, r), K.precond_ilu(F, r)
        assert z.tobytes() == K.precond_ilu_backward(F, y).tobytes()      # the pair of sweeps is the two single ones
    else:
        z = K.precond_dbsr_ilu(F, r)
        # the block solve has no one-triangle entry: its y from the same routine on a factor without U parts and identity pivots
        blocks = F.luval.reshape(-1, F.nb, F.nb)
        rows = [[(int(F.ijlu[p]), blocks[p]) for p in pos] for pos in K.read_positions(F, False)]
        y = K.precond_dbsr_ilu(K.Factor(rows, np.tile(np.eye(F.nb), (F.n, 1, 1)), F.nb), r)
    ratio_l, ratio_u = K.triangle_ratio(F, False, r, y), K.triangle_ratio(F, True, y, z)
    kind = "scalar" if F.nb == 1 else "block"
    _worst[kind] = max(_worst.get(kind, 0.0), ratio_l, ratio_u)
    print(f"error / bound: L {ratio_l:.3e}, U {ratio_u:.3e} (largest {kind} so far {_worst[kind]:.3e})")
    assert ratio_l <= 1.0 and ratio_u <= 1.0, (ratio_l, ratio_u)
    # the check has teeth: a dropped entry, a swapped pair of triangles or a forgotten pivot is far outside the bound
    if K.schedule(F, False)["real"]:
        assert K.triangle_ratio(F, True, r, y) > 1.0 and K.triangle_ratio(F, False, y, z) > 1.0
        i = int(np.argmax([len(p) for p in K.read_positions(F, False)]))
        y_bad = y.copy(); y_bad[i * F.nb] = np.nextafter(y_bad[i * F.nb], np.inf) + 1e-9
        assert K.triangle_ratio(F, False, r, y_bad) > 1.0


@pytest.mark.parametrize("case", K.SCALAR_CASES)
def test_scalar_restatement_within_the_a_priori_bound(case):
    _apriori(K.factor(case))


@pytest.mark.parametrize("case,nb", [(c, nb) for c, nb in BLOCK if nb > 1])
def test_block_restatement_within_the_a_priori_bound(case, nb):
    _apriori(K.factor(case, nb))


def test_generators_are_deterministic():
    for case, nb in (("ragged", 1), ("unsorted", 1), ("bands:65", 3)):
        a = K.factor.__wrapped__(case, nb)
        assert a.ijlu.tobytes() == K.factor(case, nb).ijlu.tobytes() and a.luval.tobytes() == K.factor(case, nb).luval.tobytes()


def _both(F):
    return K.schedule(F, False), K.schedule(F, True)


def test_one_and_diag():
    for s in _both(K.factor("one")):
        assert (s["levels"], s["chunks"], s["slab"], s["real"], s["longest"]) == (1, 1, 0, 0, 0)
    for s in _both(K.factor("diag:130")):
        assert (s["levels"], s["chunks"], s["slab"], s["real"]) == (1, 3, 0, 0) and s["chunk_live"].tolist() == [64, 64, 2]


@pytest.mark.parametrize("n", K.CHAINS)
def test_chain_has_n_levels_of_one_row(n):
    for nb in ((1, 2, 7) if n == 65 else (1,)):
        for s in _both(K.factor(f"chain:{n}", nb)):
            assert s["levels"] == n == s["chunks"] and np.all(s["level_rows"] == 1) and s["real"] == n - 1
            assert s["auto"] == (1 if n >= 25 else 0)
            assert s["level_wgs"] == n and s["flow_wgs"] == (n + 3) // 4


@pytest.mark.parametrize("m", K.BANDS)
def test_bands_has_three_levels_of_m_rows(m):
    for nb in ((1, 3) if m == 65 else (1,)):
        for s in _both(K.factor(f"bands:{m}", nb)):
            assert s["levels"] == 3 and s["level_rows"].tolist() == [m, m, m]
            assert s["chunks"] == 3 * -(-m // 64) and s["chunk_live"][-1] == (m - 1) % 64 + 1
            assert 1 <= s["chunk_kmin"][-1] and s["longest"] <= 5


def test_wide_and_cap_fill_the_grids():
    for s in _both(K.factor("wide")):
        assert s["levels"] == 2 and s["level_rows"].tolist() == [9600, 9600] and s["chunks"] == 300 and s["level_wgs"] == 2 * 38
    for s in _both(K.factor("cap")):
        assert s["levels"] == 2 and s["level_rows"].tolist() == [131200, 131200]
        assert s["chunks"] == 4100 > 4 * K.FLOW_MAX_GRID and s["flow_wgs"] == K.FLOW_MAX_GRID   # every wavefront draws again


def test_unsorted_has_stranded_entries_that_would_change_the_schedule():
    F = K.factor("unsorted")
    n = F.n
    for upper, s in zip((False, True), _both(F)):
        counted = K.levels_counting_stranded(F, upper)
        assert np.sum(counted > s["level"]) >= 5 and counted.max() + 1 != s["levels"]
    reads = [set(a) | set(b) for a, b in zip(K.read_positions(F, False), K.read_positions(F, True))]
    stranded = [set(range(F.ijlu[i], F.ijlu[i + 1])) - reads[i] for i in range(n)]
    rows = [i for i in range(n) if stranded[i]]
    assert len(rows) >= n // 4
    assert sum(any(F.ijlu[p] == i for p in stranded[i]) for i in rows) >= 5            # explicit col == i entries
    assert sum(F.ijlu[min(stranded[i])] == i for i in rows) >= 2                       # ... right where the L part stops
    assert all(any(F.ijlu[p] < i for p in stranded[i]) and any(F.ijlu[p] > i for p in stranded[i]) for i in rows)
    # shuffled parts: with each part sorted instead, the same factor gives other bits -- the order of subtraction matters
    def entry(p):
        return int(F.ijlu[p]), float(F.luval[p])
    lo, up = K.read_positions(F, False), K.read_positions(F, True)
    srt = K.Factor([sorted(entry(p) for p in lo[i]) + [entry(p) for p in sorted(stranded[i])] + sorted(entry(p) for p in up[i])
                    for i in range(n)], F.luval[:n], 1)
    assert srt.ijlu.tobytes() != F.ijlu.tobytes() and sorted(srt.luval.tolist()) == sorted(F.luval.tolist())
    assert K.precond_ilu(F, r := K.rhs(F)).tobytes() != K.precond_ilu(srt, r).tobytes()


@pytest.mark.parametrize("nb", [1, 3])
def test_ragged_has_a_long_row_beside_short_ones_and_empty_rows(nb):
    F = K.factor("ragged", nb)
    long = 300 if nb == 1 else 100
    assert F.n == (400 if nb == 1 else 150)
    for upper, s in zip((False, True), _both(F)):
        assert s["longest"] == long and np.sum(s["chunk_kmax"] == long) == 1
        c = int(np.argmax(s["chunk_kmax"]))
        assert s["chunk_live"][c] >= 2 and s["chunk_kmin"][c] < long // 4 and s["chunk_live"][c] < 64   # short rows and padding beside it
        assert np.any(s["chunk_kmin"] == 0)                                # a chunk whose shortest live row is empty
        assert np.any(s["chunk_lane0"] < s["chunk_kmax"])                  # the longest row of a chunk is not always in lane 0
        assert s["slab"] > s["real"]
        lens = np.array([len(p) for p in K.read_positions(F, upper)])
        assert np.sum(lens == 0) >= F.n // 8
        # rows that skip levels: they read level-0 rows only, three strata or more above the bottom
        depth = np.arange(F.n) * 8 // F.n
        depth = 7 - depth if upper else depth
        assert np.sum((lens > 0) & (s["level"] == 1) & (depth >= 3)) >= 3
    empty_both = [i for i in range(F.n) if F.ijlu[i] == F.ijlu[i + 1]]
    assert len(empty_both) >= 3


def test_edge_factors():
    for kind in ("u_high", "u_far", "l_neg", "stranded_out"):
        F = K.edge_factor(kind)
        cols = F.ijlu[F.n + 1:]
        assert (cols.max() >= F.n) or (cols.min() < 0)
    F = K.edge_factor("stranded_out")   # nothing reads the out-of-range columns: both triangles are the chain's
    for upper in (False, True):
        assert all(0 <= F.ijlu[p] < F.n for pos in K.read_positions(F, upper) for p in pos)
        assert K.schedule(F, upper)["levels"] == F.n
