"""The sequential sweep kernels -- k_split_rest<LR>, k_split_direct<LR>, k_split_scatter, k_tri_flow<L, PF>, k_tri_level<L, PF>
(csrc/seq_split.hip.h), k_tri_chain<FORM>, k_tri_chain_ref<FORM> (csrc/seq_chain.hip.h), k_seq_level<L> (csrc/kernels.hip.h) -- on the
irregular matrices of tests/_sweep_cases.py, one sweep at a time through fasp_hip_csr_sweep: the schedule builders and the launch half of the
cycle's own sweeps (smoothers.hip.h) under the run's tune keys.

Path and shape.  info, written at the launch sites, must name the path the run was built for and the lanes, rounds, spine rounds, virtual rows,
strips, chunks, rest-pass lanes and chain tiers that the host self-tests report for the same parameters (_sweep_cases.derive;
tests/test_sweep_cases.py holds the runs to them without a GPU).  A run that misses its kernel fails.

Untouched rows.  The entry returns the device's WHOLE vector: rows outside the sweep, and swept rows the reference leaves alone (|a_ii| <=
1e-20: a stored zero, no diagonal; of a diagonal stored twice the last hit counts), must come back bit-equal to the input, compared as int64
-- a store through a wrong row index, a padded position, a virtual row or a ghost slot shows here.  Under zero_start the input never reaches
the device: the entry itself checks that every row outside the sweep still holds +0.0 there and fails the call (status != 0) otherwise; a
swept row that is left alone comes back as that +0.0.

Row-wise a-priori bound.  Every swept row i must satisfy its OWN equation on the device's output: with v_j = u_out[j] where j is swept before
i, else the input (0 under zero_start), s = sum_{j != i} a_ij v_j over the noff off-diagonal entries, in np.longdouble,
    exact_i = (b_i - s) / d                        forms 0 and 1,       sabs_i = (|b_i| + sum |a_ij v_j|) / |d|
    exact_i = w (b_i - s) / d + (1 - w) u_in[i]    form 2,              sabs_i = |w| (|b_i| + sum |a_ij v_j|) / |d| + |(1 - w) u_in[i]|
held by _libs.sum_bound_ratio to |u_out[i] - exact_i| <= (m + 1) u / (1 - (m + 1) u) sabs_i (u = 2^-53; + 2^-63 |exact_i| for the 80-bit
side), m = the roundings a term passes through at most.  t = b_i - s is a summation tree over noff + 1 leaves whatever the path groups --
(b - rest) - lower, virtual rows (sums of their own, read with coefficient 1), a spine or the chain's tiers of fused multiply-adds (one
rounding for product and sum), the band's two accumulators: a product rounds once (or not at all inside a fused multiply-add), a leaf passes
through at most noff sums (adding the 0.0 of an unused slot is exact): noff + 1.  On top of that
  the split and chain paths 1 .. 6 (tri_update / chain_update): the stored reciprocal rd = RN(1 / d) rounds once;
      form 0  t * rd: one more                                                              m = noff + 3
      form 1  tri_div, three operations (q = t rd, r = fma(-d, q, t), fma(r, rd, q))        m = noff + 5
      form 2  tri_div, then w * . and the final sum (1 - w, its product with u_in[i] and the final sum: three roundings of the short
              term)                                                                        m = noff + 7
  k_seq_level, paths 7 and 8: form 0  t * (1.0 / d): the reciprocal and the product         m = noff + 3
      form 1  t / d                                                                         m = noff + 2
      form 2  t / d, w * ., the final sum                                                   m = noff + 4
(_sweep_cases.EXTRA).  The bound does not accumulate along the recurrence -- every row is checked against the values the device itself
produced for the rows before it -- yet the equations determine the sweep: a wrong operand, a missed entry, an old value read for a new one
exceed it by orders of magnitude (tests/test_sweep_cases.py shows that on the reference).  The largest error / bound per path and
instantiation is printed; these are measurements against the bound (<= 1), not tuned tolerances.  Measured on an MI355X:
k_tri_flow<L, PF> and k_tri_level<L, PF> 0.004 .. 0.369 (largest: <1, 4>; the pairs bit-identical), k_split_direct<LR> 0.139 .. 0.362,
k_split_rest<LR> + k_split_scatter(final) 0.174 .. 0.295, k_tri_chain<FORM> and k_tri_chain_ref<FORM> 0.150 .. 0.336, k_seq_level<L> at most
0.373 over dependency levels and 0.377 over colours; |u - reference| at most 2.6e-15 max |reference|.

Project bar.  |u - reference| <= 1e-12 max |reference| over the swept rows, against the plain sequential sweep of ItrSmootherCSR.c over the
same rows on the same inputs (_sweep_cases.reference_sweep: bit-equal to the CPU oracle's sweeps where it has them; the multicolour mode
against the sweep in ITS order, colour by colour, the colouring restated in _sweep_cases.colour_order).

Every call is made twice and must repeat itself bit for bit.  Documented bit identities: the runs of a group of _sweep_cases.GROUPS -- the
dataflow form and one launch per class, k_tri_chain and k_tri_chain_ref, every seq_grid, seq_chain_grid = 3 and the default, strips of 16 KB
and of 512 KB -- must agree bit for bit on the swept rows; seq_zero_skip 1 and 0 under zero_start and the same sweep from stored zeros must
agree as values (bit for bit apart from the sign of zero).  Bad arguments are refused with ERROR_INPUT_PAR and touch nothing."""
import ctypes as C

import numpy as np
import pytest

from faspsolver_amd import _types as T

import _sweep_cases as sc
from _libs import sum_bound_ratio

pytestmark = pytest.mark.gpu

_out = {}       # run id -> (u, info, input u)
_refs = {}      # inputs of a sweep -> the reference's result (shared by the runs of a group)
_worst = {}     # path / instantiation -> largest error / bound seen
SENTINEL = 77


def _bits(v):
    return np.ascontiguousarray(v).view(np.int64)


def _call(L, A, seq, run, b, u, info):
    return L.fasp_hip_csr_sweep(C.byref(A), seq.ctypes.data_as(C.POINTER(C.c_int)), len(seq), run["form"], run["w"], run["zero_start"],
                                T.dp(b), T.dp(u), info)


def _sweep(L, run):
    """The run's sweep, twice, under its tune keys -> (u, info, the input u)."""
    if run["id"] in _out:
        return _out[run["id"]]
    ia, ja, a = sc.matrix(*run["mat"])
    A, keep = T.as_csr(ia, ja, a)
    seq = sc.sequence(run)
    b, u0 = sc.inputs(run)
    b = np.ascontiguousarray(b)
    try:
        for key, value in run["tune"]:
            assert L.fasp_hip_tune(key.encode(), value) == 0
        res = []
        for _ in range(2):
            u = u0.copy()
            info = (C.c_int * 12)(*([SENTINEL] * 12))
            st = _call(L, A, seq, run, b, u, info)
            assert st == 0, (run["id"], st)
            res.append((u, list(info)))
    finally:
        for key, _ in run["tune"]:
            L.fasp_hip_tune(key.encode(), sc.TUNE_RESTORE[key])
    assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])), (run["id"], "the second call differs")
    assert res[0][1] == res[1][1], (run["id"], res[0][1], res[1][1])
    _out[run["id"]] = (res[0][0], res[0][1], u0)
    return _out[run["id"]]


def _reference(run):
    key = (run["mat"], run["seq"], run["form"], run["w"], run["zero_start"], run["u0"], sc.tune_of(run)["gs_multicolor"])
    if key not in _refs:
        _refs[key] = sc.reference_sweep(run)
        _refs[key].setflags(write=False)
    return _refs[key]


def _kernel_name(run, info):
    path, Lp, rounds, LR = info[0], info[1], info[2], info[3]
    name = {0: "nothing", 1: f"k_split_direct<{LR}>", 2: f"k_split_rest<{LR}> + k_split_scatter", 3: f"k_tri_flow<{Lp}, {rounds}>",
            4: f"k_tri_level<{Lp}, {rounds}>", 5: f"k_tri_chain<{run['form']}>", 6: f"k_tri_chain_ref<{run['form']}>",
            7: f"k_seq_level<{Lp}> (levels)", 8: f"k_seq_level<{Lp}> (colours)"}[path]
    return name


@pytest.mark.parametrize("run", sc.RUNS, ids=[r["id"] for r in sc.RUNS])
def test_sweep_kernel_against_its_own_equations_and_the_reference(gpu, run):
    L = gpu.lib()
    u, info, u0 = _sweep(L, run)
    rid = run["id"]
    # --- path and shape
    d = sc.derive(run)
    path, Lp, rounds, LR, spine, virtual, strips, chunks, launches, n1b, t1, t2 = info
    assert path == run["path"] == d["path"], (rid, sc.PATHS.get(path), sc.PATHS[run["path"]], info)
    assert (Lp, rounds, LR, spine, virtual, strips, chunks) == (d["L"], d["rounds"], d["LR"], d["spine"], d["virtual"], d["strips"], d["chunks"]), (rid, info, d)
    assert (n1b, t1, t2) == (d["n1b"], d["t1"], d["t2"]), (rid, info, d)
    for key, want in run["want"].items():
        got = dict(L=Lp, rounds=rounds, LR=LR, spine=spine, virtual=virtual, strips=strips, n1b=n1b, t1=t1, t2=t2, launches=launches)[key]
        assert want is None or (got > 0 if want == ">0" else got == want), (rid, key, got, want)
    classes = sc.structure(run)["classes"]
    if path in (0, 1):
        assert launches == 0, (rid, launches)
    elif path in (2, 3, 5, 6):
        assert launches == 1, (rid, launches)
    elif path == 4:                                     # a launch per class of rows (and per class of virtual rows between them), and the scatter
        assert classes + 1 <= launches <= 2 * classes + 1 and (virtual > 0 or launches == classes + 1), (rid, launches, classes)
    elif path == 8:
        assert launches == sc.colour_order(run)[1], (rid, launches)
    # --- untouched rows
    ia, ja, a = sc.matrix(*run["mat"])
    n = len(ia) - 1
    seq = sc.sequence(run)
    dg, alone = sc.diagonals(ia, ja, a)
    swept = np.zeros(n, dtype=bool)
    swept[seq] = True
    assert np.all(np.isfinite(u))
    bad = np.flatnonzero(~swept & (_bits(u) != _bits(u0)))
    assert len(bad) == 0, (rid, "rows outside the sweep were written", bad[:8])
    uin = np.zeros(n) if run["zero_start"] else u0
    bad = np.flatnonzero(swept & alone & (_bits(u) != _bits(uin)))
    assert len(bad) == 0, (rid, "rows without a usable diagonal were written", bad[:8], u[bad[:8]], uin[bad[:8]])
    if len(seq) == 0:
        return
    # --- every swept row's own equation, in np.longdouble, on the device's output
    # (u is the device's whole vector; under zero_start the rows outside the sweep, checked by the entry to hold +0.0 there, keep the caller's values)
    full = np.where(swept, u, uin) if run["zero_start"] else u
    rows, exact, sabs, m = sc.row_equation(run, full)
    ratio = sum_bound_ratio(full[rows], exact, sabs, m)
    name = _kernel_name(run, info)
    _worst[name] = max(_worst.get(name, 0.0), ratio)
    # --- the project's bar against the sequential reference
    ref = _reference(run)
    err = float(np.abs(u[seq] - ref[seq]).max()) / max(float(np.abs(ref[seq]).max()), 1e-300)
    print(f"{rid} {name}: error / bound {ratio:.3e} (largest of {name} so far {_worst[name]:.3e}), |u - reference| / max |reference| {err:.3e}")
    assert ratio <= 1.0, (rid, name, ratio)
    assert err <= 1e-12, (rid, name, err)


@pytest.mark.parametrize("group", sorted(sc.GROUPS), ids=sorted(sc.GROUPS))
def test_documented_bit_identities(gpu, group):
    L = gpu.lib()
    members = sc.GROUPS[group]
    seq = sc.sequence(sc.BY_ID[members[0]])
    outs = [_sweep(L, sc.BY_ID[i])[0][seq] for i in members]
    for i, v in zip(members[1:], outs[1:]):
        if sc.GROUP_SAME[group] == "values":            # flagged zero with and without the skip, stored zeros: equal values, the sign of a zero apart
            assert np.array_equal(v, outs[0]), (group, i, members[0], int(np.sum(v != outs[0])))
        else:
            bad = np.flatnonzero(_bits(v) != _bits(outs[0]))
            assert len(bad) == 0, (group, i, members[0], len(bad), seq[bad[:8]], v[bad[:8]], outs[0][bad[:8]])


def test_bad_arguments_are_refused_and_touch_nothing(gpu):
    L = gpu.lib()
    ia, ja, a = sc.matrix(sc.tridiag, (65,))
    n = 65
    A, keep = T.as_csr(ia, ja, a)
    Arect, keep2 = T.as_csr(ia, ja, a, n + 1)
    good = np.arange(n, dtype=np.int32)
    rng = np.random.default_rng(3)
    b = rng.standard_normal(n); u0 = rng.standard_normal(n)
    ip = lambda s: s.ctypes.data_as(C.POINTER(C.c_int))
    def seq_with(k, v):
        s = good.copy(); s[k] = v
        return s
    cases = {"A == NULL": (None, good, n, 0, b, True), "b == NULL": (A, good, n, 0, None, True), "u == NULL": (A, good, n, 0, b, False),
             "seq == NULL": (A, None, n, 0, b, True), "ns < 0": (A, good, -1, 0, b, True), "row != col": (Arect, good, n, 0, b, True),
             "form 3": (A, good, n, 3, b, True), "form -1": (A, good, n, -1, b, True), "entry n": (A, seq_with(7, n), n, 1, b, True),
             "entry -1": (A, seq_with(0, -1), n, 1, b, True), "repeated entry": (A, seq_with(64, 3), n, 2, b, True)}
    for what, (Ap, s, ns, form, bb, with_u) in cases.items():
        u = u0.copy()
        info = (C.c_int * 12)(*([SENTINEL] * 12))
        st = L.fasp_hip_csr_sweep(C.byref(Ap) if Ap is not None else None, ip(s) if s is not None else None, ns, form, 1.1, 0,
                                  T.dp(bb) if bb is not None else None, T.dp(u) if with_u else None, info)
        assert st == T.ERROR_INPUT_PAR, (what, st)
        assert np.array_equal(_bits(u), _bits(u0)) and list(info) == [SENTINEL] * 12, what
    # ... and the same call with good arguments goes through; info may be NULL
    u = u0.copy()
    assert L.fasp_hip_csr_sweep(C.byref(A), ip(good), n, 0, 1.0, 0, T.dp(b), T.dp(u), None) == 0
    assert not np.array_equal(_bits(u), _bits(u0))
