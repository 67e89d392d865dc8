"""The matrices of tests/_csr_cases.py, without a GPU: every generator's assertions hold (the matrix reaches the kernel it is built
for, by the upload rules restated there, and has the edges it exists for); the library's own coder agrees (fasp_hip_coding_selftest:
row patterns or the byte dictionary, round trip exact); and the oracle the device results are compared with is itself held, on every
case, to an independent np.longdouble evaluation inside the a-priori bound of _libs.sum_bound_ratio -- and is bit-equal to the
compiled reference where that is present."""
import ctypes as C

import numpy as np
import pytest

from faspsolver_amd import _types as T

import _csr_cases as cc
from _libs import csr_mxv_longdouble, have_ref, oracle, ref, sum_bound_ratio

CASES = cc.all_cases()
IDS = [rid for rid, _ in CASES]


@pytest.mark.parametrize("run", [r for _, r in CASES], ids=IDS)
def test_generator_assertions_and_library_coder(fa, run):
    c, _ = cc.build(run)                       # the generator's own assertions
    A, keep = T.as_csr(c["ia"], c["ja"], c["val"], c["ncol"])
    k = C.c_int(-1)
    assert fa.lib().fasp_hip_coding_selftest(C.byref(A), C.byref(k)) == 0
    assert k.value == (4 if c["kind"] == cc.KIND["dict8"] else 5), (c["name"], k.value)
    assert c["coding"]["kind"] == k.value


def test_the_empty_swept_pattern_is_accepted():
    """L = 0 of the *lengths* cases: no upload rule refuses a matrix whose swept rows are empty (nnz = 6142 >= 4096; three patterns;
    16 padded table entries), so the case is in the GPU list."""
    c = cc.p4_length(0)
    assert c["coding"]["why"] is None and c["kind"] == cc.KIND["rowpat4"]
    assert any(r["fn"] is cc.p4_length and r["args"] == (0,) for r in cc.RUNS)


def test_runs_cover_every_instantiation():
    """Every kernel instantiation has a run that must report its family: k_csr_rowpat4, k_csr_rowpat5, k_csr_rowpat forms 0 / 1 / 2 with
    1 and 2 rows per lane, k_csr_dict8 with U = 8 / 16 / 24."""
    fam = {}
    for run in cc.RUNS:
        c, kind = cc.build(run)
        fam.setdefault(kind, set()).add(run["id"])
        assert all(len(t) == 3 for t in run["tune"])
    assert set(fam) == {4, 5, 6, 9}
    forms = {(cc.build(r)[0]["form"], dict((k, v) for k, v, _ in r["tune"]).get("rpl")) for r in cc.RUNS if r["fn"] is cc.rp and r["tune"] and r["tune"][0][0] == "rpl"}
    assert forms == {(f, q) for f in (0, 1, 2) for q in (1, 2)}
    assert {r["args"][0] for r in cc.RUNS if r["fn"] is cc.d8} == set(cc.D8_MEANS)


def _longdouble_op(c, op, x, b, y0, scalar):
    """(exact, sabs, m) of row operation `op` in np.longdouble: the value, the absolute sum of its terms, the rounded operations behind it."""
    ld = np.longdouble
    ia, ja, val, n = c["ia"], c["ja"], c["val"], c["nrow"]
    lens = np.diff(ia)
    if op == 5:    # the diagonal entries leave the sum: d = the last one stored
        rows = np.repeat(np.arange(n), lens)
        ond = ja == rows
        d = np.zeros(n)
        d[rows[ond]] = val[ond]                 # (duplicates: the last assignment wins, as in the reference's loop)
        t, s, m = csr_mxv_longdouble(ia, ja, np.where(ond, 0.0, val), x)
        live = np.abs(d) > 1e-20
        dd = np.where(live, d, 1.0).astype(ld)
        w = ld(scalar)
        one_w = ld(1 - scalar)                  # (1 - w is rounded once in double: part of the expression)
        exact = np.where(live, one_w * x.astype(ld) + w * (b.astype(ld) - t) / dd, x.astype(ld))
        sabs = np.abs(one_w * x.astype(ld)) + np.abs(w / dd) * (np.abs(b).astype(ld) + s)
        return exact, sabs, np.where(live, m + 5, 0)
    t, s, m = csr_mxv_longdouble(ia, ja, val, x)
    if op in (0, 7, 8):
        return t, s, m
    if op in (1, 2, 3, 4):
        alpha = {1: -1.0, 2: 1.0, 3: -1.0, 4: scalar}[op]
        v0 = (b if op == 1 else y0).astype(ld)
        return v0 + ld(alpha) * t, np.abs(v0) + abs(ld(alpha)) * s, np.where(m > 0, m + 2, 0)
    # op 6: d = sum |a| is itself a rounded sum of m terms
    d = np.add.reduceat(np.abs(np.r_[val, 0.0]).astype(ld), np.minimum(ia[:-1], len(val)))
    d = np.where(lens > 0, d, 0.0)
    live = np.abs(d.astype(np.float64)) > 1e-20
    dd = np.where(live, d, 1.0)
    exact = np.where(live, x.astype(ld) + (b.astype(ld) - t) / dd, x.astype(ld))
    sabs = np.abs(x).astype(ld) + (np.abs(b).astype(ld) + s) / dd
    return exact, sabs, np.where(live, 2 * m + 3, 0)


@pytest.mark.parametrize("run", [r for _, r in CASES], ids=IDS)
def test_oracle_inside_the_a_priori_bound(run):
    """orc_mxv, orc_aAxpy (alpha = 1, -1, 0.7 and the residual form), orc_smoother_jacobi, orc_smoother_l1diag against np.longdouble:
    |error| <= (m + 1) u / (1 - (m + 1) u) * sum |terms| + 2^-63 |exact|, m = the rounded operations behind an entry (the row's products,
    + 2 for y + alpha t, + 5 for the Jacobi update, twice + 3 for the L1 sweep whose divisor is a rounded sum of as many terms)."""
    c, _ = cc.build(run)
    orc = oracle()
    worst = 0.0
    for op in c["ops"]:
        if op in (7, 8):
            continue                              # (their row results are op 0's)
        x, b, y0 = cc.inputs(c["nrow"], c["ncol"], op, 1000 + op)     # finite x: the bound is about rounding
        y, _ = cc.reference(orc, c, op, x, b, y0, cc.SCALAR.get(op, 0.0))
        exact, sabs, m = _longdouble_op(c, op, x, b, y0, cc.SCALAR.get(op, 0.0))
        ratio = sum_bound_ratio(y, exact, sabs, m)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (c["name"], op, ratio)
    print(f"{c['name']}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("run", [r for _, r in CASES], ids=IDS)
def test_oracle_bit_equal_to_the_compiled_reference(run):
    if not have_ref():
        pytest.skip("the compiled reference (oracle/_ref) is absent")
    R = ref()
    P = C.POINTER
    R.fasp_blas_dcsr_mxv.argtypes = [P(T.dCSRmat), T.c_double_p, T.c_double_p]
    R.fasp_blas_dcsr_aAxpy.argtypes = [C.c_double, P(T.dCSRmat), T.c_double_p, T.c_double_p]
    c, _ = cc.build(run)
    orc = oracle()
    A, keep = T.as_csr(c["ia"], c["ja"], c["val"], c["ncol"])
    x, b, y0 = cc.inputs(c["nrow"], c["ncol"], 0, 77, c["inf_rows"])
    y1, _ = cc.reference(orc, c, 0, x, b, y0, 0.0)
    y2 = np.ones(c["nrow"])
    R.fasp_blas_dcsr_mxv(C.byref(A), T.dp(x), T.dp(y2))
    assert np.array_equal(y1.view(np.int64), y2.view(np.int64))
    for op, alpha in ((2, 1.0), (3, -1.0), (4, 0.7)):
        y1, _ = cc.reference(orc, c, op, x, b, y0, alpha)
        y2 = y0.copy()
        R.fasp_blas_dcsr_aAxpy(alpha, C.byref(A), T.dp(x), T.dp(y2))
        assert np.array_equal(y1.view(np.int64), y2.view(np.int64)), (c["name"], alpha)
