"""The matrices of tests/_plain_cases.py, without a GPU: every generator's assertions hold (the restated upload rules send the matrix to the kernel
it is built for, and it has the edges it exists for); the library's own coder leaves it plain; the kernel every run names per operation is what
the restated launch plan (tests/_csr_cases.py, expected_plan) and the library's (fasp_hip_csr_plan) make of the restated traits under the run's
tune keys, and together the runs name every plain instantiation; the oracle the device results are compared with is held, on every case and
operation, to an independent np.longdouble evaluation inside the a-priori bound of _libs.sum_bound_ratio -- and is bit-equal to the compiled
reference where that is present."""
import ctypes as C

import numpy as np
import pytest

from faspsolver_amd import _types as T

import _csr_cases as cc
import _plain_cases as pc
from _libs import have_ref, oracle, ref, sum_bound_ratio

CASES = pc.all_cases()
IDS = [name for name, _ in CASES]


@pytest.mark.parametrize("run", [r for _, r in CASES], ids=IDS)
def test_generator_assertions_and_library_coder(fa, run):
    c = pc.build(run)                          # the generator's own assertions
    A, keep = T.as_csr(c["ia"], c["ja"], c["val"], c["ncol"])
    k = C.c_int(-1)
    assert fa.lib().fasp_hip_coding_selftest(C.byref(A), C.byref(k)) == 0
    assert k.value == 0, (c["name"], k.value)                  # neither row patterns nor the byte dictionary
    t = c["traits"]
    assert not (t["code"] or t["pat"] or t["rowbase"] or t["sell_code"])
    assert (t["dpos"] == 1) == (c["nrow"] == c["ncol"] and not c["sorted"])      # diagonal positions iff square and not re-sorted


def _plan(L, t, op, partials):
    traits = (C.c_int * len(cc.TRAITS))(*[int(t[k]) for k in cc.TRAITS])
    out = (C.c_int * (len(cc.PLAN) + 1))()
    assert L.fasp_hip_csr_plan(traits, op, 0, int(partials), out, None) == 0
    return dict(zip(cc.PLAN, list(out))), out[len(cc.PLAN)]


@pytest.mark.parametrize("run", pc.RUNS, ids=[r["id"] for r in pc.RUNS])
def test_every_run_names_the_planned_kernel(fa, run):
    """Per (run, op): the instantiation the run names is the one the restated if-chain plans for the restated traits under the run's tune
    keys, and the library's plan_csr agrees; op 8 is a launch of op 0."""
    L = fa.lib()
    L.fasp_hip_csr_plan.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    c = pc.build(run)
    square = c["nrow"] == c["ncol"]
    assert {op for op, _ in run["ops"]} == set(c["ops"]) and set(c["ops"]) == set(cc.OPS_SQUARE if square and c["inf_rows"] is None else cc.OPS_RECT)
    tune = pc.plan_tune(run)
    try:
        for key, value in run["tune"]:
            assert L.fasp_hip_tune(key.encode(), value) == 0
        for op, partials in run["ops"]:
            e = cc.expected_plan(c["traits"], 0 if op == 8 else op, False, partials, tune)
            assert cc.KERNELS[e["kernel"]] == pc.expect(run, op, partials), (run["id"], op, partials, cc.KERNELS[e["kernel"]])
            p, fam0 = _plan(L, c["traits"], 0 if op == 8 else op, partials)
            assert {k: p[k] for k in cc.PLAN} == {k: e[k] for k in cc.PLAN}, (run["id"], op, p, e)
            assert fam0 == cc.expected_plan(c["traits"], 0, False, False, tune)["family"]
    finally:
        for key, _ in run["tune"]:
            L.fasp_hip_tune(key.encode(), pc.TUNE_RESTORE[key])


def test_runs_cover_every_plain_instantiation():
    """k_csr_rows<2 .. 64>, the four k_csr_wstream, the four k_csr_estream, k_csr_lstream, k_csr_xtile, k_csr_wstream2: each is the kernel of
    some (run, op); and the row kernel is reached both ways the plan falls back to it (a Jacobi sweep of a stream-kernel matrix that stores a
    diagonal twice, or of one whose device copy has no diagonal positions; op 7, a launch planned as a row window and the fused Jacobi partials of
    a k_csr_estream matrix)."""
    named = {pc.expect(run, op, partials) for run in pc.RUNS for op, partials in run["ops"]}
    assert named == set(cc.KERNELS[0:10]) | set(cc.KERNELS[19:23]) | {"lstream", "xtile", "wstream2"}
    by_id = {r["id"]: r for r in pc.RUNS}
    assert len(by_id) == len(pc.RUNS)
    assert pc.expect(by_id["ws2_dup_default"], 5, True).startswith("rows") and pc.expect(by_id["ws2_dup_default"], 6, False) == "wstream2"
    for op, partials in by_id["es_L16"]["ops"]:
        want_rows = op == 7 or (op == 5 and partials)
        assert pc.expect(by_id["es_L16"], op, partials).startswith("rows" if want_rows else "estream")
    assert (5, False) in by_id["es_L16"]["ops"] and (5, True) in by_id["es_L16"]["ops"]
    assert all(pc.expect(by_id["es_L4_planned_windowed"], op, partials).startswith("rows") for op, partials in by_id["es_L4_planned_windowed"]["ops"])
    assert all(set(k for k, _ in r["tune"]) <= set(pc.TUNE_RESTORE) for r in pc.RUNS)
    # ... and a stream-kernel launch of an operator without diagonal positions: the Jacobi sweep alone keeps k_csr_rows
    r = by_id["ws2_nodpos"]
    assert pc.build(r)["traits"]["dpos"] == 0 and pc.build(r)["traits"]["dup_diag"] == 0
    for op, partials in r["ops"]:
        assert pc.expect(r, op, partials).startswith("rows") == (op == 5)
        assert op == 5 or pc.expect(r, op, partials) == "wstream2"
    assert {(5, True), (5, False)} <= set(r["ops"])
    for rid in ("ls_t65", "ws2_t65", "xt_t65"):                   # the Jacobi sweep without the fused partials on the stream kernels themselves
        assert (5, False) in by_id[rid]["ops"] and pc.expect(by_id[rid], 5, False) in ("lstream", "wstream2", "xtile")
    # a row-relative 16-bit copy is k_csr_rows' alone: sent to a stream kernel, the operator must not pass it
    r = by_id["rect_stream_ls"]
    e = cc.expected_plan(pc.build(r)["traits"], 0, False, False, pc.plan_tune(r))
    assert pc.build(r)["traits"]["jbase"] == 1 and (e["ja16"], e["jbase"]) == (0, 0)
    e = cc.expected_plan(pc.build(by_id["rows_c_L8"])["traits"], 0, False, False, pc.plan_tune(by_id["rows_c_L8"]))
    assert (e["ja16"], e["jbase"]) == (1, 1)
    e = cc.expected_plan(pc.build(by_id["rows_c_ja16_off"])["traits"], 0, False, False, pc.plan_tune(by_id["rows_c_ja16_off"]))
    assert (e["ja16"], e["jbase"]) == (0, 0)


@pytest.mark.parametrize("run", [r for _, r in CASES], ids=IDS)
def test_oracle_inside_the_a_priori_bound(run):
    """orc_mxv, orc_aAxpy (alpha = 1, -1, 0.7 and the residual form), orc_smoother_jacobi, orc_smoother_l1diag against np.longdouble:
    |error| <= (m + 1) u / (1 - (m + 1) u) * sum |terms| + 2^-63 |exact| (pc.longdouble_op has m and the terms per operation)."""
    c = pc.build(run)
    orc = oracle()
    worst = 0.0
    for op in c["ops"]:
        if op in (7, 8):
            continue                              # (their row results are op 0's)
        x, b, y0 = cc.inputs(c["nrow"], c["ncol"], op, 1000 + op)     # finite x: the bound is about rounding
        y, _ = cc.reference(orc, c, op, x, b, y0, cc.SCALAR.get(op, 0.0))
        exact, sabs, m = pc.longdouble_op(c, op, x, b, y0, cc.SCALAR.get(op, 0.0))
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
    R.fasp_smoother_dcsr_jacobi.argtypes = [P(T.dvector), C.c_int, C.c_int, C.c_int, P(T.dCSRmat), P(T.dvector), C.c_int, C.c_double]
    R.fasp_smoother_dcsr_L1diag.argtypes = [P(T.dvector), C.c_int, C.c_int, C.c_int, P(T.dCSRmat), P(T.dvector), C.c_int]
    c = pc.build(run)
    n = c["nrow"]
    orc = oracle()
    A, keep = T.as_csr(c["ia"], c["ja"], c["val"], c["ncol"])
    bits = lambda v: np.ascontiguousarray(v).view(np.int64)
    for op in c["ops"]:
        scalar = cc.SCALAR.get(op, 0.0)
        x, b, y0 = cc.inputs(n, c["ncol"], op, 77 + op, c["inf_rows"])
        want, _ = cc.reference(orc, c, op, x, b, y0, scalar)
        x = np.ascontiguousarray(x)
        if op in (0, 7, 8):
            got = np.ones(n)
            R.fasp_blas_dcsr_mxv(C.byref(A), T.dp(x), T.dp(got))
        elif op in (1, 2, 3, 4):
            got = (b if op == 1 else y0).copy()
            R.fasp_blas_dcsr_aAxpy({1: -1.0, 2: 1.0, 3: -1.0, 4: scalar}[op], C.byref(A), T.dp(x), T.dp(got))
        else:
            u, got = T.as_vec(x.copy())
            bv, keep_b = T.as_vec(b)
            if op == 5:
                R.fasp_smoother_dcsr_jacobi(C.byref(u), 0, n - 1, 1, C.byref(A), C.byref(bv), 1, scalar)
            else:
                R.fasp_smoother_dcsr_L1diag(C.byref(u), 0, n - 1, 1, C.byref(A), C.byref(bv), 1)
        assert np.array_equal(bits(want), bits(got)), (c["name"], op)
