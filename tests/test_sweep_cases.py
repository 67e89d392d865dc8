"""The runs of tests/_sweep_cases.py, without a GPU: for every run the host self-tests (fasp_hip_seq_schedule_selftest,
fasp_hip_seq_chain_selftest), called with the run's strip size, lanes, spine, tier-1 blocks, form and weight, walk the schedule to the
sequential sweep and report the shape the run was built for -- and the dispatch rules of smoothers.hip.h / seq_sched.cpp, restated in
_sweep_cases.derive, send it down the path the run names.  Together the runs cover every path 1 .. 8, every k_tri_flow / k_tri_level <L, 4 | 8>,
every k_split_direct<LR> and k_split_rest<LR>, every k_seq_level<L>, and the chain form with and without tiers 1 and 2: a generator that misses
its kernel fails here.  The Python restatement of the reference's sweep that the device results are compared with is bit-equal to the CPU
oracle's sweeps where the oracle has the sweep (whole range, u_i = t * (1 / a_ii) and SOR)."""
import ctypes as C

import numpy as np
import pytest

from faspsolver_amd import _types as T

import _sweep_cases as sc
from _libs import oracle, sum_bound_ratio

IDS = [r["id"] for r in sc.RUNS]
LANES = (1, 2, 4, 8, 16, 32, 64)


@pytest.mark.parametrize("run", sc.RUNS, ids=IDS)
def test_run_reaches_the_path_and_shape_it_was_built_for(fa, run):
    d = sc.derive(run)                      # (asserts that the host walk of the schedule reproduces the sequential sweep)
    assert d["path"] == run["path"], (run["id"], sc.PATHS[d["path"]], sc.PATHS[run["path"]])
    for key, want in run["want"].items():
        if want is None or key == "launches":
            continue
        if want == ">0":
            assert d[key] > 0, (run["id"], key, d[key])
        else:
            assert d[key] == want, (run["id"], key, d[key], want)
    if run["path"] in (3, 4):
        assert d["L"] in LANES and d["rounds"] in (4, 8) and d["spine"] in (0, 2) and d["strips"] >= 1 and d["chunks"] >= 1
        assert not (d["rounds"] == 4 and d["spine"])           # a spine comes with eight rounds
    if run["path"] in (5, 6):
        c = d["chain"]
        assert c["blocks"] == (len(sc.sequence(run)) + 63) // 64 and (c["t2_steps"] > 0) == (c["t2"] > 0) and c["band"] > 0
    assert set(k for k, _ in run["tune"]) <= set(sc.TUNE_RESTORE)


def test_runs_cover_every_path_and_instantiation(fa):
    D = {r["id"]: sc.derive(r) for r in sc.RUNS}
    R = sc.BY_ID
    def ids(pred): return [i for i in D if pred(R[i], D[i])]
    assert {d["path"] for d in D.values()} == set(range(9))
    for path in (3, 4):                                         # k_tri_flow<L, PF> and k_tri_level<L, PF>
        got = {(d["L"], d["rounds"]) for d in D.values() if d["path"] == path}
        assert got == {(L, pf) for L in LANES for pf in (4, 8)}, (path, sorted(got))
        for L in LANES:
            mine = [i for i in D if D[i]["path"] == path and D[i]["L"] == L]
            assert {R[i]["form"] for i in mine} == {0, 1, 2}, (path, L)
            assert {R[i]["seq"][0] for i in mine} >= {"asc", "desc"}, (path, L)
            assert any(D[i]["virtual"] > 0 for i in mine) and any(D[i]["virtual"] == 0 and D[i]["rounds"] == 8 for i in mine), (path, L)
            assert {D[i]["spine"] for i in mine} == ({0, 2} if L >= 2 else {0}), (path, L)
        assert any(d["strips"] > 1 for d in D.values() if d["path"] == path)
    assert {d["LR"] for d in D.values() if d["path"] == 1} == set(LANES)                 # k_split_direct<LR>
    assert {d["LR"] for d in D.values() if d["path"] == 2} == set(LANES)                 # k_split_rest<LR> in front of the final scatter
    assert {d["LR"] for d in D.values() if d["path"] in (2, 3, 4, 5, 6)} == set(LANES)
    assert {d["L"] for d in D.values() if d["path"] == 7} == {2, 4, 8, 16, 32, 64}       # k_seq_level<L>
    assert R["arrow_L1_selects_64"]["want"]["L"] == 64
    assert len(ids(lambda r, d: d["path"] == 8 and r["seq"][0] == "desc")) >= 2 and len(ids(lambda r, d: d["path"] == 8 and r["seq"][0] == "asc")) >= 2
    # the chain form: every tier populated, the band alone, tier 1 forced to one block, subsets, descending, every update form, both kernels
    for path in (5, 6):
        ch = [i for i in D if D[i]["path"] == path]
        assert any(D[i]["t1"] > 0 and D[i]["t2"] > 0 for i in ch) and any(D[i]["t1"] == 0 and D[i]["t2"] == 0 for i in ch)
        assert any(D[i]["n1b"] == 1 and D[i]["t2"] > 0 for i in ch) and any(D[i]["n1b"] == 2 for i in ch)
        assert {R[i]["form"] for i in ch if D[i]["t2"] > 0} == {0, 1, 2}
        assert {R[i]["seq"][0] for i in ch} >= {"asc", "desc", "mod3"}
        assert any(len(sc.sequence(R[i])) % 64 for i in ch) and any(len(sc.sequence(R[i])) == 64 for i in ch)
    assert any(dict(R[i]["tune"]).get("seq_chain_grid") == 3 and D[i]["t2"] > 0 for i in D if D[i]["path"] == 5)
    assert D["chain333_zero_diag_flow"]["path"] == 3 and D["chain333_asc_f0_chain"]["path"] == 5       # the same matrix but for one diagonal
    # subsets of the rows, the back sweep of SGS, fewer workgroups than strips, the zero-start pass on every kind of path
    assert {R[i]["seq"][0] for i in D if D[i]["path"] == 3} >= {"asc", "desc", "sgs", "mod3", "red", "half", "scramble"}
    assert any(dict(R[i]["tune"]).get("seq_grid") == 1 and D[i]["strips"] > 2 for i in D)
    assert {D[i]["path"] for i in D if R[i]["zero_start"]} >= {1, 2, 3, 4, 5, 8}
    # rows that are left alone sit inside sweeps of the dataflow, level, whole-row and colour forms
    assert {D[i]["path"] for i in D if R[i]["mat"] == sc.RAGGED} >= {3, 4, 8}
    # sizes
    assert {len(sc.matrix(*r["mat"])[0]) - 1 for r in sc.RUNS} >= {1, 2, 63, 64, 65}
    assert {len(sc.sequence(r)) for r in sc.RUNS} >= {0, 1}
    assert max(len(sc.matrix(*r["mat"])[1]) for r in sc.RUNS) <= 2100000 and max(len(sc.matrix(*r["mat"])[0]) for r in sc.RUNS) <= 19601
    # every group of runs that must agree bit for bit sweeps the same rows of the same matrix with the same formula
    for g, members in sc.GROUPS.items():
        assert len({(R[i]["mat"], R[i]["seq"], R[i]["form"], R[i]["w"]) for i in members}) == 1, g
        assert len({(D[i]["L"], D[i]["rounds"], D[i]["spine"], D[i]["n1b"]) for i in members}) == 1, (g, "lanes, rounds, spine and the tier split are part of the arithmetic")


def test_the_ragged_matrix_has_what_it_exists_for():
    ia, ja, a = sc.matrix(*sc.RAGGED)
    n = len(ia) - 1
    lens = np.diff(ia)
    d, alone = sc.diagonals(ia, ja, a)
    row = np.repeat(np.arange(n), lens)
    assert n == 700 and sorted(np.flatnonzero(lens == 0)) == [10, 11, 400] and all(lens[i] >= n for i in (3, 250, 699))
    assert sorted(np.flatnonzero(alone)) == [10, 11, 20, 21, 400]
    assert np.sum((row == 20) & (ja == 20)) == 1 and np.sum((row == 21) & (ja == 21)) == 0 and np.sum((row == 100) & (ja == 100)) == 2 and d[100] == 55.0
    import scipy.sparse as sp
    P = sp.csr_matrix((np.ones(len(ja)), ja, ia), shape=(n, n))
    assert (P != P.T).nnz > 0                                   # an unsymmetric pattern: anti-dependencies


def _whole_range_runs():
    """One run per (matrix, direction, formula) the oracle has a sweep for.  Matrices with a row the device leaves alone are not among them:
    ItrSmootherCSR.c:327 updates such a row with the reciprocal of an EARLIER row's diagonal, the device (and the project's tests of it) with
    nothing."""
    seen = {}
    for r in sc.RUNS:
        if sc.diagonals(*sc.matrix(*r["mat"]))[1].any():
            continue
        if r["seq"][0] in ("asc", "desc") and r["form"] in (0, 2) and not r["zero_start"] and r["u0"] == "random" and not sc.tune_of(r)["gs_multicolor"]:
            seen.setdefault((r["mat"], r["seq"], r["form"]), r)
    return list(seen.values())


@pytest.mark.parametrize("run", _whole_range_runs(), ids=lambda r: r["id"])
def test_python_reference_is_the_oracles_sweep(run):
    """orc_smoother_gs / orc_smoother_sor (the CPU restatement of ItrSmootherCSR.c:251 / :932) over the whole range, either direction."""
    orc = oracle()
    ia, ja, a = sc.matrix(*run["mat"])
    n = len(ia) - 1
    A, keep = T.as_csr(ia, ja, a)
    b, u0 = sc.inputs(run)
    u = u0.copy()
    i1, i2, s = (0, n - 1, 1) if run["seq"][0] == "asc" else (n - 1, 0, -1)
    if run["form"] == 0:
        orc.orc_smoother_gs(T.dp(u), i1, i2, s, C.byref(A), T.dp(np.ascontiguousarray(b)), 1)
    else:
        orc.orc_smoother_sor(T.dp(u), i1, i2, s, C.byref(A), T.dp(np.ascontiguousarray(b)), 1, run["w"])
    mine = sc.reference_sweep(run)
    assert np.array_equal(mine.view(np.int64), u.view(np.int64)), (run["id"], np.abs(mine - u).max())


def test_row_equation_holds_for_the_reference_itself():
    """The a-priori bound the device results are held to, applied to the sequential reference: its rows satisfy their own equation inside
    the bound (a check of the checker: operands, orders and the counts of roundings)."""
    worst = 0.0
    for rid in ("ragged_asc_f0_flow", "ragged_desc_f2_flow", "ragged_mod3_f0_flow", "chain333_mod3_f2_chain", "L8_bw80_asc_spine0_flow", "mc_ragged_desc",
                "ragged_asc_f2_zero_skip", "arrow_L2", "upper_asc"):
        run = sc.BY_ID[rid]
        u = sc.reference_sweep(run)
        rows, exact, sabs, m = sc.row_equation(run, u)
        ratio = sum_bound_ratio(u[rows], exact, sabs, m)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (rid, ratio)
        # ... and a sweep with one wrong operand does not: an old value read for a new one
        seq = sc.effective_sequence(run)
        if len(seq) > 10 and run["path"] not in (1, 2) and rid != "arrow_L2":
            b, u0 = sc.inputs(run)
            bad = u.copy()
            bad[seq[len(seq) // 2]] += 1e-9 * (1.0 + abs(bad[seq[len(seq) // 2]]))
            rows, exact, sabs, m = sc.row_equation(run, bad)
            assert sum_bound_ratio(bad[rows], exact, sabs, m) > 100.0, rid
    print(f"worst error / bound of the reference: {worst:.3f}")
