"""The block smoother entries without a GPU: the fixture tests/golden/bsr_smoothers.npz (the compiled reference's results) against the numpy
restatement of tests/_bsr_smoother_cases.py, bit for bit; the sweep plan of csrc/bsr_sweep_plan.cpp (fasp_hip_bsr_sweep_plan, host code)
against a restatement of its rule; the refusals that come before any device work; the new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _bsr_smoother_cases as S
from _libs import ROOT, T


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def golden():
    return np.load(S.GOLDEN)


def test_fixture_holds_every_case_and_its_inputs(golden):
    want = {c["id"] + "/out" for c in S.CASES}
    for m in S.MATRICES:
        base = m[len("scaled:"):] if m.startswith("scaled:") else m
        want |= {base + "/b", base + "/u0"}
        b, u0 = S.inputs(m)
        assert np.array_equal(bits(golden[base + "/b"]), bits(b)) and np.array_equal(bits(golden[base + "/u0"]), bits(u0)), m
    assert set(golden.files) == want
    assert os.path.getsize(S.GOLDEN) < 1 << 20


def test_cases_cover_what_they_are_for():
    entries = {c["entry"] for c in S.CASES}
    assert entries == set(S.ENTRIES)
    assert {c["w"] for c in S.CASES if S.ENTRIES[c["entry"]][0] == S.SOR} == {1.0, 1.3}
    assert {c["order"] for c in S.CASES} >= {"asc", "desc", "perm", "rb", "ident", "rev", "none"}
    assert {c["u0"] for c in S.CASES} == {"rand", "zero"}
    assert {S.matrix(c["mat"])[3] for c in S.CASES} == set(range(1, 8))
    for ROW in (1, 63, 64, 65, 129):
        assert any(c["mat"] == f"chain:{ROW}" for c in S.CASES)
    ia, ja, val, nb = S.matrix("odd:3")
    lens = np.diff(ia)
    rows = np.repeat(np.arange(len(ia) - 1), lens)
    assert (lens == 0).sum() == 2 and np.bincount(rows[ja == rows], minlength=len(lens)).max() == 2
    assert any(lens[i] == 1 and ja[ia[i]] == i for i in range(len(lens)))
    for name in S.MATRICES:   # the identity-diagonal entries run on matrices scaled by the inverse diagonal blocks
        if name.startswith("scaled:"):
            ia, ja, val, nb = S.matrix(name)
            rows = np.repeat(np.arange(len(ia) - 1), np.diff(ia))
            d = val.reshape(-1, nb, nb)[ja == rows]
            if "odd" not in name:   # (its row with two diagonal blocks is scaled by the inverse of the last one)
                assert np.max(np.abs(d - np.eye(nb))) < 1e-12, name


@pytest.mark.parametrize("cid", [c["id"] for c in S.CASES])
def test_restatement_equals_the_reference_bit_for_bit(golden, cid):
    case = S.BY_ID[cid]
    assert np.array_equal(bits(S.restated(case)), bits(golden[cid + "/out"]))


def test_identity_and_reversed_marks_equal_ascending_and_descending(golden):
    n = 0
    for c in S.CASES:
        twin = {"ident": "asc", "rev": "desc"}.get(c["order"])
        if twin:
            other = S._case(c["mat"], c["entry"], twin, c["w"], c["u0"])["id"]
            assert np.array_equal(bits(golden[c["id"] + "/out"]), bits(golden[other + "/out"])), c["id"]
            n += 1
    assert n >= 4
    for c in S.CASES:
        if c["order"] == "none":
            assert np.array_equal(bits(golden[c["id"] + "/out"]), bits(S.start_of(c)[1])), c["id"]


PLAN_CASES = [(m, o) for m in ("chain:1", "chain:63", "chain:64", "chain:65", "chain:129", "p7:6:3", "p7:10:3", "ragged:3", "odd:3", "odd:1")
              for o in ("asc", "desc", "perm")] + [("p7:6:3", "rb"), ("p7:10:3", "rb")]


def _seq(mat, order):
    return S.sequence(dict(mat=mat, entry="gs1", order=order))


@pytest.mark.parametrize("mat,order", PLAN_CASES)
def test_plan_follows_the_rule(fa, mat, order):
    ia, ja, val, nb = S.matrix(mat)
    ROW = len(ia) - 1
    seq = _seq(mat, order)
    o, mark = S.order_args(dict(mat=mat, order=order))
    P = fa.bsr_sweep_plan(ia, ja, nb, o, mark)
    level, entries = S.plan_rule(ia, ja, seq)
    assert np.array_equal(P["level"], level)                       # level = 1 + max over the entries that read new
    assert P["levels"] == int(level.max()) + 1 and len(P["lvl_chunk"]) == P["levels"] + 1
    rows = P["rows"]
    real = rows[rows >= 0]
    assert sorted(real.tolist()) == list(range(ROW))               # every row in exactly one chunk
    assert P["chunks"] == sum(-(-int((level == l).sum()) // 64) for l in range(P["levels"]))
    assert P["nreal"] == sum(len(e) for e in entries.values())
    seen_pad = False
    for c in range(P["chunks"]):
        lv = int(np.searchsorted(P["lvl_chunk"], c, side="right")) - 1
        slot_rows = rows[64 * c:64 * c + 64]
        kmax = max([len(entries[int(i)]) for i in slot_rows if i >= 0], default=0)
        nxt = P["cbase"][c + 1] if c + 1 < P["chunks"] else P["nent"]
        assert nxt - P["cbase"][c] == 64 * kmax
        live = slot_rows[slot_rows >= 0]
        assert len(live) > 0 and np.all(np.diff(live) > 0) and np.all(slot_rows[len(live):] == -1)   # padding at the chunk's end only
        for lane, i in enumerate(slot_rows):
            col = P["cols"][P["cbase"][c] + lane:nxt:64] if kmax else np.zeros(0, dtype=np.int32)
            if i < 0:
                seen_pad = True
                assert P["len"][64 * c + lane] == 0 and np.all(col == -1)                            # padded slots are marked
                continue
            assert level[i] == lv
            e = entries[int(i)]
            assert P["len"][64 * c + lane] == len(e)
            assert [(int(w) & 0x7fffffff, bool(w < 0)) for w in col[:len(e)]] == e                   # storage order, the bit = pos(j) < pos(i)
            assert np.all(col[len(e):] == -1)
    if ROW % 64:
        assert seen_pad
    if mat.startswith("chain") and order in ("asc", "desc"):
        assert P["levels"] == ROW
    if order == "rb":
        assert P["levels"] == 2
    if mat == "p7:6:3" and order in ("asc", "desc"):
        assert P["levels"] == 16
    if mat == "p7:10:3" and order in ("asc", "desc"):
        assert P["levels"] == 28


@pytest.mark.parametrize("mat", ["p7:6:3", "odd:3", "chain:65"])
def test_identity_and_reversed_marks_give_the_ascending_and_descending_plans(fa, mat):
    ia, ja, val, nb = S.matrix(mat)
    for order, mark_order in ((S.ASCEND, "ident"), (S.DESCEND, "rev")):
        a = fa.bsr_sweep_plan(ia, ja, nb, order, None)
        b = fa.bsr_sweep_plan(ia, ja, nb, 0, S.mark_of(mat, mark_order))
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), (mat, order, k)


def test_plan_refusals_and_nothing_to_sweep(fa):
    ia, ja, val, nb = S.matrix("p7:6:3")
    ROW = len(ia) - 1
    assert fa.bsr_sweep_plan(ia, ja, nb, 5, None) is None          # mark NULL, order neither ASCEND nor DESCEND
    bad = np.arange(ROW, dtype=np.int32); bad[3] = 4               # a row named twice
    for mark in (bad, np.r_[np.arange(ROW - 1), ROW].astype(np.int32), np.r_[-1, np.arange(1, ROW)].astype(np.int32)):
        with pytest.raises(ValueError) as e:
            fa.bsr_sweep_plan(ia, ja, nb, 0, mark)
        assert e.value.args[0] == T.ERROR_INPUT_PAR
    for bad_nb in (0, 8):
        with pytest.raises(ValueError) as e:
            fa.bsr_sweep_plan(ia, ja, bad_nb, S.ASCEND, None)
        assert e.value.args[0] == fa.ERROR_NUM_BLOCKS
    # the handle refuses the same before it looks for a device
    L = fa.lib()
    h = C.c_void_p()
    A, keep = T.as_bsr(ia, ja, np.zeros(len(ja) * 64), 8)
    assert L.fasp_hip_bsr_smoother_create(C.byref(h), C.byref(A), None, S.ASCEND, None) == fa.ERROR_NUM_BLOCKS and not h
    A, keep = T.as_bsr(ia, ja, val, nb)
    assert L.fasp_hip_bsr_smoother_create(C.byref(h), C.byref(A), None, 0, bad.ctypes.data_as(T.c_int_p)) == T.ERROR_INPUT_PAR and not h
    assert L.fasp_hip_tune(b"bsr_sweep_form", -1) == 0 and L.fasp_hip_tune(b"bsr_cycle_sweep", 0) == 0


def test_jacobi_setup_is_host_code_and_keeps_the_last_diagonal(fa):
    ia, ja, val, nb = S.matrix("odd:3")
    A, keep = T.as_bsr(ia, ja, val, nb)
    d = np.zeros((len(ia) - 1) * nb * nb)
    fa.lib().fasp_smoother_dbsr_jacobi_setup(C.byref(A), T.dp(d))
    k = ia[20] + 2                                                  # row 20: [20, 33, 20, 2] -- the second stored diagonal counts
    blk = val.reshape(-1, nb, nb)[k]
    assert np.allclose(d.reshape(-1, nb, nb)[20] @ blk, np.eye(nb), atol=1e-12)


def test_new_symbols_are_declared_and_exported(fa):
    hdr = open(os.path.join(ROOT, "include", "fasp_hip.h")).read()
    dev = open(os.path.join(ROOT, "include", "fasp_hip_dev.h")).read()
    L = fa.lib()
    for name in S.ENTRIES:
        sym = "fasp_smoother_dbsr_" + name
        assert re.search(r"\b%s\s*\(" % sym, hdr) and hasattr(L, sym) and sym in fa.EXPORTS, sym
    for sym in ("fasp_smoother_dbsr_jacobi_setup", "fasp_hip_bsr_smoother_create", "fasp_hip_bsr_smoother_apply", "fasp_hip_bsr_smoother_destroy"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and hasattr(L, sym) and sym in fa.EXPORTS, sym
    for sym in ("fasp_hip_bsr_smoother_info", "fasp_hip_bsr_sweep_plan", "fasp_hip_bsr_sweep_time"):
        assert re.search(r"\b%s\s*\(" % sym, dev) and hasattr(L, sym) and sym in fa.EXPORTS, sym
    assert hasattr(fa, "BSRSmoother")
