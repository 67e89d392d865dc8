"""The row-group coding of k_csr_rgroup (csrc/kernels5.hip.h; device_csr.hip.h: build_rgroup) checked on the CPU through
fasp_hip_rgroup_selftest: the coded form decodes back to IA / JA / val (values bit for bit; every row comes back sorted by column, the
order of the sorted device copy), a host walk in the kernel's order agrees with the left-to-right row sums to 1e-13 of the row's
absolute sum, two builds are identical, every refusal rule fires on a matrix made for it, and the form reads fewer bytes than the 10 per
entry of the 16-bit-column copy.  The arithmetic on the device is tests/test_gpu_rgroup.py (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

import faspsolver_amd as fa
from faspsolver_amd import _types as T

import _rgroup_cases as RG
from _libs import default_params, poisson7pt


def _check(ia, ja, val, rows, waves, min_reuse=0.0):
    n = len(ia) - 1
    x = np.random.default_rng(5).standard_normal(n)
    d, nb, dec, y = RG.selftest(ia, ja, val, rows=rows, waves=waves, min_reuse=min_reuse, x=x)
    assert d["coded"], d
    ia2, ja2, v2 = dec
    js, vs = RG.sorted_rows(ia, ja, val)
    assert np.array_equal(ia2, ia) and np.array_equal(ja2, js)
    assert np.array_equal(v2.view(np.uint64), vs.view(np.uint64))          # bit for bit (-0.0 stays -0.0)
    ref, rowabs = RG.row_sums_left_to_right(ia, ja, val, x)
    err = np.abs(y - ref)
    print(f"R {rows} W {waves}: {d}, {nb / len(ja):.3f} bytes per entry, max err / rowabs {np.max(err / np.maximum(rowabs, 1e-300)):.2e}")
    assert np.all(err <= 1e-13 * rowabs)
    assert np.all(y[np.diff(ia) == 0] == 0.0)
    assert d["R"] == rows and d["groups"] == (n + rows - 1) // rows
    assert nb == 8.0 * len(ja) + 4.0 * d["words"] + 16.0 * (d["groups"] + 1)
    assert d["words"] == d["ucols"] + d["chunks"] + d["groups"]
    return d, nb, y


@pytest.mark.parametrize("rows,waves", [(16, 4), (16, 8), (8, 4), (8, 8), (16, 2), (8, 2)])
def test_banded_round_trip_and_walk(rows, waves):
    ia, ja, val = RG.banded()
    d, nb, y = _check(ia, ja, val, rows, waves)
    assert nb < 10.0 * len(ja)
    if rows == 16:
        # the special groups are what they were built to be: unions of 64, 65 and 1 columns -> 1, 2 and 1 chunks
        lens = np.diff(ia)
        for g, nu in ((10, 64), (11, 65), (12, 1)):
            assert len(np.unique(ja[ia[16 * g]:ia[16 * g + 16]])) == nu
        assert lens[16 * 11 + 15] == 1 and lens[16 * 12 + 1] == 0 and lens[16 * 20 + 5] == 0
    # two builds are identical
    d2, nb2, dec2, _ = RG.selftest(ia, ja, val, rows=rows, waves=waves)
    assert d2 == d and nb2 == nb


def test_numpy_reference_alone_meets_the_bar():
    """The left-to-right sums the device tests compare with lie within 1e-13 of the row's absolute sum of the exactly rounded sums."""
    for ia, ja, val in (RG.banded(), RG.scattered()):
        x = np.random.default_rng(3).standard_normal(len(ia) - 1)
        ref, rowabs = RG.row_sums_left_to_right(ia, ja, val, x)
        assert np.all(np.abs(ref - RG.exact_row_sums(ia, ja, val, x)) <= 1e-13 * rowabs)


def test_unsorted_rows_come_back_sorted():
    ia, ja, val = RG.banded()
    rng = np.random.default_rng(9)
    ja = ja.copy(); val = val.copy()
    for i in range(0, len(ia) - 1, 3):
        p = rng.permutation(ia[i + 1] - ia[i])
        ja[ia[i]:ia[i + 1]] = ja[ia[i]:ia[i + 1]][p]; val[ia[i]:ia[i + 1]] = val[ia[i]:ia[i + 1]][p]
    _check(ia, ja, val, 16, 4)


def test_widest_span_is_coded_and_one_more_is_refused():
    ia, ja, val = RG.wide(65535)
    assert ja[ia[0]:ia[16]].max() - ja[ia[0]:ia[16]].min() == 65535
    d, nb, y = _check(ia, ja, val, 16, 4)
    ia, ja, val = RG.wide(65536)
    d, *_ = RG.selftest(ia, ja, val)
    assert not d["coded"] and d["why"] == RG.NOT_SPAN, d


def test_rules_refuse():
    ia, ja, val = RG.banded()
    n = len(ia) - 1
    # a rectangular matrix
    d, *_ = RG.selftest(ia, ja, val, ncol=n + 1)
    assert not d["coded"] and d["why"] == RG.NOT_SQUARE
    # a duplicated column
    jd = ja.copy(); jd[ia[500] + 1] = jd[ia[500]]
    d, *_ = RG.selftest(ia, jd, val)
    assert not d["coded"] and d["why"] == RG.NOT_DUPLICATE
    # mean row of 127 (and exactly 128 is served)
    for per_row, ok in ((127, False), (128, True)):
        ib, jb, vb = RG.banded(n=1000 + 3, lo=per_row, hi=per_row, seed=4, special=False)
        assert len(jb) == per_row * (len(ib) - 1)
        d, *_ = RG.selftest(ib, jb, vb)
        assert d["min_row"] == 128 and (d["coded"] == 1) == ok and (ok or d["why"] == RG.NOT_ROWLEN), d
    # reuse below the bound; the same matrix is coded when the bound is lowered
    ic, jc, vc = RG.scattered()
    d, *_ = RG.selftest(ic, jc, vc)
    assert not d["coded"] and d["why"] == RG.NOT_REUSE
    _check(ic, jc, vc, 16, 4, min_reuse=1.0)
    # ... the bound is on entries / union columns
    d, *_ = RG.selftest(ia, ja, val)
    reuse = len(ja) / d["ucols"]
    assert reuse > 3.0
    assert RG.selftest(ia, ja, val, min_reuse=reuse * 0.999)[0]["coded"] and RG.selftest(ia, ja, val, min_reuse=reuse * 1.001)[0]["why"] == RG.NOT_REUSE
    # bad arguments
    A, keep = T.as_csr(ia, ja, val)
    info = (C.c_int * 10)()
    L = fa.lib()
    assert L.fasp_hip_rgroup_selftest(C.byref(A), 12, 4, 0.0, info, None, None, None, None, None, None) < 0
    assert L.fasp_hip_rgroup_selftest(C.byref(A), 16, 5, 0.0, info, None, None, None, None, None, None) < 0


def _brick_level(n, level):
    """Level `level` of the P7(n) hierarchy in the brick numbering an upload gives it (fasp_hip_cluster_order, chunk 262 144)."""
    ia, ja, a, f, ue = poisson7pt(n)
    itp, amgp = default_params()
    amgp.smoother = T.SMOOTHER_JACOBI; amgp.relaxation = 0.6667
    H = fa.AMG(ia, ja, a, amgp, host_only=True)
    if level >= H.num_levels - 1:
        H.close()
        return None
    nr, nc, lia, lja, lval = H.matrix(level, 0)
    lia = np.array(lia, dtype=np.int32); lja = np.array(lja, dtype=np.int32); lval = np.array(lval, dtype=np.float64)
    H.close()
    A, keep = T.as_csr(lia, lja, lval)
    L = fa.lib()
    P = C.POINTER
    order = np.zeros(nr, np.int32)
    L.fasp_hip_cluster_order.argtypes = [P(T.dCSRmat), C.c_int, P(C.c_int)]
    assert L.fasp_hip_cluster_order(C.byref(A), 262144, order.ctypes.data_as(P(C.c_int))) == 0
    inv = np.zeros(nr, np.int32); inv[order] = np.arange(nr, dtype=np.int32)
    ia2 = np.zeros(nr + 1, np.int32); ja2 = np.zeros(len(lja), np.int32); v2 = np.zeros(len(lja))
    L.fasp_hip_permute_csr.argtypes = [P(T.dCSRmat), P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_double)]
    ip = lambda q: q.ctypes.data_as(P(C.c_int))
    assert L.fasp_hip_permute_csr(C.byref(A), ip(order), ip(inv), ip(ia2), ip(ja2), T.dp(v2)) == 0
    return ia2, ja2, v2


def test_bytes_per_entry_below_the_16_bit_column_copy():
    """Level 5 of P7(64) in its brick numbering when it qualifies (long enough rows, reuse of 3); else the banded matrix."""
    lvl = _brick_level(64, 5)
    what = "level 5 of P7(64)"
    if lvl is not None:
        d, nb, dec, _ = RG.selftest(*lvl)
        print(f"{what}: {len(lvl[0]) - 1} rows, {len(lvl[1])} entries, {d}")
    if lvl is None or not d["coded"]:
        lvl = RG.banded()
        what = "banded matrix"
        d, nb, dec, _ = RG.selftest(*lvl)
    assert d["coded"], d
    print(f"{what}: {nb / len(lvl[1]):.3f} bytes per entry, reuse {len(lvl[1]) / d['ucols']:.2f}")
    assert nb < 10.0 * len(lvl[1])
    if what != "banded matrix":
        _check(*lvl, 16, 4)
