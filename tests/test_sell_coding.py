"""The value-indexed sliced-ELL coding of k_csr_sell (csrc/kernels4.hip.h; device_csr.hip.h: build_sell) checked on the CPU through
fasp_hip_sell_selftest: the coded form decodes back to IA / JA / val exactly (values bit for bit), a host SpMV that walks the coded form
the way the kernel does (slice by slice, every row left to right) equals the plain CSR row loop bit for bit, and operators that break a
qualification rule are reported as not coded.  The arithmetic on the device is tests/test_gpu_sell.py (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

import faspsolver_amd as fa
from faspsolver_amd import _types as T

from _libs import default_params, poisson7pt

NOT_RANGE, NOT_ROWLEN, NOT_PADDING, NOT_VALUES, NOT_BITS = 1, 2, 3, 4, 5


def _sell(ia, ja, val, ncol=None, cap=0, x=None):
    """-> (info dict, bytes, (ia, ja, val) decoded or None, y or None)"""
    ia = np.ascontiguousarray(ia, dtype=np.int32); ja = np.ascontiguousarray(ja, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float64)
    A, keep = T.as_csr(ia, ja, val)
    if ncol is not None:
        A.col = ncol
    L = fa.lib()
    P = C.POINTER
    L.fasp_hip_sell_selftest.argtypes = [P(T.dCSRmat), C.c_int, P(C.c_int), P(C.c_double), P(C.c_int), P(C.c_int), P(C.c_double),
                                         P(C.c_double), P(C.c_double)]
    info = (C.c_int * 8)()
    nbytes = C.c_double(0)
    n, nnz = len(ia) - 1, len(ja)
    ia2 = np.zeros(n + 1, np.int32); ja2 = np.full(max(nnz, 1), -7, np.int32); v2 = np.full(max(nnz, 1), np.nan)
    y = np.full(max(n, 1), np.nan)
    if x is False:                          # (no product: operators too wide for a test vector)
        xp = yp = None
    else:
        x = np.random.default_rng(5).standard_normal(A.col) if x is None else np.ascontiguousarray(x, dtype=np.float64)
        xp, yp = T.dp(x), T.dp(y)
    ip = lambda q: q.ctypes.data_as(P(C.c_int))
    st = L.fasp_hip_sell_selftest(C.byref(A), cap, info, C.byref(nbytes), ip(ia2), ip(ja2), T.dp(v2), xp, yp)
    assert st == 0
    keys = ("coded", "why", "nv", "vbits", "obits", "nslice", "slotrows", "maxv")
    d = dict(zip(keys, list(info)))
    if not d["coded"]:
        return d, 0.0, None, None
    return d, nbytes.value, (ia2, ja2[:nnz], v2[:nnz]), y[:n]


def _row_loop(ia, ja, val, x):
    """The plain CSR row loop, every row summed left to right from 0.0 (BlaSpmvCSR.c:242) -- step k of all rows at once."""
    ia = np.asarray(ia, dtype=np.int64)
    n = len(ia) - 1
    lens = np.diff(ia)
    acc = np.zeros(n)
    for k in range(int(lens.max()) if n else 0):
        rows = np.nonzero(lens > k)[0]
        e = ia[rows] + k
        acc[rows] = acc[rows] + val[e] * x[ja[e]]
    return acc


def _check_roundtrip(ia, ja, val, d, dec, y, x):
    ia2, ja2, v2 = dec
    assert np.array_equal(ia2, ia) and np.array_equal(ja2, ja)
    assert np.array_equal(v2.view(np.uint64), np.asarray(val, dtype=np.float64).view(np.uint64))   # bit for bit (-0.0, NaN payloads)
    assert np.array_equal(y.view(np.uint64), _row_loop(ia, ja, val, x).view(np.uint64))
    assert d["vbits"] + d["obits"] <= 32 and d["nv"] <= d["maxv"] and d["nslice"] == (len(ia) - 1 + 63) // 64


def _level(n, level):
    ia, ja, a, f, ue = poisson7pt(n)
    itp, amgp = default_params()
    amgp.smoother = T.SMOOTHER_JACOBI; amgp.relaxation = 0.6667
    H = fa.AMG(ia, ja, a, amgp, host_only=True)
    nr, nc, lia, lja, lval = H.matrix(level, 0)
    H.close()
    return nr, nc, lia, lja, lval


@pytest.mark.parametrize("n", [24, 48])
def test_level2_of_p7_round_trip(n):
    nr, nc, ia, ja, val = _level(n, 2)
    x = np.random.default_rng(n).standard_normal(nc)
    d, nb, dec, y = _sell(ia, ja, val, x=x)
    if not d["coded"]:
        # small grids are mostly boundary: ragged slices.  The rule that refused must be the padding cap; the form itself is
        # exercised with the cap lifted
        assert d["why"] == NOT_PADDING, d
        d, nb, dec, y = _sell(ia, ja, val, cap=1000, x=x)
    assert d["coded"], d
    _check_roundtrip(ia, ja, val, d, dec, y, x)


def _random_few_values(nrow, ncol, lens, nvals, seed, band=4000):
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    ia = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    table = rng.standard_normal(nvals)
    ja = np.zeros(ia[-1], np.int32)
    for r in range(nrow):
        lo = max(0, min(ncol - band, r * ncol // max(nrow, 1) - band // 2))
        ja[ia[r]:ia[r + 1]] = rng.choice(np.arange(lo, min(ncol, lo + band)), size=lens[r], replace=False)   # unsorted: storage order matters
    val = table[rng.integers(0, nvals, ia[-1])]
    return ia, ja, val


def test_random_matrix_with_few_values():
    rng = np.random.default_rng(1)
    nrow = 5000
    lens = rng.integers(20, 27, nrow)
    ia, ja, val = _random_few_values(nrow, 6000, lens, 300, 2)
    d, nb, dec, y = _sell(ia, ja, val, ncol=6000)
    assert d["coded"] and d["nv"] <= 300 and d["vbits"] == 9, d
    x = np.random.default_rng(5).standard_normal(6000)
    _check_roundtrip(ia, ja, val, d, dec, y, x)
    # deterministic
    d2, nb2, dec2, y2 = _sell(ia, ja, val, ncol=6000)
    assert d2 == d and nb2 == nb


def test_corner_cases():
    rng = np.random.default_rng(3)
    nrow = 64 * 9 + 17                      # not a multiple of 64
    lens = rng.integers(12, 15, nrow)
    lens[5] = 0; lens[64:128] = 12          # an empty row; a slice whose rows all have equal length
    lens[200] = 1; lens[nrow - 1] = 0; lens[300:303] = 0
    ia, ja, val = _random_few_values(nrow, 700, lens, 40, 4, band=600)
    val[::7] = 0.0; val[3::11] = -0.0       # signed zeros are distinct values
    val[ia[200]] = -0.0
    assert ia[-1] >= 4096
    x = np.random.default_rng(6).standard_normal(700)
    x[::13] = np.inf                        # padding must be skipped, not multiplied: 0 * inf would poison the sum
    d, nb, dec, y = _sell(ia, ja, val, ncol=700, x=x)
    assert d["coded"], d
    _check_roundtrip(ia, ja, val, d, dec, y, x)
    zeros = np.unique(val[val == 0.0].view(np.uint64))
    assert len(zeros) == 2                  # +0.0 and -0.0 both present, and both came back (checked bitwise above)


def test_rules_refuse():
    rng = np.random.default_rng(8)
    nrow = 4000
    lens = np.full(nrow, 12)
    # too many distinct values
    ia, ja, val = _random_few_values(nrow, 5000, lens, 20, 9)
    d, *_ = _sell(ia, ja, rng.standard_normal(len(val)), ncol=5000)
    assert not d["coded"] and d["why"] == NOT_VALUES
    d, *_ = _sell(ia, ja, val, ncol=5000)
    assert d["coded"]
    # exactly the largest table qualifies, one more value does not
    maxv = d["maxv"]
    assert maxv >= 8245                     # level 2 of P7(256) has 8 245 distinct values
    v = np.arange(len(val)) % maxv + 1.0
    assert _sell(ia, ja, v, ncol=5000)[0]["coded"]
    v = np.arange(len(val)) % (maxv + 1) + 1.0
    d, *_ = _sell(ia, ja, v, ncol=5000)
    assert not d["coded"] and d["why"] == NOT_VALUES
    # offsets too wide for what the value index leaves: 2^27 columns of span, 300 values
    ncol = 1 << 27
    ja_w = ja.copy()
    ja_w[ia[:-1]] = 0; ja_w[ia[:-1] + 1] = ncol - 1
    v = np.arange(len(val)) % 300 + 1.0
    d, *_ = _sell(ia, ja_w, v, ncol=ncol, x=False)
    assert not d["coded"] and d["why"] == NOT_BITS, d
    # padding over the cap: one long row per slice
    lens2 = np.full(nrow, 10); lens2[::64] = 40
    ia2, ja2, val2 = _random_few_values(nrow, 5000, lens2, 20, 10)
    d, *_ = _sell(ia2, ja2, val2, ncol=5000)
    assert not d["coded"] and d["why"] == NOT_PADDING
    assert _sell(ia2, ja2, val2, ncol=5000, cap=400)[0]["coded"]
    # a row beyond 255 entries
    lens3 = np.full(nrow, 12); lens3[77] = 300
    ia3, ja3, val3 = _random_few_values(nrow, 5000, lens3, 20, 11)
    d, *_ = _sell(ia3, ja3, val3, ncol=5000)
    assert not d["coded"] and d["why"] == NOT_ROWLEN
    # short rows (k_csr_lstream's range) and tiny operators stay what they are
    ia4, ja4, val4 = _random_few_values(nrow, 5000, np.full(nrow, 5), 20, 12)
    assert _sell(ia4, ja4, val4, ncol=5000)[0]["why"] == NOT_RANGE
    ia5, ja5, val5 = _random_few_values(100, 5000, np.full(100, 12), 20, 13)
    assert _sell(ia5, ja5, val5, ncol=5000)[0]["why"] == NOT_RANGE


def test_level2_of_p7_128_qualifies_at_4_3_bytes_per_nonzero():
    """The level the coding was designed for (level 2 of the benchmark's hierarchy, here at 128^3): 1.037 slots per nonzero x 4 bytes
    + a length per row + a base and a pointer per slice + the table."""
    nr, nc, ia, ja, val = _level(128, 2)
    nnz = len(ja)
    x = np.random.default_rng(7).standard_normal(nc)
    d, nb, dec, y = _sell(ia, ja, val, x=x)
    print(f"level 2 of P7(128): {nr} rows, {nnz} nnz, {d}, {nb / nnz:.4f} bytes per nonzero")
    assert d["coded"], d
    assert nb / nnz <= 4.3
    _check_roundtrip(ia, ja, val, d, dec, y, x)
