"""Matrices and references shared by tests/test_rgroup_coding.py (CPU) and tests/test_gpu_rgroup.py (-m gpu): the row-group coding of
k_csr_rgroup (csrc/kernels5.hip.h; device_csr.hip.h: build_rgroup).  Built once per process and never changed by a test."""
import ctypes as C
import functools
import math

import numpy as np

import faspsolver_amd as fa
from faspsolver_amd import _types as T

R = 16                      # rows per group the special groups are laid out for
NOT_SQUARE, NOT_ROWLEN, NOT_SPAN, NOT_DUPLICATE, NOT_REUSE = 1, 2, 3, 4, 5
INFO = ("coded", "why", "R", "groups", "chunks", "ucols", "words", "hash_lo", "hash_hi", "min_row")


def selftest(ia, ja, val, ncol=None, rows=16, waves=4, min_reuse=0.0, x=None):
    """fasp_hip_rgroup_selftest -> (info dict, bytes, (ia, ja, val) decoded or None, y or None)"""
    ia = np.ascontiguousarray(ia, dtype=np.int32); ja = np.ascontiguousarray(ja, dtype=np.int32)
    val = np.ascontiguousarray(val, dtype=np.float64)
    A, keep = T.as_csr(ia, ja, val)
    if ncol is not None:
        A.col = ncol
    L = fa.lib()
    P = C.POINTER
    L.fasp_hip_rgroup_selftest.argtypes = [P(T.dCSRmat), C.c_int, C.c_int, C.c_double, P(C.c_int), P(C.c_double), P(C.c_int), P(C.c_int),
                                           P(C.c_double), P(C.c_double), P(C.c_double)]
    info = (C.c_int * 10)()
    nbytes = C.c_double(0)
    n, nnz = len(ia) - 1, len(ja)
    ia2 = np.zeros(n + 1, np.int32); ja2 = np.full(max(nnz, 1), -7, np.int32); v2 = np.full(max(nnz, 1), np.nan)
    y = np.full(max(n, 1), np.nan)
    if x is None:
        xp = yp = None
    else:
        x = np.ascontiguousarray(x, dtype=np.float64)
        xp, yp = T.dp(x), T.dp(y)
    ip = lambda q: q.ctypes.data_as(P(C.c_int))
    st = L.fasp_hip_rgroup_selftest(C.byref(A), rows, waves, min_reuse, info, C.byref(nbytes), ip(ia2), ip(ja2), T.dp(v2), xp, yp)
    assert st == 0
    d = dict(zip(INFO, list(info)))
    if not d["coded"]:
        return d, 0.0, None, None
    return d, nbytes.value, (ia2, ja2[:nnz], v2[:nnz]), (y[:n] if x is not None else None)


def sorted_rows(ia, ja, val):
    """Every row sorted by column (stable): the order the coded form gives back, and the order of the sorted device copy."""
    ia = np.asarray(ia, dtype=np.int64)
    rows = np.repeat(np.arange(len(ia) - 1), np.diff(ia))
    o = np.lexsort((ja, rows))
    return ja[o], val[o]


def row_sums_left_to_right(ia, ja, val, x, skip_diag=False):
    """The plain CSR row loop, every row summed left to right from 0.0 -- step k of all rows at once; -> (sums, sums of |a_ij x_j|).
    skip_diag: the entries j == i are left out (the reference's Jacobi sweep)."""
    ia = np.asarray(ia, dtype=np.int64)
    n = len(ia) - 1
    lens = np.diff(ia)
    acc = np.zeros(n); ab = np.zeros(n)
    for k in range(int(lens.max()) if n else 0):
        rows = np.nonzero(lens > k)[0]
        e = ia[rows] + k
        p = val[e] * x[ja[e]]
        if skip_diag:
            p = np.where(ja[e] == rows, 0.0, p)
        acc[rows] = acc[rows] + p
        ab[rows] = ab[rows] + np.abs(val[e] * x[ja[e]])
    return acc, ab


def exact_row_sums(ia, ja, val, x):
    return np.array([math.fsum((val[ia[i]:ia[i + 1]] * x[ja[ia[i]:ia[i + 1]]]).tolist()) for i in range(len(ia) - 1)])


def _assemble(rows_cols, rng):
    lens = np.array([len(c) for c in rows_cols], dtype=np.int64)
    ia = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ja = np.concatenate([np.asarray(c, dtype=np.int32) for c in rows_cols if len(c)]).astype(np.int32)
    val = rng.standard_normal(len(ja))
    return ia, ja, val


@functools.lru_cache(maxsize=None)
def banded(n=2407, lo=130, hi=300, width=420, seed=1, special=True):
    """Square banded-neighbourhood matrix: the rows of a group of 16 draw lo .. hi columns (the diagonal among them, sorted) from ONE window of
    `width` columns around the group -- consecutive rows read mostly the same columns.  n is no multiple of 16 or 8.  special: the groups
      10: a union of exactly 64 columns -- row 0 holds all of them, one column is in all 16 rows;
      11: a union of exactly 65 columns -- 64 below the group and the diagonal of its last row, which is that row's only entry: all of
          its entries lie in the last chunk, the column is present in one row only, and with two chunks two of four waves have nothing to do;
      12: a union of exactly 1 column, held by three rows; the other 13 rows are empty;
      20: an empty row between full ones;
    signed zeros among the values."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        g0 = i // R * R
        c0 = min(max(0, g0 - width // 2 + R // 2), n - width)
        L = int(rng.integers(lo, hi + 1))
        c = c0 + rng.choice(width, size=L, replace=False)
        if i not in c:
            c[0] = i
        rows.append(np.sort(c))
    if special:
        r0 = 10 * R
        S = np.concatenate([np.arange(r0, r0 + R), r0 + R + rng.choice(200, size=48, replace=False)])
        assert len(np.unique(S)) == 64
        for q in range(R):
            pick = S if q == 0 else np.unique(np.concatenate([[r0 + q, S[20]], rng.choice(S, size=int(rng.integers(5, 50)), replace=False)]))
            rows[r0 + q] = np.sort(pick)
        r0 = 11 * R
        S = r0 - 150 + rng.choice(100, size=64, replace=False)
        for q in range(R - 1):
            rows[r0 + q] = np.sort(S if q == 2 else rng.choice(S, size=int(rng.integers(3, 60)), replace=False))
        rows[r0 + R - 1] = np.array([r0 + R - 1])
        r0 = 12 * R
        for q in range(R):
            rows[r0 + q] = np.array([r0 + 3]) if q in (0, 3, 7) else np.array([], dtype=np.int64)
        rows[20 * R + 5] = np.array([], dtype=np.int64)
    ia, ja, val = _assemble(rows, rng)
    val[::97] = 0.0; val[5::101] = -0.0
    assert n % 16 and n % 8 and (not special or len(ja) >= 130 * n)
    return ia, ja, val


@functools.lru_cache(maxsize=None)
def wide(last_col=65535, per_row=128, seed=2):
    """Square operator of 65 552 rows whose first group spans the columns 0 .. last_col: every row of a group holds the same per_row
    offsets from the group (reuse 16); row 3 trades one entry for the column last_col.  65 535: the widest span a 16-bit offset holds."""
    n = 65536 + R
    rng = np.random.default_rng(seed)
    fixed = np.concatenate([[-200], np.arange(R)])       # the smallest offset; the diagonals of a group
    rest = np.setdiff1d(np.arange(-199, 201), fixed)
    D = np.sort(np.concatenate([fixed, rng.choice(rest, size=per_row - len(fixed), replace=False)]))
    base = np.clip(np.arange(n) // R * R, 200, n - 201)
    cols = base[:, None] + D[None, :]
    # the diagonal: the column nearest to it gives way
    i = np.arange(n)
    has = (cols == i[:, None]).any(axis=1)
    near = np.abs(cols - i[:, None]).argmin(axis=1)
    cols[i[~has], near[~has]] = i[~has]
    cols[3, -1] = last_col
    cols = np.sort(cols, axis=1)
    assert cols[:R].min() == 0 and np.all(np.diff(cols, axis=1) > 0)
    ia = (np.arange(n + 1) * cols.shape[1]).astype(np.int32)
    ja = cols.reshape(-1).astype(np.int32)
    val = rng.standard_normal(len(ja))
    return ia, ja, val


@functools.lru_cache(maxsize=None)
def scattered(n=2000, per_row=130, seed=3):
    """Rows of per_row columns drawn from the whole width: the rows of a group share next to nothing (reuse about 1)."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        c = rng.choice(n, size=per_row, replace=False)
        if i not in c:
            c[0] = i
        rows.append(np.sort(c))
    return _assemble(rows, rng)
