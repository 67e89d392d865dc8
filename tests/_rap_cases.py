"""Inputs and expected results of the Galerkin-product tests (test_rap_entry.py, test_gpu_rap.py): the pinned random operands and a
literal restatement of fasp_blas_dcsr_rap's loop (BlaSpmvCSR.c:999) in plain Python floats.  Every case is generated and restated
once per session."""
import ctypes as C
import functools

import numpy as np

from _libs import T


def rnd(rng, m, n, maxlen, empty_every=0):          # distinct, unsorted columns; values uniform(-1, 1)
    ia, ja = [0], []
    for i in range(m):
        k = int(rng.integers(0, maxlen + 1))
        if empty_every and i % empty_every == 0: k = 0
        cols = rng.choice(n, size=min(k, n), replace=False)
        ja += list(cols); ia.append(len(ja))
    return np.array(ia, np.int32), np.array(ja, np.int32), rng.uniform(-1, 1, len(ja))


# seed: (nf, nc, lr, la, lp, ee), result nnz, longest row
SEEDED = {
    0: ((300, 97, 9, 12, 4, 7), 2612, 70),       # ragged sizes, empty rows in all three operands, R != P^T
    1: ((65, 64, 3, 5, 2, 0), 283, 13),          # exactly one wavefront of rows
    2: ((1, 1, 1, 1, 1, 0), 1, 1),               # one row
    3: ((513, 130, 40, 40, 20, 5), 13056, 130),  # rows that fill up (130 of 130 columns), nc = 2 * 64 + 2
    4: ((2000, 3, 1500, 30, 3, 0), 9, 3),        # very long R rows onto three columns: "seen again" thousands of times per row
}
CASES = [f"seed{s}" for s in SEEDED] + ["repeated", "wide"]
SIZES = {**{f"seed{s}": v[1:] for s, v in SEEDED.items()}, "repeated": (1861, 55), "wide": (181899, 2981)}


def _seeded(s, nf, nc, lr, la, lp, ee):
    rng = np.random.default_rng(s)
    R = rnd(rng, nc, nf, lr, ee)
    A = rnd(rng, nf, nf, la, ee and ee + 4)
    P = rnd(rng, nf, nc, lp, ee and ee + 2)
    return R, A, P


def _repeat_first(M, every):
    """every `every`-th row (that has an entry) gets its first column appended again with value 0.5 v + 0.25"""
    ia, ja, v = M
    nia, nja, nv = [0], [], []
    for i in range(len(ia) - 1):
        b, e = int(ia[i]), int(ia[i + 1])
        nja += list(ja[b:e]); nv += list(v[b:e])
        if i % every == 0 and e > b:
            nja.append(ja[b]); nv.append(0.5 * v[b] + 0.25)
        nia.append(len(nja))
    return np.array(nia, np.int32), np.array(nja, np.int32), np.array(nv, np.float64)


def _wide():
    nf, nc = 4096, 3000
    rng = np.random.default_rng(12)
    ia, ja, _ = rnd(rng, nc, nf, 2, 0)
    first, last = rng.choice(nf, 600, replace=False), rng.choice(nf, 600, replace=False)
    rows = [list(ja[ia[i]:ia[i + 1]]) for i in range(nc)]
    rows[0], rows[nc - 1] = list(first), list(last)
    nia = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    nja = np.array([c for r in rows for c in r], np.int32)
    R = (nia, nja, rng.uniform(-1, 1, len(nja)))
    A = rnd(rng, nf, nf, 30, 0)
    P = rnd(rng, nf, nc, 8, 0)
    return R, A, P


@functools.lru_cache(maxsize=None)
def operands(name):
    """-> ((R), (A), (P), nf, nc), each operand (ia, ja, val)"""
    if name == "repeated":
        R, A, P = _seeded(11, 200, 70, 8, 10, 4, 0)
        return _repeat_first(R, 4), _repeat_first(A, 3), _repeat_first(P, 3), 200, 70
    if name == "wide":
        return _wide() + (4096, 3000)
    s = int(name[4:])
    nf, nc = SEEDED[s][0][:2]
    return _seeded(s, *SEEDED[s][0]) + (nf, nc)


def restate(R, A, P):
    """fasp_blas_dcsr_rap (BlaSpmvCSR.c:999) literally: the diagonal slot first (0.0, only added to), the other columns in discovery
    order of j1 over R-row ic, j2 over A-row i1, j3 over P-row i2; (r*a)*p, first contribution assigned, later ones added.
    -> (ia, ja, val) as int32 / int32 / float64 arrays"""
    Ri, Rj, Rv = (x.tolist() for x in R)
    Ai, Aj, Av = (x.tolist() for x in A)
    Pi, Pj, Pv = (x.tolist() for x in P)
    ia, ja, val = [0], [], []
    for ic in range(len(Ri) - 1):
        where = {ic: len(ja)}
        ja.append(ic); val.append(0.0)
        for j1 in range(Ri[ic], Ri[ic + 1]):
            r, i1 = Rv[j1], Rj[j1]
            for j2 in range(Ai[i1], Ai[i1 + 1]):
                ra, i2 = r * Av[j2], Aj[j2]
                for j3 in range(Pi[i2], Pi[i2 + 1]):
                    rap, i3 = ra * Pv[j3], Pj[j3]
                    p = where.get(i3)
                    if p is None:
                        where[i3] = len(ja)
                        ja.append(i3); val.append(rap)
                    else:
                        val[p] += rap
        ia.append(len(ja))
    return np.array(ia, np.int32), np.array(ja, np.int32), np.array(val, np.float64)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restated result of a case as bytes (IA, JA, val)"""
    R, A, P, _nf, _nc = operands(name)
    ia, ja, val = restate(R, A, P)
    assert (len(ja), int(np.diff(ia).max())) == SIZES[name], name
    return ia.tobytes(), ja.tobytes(), val.tobytes()


def as_mats(R, A, P, nf, nc):
    """the three dCSRmat structs (and what keeps their arrays alive)"""
    r, k1 = T.as_csr(*R, ncol=nf)
    a, k2 = T.as_csr(*A, ncol=nf)
    p, k3 = T.as_csr(*P, ncol=nc)
    return r, a, p, (k1, k2, k3)


def take(M, free):
    """(IA, JA, val) bytes of a product the library allocated, which is then released with `free`"""
    ia = np.ctypeslib.as_array(M.IA, (M.row + 1,)).tobytes()
    ja = np.ctypeslib.as_array(M.JA, (max(M.nnz, 1),))[:M.nnz].tobytes()
    val = np.ctypeslib.as_array(M.val, (max(M.nnz, 1),))[:M.nnz].tobytes()
    free(C.byref(M))
    return ia, ja, val
