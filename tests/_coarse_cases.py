"""The selection table of the coarsest-level solvers, restated (numpy only, no GPU): which kernel coarse_spcg() (csrc/coarse_cg.hip.h) and
mgcycle_bsr() (csrc/bsr.hip.h) take for a matrix under the tune keys in force, and the matrices the cases are built from.
tests/test_coarse_plan.py holds the library's own plan (fasp_hip_coarse_plan, fasp_hip_bsr_coarse_plan) to it on the CPU,
tests/test_gpu_coarse_direct.py the kernels that ran (fasp_hip_coarse_kernel_info) on the device."""
import heapq

import numpy as np

FAMILY = {0: "none", 1: "k_spcg_dpp", 2: "k_spcg_reg", 3: "k_spcg_wave", 4: "k_spcg_small", 5: "k_spcg_fused",
          6: "k_spcg_persist", 7: "launch_csr + k_spcg_step"}


def max_it(m):
    return max(250, min(m * m, 1000))

# ---------------------------------------------------------------------------------------------------------------------
# matrices (numpy only; COO triples -> CSR that keeps duplicates and the order it is given)
# ---------------------------------------------------------------------------------------------------------------------
def to_csr(m, rows, cols, vals, rng=None):
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64); vals = np.asarray(vals, dtype=np.float64)
    if rng is not None:                      # columns in no order, the diagonal anywhere in the row
        p = rng.permutation(len(rows)); rows, cols, vals = rows[p], cols[p], vals[p]
    o = np.argsort(rows, kind="stable")
    rows, cols, vals = rows[o], cols[o], vals[o]
    ia = np.zeros(m + 1, dtype=np.int32)
    ia[1:] = np.cumsum(np.bincount(rows, minlength=m))
    return ia, cols.astype(np.int32), vals


def rows_of(ia):
    return np.repeat(np.arange(len(ia) - 1), np.diff(ia))


def laplacian(m, dim, shift=0.1):
    """The dim-D Laplacian stencil on the smallest grid with at least m nodes, cut to its first m rows and columns, plus
    shift * I: symmetric, strictly diagonally dominant."""
    n = 1
    while n ** dim < m:
        n += 1
    idx = np.arange(m)
    rows, cols, vals = [idx], [idx], [np.full(m, 2.0 * dim + shift)]
    stride = 1
    for _ in range(dim):
        coord = (idx // stride) % n
        for sgn in (-1, 1):
            nb = idx + sgn * stride
            ok = (coord + sgn >= 0) & (coord + sgn < n) & (nb >= 0) & (nb < m)
            rows.append(idx[ok]); cols.append(nb[ok]); vals.append(np.full(ok.sum(), -1.0))
        stride *= n
    return to_csr(m, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def sym_from_pairs(m, pi, pj, pv, rng, extra_diag=1.0, dup=True, zeros=True):
    """Symmetric matrix from off-diagonal pairs (i < j, value v; dyadic values, so every sum below is exact), diagonal = sum of
    |off-diagonals| + extra_diag; then unsorted columns, explicit stored zeros and one off-diagonal entry stored in two pieces."""
    rows = np.concatenate([pi, pj]); cols = np.concatenate([pj, pi]); vals = np.concatenate([pv, pv])
    d = np.bincount(rows, weights=np.abs(vals), minlength=m) + extra_diag
    if dup and len(pi):                     # a_ij stored as a_ij / 4 + 3 a_ij / 4 (exact), both directions
        k = int(rng.integers(len(pi)))
        for kk in (k, k + len(pi)):
            vals[kk] *= 0.25
        rows = np.concatenate([rows, [pi[k], pj[k]]]); cols = np.concatenate([cols, [pj[k], pi[k]]])
        vals = np.concatenate([vals, [3.0 * vals[k], 3.0 * vals[k]]])
    if zeros and m > 2:                     # stored zeros at places that hold nothing else (columns i + 2 .. of a few rows)
        zi = rng.choice(m, size=max(1, m // 7), replace=False)
        zj = (zi + 2 + rng.integers(0, 3, size=len(zi))) % m
        have = set(zip(rows.tolist(), cols.tolist()))
        keep = [q for q in range(len(zi)) if (int(zi[q]), int(zj[q])) not in have and zi[q] != zj[q]]
        rows = np.concatenate([rows, zi[keep]]); cols = np.concatenate([cols, zj[keep]]); vals = np.concatenate([vals, np.zeros(len(keep))])
    idx = np.arange(m)
    return to_csr(m, np.concatenate([rows, idx]), np.concatenate([cols, idx]), np.concatenate([vals, d]), rng)


def dyadic(rng, n):
    v = rng.integers(-64, 65, size=n).astype(np.float64)
    v[v == 0] = 17.0
    return v / 64.0


def random_sparse(m, rng):
    """(ii) random symmetric pattern, about six off-diagonals per row."""
    if m == 1:
        return to_csr(1, [0], [0], [1.5])
    npairs = max(1, 3 * m) if m > 3 else m - 1
    pi = rng.integers(0, m, size=npairs); pj = rng.integers(0, m, size=npairs)
    lo, hi = np.minimum(pi, pj), np.maximum(pi, pj)
    ok = lo != hi
    key = np.unique(lo[ok] * m + hi[ok])
    if len(key) == 0:
        key = np.array([1])                 # pair (0, 1)
    return sym_from_pairs(m, key // m, key % m, dyadic(rng, len(key)), rng)


def band_sparse(m, rng, s=37):
    """(ii) with at most 7 stored entries per row: off-diagonals at distance 1 and s, a stored zero, a split entry."""
    i1 = np.arange(m - 1); i2 = np.arange(max(m - s, 0))
    pi = np.concatenate([i1, i2]); pj = np.concatenate([i1 + 1, i2 + s])
    ia, ja, a = sym_from_pairs(m, pi, pj, dyadic(rng, len(pi)), rng, extra_diag=0.125)
    assert np.diff(ia).max() <= 7
    return ia, ja, a


def dense_spd(m, rng):
    """(iii) every entry stored: every register of the 16 x 16 blocks in use."""
    iu, ju = np.triu_indices(m, 1)
    return sym_from_pairs(m, iu, ju, dyadic(rng, len(iu)), rng, extra_diag=1.0, dup=m > 1, zeros=False)


def block_diag(m, rng, size=24, first=8):
    """(iii) dense diagonal blocks [0, 8), [8, 32), [32, 56), ..: they straddle the 16- and 64-row tile edges."""
    edges = [0] + list(range(first, m, size)) + [m]
    pi, pj = [], []
    for lo, hi in zip(edges[:-1], edges[1:]):
        iu, ju = np.triu_indices(hi - lo, 1)
        pi.append(iu + lo); pj.append(ju + lo)
    pi = np.concatenate(pi); pj = np.concatenate(pj)
    return sym_from_pairs(m, pi, pj, dyadic(rng, len(pi)), rng, extra_diag=0.5, zeros=False)


def scaled(m, d_hi=1e6, d_lo=1e-6):
    """(iv) D A D, D = diag(10^+-6) alternating in blocks of three rows, A the 2-D Laplacian: SPD with a condition number of
    about 1e24.  The reference's safe CG stagnates on it and the SPVGMRES net runs out of iterations (CPU half of section 2), so
    it is a verdict case, not a case of section 1."""
    ia, ja, a = laplacian(m, 2, shift=0.5)
    d = np.where((np.arange(m) // 3) % 2 == 0, d_hi, d_lo)
    return ia, ja, a * (d[rows_of(ia)] * d[ja])     # (d_i d_j first: the same double for (i, j) and (j, i))


def diagonal(m, values):
    idx = np.arange(m)
    return to_csr(m, idx, idx, np.resize(np.asarray(values, dtype=np.float64), m))


def wide_rows(m, rng, per_row=260):
    """m = 600 with about 250 entries per row: nnz > 131072, a small m on the big path."""
    half = per_row // 2
    i = np.repeat(np.arange(m), half); j = i + np.tile(np.arange(1, half + 1), m)
    ok = j < m
    return sym_from_pairs(m, i[ok], j[ok], dyadic(rng, int(ok.sum())) / 16.0, rng, extra_diag=0.25)


def arrowhead(m, lengths, rng):
    """SPD arrowhead: row / column q holds its first lengths[q] columns / rows, the rest is tridiagonal."""
    pairs = {}
    for i in range(m - 1):
        pairs[(i, i + 1)] = -0.5
    for q, ln in enumerate(lengths):
        for j in range(ln):
            if j != q:
                pairs[(min(q, j), max(q, j))] = -1.0 / 64.0
    key = np.array(sorted(pairs), dtype=np.int64)
    val = np.array([pairs[tuple(k)] for k in key])
    return sym_from_pairs(m, key[:, 0], key[:, 1], val, rng, extra_diag=0.25, dup=False, zeros=False)


ARROW = [(4200, (1900,)), (4200, (2900, 1900)), (4200, (3400, 2900, 1900)), (4200, (3900,)), (4200, (4200,)),
         (5500, (1900,)), (5500, (2900,)), (5500, (3400, 1900)), (5500, (3900, 2900, 1900)), (5500, (4200,))]


# The library's own defaults of the switches this module moves (struct Tuning, csrc/device_csr.hip.h; fasp_hip_tune has no getter,
# so "restore" means "set these"): test_switch_defaults_are_the_library_s reads them off the source and fails when they drift.
DEFAULTS = {"small_onewave": 4, "small_lds": 1, "spcg_fused": 1, "spcg_persist": 1, "spcg_batch": 16}


# ---------------------------------------------------------------------------------------------------------------------
# which kernel coarse_spcg() takes -- the table of the selection, restated
# ---------------------------------------------------------------------------------------------------------------------
def persist_ne(ia, num_cu):
    """build_persist_plan's arithmetic: ceil(len / 64) slots per row, longest first to the least loaded of (num_cu - 1) * 8 waves,
    at most 8 rows per wave; NE = the heaviest wave rounded up to 32 / 48 / 56 / 64; 0 = refused."""
    m = len(ia) - 1
    nw = (num_cu - 1) * 8
    slots = (np.diff(ia) + 63) // 64
    if m < 1 or m > 6144 or nw < 8 or (slots == 0).any():
        return 0
    heap = [(0, w) for w in range(nw)]
    cnt = [0] * nw
    for i in np.argsort(-slots, kind="stable"):
        load, w = heapq.heappop(heap)
        if cnt[w] >= 8:
            return 0
        cnt[w] += 1
        heapq.heappush(heap, (load + int(slots[i]), w))
    top = max(l for l, w in heap)
    return 32 if top <= 32 else 48 if top <= 48 else 56 if top <= 56 else 64 if top <= 64 else 0


def expected_kernel(ia, tune, num_cu, coded, small_coarse=True):
    m, nnz = len(ia) - 1, int(ia[-1])
    if small_coarse and m <= 4096 and nnz <= 131072:
        form = tune.get("small_onewave", 4)
        if form and m <= 128:
            if form >= 3:
                return (1, 4 if m <= 64 else 6 if m <= 96 else 8, 1 if form >= 4 else 0)
            if form == 2:
                return (2, 32 if m <= 64 else 48 if m <= 96 else 64, 0)
            return (3, 0, 0)
        lds_v, lds_m = 40 * m, 12 * nnz + 4 * (m + 1)
        if tune.get("small_lds", 1) and lds_v + lds_m <= 148 * 1024:
            return (4, 2, 0)
        if tune.get("small_lds", 1) and lds_v <= 148 * 1024:
            return (4, 1, 0)
        return (4, 0, 0)
    fused = tune.get("spcg_fused", 1) and m <= 8000 and not coded
    if fused and tune.get("spcg_persist", 1) and m * 24 <= 150 * 1024:
        ne = persist_ne(ia, num_cu)
        if ne:
            return (6, ne, 1 if 32 * m + 1024 <= 160 * 1024 else 0)
    inst = 4 if m <= 2048 else 10 if m <= 5120 else None
    if fused:
        return (5, inst or 16, 0)
    return (7, inst or 0, 0)


def kernel_name(k):
    return f"{FAMILY[k[0]]}<{k[1]},{k[2]}>"


GM_NE, GM_CB, SMALL_BLOCK, GM_RESTART = 16, 14, 512, 25


def expected_block_kernel(nb, ROW, NNZ, small_lds):
    n = ROW * nb
    if not (n <= 4096 and NNZ * nb * nb <= 131072):
        return (9, 0, 0)
    lds = 8 * (GM_RESTART + 2) * n
    cache2 = 0
    if nb == 3 and n <= 2 * SMALL_BLOCK and lds + max(n - SMALL_BLOCK, 0) * GM_CB * 28 <= 140 * 1024:
        cache2 = 1
        lds += max(n - SMALL_BLOCK, 0) * GM_CB * 28
    return (8, 1 if small_lds and lds <= 140 * 1024 else 0, cache2)
