"""Hand-built incomplete LU factors at the edges of the device schedule of csrc/ilu.hip.h, literal restatements of the solves that
apply them (PreCSR.c:198 / :263 / :317, PreBSR.c:347 with BlaSmallMat.c's products) in plain Python floats, and the schedule rule of
ilu_build_tri restated.  No GPU code, and the library under test is not loaded: test_ilu_cases.py proves the restatements against the
compiled reference on the CPU, test_gpu_ilu_kernels.py holds the kernels to them bit for bit.

A factor is in the reference's MSR layout: ijlu[0..n] row pointers, ijlu[p] / luval[p nb^2 ..] the entries in storage order,
luval[i nb^2 ..], i < n, the inverse pivot (block, row-major).  L reads a row's entries in storage order up to the first column >= i,
U reads them from the end back to the first column <= i; what lies between ("stranded") is read by neither.

Cases (`name`, scalar unless nb is given; B: also built with nb x nb blocks, same pattern):
  one           n = 1
  diag:130      no entries: one level of 130 rows per triangle, 3 chunks, the last with 2 live lanes
  chain:n       L row i reads i - 1, U row i reads i + 1: n levels of one row (B: chain:65)
  bands:m       n = 3 m; L rows of band k read 1..5 rows of band k - 1, U rows 1..5 of band k + 1: 3 levels of m rows (B: bands:65)
  ragged        n = 400 (B: n = 150, long row 100): eight strata of rows, L parts of 0..40 entries from lower strata, U parts from
                higher ones, about every 7th row empty in L, every 5th in U, some in both, rows that read level-0 rows only; row
                n - 1 holds 300 L entries, row 0 holds 300 U entries, each in a chunk with short rows and padding
  unsorted      n = 70: shuffled parts; a third of the rows carry a stranded run, with explicit col == i entries, whose columns
                would raise the row's level if a schedule counted them
  wide          n = 19200: 9600 level-0 rows, 9600 rows reading one of them each, mirrored for U: 150 chunks per level
  cap           n = 262400: the same with 131200 rows per level: 4100 chunks per triangle, more than 4 x 1024"""
import functools

import numpy as np

from _libs import T

CHUNK = 64
FLOW_MIN_LEVELS = 24      # ILU_FLOW_MIN_LEVELS of csrc/ilu.hip.h: the single launch beyond this many levels
FLOW_MAX_GRID = 1024      # workgroups of the single launch at the most, four wavefronts each

CHAINS = (2, 24, 25, 26, 63, 64, 65, 129)
BANDS = (63, 64, 65, 128, 129)
SCALAR_CASES = (["one", "diag:130"] + [f"chain:{n}" for n in CHAINS] + [f"bands:{m}" for m in BANDS] +
                ["ragged", "unsorted", "wide", "cap"])
BLOCK_CASES = ["chain:65", "bands:65", "ragged"]


class Factor:
    """An MSR factor from per-row lists.  rows[i]: [(column, value or nb x nb block), ..] in storage order; pivots[i]: the inverse
    pivot (block).  .ijlu (int32), .luval (float64, flat), .n, .nb, .nzlu; ilu_data() wraps copies in a caller-built ILU_data."""

    def __init__(self, rows, pivots, nb=1):
        n, nb2 = len(rows), nb * nb
        lens = np.array([len(r) for r in rows], dtype=np.int64)
        nnz = int(lens.sum())
        self.n, self.nb, self.nzlu = n, nb, n + 1 + nnz
        self.ijlu = np.empty(self.nzlu, dtype=np.int32)
        self.ijlu[:n + 1] = n + 1 + np.concatenate(([0], np.cumsum(lens)))
        lu = np.zeros((self.nzlu, nb2))
        lu[:n] = np.asarray(pivots, dtype=np.float64).reshape(n, nb2)
        if nnz:
            self.ijlu[n + 1:] = [c for r in rows for c, _ in r]
            lu[n + 1:] = np.asarray([v for r in rows for _, v in r], dtype=np.float64).reshape(nnz, nb2)
        self.luval = lu.reshape(-1)
        self.ijlu.setflags(write=False)
        self.luval.setflags(write=False)

    def ilu_data(self):
        """-> (T.ILU_data over fresh copies of the arrays, the arrays that keep it alive: ijlu, luval, work).  The work space
        holds 5 n nb + nb doubles: what the reference's block solve (zz, zr, mult) and its smoother ask for."""
        ijlu, luval = self.ijlu.copy(), self.luval.copy()
        work = np.zeros(5 * self.n * self.nb + self.nb)
        d = T.ILU_data()
        d.type, d.row, d.col, d.nzlu, d.nb, d.nwork = T.ILUk, self.n, self.n, self.nzlu, self.nb, len(work)
        d.ijlu, d.luval, d.work = ijlu.ctypes.data_as(T.c_int_p), T.dp(luval), T.dp(work)
        return d, (ijlu, luval, work)

    def row_cols(self, i):
        return self.ijlu[self.ijlu[i]:self.ijlu[i + 1]]


# --- patterns: per row, the columns in storage order ---------------------------------------------
def _pat_chain(n):
    return [([i - 1] if i > 0 else []) + ([i + 1] if i < n - 1 else []) for i in range(n)]


def _pat_bands(m, seed):
    rng = np.random.default_rng(seed)
    pat = []
    for i in range(3 * m):
        k = i // m
        lo = [] if k == 0 else ((k - 1) * m + rng.choice(m, size=int(rng.integers(1, 6)), replace=False)).tolist()
        up = [] if k == 2 else ((k + 1) * m + rng.choice(m, size=int(rng.integers(1, 6)), replace=False)).tolist()
        pat.append(lo + up)
    return pat


def _pat_ragged(n, long, seed):
    rng = np.random.default_rng(seed)
    stratum = np.arange(n) * 8 // n
    l_empty = [i for i in range(n) if i % 7 == 3]
    u_empty = [i for i in range(n) if i % 5 == 2]
    pat = []
    for i in range(n):
        below = np.flatnonzero(stratum < stratum[i])            # rows L may read
        above = np.flatnonzero(stratum > stratum[i])            # rows U may read
        lo = rng.choice(below, size=min(int(rng.integers(0, 41)), len(below)), replace=False).tolist()
        up = rng.choice(above, size=min(int(rng.integers(0, 41)), len(above)), replace=False).tolist()
        if i % 11 == 6:   # level-0 rows only: this row skips the levels between
            lo = [j for j in l_empty if j < i and stratum[j] < stratum[i]][:3]
        if i % 11 == 8:
            up = [j for j in u_empty if j > i and stratum[j] > stratum[i]][-3:]
        if i % 7 == 3:
            lo = []
        if i % 5 == 2:
            up = []
        if i == n - 1:
            lo = rng.choice(below, size=long, replace=False).tolist()
        if i == 0:
            up = rng.choice(above, size=long, replace=False).tolist()
        pat.append(lo + up)
    assert any(i % 7 == 3 and i % 5 == 2 for i in range(n))     # rows empty in both triangles
    return pat


def _levels(pat, upper, count_all=False):
    """level of every row of a pattern (the rule of schedule() on lists; count_all: every column on the triangle's side counts)"""
    n = len(pat)
    level = [0] * n
    for i in (range(n - 1, -1, -1) if upper else range(n)):
        lv = 0
        for c in (reversed(pat[i]) if upper else pat[i]):
            if (c > i) if upper else (c < i):
                lv = max(lv, level[c] + 1)
            elif not count_all:
                break
        level[i] = lv
    return level


def _pat_unsorted(n, seed):
    rng = np.random.default_rng(seed)
    lo, up = [], []
    for i in range(n):
        lo.append(rng.permutation(i)[:int(rng.integers(0, 7))].tolist())
        up.append((i + 1 + rng.permutation(n - 1 - i)[:int(rng.integers(0, 7))]).tolist())
    marked = [i for i in range(n) if i % 3 == 1 and 5 <= i < n - 5]
    for i in marked:   # the rows that get a stranded run read low rows only, so a deeper row exists on either side
        lo[i] = rng.permutation(4)[:int(rng.integers(1, 4))].tolist()
        up[i] = (n - 4 + rng.permutation(4)[:int(rng.integers(1, 4))]).tolist()
    legit = [lo[i] + up[i] for i in range(n)]
    lev_l, lev_u = _levels(legit, False), _levels(legit, True)
    pat, with_self = [], 0
    for i in range(n):
        if i not in marked:
            pat.append(legit[i])
            continue
        # the run: first a column >= i (L stops there), last a column <= i (U stops there), both sides between
        deep_l = max(range(i), key=lambda j: (lev_l[j], j))          # a row below i that is deeper in L than i's own reads
        deep_u = max(range(i + 1, n), key=lambda j: (lev_u[j], -j))
        first = i if i % 6 == 1 else deep_u
        last = i if i % 6 == 4 and first != i else deep_l
        mid = [int(rng.integers(0, i)), int(rng.integers(i + 1, n))]
        if first != i and last != i and i % 2 == 0:
            mid.insert(1, i)
        if first == i:
            mid.append(deep_u)
        if last == i:
            mid.insert(0, deep_l)
        run = [first] + mid + [last]
        with_self += i in run
        assert run[0] >= i and run[-1] <= i and any(c < i for c in run) and any(c > i for c in run)
        pat.append(lo[i] + run + up[i])
    # what the tests rely on
    assert len(marked) >= n // 4 and with_self >= 5
    assert any(len(p) > 1 and p != sorted(p) for p in lo) and any(len(p) > 1 and p != sorted(p) for p in up)
    assert _levels(pat, False) == lev_l and _levels(pat, True) == lev_u          # the run changes nothing either triangle reads
    for upper, lev in ((False, lev_l), (True, lev_u)):
        counted = _levels(pat, upper, count_all=True)
        assert sum(a > b for a, b in zip(counted, lev)) >= 5 and max(counted) != max(lev)
    return pat


def _pat_two_levels(half):
    i = np.arange(half, dtype=np.int64)
    return [[int(half + (7 * k + 3) % half)] for k in i] + [[int((5 * k + 1) % half)] for k in i]


def pattern(name, block=False):
    kind, _, arg = name.partition(":")
    if kind == "one":
        return [[]]
    if kind == "diag":
        return [[] for _ in range(int(arg))]
    if kind == "chain":
        return _pat_chain(int(arg))
    if kind == "bands":
        return _pat_bands(int(arg), 300 + int(arg))
    if kind == "ragged":
        return _pat_ragged(150, 100, 42) if block else _pat_ragged(400, 300, 41)
    if kind == "unsorted":
        return _pat_unsorted(70, 43)
    if kind == "wide":
        return _pat_two_levels(9600)
    if kind == "cap":
        return _pat_two_levels(131200)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def factor(name, nb=1):
    """The factor of a case (read-only, built once): entries uniform(-1, 1) / (entries of the row + 1), scalar inverse pivots in
    [0.5, 1.5]; a block's inverse pivot is the inverse of a diagonally dominant block (diagonal in [1, 2], the rest of a row below 1/2
    in sum), so a chain of any length stays far from overflow."""
    pat = pattern(name, block=nb > 1)
    n = len(pat)
    seed = 1000 * nb + sum(name.encode())
    rng = np.random.default_rng(seed)
    lens = np.array([len(p) for p in pat], dtype=np.int64)
    vals = rng.uniform(-1.0, 1.0, (int(lens.sum()), nb, nb)) / (np.repeat(lens, lens) + 1.0)[:, None, None]
    if nb == 1:
        piv = rng.uniform(0.5, 1.5, n)
    else:
        D = rng.uniform(-1.0, 1.0, (n, nb, nb)) / (2.0 * nb)
        D[:, np.arange(nb), np.arange(nb)] = rng.uniform(1.0, 2.0, (n, nb))
        piv = np.linalg.inv(D)
    vl = vals.reshape(-1).tolist() if nb == 1 else list(vals)
    start = np.concatenate(([0], np.cumsum(lens))).tolist()
    rows = [list(zip(pat[i], vl[start[i]:start[i + 1]])) for i in range(n)]
    return Factor(rows, piv, nb)


def rhs(F, seed=7):
    return np.random.default_rng(seed + F.n).uniform(-1.0, 1.0, F.n * F.nb)


# --- the solves, restated ------------------------------------------------------------------------
def _forward(m, ijlu, lu, zr, zz):
    zz[0] = zr[0]
    for i in range(1, m):
        for j in range(ijlu[i], ijlu[i + 1]):
            jj = ijlu[j]
            if jj < i:
                zr[i] -= lu[j] * zz[jj]
            else:
                break
        zz[i] = zr[i]


def _backward(m, ijlu, lu, zz, z):
    z[m - 1] = zz[m - 1] * lu[m - 1]
    for i in range(m - 2, -1, -1):
        for j in range(ijlu[i + 1] - 1, ijlu[i] - 1, -1):
            jj = ijlu[j]
            if jj > i:
                zz[i] -= lu[j] * z[jj]
            else:
                break
        z[i] = zz[i] * lu[i]


def _lists(F, r):
    return F.n, F.ijlu.tolist(), F.luval.tolist(), np.asarray(r, dtype=np.float64).tolist()


def precond_ilu(F, r):
    """fasp_precond_ilu: both sweeps"""
    m, ijlu, lu, zr = _lists(F, r)
    zz, z = [0.0] * m, [0.0] * m
    _forward(m, ijlu, lu, zr, zz)
    _backward(m, ijlu, lu, zz, z)
    return np.array(z)


def precond_ilu_forward(F, r):
    m, ijlu, lu, zr = _lists(F, r)
    zz = [0.0] * m
    _forward(m, ijlu, lu, zr, zz)
    return np.array(zz)


def precond_ilu_backward(F, r):
    m, ijlu, lu, zz = _lists(F, r)
    z = [0.0] * m
    _backward(m, ijlu, lu, zz, z)
    return np.array(z)


def _smat_mxv(a, ao, b, bo, nb):
    """c = a b for the nb x nb block at a[ao:], b at b[bo:]: 2, 3, 4, 5, 7 are written out as one left-to-right sum of products,
    every other size (6) adds its products to 0.0"""
    c = [0.0] * nb
    if nb in (2, 3, 4, 5, 7):
        for i in range(nb):
            s = a[ao + i * nb] * b[bo]
            for j in range(1, nb):
                s = s + a[ao + i * nb + j] * b[bo + j]
            c[i] = s
    else:
        for i in range(nb):
            temp = 0.0
            for j in range(nb):
                temp += a[ao + i * nb + j] * b[bo + j]
            c[i] = temp
    return c


def precond_dbsr_ilu(F, r):
    """fasp_precond_dbsr_ilu: nb = 1 is the scalar pair of sweeps; otherwise mult = block * vector, subtracted component by
    component, and the row ends with the inverse pivot block times what is left"""
    nb = F.nb
    if nb == 1:
        return precond_ilu(F, r)
    m, ijlu, lu, zr = _lists(F, r)
    nb2 = nb * nb
    zz, z = [0.0] * (m * nb), [0.0] * (m * nb)
    zz[0:nb] = zr[0:nb]
    for i in range(1, m):
        ib0 = i * nb
        for j in range(ijlu[i], ijlu[i + 1]):
            jj = ijlu[j]
            if jj < i:
                mult = _smat_mxv(lu, j * nb2, zz, jj * nb, nb)
                for ib in range(nb):
                    zr[ib0 + ib] -= mult[ib]
            else:
                break
        zz[ib0:ib0 + nb] = zr[ib0:ib0 + nb]
    z[(m - 1) * nb:m * nb] = _smat_mxv(lu, (m - 1) * nb2, zz, (m - 1) * nb, nb)
    for i in range(m - 2, -1, -1):
        ib0 = i * nb
        for j in range(ijlu[i + 1] - 1, ijlu[i] - 1, -1):
            jj = ijlu[j]
            if jj > i:
                mult = _smat_mxv(lu, j * nb2, z, jj * nb, nb)
                for ib in range(nb):
                    zz[ib0 + ib] -= mult[ib]
            else:
                break
        z[ib0:ib0 + nb] = _smat_mxv(lu, i * nb2, zz, ib0, nb)
    return np.array(z)


ENTRIES = {"fasp_precond_ilu": precond_ilu, "fasp_precond_ilu_forward": precond_ilu_forward,
           "fasp_precond_ilu_backward": precond_ilu_backward, "fasp_precond_dbsr_ilu": precond_dbsr_ilu}


@functools.lru_cache(maxsize=None)
def restated(name, nb, entry):
    """the restated z of an entry on a case's factor and rhs(factor) (read-only, computed once and shared)"""
    F = factor(name, nb)
    z = ENTRIES[entry](F, rhs(F))
    z.setflags(write=False)
    return z


# --- bits ----------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_values(got, want):
    """NaN in the same places (a generated NaN's sign differs between machines), every other value equal in all its bits
    -> (ok, indices that differ)"""
    got, want = np.asarray(got), np.asarray(want)
    ng, nw = np.isnan(got), np.isnan(want)
    bad = np.flatnonzero((ng != nw) | (~ng & ~nw & (bits(got) != bits(want))))
    return len(bad) == 0, bad


# --- the schedule rule of ilu_build_tri, restated -------------------------------------------------
def read_positions(F, upper):
    """per row, the positions in ijlu / luval one triangle reads, in the order it subtracts them"""
    cache = F.__dict__.setdefault("_reads", {})
    if upper in cache:
        return cache[upper]
    n, ijlu = F.n, F.ijlu.tolist()
    out = cache[upper] = []
    for i in range(n):
        pos = []
        if upper and i < n - 1:       # the backward sweep starts at row n - 2 ...
            for p in range(ijlu[i + 1] - 1, ijlu[i] - 1, -1):
                if ijlu[p] > i:
                    pos.append(p)
                else:
                    break
        elif not upper and i > 0:     # ... and the forward sweep at row 1
            for p in range(ijlu[i], ijlu[i + 1]):
                if ijlu[p] < i:
                    pos.append(p)
                else:
                    break
        out.append(pos)
    return out


def schedule(F, upper):
    """level(i) = 1 + the largest level of the rows i reads (0: reads none); the rows of a level in ascending order, cut into
    chunks of 64; a chunk's slab holds 64 x its longest row.  -> dict(levels, chunks, slab, real, longest, auto (1: the depth
    selects the single launch), level_wgs (workgroups of the level launches, four chunks each, summed), flow_wgs, level (per
    row), level_rows (rows per level), chunk_kmax / chunk_kmin / chunk_live / chunk_lane0 (per chunk: longest, shortest live row, live
    rows, the row in lane 0))"""
    n, ijlu = F.n, F.ijlu.tolist()
    reads = read_positions(F, upper)
    level = [0] * n
    for i in (range(n - 1, -1, -1) if upper else range(n)):
        lv = 0
        for p in reads[i]:
            lv = max(lv, level[ijlu[p]] + 1)
        level[i] = lv
    level = np.array(level)
    lens = np.array([len(p) for p in reads])
    nlev = int(level.max()) + 1
    order = np.argsort(level, kind="stable")
    level_rows = np.bincount(level, minlength=nlev)
    kmax, kmin, live, lane0, level_wgs, at = [], [], [], [], 0, 0
    for cnt in level_rows.tolist():
        for q in range(at, at + cnt, CHUNK):
            k = lens[order[q:min(q + CHUNK, at + cnt)]]
            kmax.append(int(k.max())); kmin.append(int(k.min())); live.append(len(k)); lane0.append(int(k[0]))
        level_wgs += (-(-cnt // CHUNK) + 3) // 4
        at += cnt
    chunks = len(kmax)
    return dict(levels=nlev, chunks=chunks, slab=CHUNK * sum(kmax), real=int(lens.sum()), longest=max(kmax),
                auto=int(nlev > FLOW_MIN_LEVELS), level_wgs=level_wgs, flow_wgs=max(1, min((chunks + 3) // 4, FLOW_MAX_GRID)),
                level=level, level_rows=level_rows, chunk_kmax=np.array(kmax), chunk_kmin=np.array(kmin), chunk_live=np.array(live),
                chunk_lane0=np.array(lane0))


def levels_counting_stranded(F, upper):
    """the levels a schedule would give if every entry on the triangle's side of the diagonal counted, stranded ones too"""
    return np.array(_levels([F.row_cols(i).tolist() for i in range(F.n)], upper, count_all=True))


# --- a-priori check of a restated solve in np.longdouble -------------------------------------------
def triangle_ratio(F, upper, b, x):
    """Worst |x_i - fl-free value| / bound over the components: with the COMPUTED x on the right, row i of L gives
    x_i = b_i - sum l_ij x_j and row i of U gives x_i = Dinv_i (b_i - sum u_ij x_j); evaluated in double in the reference's order each
    is m = (entries of the row + 1 for the pivot block) nb + 1 rounded operations at the most on terms of absolute sum
    s_i = |b_i| + sum |l_ij| |x_j| (U: |Dinv_i| times that), so |x_i - exact_i| <= gamma_(m+1) s_i (the backward error of a
    substitution, one row at a time; _libs.sum_bound_ratio, which adds the +1).  A ratio <= 1 passes."""
    from _libs import sum_bound_ratio
    ld = np.longdouble
    n, nb = F.n, F.nb
    reads = read_positions(F, upper)
    lens = np.array([len(p) for p in reads], dtype=np.int64)
    pos = np.array([p for r in reads for p in r], dtype=np.int64)
    xl = np.asarray(x).astype(ld).reshape(n, nb)
    acc = np.asarray(b).astype(ld).reshape(n, nb).copy()
    sab = np.abs(acc)
    if len(pos):
        blk = F.luval.reshape(-1, nb, nb)[pos].astype(ld)
        xg = xl[F.ijlu[pos].astype(np.int64)]
        prod = np.einsum("epq,eq->ep", blk, xg)
        pabs = np.einsum("epq,eq->ep", np.abs(blk), np.abs(xg))
        rows = np.flatnonzero(lens > 0)
        first = np.concatenate(([0], np.cumsum(lens)))[:-1][rows]
        acc[rows] -= np.add.reduceat(prod, first, axis=0)
        sab[rows] += np.add.reduceat(pabs, first, axis=0)
    if upper:
        piv = F.luval.reshape(-1, nb, nb)[:n].astype(ld)
        acc = np.einsum("ipq,iq->ip", piv, acc)
        sab = np.einsum("ipq,iq->ip", np.abs(piv), sab)
    m = np.repeat((lens + 1) * nb + 1, nb)
    return sum_bound_ratio(np.asarray(x), acc.reshape(-1), sab.reshape(-1), m)


# --- the block smoother's matrix -----------------------------------------------------------------
def smoother_matrix(F, seed=11):
    """BSR matrix on the union pattern of the factor plus the diagonal, columns ascending, seeded values -> (ia, ja, val)"""
    rng = np.random.default_rng(seed + F.n + F.nb)
    cols = [sorted(set(F.row_cols(i).tolist()) | {i}) for i in range(F.n)]
    ia = np.concatenate(([0], np.cumsum([len(c) for c in cols]))).astype(np.int32)
    ja = np.array([c for r in cols for c in r], dtype=np.int32)
    val = rng.uniform(-1.0, 1.0, len(ja) * F.nb * F.nb)
    return ia, ja, val


# --- factors the library must refuse (or accept) without a launch -----------------------------------
def edge_factor(kind):
    """n = 6.  "u_high": a U entry with column n; "u_far": with column n + 1000; "l_neg": an L entry with column -1; "stranded_out":
    columns n + 3 and -2 inside a stranded run, which nothing reads (a valid factor)"""
    n = 6
    pat = _pat_chain(n)
    if kind == "u_high":
        pat[2] = [1, 3, n]
    elif kind == "u_far":
        pat[2] = [1, n + 1000, 3]
    elif kind == "l_neg":
        pat[3] = [2, -1, 4]
    elif kind == "stranded_out":
        pat[3] = [2, n + 3, -2, 4]
    else:
        raise KeyError(kind)
    return Factor([[(c, 0.25) for c in p] for p in pat], np.ones(n), 1)
