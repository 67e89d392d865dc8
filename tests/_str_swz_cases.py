"""Block Gauss-Seidel (Schwarz) cases shared by tools/gen_golden_str_swz.py and the structured block-GS tests: neighbour sets, orders, seeded
matrices, a numpy restatement of the reference (fasp_generate_diaginv_block ItrSmootherSTR.c:1543, fasp_smoother_dstr_swz :1665,
fasp_smat_lu_decomp / _solve BlaSmallMatLU.c:52 / :124) and the calls into a library -- ours or the compiled reference.

The restatement.  The patch of point i is the member list [i, p_0, p_1, ...] of its neighbours that are not absent (< 0); its matrix holds every
member's diagonal block on the diagonal, A(i, p) in block (0, a) and A(p, i) in block (a, 0) for member a >= 1 where a band has that offset, and
nothing between two members that are not the centre.  LU with the first row of largest magnitude as the pivot, whole rows interchanged, stopping
where a pivot is below 1e-20.  A visit gathers the residual b - A u at the members (the rows of _str_cases.model_aAxpy(-1, .): the reference
recomputes the whole residual after every visit, every row of it is a fresh function of b and u), solves, and adds the correction to u in
member order.  sequential=True visits point after point; the default evaluates the same visits in batches of independent ones (visit_levels),
which is the same arithmetic on the same operands."""
import ctypes as C
import hashlib
import os
import zlib

import numpy as np

import _str_cases as S
import _str_ilu_cases as I
from _libs import ROOT, T

GOLDEN = os.path.join(ROOT, "tests", "golden", "str_swz.npz")
P = C.POINTER
SMALLREAL = 1e-20
HEAD = 8
WHOLE = 2000     # factors / results of at most this many doubles may be recorded whole


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def ngrid_of(case):
    return case["nx"] * case["ny"] * case["nz"]


def with_form(case):
    """The case with the arithmetic form of its products (what fasp_hip_str_form says), as _str_cases.model_aAxpy wants it."""
    if "form" in case:
        return case
    n, offs, nc = ngrid_of(case), sorted(case["offsets"]), case["nc"]
    nx, nxy = case["nx"], case["nx"] * case["ny"]
    canon = False
    if len(offs) == 6:
        canon = nx > 1 and nxy > nx and n >= 2 * nxy and offs == [-nxy, -nx, -1, 1, nx, nxy]
    elif len(offs) == 4:
        nline = case["ny"] if nx == 1 else nx
        canon = nline > 1 and n >= 2 * nline and offs == [-nline, -1, 1, nline]
    form = S.FORM_G if not canon else S.FORM_S if nc == 1 else S.FORM_B if nc in (3, 5) else S.FORM_N
    return dict(case, form=form)


# ---- matrices -------------------------------------------------------------------------------------------------------------------------
def grid_case(grid, nc, order=None, tag=""):
    """The dominant grid-derived matrix of _str_ilu_cases: no patch of it interchanges a row."""
    return with_form(I.grid_case(grid, nc, order=order, tag=tag))


def weak_case(grid, nc):
    """grid_case with plain standard normal diagonal blocks (no shift): nearly every patch interchanges rows.  The seed tag is the first of
    _weak, _weak1, ... at which at least 90 % of the nc = 1 patches with geometric neighbours interchange on each of the grids used (a patch
    at a grid corner has three or four rows only); tools/gen_golden_str_swz.py asserts it."""
    c = I.grid_case(grid, nc, tag="_weak6")
    n = ngrid_of(c)
    c["diag"] = _rng(c["name"] + "/weakdiag").standard_normal(n * nc * nc)
    return with_form(c)


def wrap_case(grid, nc):
    """grid_case with one non-zero coefficient between points that are not geometric neighbours (the -1 band at the start of line 1)."""
    c = I.grid_case(grid, nc, tag="_wrap")
    gx = I.geometry(*grid)[0]
    k = c["offsets"].index(-1)
    band = c["bands"][k].copy()
    band[(gx - 1) * nc * nc] = 0.375
    c["bands"][k] = band
    return with_form(c)


def stopped_case():
    """nc = 1 on 5 x 4 x 3 with one diagonal entry 0.0: without neighbours the patch of point 7 stops at its first pivot."""
    c = I.grid_case((5, 4, 3), 1, tag="_stop")
    d = c["diag"].copy()
    d[7] = 0.0
    c["diag"] = d
    return with_form(c)


NONCANON = {6: [1, 0, 4, 5, 3, 2], 4: [1, 0, 3, 2]}


def vectors(case):
    r = _rng(case["name"] + "/swz_vectors")
    n = ngrid_of(case) * case["nc"]
    return r.standard_normal(n), r.standard_normal(n)   # b, u0


def as_str(case):
    return T.as_str(case["nx"], case["ny"], case["nz"], case["nc"], case["offsets"], case["diag"], case["bands"])


# ---- neighbour sets and orders --------------------------------------------------------------------------------------------------------
def geometric(grid):
    """[ngrid, 6] (3-D) or [ngrid, 4] (2-D): -x, +x, -y, +y, -z, +z, -1 where the grid ends."""
    gx, gy, gz = I.geometry(*grid)
    n = gx * gy * gz
    i = np.arange(n)
    x, y, z = i % gx, (i // gx) % gy, i // (gx * gy)
    cols = [np.where(x > 0, i - 1, -1), np.where(x < gx - 1, i + 1, -1), np.where(y > 0, i - gx, -1), np.where(y < gy - 1, i + gx, -1)]
    if gz > 1:
        cols += [np.where(z > 0, i - gx * gy, -1), np.where(z < gz - 1, i + gx * gy, -1)]
    return np.stack(cols, axis=1).astype(np.int32)


def far_set(grid):
    """Three entries per point: the point i + 1 (so that the natural order is one chain of ngrid levels), a far point -- absent for a
    quarter of the points, the point i + 1 a second time for every third --, and for every fifth point the point itself."""
    n = grid[0] * grid[1] * grid[2]
    r = _rng(f"far_{grid}")
    i = np.arange(n)
    nxt = np.where(i + 1 < n, i + 1, -1)
    a = np.where(i % 3 == 0, nxt, np.where(r.random(n) < 0.25, -1, (i * 7 + 11) % n))
    c = np.where(i % 5 == 0, i, -1)
    return np.stack([nxt, a, c], axis=1).astype(np.int32)


def neigh_of(grid, key):
    if key == "geo":
        return geometric(grid)
    if key == "none":
        return None
    if key == "absent":
        return np.full((grid[0] * grid[1] * grid[2], 2), -1, dtype=np.int32)
    if key == "far":
        return far_set(grid)
    raise KeyError(key)


def colour12(grid):
    gx, gy, gz = I.geometry(*grid)
    i = np.arange(gx * gy * gz)
    c = (i % gx + 3 * ((i // gx) % gy) + 7 * (i // (gx * gy))) % 12
    return np.argsort(c, kind="stable").astype(np.int32)


def order_of(grid, key):
    n = grid[0] * grid[1] * grid[2]
    if key == "natural":
        return None
    if key == "reversed":
        return np.arange(n - 1, -1, -1, dtype=np.int32)
    if key == "random":
        return _rng(f"swzperm_{grid}").permutation(n).astype(np.int32)
    if key == "colour":
        return colour12(grid)
    if key == "twice":      # a sequence that names points twice (and so leaves others out)
        o = _rng(f"swztwice_{grid}").permutation(n).astype(np.int32)
        o[3], o[n - 2] = o[0], o[n // 2]
        return o
    raise KeyError(key)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def members(i, neigh):
    if neigh is None:
        return [int(i)]
    return [int(i)] + [int(p) for p in neigh[i] if p >= 0]


def patch_matrix(case, i, mem):
    nc, n = case["nc"], ngrid_of(case)
    m = len(mem) * nc
    M = np.zeros((m, m))
    D = np.asarray(case["diag"]).reshape(n, nc, nc)
    for a, p in enumerate(mem):
        M[a * nc:(a + 1) * nc, a * nc:(a + 1) * nc] = D[p]
    for a, p in enumerate(mem):
        if a == 0:
            continue
        for off, band in zip(case["offsets"], case["bands"]):
            B = np.asarray(band).reshape(-1, nc, nc)
            if off == p - i:
                M[0:nc, a * nc:(a + 1) * nc] = B[p - max(p - i, 0)]
            if off == i - p:
                M[a * nc:(a + 1) * nc, 0:nc] = B[i - max(i - p, 0)]
    return M


def lu_decomp(M):
    """fasp_smat_lu_decomp on a copy -> (LU, pivot, stopped)."""
    A = M.copy()
    m = A.shape[0]
    piv = np.zeros(m, dtype=np.int32)
    for k in range(m):
        col = np.abs(A[k:, k])
        j = k + int(np.argmax(col))          # the first of the largest: strict <
        piv[k] = j
        if j != k:
            A[[k, j]] = A[[j, k]]
        if abs(A[k, k]) < SMALLREAL:
            return A, piv, True
        A[k + 1:, k] = A[k + 1:, k] / A[k, k]
        A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - A[k + 1:, k:k + 1] * A[k:k + 1, k + 1:]
    return A, piv, False


def lu_solve_batch(F, piv, rhs):
    """fasp_smat_lu_solve on a batch of equal size: F [B, m, m], piv [B, m], rhs [B, m] -> x [B, m]."""
    Bn, m = rhs.shape
    b = rhs.copy()
    x = np.zeros_like(b)
    rows = np.arange(Bn)
    for k in range(m):
        pk = piv[:, k]
        bk, bp = b[rows, k].copy(), b[rows, pk].copy()
        b[rows, pk] = bk
        b[rows, k] = bp
        xk = b[:, k].copy()
        for i in range(k):
            xk = xk - x[:, i] * F[:, k, i]
        x[:, k] = xk
    for k in range(m - 1, -1, -1):
        xk = x[:, k].copy()
        for i in range(k + 1, m):
            xk = xk - x[:, i] * F[:, k, i]
        x[:, k] = xk / F[:, k, k]
    return x


def factor_all(case, neigh):
    """Per point: (members, LU, pivot, stopped)."""
    return [(mem,) + lu_decomp(patch_matrix(case, i, mem)) for i, mem in ((i, members(i, neigh)) for i in range(ngrid_of(case)))]


def packed(fac, case, neigh):
    """The reference's host layout: all factors / pivots one after the other in ONE zero-initialised block of ((nneigh+1) nc)^2 ngrid doubles /
    (nneigh+1) nc ngrid ints."""
    n, nc = ngrid_of(case), case["nc"]
    w = ((0 if neigh is None else neigh.shape[1]) + 1) * nc
    d, p = np.zeros(w * w * n), np.zeros(w * n, dtype=np.int32)
    at_d = at_p = 0
    for mem, F, piv, _ in fac:
        d[at_d:at_d + F.size] = F.reshape(-1); at_d += F.size
        p[at_p:at_p + piv.size] = piv; at_p += piv.size
    return d, p


def read_sets(case):
    """Per point: the points its row has a term to whose coefficient block is not all 0.0 (a zero block is no read: for finite u the product
    is a zero whichever u is read)."""
    n, nc = ngrid_of(case), case["nc"]
    out = [[] for _ in range(n)]
    for off, band in zip(case["offsets"], case["bands"]):
        m = n - abs(off)
        if m <= 0:
            continue
        nz = np.any(np.asarray(band).reshape(m, nc * nc) != 0.0, axis=1)
        lo = -off if off < 0 else 0
        for i in np.flatnonzero(nz) + lo:
            out[int(i)].append(int(i) + off)
    return out


def visit_levels(case, neigh, pts):
    """level(v) = 1 + the largest level among the earlier visits that wrote what v reads, read what v writes or wrote what v writes."""
    n = ngrid_of(case)
    rs = read_sets(case)
    lw, mr = [-1] * n, [-1] * n
    lev = np.zeros(len(pts), dtype=np.int64)
    for v, i in enumerate(int(p) for p in pts):
        mem = members(i, neigh)
        reads = set(mem)
        for p in mem:
            reads.update(rs[p])
        L = max([lw[j] for j in reads] + [mr[j] for j in mem]) + 1
        lev[v] = L
        for j in mem:
            lw[j] = L
        for j in reads:
            if mr[j] < L:
                mr[j] = L
    return lev


def visits(case, order):
    n = ngrid_of(case)
    return np.arange(n) if order is None else np.asarray(order[:n], dtype=np.int64)


def model_sweep(case, neigh, order, fac, b, u0, sequential=False):
    """One sweep of fasp_smoother_dstr_swz in numpy -> u.  fac: factor_all(case, neigh)."""
    n, nc = ngrid_of(case), case["nc"]
    u = np.array(u0, dtype=np.float64)
    pts = visits(case, order)
    if sequential:
        batches = [pts[v:v + 1] for v in range(len(pts))]
    else:
        lev = visit_levels(case, neigh, pts)
        by = np.argsort(lev, kind="stable")
        batches = [pts[g] for g in np.split(by, np.flatnonzero(np.diff(lev[by])) + 1)] if len(pts) else []
    for batch in batches:
        r = S.model_aAxpy(case, np.asarray(case["diag"]), case["bands"], -1.0, u, np.asarray(b)).reshape(n, nc)
        es = []
        for m in sorted({fac[int(i)][1].shape[0] for i in batch}):     # one batched solve per patch size
            idx = [int(i) for i in batch if fac[int(i)][1].shape[0] == m]
            rhs = np.stack([r[fac[i][0]].reshape(-1) for i in idx])
            e = lu_solve_batch(np.stack([fac[i][1] for i in idx]), np.stack([fac[i][2] for i in idx]), rhs)
            es += list(zip(idx, e))
        ug = u.reshape(n, nc)
        for i, e in es:      # the visits of a batch write disjoint points; within a visit in member order
            for a, p in enumerate(fac[i][0]):
                ug[p] = ug[p] + e[a * nc:(a + 1) * nc]
    return u


def interchanges(fac):
    """Number of patches with at least one row interchange."""
    return sum(1 for _, _, piv, _ in fac if np.any(piv != np.arange(piv.size)))


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


# ---- calls into a library (ours or the compiled reference) ------------------------------------------------------------------------------
def protos(L):
    L.fasp_generate_diaginv_block.argtypes = [P(T.dSTRmat), P(T.ivector), P(T.dvector), P(T.ivector)]
    L.fasp_generate_diaginv_block.restype = None
    L.fasp_smoother_dstr_swz.argtypes = [P(T.dSTRmat), P(T.dvector), P(T.dvector), P(T.dvector), P(T.ivector), P(T.ivector), P(T.ivector)]
    L.fasp_smoother_dstr_swz.restype = None
    L.fasp_precond_dstr_blockgs.argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
    L.fasp_precond_dstr_blockgs.restype = None
    L.fasp_solver_dstr_krylov_blockgs.argtypes = [P(T.dSTRmat), P(T.dvector), P(T.dvector), P(T.ITS_param), P(T.ivector), P(T.ivector)]
    L.fasp_solver_dstr_krylov_blockgs.restype = C.c_int
    return L


def _ivec(a):
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    return T.ivector(a.size, a.ctypes.data_as(T.c_int_p)), a


class Factors:
    """The arrays of dvector / ivector a library's fasp_generate_diaginv_block filled, with numpy copies of the two blocks they are carved
    from: d (((nneigh+1) nc)^2 ngrid doubles) and p ((nneigh+1) nc ngrid ints).  Built from numpy blocks too (for a recorded factor)."""

    def __init__(self, n, w):
        self.n, self.w = n, w
        self.dv, self.pv = (T.dvector * n)(), (T.ivector * n)()
        self.d = self.p = None

    def adopt(self):
        """Copy the blocks out of the library's allocation (the first entries hold the bases) and point the vectors at the copies."""
        n, w = self.n, self.w
        rows = [self.dv[i].row for i in range(n)]
        assert all(0 <= r <= w * w for r in rows)
        self.d = np.ctypeslib.as_array(self.dv[0].val, shape=(w * w * n,)).copy()
        self.p = np.ctypeslib.as_array(self.pv[0].val, shape=(w * n,)).copy()
        d0, p0 = C.addressof(self.dv[0].val.contents), C.addressof(self.pv[0].val.contents)
        self.doff = [(C.addressof(self.dv[i].val.contents) - d0) // 8 for i in range(n)]
        self.poff = [(C.addressof(self.pv[i].val.contents) - p0) // 4 for i in range(n)]
        self.point()
        return self

    def point(self):
        for i in range(self.n):
            self.dv[i].val = C.cast(C.c_void_p(self.d.ctypes.data + 8 * int(self.doff[i])), T.c_double_p)
            self.pv[i].val = C.cast(C.c_void_p(self.p.ctypes.data + 4 * int(self.poff[i])), T.c_int_p)

    @classmethod
    def from_blocks(cls, n, w, d, p, msizes):
        f = cls(n, w)
        f.d, f.p = np.array(d, dtype=np.float64), np.array(p, dtype=np.int32)
        f.doff = list(np.concatenate([[0], np.cumsum(np.asarray(msizes) ** 2)[:-1]]).astype(int))
        f.poff = list(np.concatenate([[0], np.cumsum(msizes)[:-1]]).astype(int))
        for i, m in enumerate(msizes):
            f.dv[i].row, f.pv[i].row = int(m) * int(m), int(m)
        f.point()
        return f


def generate(L, case, neigh):
    """fasp_generate_diaginv_block of library L -> Factors (the library's allocation is left to it)."""
    A, keep = as_str(case)
    n, nc = ngrid_of(case), case["nc"]
    nv, nk = _ivec(neigh)
    f = Factors(n, ((0 if neigh is None else neigh.shape[1]) + 1) * nc)
    L.fasp_generate_diaginv_block(C.byref(A), None if nv is None else C.byref(nv), f.dv, f.pv)
    return f.adopt()


def call_swz(L, case, neigh, order, f, b, u0):
    """fasp_smoother_dstr_swz of library L on copies -> u."""
    A, keep = as_str(case)
    bb, u = np.array(b), np.array(u0)
    bv, uv = T.dvector(bb.size, T.dp(bb)), T.dvector(u.size, T.dp(u))
    nv, nk = _ivec(neigh)
    ov, ok = _ivec(order)
    L.fasp_smoother_dstr_swz(C.byref(A), C.byref(bv), C.byref(uv), f.dv, f.pv, None if nv is None else C.byref(nv), None if ov is None else C.byref(ov))
    return u


class PcData:
    """A precond_data_str over (A, factors, neigh, order) and everything it points to."""

    def __init__(self, case, neigh, order, f):
        self.A, self.keep = as_str(case)
        self.nv, self.nk = _ivec(neigh)
        self.ov, self.ok = _ivec(order)
        self.f = f
        d = T.precond_data_str()
        C.memset(C.byref(d), 0, C.sizeof(d))
        d.A_str = C.pointer(self.A)
        d.diaginv = C.cast(f.dv, P(T.dvector)) if f is not None else None
        d.pivot = C.cast(f.pv, P(T.ivector)) if f is not None else None
        d.neigh = C.pointer(self.nv) if self.nv is not None else None
        d.order = C.pointer(self.ov) if self.ov is not None else None
        self.d = d

    def ptr(self):
        return C.cast(C.pointer(self.d), C.c_void_p)


def solve_blockgs(L, case, b, neigh, order, method, restart, maxit=500):
    """fasp_solver_dstr_krylov_blockgs of L from a zero guess -> (status, x)."""
    A, keep = as_str(case)
    x = np.zeros_like(b)
    bv, kb = T.as_vec(b)
    xv = T.dvector(x.size, T.dp(x))
    p = S.its_param(method, restart, maxit)
    nv, nk = _ivec(neigh)
    ov, ok = _ivec(order)
    st = L.fasp_solver_dstr_krylov_blockgs(C.byref(A), C.byref(bv), C.byref(xv), C.byref(p), None if nv is None else C.byref(nv), None if ov is None else C.byref(ov))
    return st, x


# ---- recorded cases (tools/gen_golden_str_swz.py, tests/test_str_swz_host.py) -----------------------------------------------------------
HOST_GRIDS = ((5, 4, 3), (9, 7, 1), (1, 8, 6))
HOST_NC = (1, 2, 3, 5, 7)


def host_cases():
    """(key, case, grid, neighbour key, order key)"""
    out = []
    for grid in HOST_GRIDS:
        g = "x".join(str(v) for v in grid)
        for nc in HOST_NC:
            for kind, c in (("dom", grid_case(grid, nc)), ("weak", weak_case(grid, nc))):
                combos = [("geo", "natural"), ("none", "natural")]
                if nc in (1, 3):
                    combos += [("geo", "reversed"), ("geo", "random"), ("geo", "colour"), ("geo", "twice"), ("absent", "random")]
                    if grid == (5, 4, 3):
                        combos += [("far", "natural"), ("far", "random")]
                for nk, ok in combos:
                    out.append((f"{kind}_{g}_nc{nc}/{nk}/{ok}", c, grid, nk, ok))
    return out


WHOLE_KEYS = ("dom_5x4x3_nc1/geo/natural", "weak_5x4x3_nc1/geo/natural", "weak_9x7x1_nc2/none/natural", "weak_5x4x3_nc3/far/random")

KRYLOV = [("bicgstab", T.SOLVER_BiCGstab, 25), ("gmres", T.SOLVER_GMRES, 10), ("vgmres", T.SOLVER_VGMRES, 10)]
KRYLOV_SETS = [("geo", "natural"), ("geo", "random"), ("none", "natural")]


def scalar_system():
    """The upwind 9 x 8 x 7 system of _str_cases.scalar_system(False) as a case dict, and b."""
    case, diag, bands, b = S.scalar_system(False)
    return dict(case, diag=diag, bands=bands), b


def block_system(nc):
    case, diag, bands, b = S.block_system(nc, False)
    return dict(case, diag=diag, bands=bands), b
