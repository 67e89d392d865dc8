"""Structured-smoother cases shared by tools/gen_golden_str_smoother.py and the structured-smoother tests: seeded matrices (the builders of
_str_cases / _str_ilu_cases), the orders, a numpy restatement of the reference's sweeps (ItrSmootherSTR.c) and the
calls into a library -- ours or the compiled reference.

The restatement, model_sweep: a visit of grid point i starts from b_i, subtracts the terms that exist by the reference's rule (0 <= i + d <
ngrid; a lower band indexed by its column) in band storage order, rhs_p = rhs_p - a_pq u_q with q ascending, and closes as the variant does
(GS: a division for nc = 1, diaginv rhs summed as fasp_blas_smat_mxv for nc > 1; SOR: (1 - w) u + w (rhs / diag) for nc = 1, the file's
aAxpby for nc > 1; the scalar C/F SOR closes its SECOND pass as GS does, ItrSmootherSTR.c:1443).  sequential=True visits point after point
as the reference's loops do; the default evaluates the same visits in batches of independent ones (a visit waits for every earlier visit
that wrote what it reads, read what it writes or wrote the same point; a term whose coefficients are all 0.0 counts as no read: for finite
vectors rhs - 0 u is rhs whichever u is read), which is the same arithmetic on the same operands --
tests/test_str_smoother_host.py holds the two to each other and the sequential one to the reference, bit for bit."""
import ctypes as C
import hashlib
import os
import zlib

import numpy as np

import _str_cases as S
import _str_ilu_cases as I
from _libs import ROOT, T

GOLDEN = os.path.join(ROOT, "tests", "golden", "str_smoother.npz")
P = C.POINTER
JACOBI, GS, SOR = 0, 1, 2
ASCEND, DESCEND, USERDEFINED, CPFIRST, FPFIRST = 12, 21, 0, 1, -1
FORM_LEVEL, FORM_PIPE, FORM_LIST, FORM_JACOBI = 0, 1, 2, 3
WEIGHTS = (1.1, 0.0, 1.0)
WHOLE = 2000   # a result of at most this many doubles may be recorded whole
WHOLE_KEYS = ("jacobi", "gs_ascend", "gs_cf_part_f", "sor_descend_w1.1", "sor_cf_rb_c_w1.1", "sor_order_rnd_w0.0")   # ... and is, for these variants
HEAD = 8       # of every other result: the SHA-256 and its first doubles


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def ngrid_of(case):
    return case["nx"] * case["ny"] * case["nz"]


def grid_case(grid, nc, order=None, tag=""):
    """The grid-derived matrix of _str_ilu_cases (dominant diagonal blocks, zero coefficients across line and plane ends)."""
    return I.grid_case(grid, nc, order=order, tag=tag)


NONCANON = {6: [1, 0, 4, 5, 3, 2], 4: [1, 0, 3, 2]}   # +1 before -1, planes first


def wrap_case(grid, nc):
    """grid_case with ONE non-zero coefficient between points that are not geometric neighbours: the -1 band at the start of line 1."""
    c = grid_case(grid, nc, tag="_wrap")
    gx = I.geometry(*grid)[0]
    k = c["offsets"].index(-1)
    band = c["bands"][k].copy()
    band[(gx - 1) * nc * nc] = 0.375   # row gx (x = 0, y = 1) reads point gx - 1 (x = gx - 1, y = 0); a lower band is stored by column
    c["bands"][k] = band
    return c


def extra_offset_case(grid, nc):
    """grid_case plus two bands outside the six (+-(nline + 1)), random values."""
    c = grid_case(grid, nc, tag="_extra")
    gx = I.geometry(*grid)[0]
    n, r = ngrid_of(c), _rng(c["name"] + "/extra")
    for o in (gx + 1, -(gx + 1)):
        c["offsets"] = c["offsets"] + [o]
        c["bands"] = c["bands"] + [0.3 * r.standard_normal((n - abs(o)) * nc * nc)]
    return c


def diffusion_case(grid):
    """Variable-coefficient diffusion operator (SPD, nc = 1) on `grid`, canonical band order; the stored zeros carry the grid lines."""
    nx, ny, nz = grid
    gx, gy, gz = I.geometry(nx, ny, nz)
    n = nx * ny * nz
    r = _rng(f"diffusion_{nx}x{ny}x{nz}")
    i = np.arange(n)
    diag = np.full(n, 0.05)
    bands = {}
    for d, inside in ((1, i % gx < gx - 1), (gx, (i // gx) % gy < gy - 1), (gx * gy, i // (gx * gy) < gz - 1)):
        if d >= n:
            continue
        k = np.where(inside, np.exp(r.uniform(-1.0, 1.0, n)), 0.0)[:n - d]
        diag[:n - d] += k
        diag[d:] += k
        bands[d], bands[-d] = -k, -k.copy()
    offsets = [o for d in sorted(set(abs(o) for o in bands)) for o in (-d, d)]
    return dict(name=f"diffusion_{nx}x{ny}x{nz}", nx=nx, ny=ny, nz=nz, nc=1, offsets=offsets, diag=diag, bands=[bands[o] for o in offsets])


def vectors(case):
    r = _rng(case["name"] + "/smoother_vectors")
    n = ngrid_of(case) * case["nc"]
    return r.standard_normal(n), r.standard_normal(n)   # b, u0


def as_str(case):
    return T.as_str(case["nx"], case["ny"], case["nz"], case["nc"], case["offsets"], case["diag"], case["bands"])


# ---- orders ---------------------------------------------------------------------------------------------------------------------------
def red_black(grid):
    gx, gy, gz = I.geometry(*grid)
    i = np.arange(gx * gy * gz)
    par = (i % gx + (i // gx) % gy + i // (gx * gy)) % 2
    return np.where(par == 0, 1, -1).astype(np.int32)


def partial_marks(grid):
    """A C/F marking that leaves some points unmarked (0) and is no colouring."""
    n = grid[0] * grid[1] * grid[2]
    return _rng(f"marks_{grid}").choice(np.array([1, -1, 0], dtype=np.int32), size=n, p=[0.4, 0.4, 0.2]).astype(np.int32)


def permutation(grid, which):
    n = grid[0] * grid[1] * grid[2]
    if which == "reversed":
        return np.arange(n - 1, -1, -1, dtype=np.int32)
    if which == "natural":
        return np.arange(n, dtype=np.int32)
    return _rng(f"perm_{grid}").permutation(n).astype(np.int32)


def visits(ngrid, order, mark, cf_entry=False):
    """(points, second) of a GS / SOR sweep as _gs1 / _sor1 dispatch it, None when nothing is swept.  second: the visit belongs to the SECOND
    pass of the C/F form."""
    if mark is None:
        if cf_entry or order not in (ASCEND, DESCEND):
            return None
        pts = np.arange(ngrid) if order == ASCEND else np.arange(ngrid - 1, -1, -1)
        return pts, np.zeros(ngrid, dtype=bool)
    mark = np.asarray(mark)
    if order == USERDEFINED and not cf_entry:
        return mark.astype(np.int64), np.zeros(ngrid, dtype=bool)
    first, second = np.flatnonzero(mark == order), np.flatnonzero(mark == -order)
    return np.concatenate([first, second]), np.concatenate([np.zeros(first.size, dtype=bool), np.ones(second.size, dtype=bool)])


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _aligned(case):
    """(offset, blocks[ngrid, nc, nc] aligned to the row, exists[ngrid]) of the bands that have terms, in storage order."""
    n, nc = ngrid_of(case), case["nc"]
    out = []
    for off, band in zip(case["offsets"], case["bands"]):
        m = n - abs(off)
        if m <= 0:
            continue
        full = np.zeros((n, nc, nc))
        ex = np.zeros(n, dtype=bool)
        lo = -off if off < 0 else 0   # a lower band is stored by column
        full[lo:lo + m] = np.asarray(band).reshape(m, nc, nc)
        ex[lo:lo + m] = True
        out.append((off, full, ex))
    return out


def visit_levels(case, pts, zero_is_no_term=False):
    """Level of every visit by the rule of the module docstring, with the reference's terms (every index in range).  zero_is_no_term: a
    term whose coefficient block is all 0.0 is no dependency (for finite vectors rhs - 0 u is rhs whichever u is read)."""
    n = ngrid_of(case)
    terms = [(off, ex & (np.any(full != 0.0, axis=(1, 2)) if zero_is_no_term else True)) for off, full, ex in _aligned(case)]
    nbrs = [[] for _ in range(n)]
    for off, dep in terms:
        for i in np.flatnonzero(dep):
            nbrs[i].append(int(i) + off)
    lw, mr = [-1] * n, [-1] * n
    lev = np.zeros(len(pts), dtype=np.int64)
    for v, i in enumerate(int(p) for p in pts):
        nb = nbrs[i]
        L = max([lw[i], mr[i]] + [lw[j] for j in nb]) + 1
        lev[v] = L
        lw[i] = L
        for j in nb:
            if mr[j] < L:
                mr[j] = L
    return lev


def _close(kind, nc, w, dg, rhs, uold, as_gs):
    """The closing step on a batch: rhs, uold [m, nc]; dg [m] (nc = 1: the diagonal) or [m, nc, nc] (the inverted blocks)."""
    w = np.float64(w)
    if nc == 1:
        q = rhs[:, 0] / dg
        if kind == SOR:
            omw = np.float64(1.0) - w
            q = np.where(as_gs, q, omw * uold[:, 0] + w * q)
        return q[:, None]
    if kind != SOR:
        s = dg[:, :, 0] * rhs[:, None, 0]
        if nc == 6:   # fasp_blas_smat_mxv's general text starts from 0.0
            s = 0.0 + s
        for q in range(1, nc):
            s = s + dg[:, :, q] * rhs[:, None, q]
        return s
    omw = np.float64(1.0) - w
    if w == 0.0:
        return uold * omw
    y = uold * (omw / w)
    for q in range(nc):
        y = y + dg[:, :, q] * rhs[:, None, q]
    return y * w


def model_sweep(case, kind, order, mark, w, dinv, b, u0, cf_entry=False, sequential=False):
    """One sweep of the reference in numpy -> u.  dinv: the inverted diagonal blocks (nc > 1)."""
    n, nc = ngrid_of(case), case["nc"]
    terms = _aligned(case)
    dg = np.asarray(case["diag"]) if nc == 1 else np.asarray(dinv).reshape(n, nc, nc)
    bg = np.asarray(b).reshape(n, nc)
    u = np.array(u0, dtype=np.float64).reshape(n, nc)
    if kind == JACOBI:
        src, batches = u.copy(), [(np.arange(n), np.zeros(n, dtype=bool))]
    else:
        vs = visits(n, order, mark, cf_entry)
        if vs is None:
            return u.reshape(-1)
        pts, second = vs
        src = u
        if sequential:
            batches = [(pts[v:v + 1], second[v:v + 1]) for v in range(len(pts))]
        else:
            lev = visit_levels(case, pts, zero_is_no_term=True)
            by = np.argsort(lev, kind="stable")
            cuts = np.flatnonzero(np.diff(lev[by])) + 1
            batches = [(pts[g], second[g]) for g in np.split(by, cuts)] if len(pts) else []
    for idx, sec in batches:
        rhs = bg[idx].copy()
        for off, full, ex in terms:
            e = ex[idx][:, None]
            xs = src[np.clip(idx + off, 0, n - 1)]
            a = full[idx]
            for q in range(nc):
                rhs = np.where(e, rhs - a[:, :, q] * xs[:, None, q], rhs)
        u[idx] = _close(kind, nc, w, dg[idx], rhs, u[idx], sec & (kind == SOR) & (nc == 1))
    return u.reshape(-1)


def residual_norm(case, b, u):
    """||b - A u||_2 in numpy, one fixed order of operations (compared between two u with equal bits only)."""
    n, nc = ngrid_of(case), case["nc"]
    ug = np.asarray(u).reshape(n, nc)
    r = np.asarray(b).reshape(n, nc) - np.einsum("ipq,iq->ip", np.asarray(case["diag"]).reshape(n, nc, nc), ug)
    for off, full, ex in _aligned(case):
        r = r - np.where(ex[:, None], np.einsum("ipq,iq->ip", full, ug[np.clip(np.arange(n) + off, 0, n - 1)]), 0.0)
    return float(np.sqrt(np.sum(r * r)))


# ---- calls into a library (ours or the compiled reference) --------------------------------------------------------------------------------
ENTRIES = {   # name -> extra argument types after (A, b, u)
    "jacobi": [], "jacobi1": [T.c_double_p], "gs": [C.c_int, T.c_int_p], "gs1": [C.c_int, T.c_int_p, T.c_double_p],
    "gs_ascend": [T.c_double_p], "gs_descend": [T.c_double_p], "gs_order": [T.c_double_p, T.c_int_p], "gs_cf": [T.c_double_p, T.c_int_p, C.c_int],
    "sor": [C.c_int, T.c_int_p, C.c_double], "sor1": [C.c_int, T.c_int_p, T.c_double_p, C.c_double], "sor_ascend": [T.c_double_p, C.c_double],
    "sor_descend": [T.c_double_p, C.c_double], "sor_order": [T.c_double_p, T.c_int_p, C.c_double],
    "sor_cf": [T.c_double_p, T.c_int_p, C.c_int, C.c_double]}


def protos(L):
    for name, extra in ENTRIES.items():
        f = getattr(L, "fasp_smoother_dstr_" + name)
        f.argtypes = [P(T.dSTRmat), P(T.dvector), P(T.dvector)] + extra
        f.restype = None
    return L


def _ip(mark):
    return None if mark is None else np.ascontiguousarray(mark, dtype=np.int32).ctypes.data_as(T.c_int_p)


def call(L, name, case, b, u0, order=None, mark=None, w=None, dinv=None):
    """fasp_smoother_dstr_<name> of library L on copies -> u."""
    A, keep = as_str(case)
    bb, u = np.array(b), np.array(u0)
    bv, uv = T.dvector(bb.size, T.dp(bb)), T.dvector(u.size, T.dp(u))
    mk = None if mark is None else np.ascontiguousarray(mark, dtype=np.int32)
    dv = None if dinv is None else T.dp(dinv)
    args = {"jacobi": [], "jacobi1": [dv], "gs": [order, _ip(mk)], "gs1": [order, _ip(mk), dv], "gs_ascend": [dv], "gs_descend": [dv],
            "gs_order": [dv, _ip(mk)], "gs_cf": [dv, _ip(mk), order], "sor": [order, _ip(mk), w], "sor1": [order, _ip(mk), dv, w],
            "sor_ascend": [dv, w], "sor_descend": [dv, w], "sor_order": [dv, _ip(mk), w], "sor_cf": [dv, _ip(mk), order, w]}[name]
    getattr(L, "fasp_smoother_dstr_" + name)(C.byref(A), C.byref(bv), C.byref(uv), *args)
    return u


def dinv_of(L, case):
    """The inverted diagonal blocks as library L's own smoothers form them (fasp_smat_inv; ours: through fasp_dbsr_getdiaginv), None for nc = 1."""
    nc = case["nc"]
    if nc == 1:
        return None
    if hasattr(L, "fasp_smat_inv"):
        return S.ref_dinv(S.ref_protos(L), nc, np.asarray(case["diag"]))
    n = ngrid_of(case)
    D, keep = T.as_bsr(np.arange(n + 1), np.arange(n), np.asarray(case["diag"]), nc)
    v = L.fasp_dbsr_getdiaginv(C.byref(D))
    return np.ctypeslib.as_array(v.val, shape=(v.row,)).copy()


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).digest(), dtype=np.uint8)


# ---- host cases (tests/test_str_smoother_host.py, recorded in tests/golden/str_smoother.npz) -----------------------------------------------
HOST_GRIDS = ((5, 4, 3), (9, 7, 1), (1, 8, 6))
HOST_NC = (1, 2, 3, 4, 5, 6, 7)


def variants(grid):
    """(key, entry, kind, order, mark, w, cf_entry): every variant and order of the file on one grid."""
    rb, pm = red_black(grid), partial_marks(grid)
    rev, rnd = permutation(grid, "reversed"), permutation(grid, "random")
    out = [("jacobi", "jacobi", JACOBI, None, None, None, False)]
    for kind, fam, ws in ((GS, "gs", (None,)), (SOR, "sor", WEIGHTS)):
        for w in ws:
            t = "" if w is None else f"_w{w}"
            out += [(f"{fam}_ascend{t}", f"{fam}_ascend", kind, ASCEND, None, w, False),
                    (f"{fam}_descend{t}", f"{fam}_descend", kind, DESCEND, None, w, False),
                    (f"{fam}_order_rev{t}", f"{fam}_order", kind, USERDEFINED, rev, w, False),
                    (f"{fam}_order_rnd{t}", f"{fam}_order", kind, USERDEFINED, rnd, w, False),
                    (f"{fam}_cf_rb_c{t}", f"{fam}_cf", kind, CPFIRST, rb, w, True),
                    (f"{fam}_cf_rb_f{t}", f"{fam}_cf", kind, FPFIRST, rb, w, True),
                    (f"{fam}_cf_part_c{t}", f"{fam}_cf", kind, CPFIRST, pm, w, True),
                    (f"{fam}_cf_part_f{t}", f"{fam}_cf", kind, FPFIRST, pm, w, True)]
    return out


def host_cases():
    """(key, case, variant)"""
    out = []
    for grid in HOST_GRIDS:
        for nc in HOST_NC:
            c = grid_case(grid, nc)
            for v in variants(grid):
                out.append((f"{c['name']}/{v[0]}", c, v))
    return out
