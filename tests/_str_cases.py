"""Structured-matrix (dSTRmat) cases shared by tools/gen_golden_str.py and the STR tests: seeded inputs, the reference's four arithmetic
forms restated in numpy (BlaSpmvSTR.c) and the calls into the compiled reference.

A case is a dict(name, nx, ny, nz, nc, offsets, form): `form` is what fasp_hip_str_form must say (0 S, 1 B, 2 N, 3 G).
Nothing here calls the reference's fasp_blas_dstr_mxv or a reference fasp_solver_dstr_* with nc > 1: its mxv clears ngrid*nc*nc doubles
of a vector of ngrid*nc (BlaSpmvSTR.c:135)."""
import ctypes as C
import hashlib
import os
import zlib

import numpy as np

from _libs import ROOT, T

GOLDEN = os.path.join(ROOT, "tests", "golden", "str_cases.npz")
DATA_FILE = os.path.join(ROOT, "tests", "golden", "data", "str_5x4x3_nc2.dat")
ALPHAS = (1.0, -1.0, 0.37, "mxv", 0.0)   # "mxv": y = A x (alpha = 1 on zeros)
FORM_S, FORM_B, FORM_N, FORM_G = 0, 1, 2, 3


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _canon_form(nc):
    return FORM_S if nc == 1 else FORM_B if nc in (3, 5) else FORM_N


def _case(kind, grid, nc, offsets, form):
    nx, ny, nz = grid
    name = f"{kind}_{nx}x{ny}x{nz}_nc{nc}"
    offsets = [int(o) for o in _rng(name + "/order").permutation(offsets)]   # stored scrambled
    # the reference's block texts of the 2D product start their middle loop at nx where they mean nline (BlaSpmvSTR.c:701, :906, :1062):
    # with nx == 1 they visit rows 1 .. nline-1 twice and read before the start of the -nline band and of x.  Such a call is never made;
    # the case is held to the restated form (model_aAxpy), which every other case proves against the reference bit for bit.
    ref_ok = not (kind == "c2d" and nx == 1 and nc > 1)
    return dict(name=name, nx=nx, ny=ny, nz=nz, nc=nc, offsets=offsets, form=form, ref_ok=ref_ok)


def op_cases():
    out = []
    for grid in ((5, 4, 3), (37, 11, 7)):   # 3D canonical
        nx, nxy = grid[0], grid[0] * grid[1]
        for nc in (1, 2, 3, 5, 7):
            out.append(_case("c3d", grid, nc, [-1, 1, -nx, nx, -nxy, nxy], _canon_form(nc)))
    for grid in ((7, 5, 1), (1, 6, 5)):     # 2D canonical; the second has nline = ny
        nline = grid[1] if grid[0] == 1 else grid[0]
        for nc in (1, 3, 2):
            out.append(_case("c2d", grid, nc, [-1, 1, -nline, nline], _canon_form(nc)))
    grid, nx, nxy, ngrid = (5, 4, 3), 5, 20, 60
    for nc in (1, 3):                       # the generic path
        out.append(_case("g0", grid, nc, [], FORM_G))
        out.append(_case("g2", grid, nc, [-1, 1], FORM_G))
        out.append(_case("g8", grid, nc, [-1, 1, -nx, nx, -nxy, nxy, nx + 1, -(nx - 1)], FORM_G))
        out.append(_case("g6warn", grid, nc, [-1, 1, -nx, nx, -nxy, nxy - 1], FORM_G))   # the reference's warning path
        out.append(_case("gfar", grid, nc, [-1, ngrid + 15, 1], FORM_G))                 # a legal, empty band
    return out


def form_only_cases():
    """Matrices whose form is asked but whose product is never compared: the reference reads out of bounds on grids that fail
    its non-overlap condition."""
    return [
        dict(name="deg3d", nx=3, ny=2, nz=1, nc=1, offsets=[-1, 1, -3, 3, -6, 6], form=FORM_G),   # ngrid 6 < 2 nxy
        dict(name="deg2d", nx=7, ny=1, nz=1, nc=3, offsets=[-1, 1, -7, 7], form=FORM_G),          # ngrid 7 < 2 nline
        dict(name="c3d_min", nx=2, ny=2, nz=2, nc=1, offsets=[1, -1, 2, -2, 4, -4], form=FORM_S),  # ngrid = 2 nxy exactly
        dict(name="c2d_nc4", nx=3, ny=2, nz=1, nc=4, offsets=[3, -3, 1, -1], form=FORM_N),
        dict(name="c2d_in3d", nx=4, ny=3, nz=2, nc=5, offsets=[-4, 4, -1, 1], form=FORM_B),       # a 2D stencil on a 3D grid
        dict(name="g4_other", nx=4, ny=3, nz=2, nc=1, offsets=[-1, 1, -12, 12], form=FORM_G),     # nband 4, not {+-1, +-nx}
    ]


def build(case):
    """The arrays of a case: (diag, bands).  Seeded standard normal."""
    r = _rng(case["name"] + "/values")
    ngrid, nc2 = case["nx"] * case["ny"] * case["nz"], case["nc"] ** 2
    diag = r.standard_normal(ngrid * nc2)
    bands = [r.standard_normal(max(ngrid - abs(o), 0) * nc2) for o in case["offsets"]]
    return diag, bands


def vectors(case):
    r = _rng(case["name"] + "/vectors")
    n = case["nx"] * case["ny"] * case["nz"] * case["nc"]
    return r.standard_normal(n), r.standard_normal(n)   # x, y0


def as_str(case, diag, bands):
    return T.as_str(case["nx"], case["ny"], case["nz"], case["nc"], case["offsets"], diag, bands)


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).digest(), dtype=np.uint8)


# ---- the four forms in numpy: rows are independent, so one vector operation per band keeps every row's own order ---------
def _terms(case, diag, bands, order):
    """(offset, blocks[ngrid, nc, nc] aligned to the row, exists[ngrid]) for the diagonal (None) and the bands in `order`."""
    ngrid, nc = case["nx"] * case["ny"] * case["nz"], case["nc"]
    for b in order:
        off = 0 if b is None else case["offsets"][b]
        src = diag if b is None else bands[b]
        full = np.zeros((ngrid, nc, nc))
        ex = np.zeros(ngrid, dtype=bool)
        m = ngrid - abs(off)
        if m > 0:
            lo = -off if off < 0 else 0   # a lower band is stored by column
            full[lo:lo + m] = src.reshape(m, nc, nc)
            ex[lo:lo + m] = True
        yield off, full, ex


def model_aAxpy(case, diag, bands, alpha, x, y0):
    """y = alpha A x + y0 with the arithmetic of the form case['form'] (alpha == 'mxv': alpha 1 on zeros)."""
    ngrid, nc, form = case["nx"] * case["ny"] * case["nz"], case["nc"], case["form"]
    if alpha == "mxv":
        alpha, y0 = 1.0, np.zeros(ngrid * nc)
    alpha = np.float64(alpha)
    y = y0.reshape(ngrid, nc).copy()
    xg = x.reshape(ngrid, nc)
    offs = case["offsets"]
    if form == FORM_G:
        if alpha == 0.0:
            return y.reshape(-1)
        order = [None] + list(range(len(offs)))
        y = y * (np.float64(1.0) / alpha)
    else:
        asc = sorted(range(len(offs)), key=lambda b: offs[b])
        order = asc[:len(asc) // 2] + [None] + asc[len(asc) // 2:]
    t = np.zeros(ngrid)
    have = np.zeros(ngrid, dtype=bool)
    for off, a, ex in _terms(case, diag, bands, order):
        idx = np.clip(np.arange(ngrid) + off, 0, ngrid - 1)
        xs = xg[idx]                       # x of the neighbour block (unused where the term does not exist)
        if form == FORM_S:
            p = a[:, 0, 0] * xs[:, 0]
            t = np.where(ex, np.where(have, t + p, p), t)
            have |= ex
        elif form == FORM_B:
            s = a[:, :, 0] * xs[:, None, 0]
            for q in range(1, nc):
                s = s + a[:, :, q] * xs[:, None, q]
            y = np.where(ex[:, None], y + alpha * s, y)
        elif form == FORM_N:
            for q in range(nc):
                y = np.where(ex[:, None], y + (alpha * a[:, :, q]) * xs[:, None, q], y)
        else:
            for q in range(nc):
                y = np.where(ex[:, None], y + a[:, :, q] * xs[:, None, q], y)
    if form == FORM_S:
        y = y + (alpha * t)[:, None]
    if form == FORM_G:
        y = y * alpha
    return y.reshape(-1)


def model_dinv_apply(nc, dinv, r):
    """fasp_precond_dstr_diag: fasp_blas_smat_mxv sums from the first product for nc = 2, 3, 4, 5, 7, from 0.0 otherwise."""
    m = dinv.size // (nc * nc)
    D, rr = dinv.reshape(m, nc, nc), r.reshape(m, nc)
    s = D[:, :, 0] * rr[:, None, 0]
    if nc not in (2, 3, 4, 5, 7):
        s = 0.0 + s
    for q in range(1, nc):
        s = s + D[:, :, q] * rr[:, None, q]
    return s.reshape(-1)


DINV_NC = (1, 2, 3, 5, 7)


def dinv_inputs(nc):
    """fasp_precond_dstr_diag on 5 x 4 x 3: (diagonal blocks to invert, r)."""
    r = _rng(f"dinv/{nc}")
    ngrid = 60
    diag = (r.standard_normal((ngrid, nc, nc)) + 3.0 * np.eye(nc)[None]).reshape(-1)
    return diag, r.standard_normal(ngrid * nc)


def mxv_longdouble(case, diag, bands, x):
    ngrid, nc = case["nx"] * case["ny"] * case["nz"], case["nc"]
    y = np.zeros((ngrid, nc), dtype=np.longdouble)
    xg = x.reshape(ngrid, nc).astype(np.longdouble)
    for off, a, ex in _terms(case, diag, bands, [None] + list(range(len(case["offsets"])))):
        idx = np.clip(np.arange(ngrid) + off, 0, ngrid - 1)
        y += np.where(ex[:, None], np.einsum("ipq,iq->ip", a.astype(np.longdouble), xg[idx]), 0)
    return y.reshape(-1)


# ---- the compiled reference -------------------------------------------------------------------------------------------------
def ref_protos(R):
    P = C.POINTER
    R.fasp_blas_dstr_aAxpy.argtypes = [C.c_double, P(T.dSTRmat), T.c_double_p, T.c_double_p]
    R.fasp_blas_dstr_aAxpy.restype = None
    R.fasp_format_dstr_dcsr.argtypes = [P(T.dSTRmat), P(T.dCSRmat)]
    R.fasp_format_dstr_dbsr.argtypes = [P(T.dSTRmat)]
    R.fasp_format_dstr_dbsr.restype = T.dBSRmat
    R.fasp_precond_dstr_diag.argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
    R.fasp_precond_dstr_diag.restype = None
    R.fasp_solver_dstr_krylov.argtypes = [P(T.dSTRmat), P(T.dvector), P(T.dvector), P(T.ITS_param)]
    R.fasp_solver_dstr_krylov_diag.argtypes = R.fasp_solver_dstr_krylov.argtypes
    R.fasp_solver_dstr_pminres.argtypes = [P(T.dSTRmat), P(T.dvector), P(T.dvector), P(T.precond), C.c_double, C.c_double,
                                           C.c_int, C.c_short, C.c_short]
    R.fasp_solver_dbsr_krylov_diag.argtypes = [P(T.dBSRmat), P(T.dvector), P(T.dvector), P(T.ITS_param)]
    R.fasp_smat_inv.argtypes = [T.c_double_p, C.c_int]
    R.fasp_smat_inv.restype = C.c_short
    R.fasp_dstr_write.argtypes = [C.c_char_p, P(T.dSTRmat)]
    R.fasp_dstr_write.restype = None
    return R


def ref_aAxpy(R, case, diag, bands, alpha, x, y0):
    """The reference's product; alpha == 'mxv' is its aAxpy(1.0) onto a cleared y, which is what its mxv computes."""
    A, keep = as_str(case, diag, bands)
    y = np.zeros_like(y0) if alpha == "mxv" else y0.copy()
    R.fasp_blas_dstr_aAxpy(1.0 if alpha == "mxv" else alpha, C.byref(A), T.dp(x), T.dp(y))
    return y


def ref_dinv(R, nc, diag):
    d = diag.copy()
    for i in range(d.size // (nc * nc)):
        blk = np.ascontiguousarray(d[i * nc * nc:(i + 1) * nc * nc])
        R.fasp_smat_inv(T.dp(blk), nc)
        d[i * nc * nc:(i + 1) * nc * nc] = blk
    return d


# ---- solve cases ------------------------------------------------------------------------------------------------------------
SOLVE_GRID = (9, 8, 7)
BLOCK_GRID = (6, 5, 4)
TOL = 1e-8


def scalar_system(sym):
    """7-band scalar matrix on 9 x 8 x 7: a variable-coefficient diffusion operator (SPD), plus first-order upwinded convection when
    not `sym`.  The stored zeros carry the grid lines.  Returns (case, diag, bands, b).

    The reaction term (0.05 symmetric, 0.5 with convection) is chosen on the CPU, from the reference alone: a case is fit for the pin
    "equal iteration counts, max|dx| <= 1e-9 max|x|" only if the reference's own count does not move when b is perturbed in its last
    bits -- a device sums its dot products in another order, which is such a perturbation.  Over 20 perturbations b (1 + 1e-15 N(0,1)),
    with 0.05 the reference's BiCGstab on the convection matrix takes 49, 50 or 51 iterations and x moves by 3.3e-8 of its size; with
    0.5 every method keeps its count (BiCGstab 35 / 27 without / with the diagonal preconditioner, GMRES(10) and VGMRES 62 / 57: six
    restart cycles) and x moves by at most 3.6e-13.  The symmetric matrix with 0.05: CG and MinRes keep their counts (83 / 72 and 83 / 71)
    and x moves by at most 2.3e-10 without a preconditioner, 1.7e-14 with the diagonal one."""
    nx, ny, nz = SOLVE_GRID
    nxy, ngrid = nx * ny, nx * ny * nz
    name = "spd" if sym else "upwind"
    r = _rng("solve/" + name)
    i = np.arange(ngrid)
    ix, iy, iz = i % nx, (i // nx) % ny, i // nxy
    diag = np.full(ngrid, 0.05 if sym else 0.5)
    bands, offsets = {}, [-1, 1, -nx, nx, -nxy, nxy]
    vel = {1: 0.0 if sym else 0.9, nx: 0.0 if sym else 0.5, nxy: 0.0 if sym else 0.3}
    for d, inside in ((1, ix < nx - 1), (nx, iy < ny - 1), (nxy, iz < nz - 1)):
        k = np.where(inside, np.exp(r.uniform(-1.0, 1.0, ngrid)), 0.0)[:ngrid - d]   # conductance of the face between i and i + d
        up = -k.copy()                         # A(i, i + d)
        lo = -k - np.where(k > 0, vel[d], 0)   # A(i + d, i): flow in the +d direction, upwinded
        diag[:ngrid - d] += k
        diag[d:] += k + np.where(k > 0, vel[d], 0)
        bands[d], bands[-d] = up, lo
    order = [int(o) for o in _rng("solve/order").permutation(offsets)]
    case = dict(name="solve_" + name, nx=nx, ny=ny, nz=nz, nc=1, offsets=order, form=FORM_S)
    return case, diag, [bands[o] for o in order], r.standard_normal(ngrid)


def block_system(nc, sym):
    """Block 7-band matrix on 6 x 5 x 4 with dominant diagonal blocks (symmetric when `sym`).  Returns (case, diag, bands, b)."""
    nx, ny, nz = BLOCK_GRID
    nxy, ngrid = nx * ny, nx * ny * nz
    name = f"block{nc}_{'sym' if sym else 'gen'}"
    r = _rng("solve/" + name)
    i = np.arange(ngrid)
    inside = {1: i % nx < nx - 1, nx: (i // nx) % ny < ny - 1, nxy: i // nxy < nz - 1}
    bands = {}
    for d in (1, nx, nxy):
        up = r.standard_normal((ngrid, nc, nc)) * inside[d][:, None, None]
        up = up[:ngrid - d]
        lo = np.transpose(up, (0, 2, 1)) if sym else r.standard_normal((ngrid, nc, nc))[:ngrid - d] * inside[d][:ngrid - d, None, None]
        bands[d], bands[-d] = up, lo
    dg = r.standard_normal((ngrid, nc, nc))
    if sym:
        dg = dg + np.transpose(dg, (0, 2, 1))
    # the shift of the diagonal blocks is chosen so that the reference's BSR solvers take 10 to 30 iterations (checked on the CPU:
    # CG 17 / 13 / 11, BiCGstab 14 / 13 / 12, GMRES(10) and VGMRES 25 / 24 / 21 for nc = 2 / 3 / 5)
    dg = dg + (6.0 if sym else {2: 3.5, 3: 3.0, 5: 2.5}[nc]) * nc * np.eye(nc)[None]
    offsets = [-1, 1, -nx, nx, -nxy, nxy]
    order = [int(o) for o in _rng("solve/order").permutation(offsets)]
    case = dict(name="solve_" + name, nx=nx, ny=ny, nz=nz, nc=nc, offsets=order, form=_canon_form(nc))
    return case, dg.reshape(-1), [np.ascontiguousarray(bands[o]).reshape(-1) for o in order], r.standard_normal(ngrid * nc)


SCALAR_SOLVES = [   # (key, symmetric system, method, restart)
    ("cg", True, T.SOLVER_CG, 25), ("bicgstab", False, T.SOLVER_BiCGstab, 25), ("gmres", False, T.SOLVER_GMRES, 10),
    ("vgmres", False, T.SOLVER_VGMRES, 10)]
BLOCK_SOLVES = [("cg", True, T.SOLVER_CG, 25), ("bicgstab", False, T.SOLVER_BiCGstab, 25), ("gmres", False, T.SOLVER_GMRES, 10),
                ("vgmres", False, T.SOLVER_VGMRES, 10)]
BLOCK_NC = (2, 3, 5)


def its_param(method, restart, maxit=500):
    p = T.ITS_param()
    p.print_level = 0; p.itsolver_type = method; p.decoup_type = 0; p.precond_type = 0; p.stop_type = T.STOP_REL_RES
    p.restart = restart; p.maxit = maxit; p.tol = TOL; p.abstol = 1e-18
    return p


def solve_with(L, entry, case, diag, bands, b, method, restart):
    """Iterations and x of `entry` (fasp_solver_dstr_krylov / _krylov_diag of L: the product or the reference) from a zero guess."""
    A, keep = as_str(case, diag, bands)
    x = np.zeros_like(b)
    bv, kb = T.as_vec(b)
    xv = T.dvector(x.size, T.dp(x))
    p = its_param(method, restart)
    st = getattr(L, entry)(C.byref(A), C.byref(bv), C.byref(xv), C.byref(p))
    return st, x


def minres_with(L, case, diag, bands, b, dinv):
    """fasp_solver_dstr_pminres of L without a preconditioner (dinv None) or with {fasp_precond_dstr_diag, &precond_diag_str}."""
    A, keep = as_str(case, diag, bands)
    x = np.zeros_like(b)
    bv, kb = T.as_vec(b)
    xv = T.dvector(x.size, T.dp(x))
    pc = None
    if dinv is not None:
        dd = T.precond_diag_str(case["nc"], T.dvector(dinv.size, T.dp(dinv)))
        pc = T.precond(C.cast(C.pointer(dd), C.c_void_p), C.cast(L.fasp_precond_dstr_diag, T.PRECOND_FCT))
    st = L.fasp_solver_dstr_pminres(C.byref(A), C.byref(bv), C.byref(xv), C.byref(pc) if pc is not None else None,
                                    TOL, 1e-18, 500, T.STOP_REL_RES, 0)
    return st, x


def ref_bsr_krylov_diag(R, case, diag, bands, b, method, restart):
    """The reference's BSR solve of the converted matrix with its block-diagonal preconditioner."""
    A, keep = as_str(case, diag, bands)
    B = R.fasp_format_dstr_dbsr(C.byref(A))
    x = np.zeros_like(b)
    bv, kb = T.as_vec(b)
    xv = T.dvector(x.size, T.dp(x))
    p = its_param(method, restart)
    st = R.fasp_solver_dbsr_krylov_diag(C.byref(B), C.byref(bv), C.byref(xv), C.byref(p))
    return st, x


def true_relres(case, diag, bands, b, x):
    r = b.astype(np.longdouble) - mxv_longdouble(case, diag, bands, x)
    return float(np.sqrt(np.sum(r * r)) / np.sqrt(np.sum(b.astype(np.longdouble) ** 2)))
