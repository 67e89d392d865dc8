"""Structured ILU(0) / ILU(1) cases shared by tools/gen_golden_str_ilu.py and the structured-ILU tests: seeded grid-derived matrices, the
calls that factor them (the library's or the compiled reference's fasp_ilu_dstr_setup0 / _setup1), snapshots of a factor as numpy arrays,
and the solve systems.

A case is a dict(name, nx, ny, nz, nc, offsets, diag, bands).  The matrices are grid-derived: the entries of a band that would couple two
grid points across the end of a line or of a plane are zero, as in a real discretisation; everything else is standard normal and
non-symmetric, the diagonal blocks shifted by (nband + 1) nc so that the factorisation stays well conditioned."""
import ctypes as C
import hashlib
import os
import zlib

import numpy as np

import _str_cases as S
from _libs import ROOT, T

GOLDEN = os.path.join(ROOT, "tests", "golden", "str_ilu.npz")
P = C.POINTER


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def lines(nx, ny, nz):
    """(nline, nplane) by the reference's rule (BlaILUSetupSTR.c:63)."""
    ngrid = nx * ny * nz
    if nx == 1:
        return ny, ngrid
    if ny == 1 or nz == 1:
        return nx, ngrid
    return nx, nx * ny


def geometry(nx, ny, nz):
    """(gx, gy, gz): the grid as the factorisation sees it -- lines of gx points, gy lines per plane, gz planes."""
    nline, nplane = lines(nx, ny, nz)
    ngrid = nx * ny * nz
    return nline, nplane // nline, ngrid // nplane


def canonical_offsets(nx, ny, nz, nband):
    nline, nplane = lines(nx, ny, nz)
    return [-1, 1, -nline, nline, -nplane, nplane][:nband]


def grid_case(grid, nc, order=None, tag=""):
    """Random grid-derived matrix on `grid` with nc x nc blocks: 6 bands on a 3-D grid, 4 on a 2-D one, stored in canonical order or
    in `order` (a permutation of range(nband))."""
    nx, ny, nz = grid
    gx, gy, gz = geometry(nx, ny, nz)
    nband = 6 if gz > 1 else 4
    ngrid, nc2 = nx * ny * nz, nc * nc
    name = f"ilu_{nx}x{ny}x{nz}_nc{nc}{tag}"
    r = _rng(name)
    i = np.arange(ngrid)
    inside = {1: i % gx < gx - 1, gx: (i // gx) % gy < gy - 1, gx * gy: i // (gx * gy) < gz - 1}   # the point i + d is i's neighbour
    canon = canonical_offsets(nx, ny, nz, nband)
    diag = (r.standard_normal((ngrid, nc, nc)) + (nband + 1.0) * nc * np.eye(nc)[None]).reshape(-1)
    bands = {}
    for o in canon:
        d = abs(o)
        blk = r.standard_normal((ngrid, nc, nc)) * inside[d][:, None, None]   # indexed by the lower of the two points, as both bands are stored
        bands[o] = np.ascontiguousarray(blk[:ngrid - d]).reshape(-1)
    order = list(range(nband)) if order is None else list(order)
    offsets = [canon[k] for k in order]
    return dict(name=name, nx=nx, ny=ny, nz=nz, nc=nc, offsets=offsets, diag=diag, bands=[bands[o] for o in offsets])


def as_str(case):
    return T.as_str(case["nx"], case["ny"], case["nz"], case["nc"], case["offsets"], case["diag"], case["bands"])


def protos(L):
    """Prototypes of the structured-ILU entries on a library (ours or the compiled reference)."""
    for f in ("fasp_ilu_dstr_setup0", "fasp_ilu_dstr_setup1"):
        getattr(L, f).argtypes = [P(T.dSTRmat), P(T.dSTRmat)]
        getattr(L, f).restype = None
    for f in ("fasp_precond_dstr_ilu0", "fasp_precond_dstr_ilu1"):
        getattr(L, f).argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
        getattr(L, f).restype = None
    L.fasp_dstr_free.argtypes = [P(T.dSTRmat)]
    L.fasp_dstr_free.restype = None
    L.fasp_solver_dstr_krylov_ilu.argtypes = [P(T.dSTRmat), P(T.dvector), P(T.dvector), P(T.ITS_param), P(T.ILU_param)]
    L.fasp_solver_dstr_krylov_ilu.restype = C.c_int
    return L


def snapshot(LU):
    """A factor as numpy copies: dict(nx, ny, nz, nxy, nc, ngrid, nband, offsets, diag, bands)."""
    nc2 = LU.nc * LU.nc
    offsets = [int(LU.offsets[b]) for b in range(LU.nband)]
    bands = []
    for b, o in enumerate(offsets):
        m = max(LU.ngrid - abs(o), 0) * nc2
        bands.append(np.ctypeslib.as_array(LU.offdiag[b], shape=(m,)).copy() if m else np.zeros(0))
    diag = np.ctypeslib.as_array(LU.diag, shape=(LU.ngrid * nc2,)).copy()
    return dict(nx=LU.nx, ny=LU.ny, nz=LU.nz, nxy=LU.nxy, nc=LU.nc, ngrid=LU.ngrid, nband=LU.nband, offsets=offsets, diag=diag, bands=bands)


def factor(L, case, lfil):
    """fasp_ilu_dstr_setup<lfil> of library L -> snapshot (None when LU came back zeroed)."""
    A, keep = as_str(case)
    LU = T.dSTRmat()
    C.memset(C.byref(LU), 0x55, C.sizeof(LU))   # a refusal must clear it
    getattr(L, f"fasp_ilu_dstr_setup{lfil}")(C.byref(A), C.byref(LU))
    if LU.ngrid == 0 and not LU.diag:
        return None
    snap = snapshot(LU)
    L.fasp_dstr_free(C.byref(LU))
    return snap


def factor_struct(snap):
    """A dSTRmat over the arrays of a snapshot -> (struct, keepalive)."""
    A, keep = T.as_str(snap["nx"], snap["ny"], snap["nz"], snap["nc"], snap["offsets"], snap["diag"], snap["bands"])
    A.nxy = snap["nxy"]
    return A, keep


def factor_bytes(snap):
    return snap["diag"].tobytes() + b"".join(b.tobytes() for b in snap["bands"])


def digest(raw):
    return np.frombuffer(hashlib.sha256(raw).digest(), dtype=np.uint8)


def rhs(case):
    return _rng(case["name"] + "/rhs").standard_normal(case["nx"] * case["ny"] * case["nz"] * case["nc"])


def host_apply(L, snap, lfil, r):
    """fasp_precond_dstr_ilu<lfil> of library L on host vectors."""
    LU, keep = factor_struct(snap)
    z = np.full_like(r, np.nan)
    getattr(L, f"fasp_precond_dstr_ilu{lfil}")(T.dp(r.copy()), T.dp(z), C.cast(C.pointer(LU), C.c_void_p))
    return z


def _row_dot(B, x, nc):
    """(B x)_p summed left to right from the first product; nc = 6 (fasp_blas_smat_mxv's general text) from 0.0."""
    s = B[:, 0] * x[0]
    if nc == 6:
        s = 0.0 + s
    for q in range(1, nc):
        s = s + B[:, q] * x[q]
    return s


def model_apply(snap, lfil, r):
    """fasp_precond_dstr_ilu<lfil> restated in numpy, row after row: the arithmetic of the reference's general block text (PreSTR.c:278 /
    :716) for every nc > 1, its scalar text for nc = 1.  The reference's own texts for nc = 3, 5 and 7 subtract with
    fasp_blas_darray_axpy_nc3 / _nc5 / _nc7, which run over nc * nc entries: they read past the nc-entry product and write past the row
    (past the vector in the last rows), so their result depends on what the heap holds.  Those are never called; nc = 3, 5, 7 are held to this
    restatement, which nc = 2, 4, 6 prove against the reference bit for bit."""
    nc, m = snap["nc"], snap["ngrid"]
    nline, nplane = lines(snap["nx"], snap["ny"], snap["nz"])
    back = [1, nline, nplane] if lfil == 0 else [1, nline - 1, nline, nplane - nline, nplane - 1, nplane]
    d = snap["diag"].reshape(m, nc, nc)
    o = [b.reshape(-1, nc, nc) for b in snap["bands"]]
    zz = r.reshape(m, nc).copy()
    z = np.zeros((m, nc))
    for i in range(1, m):
        for k, bk in enumerate(back):
            if 2 * k < len(o) and i >= bk and (k == 0 or i - bk >= 0):
                zz[i] = zz[i] - _row_dot(o[2 * k][i - bk], zz[i - bk], nc)
    for i in range(m - 1, -1, -1):
        for k, bk in enumerate(back):
            if 2 * k + 1 < len(o) and i + bk < m:
                zz[i] = zz[i] - _row_dot(o[2 * k + 1][i], z[i + bk], nc)
        z[i] = zz[i] * d[i, 0] if nc == 1 else _row_dot(d[i], zz[i], nc)
    return z.reshape(-1)


REF_APPLY_OK = (1, 2, 4, 6)   # block sizes at which the reference's fasp_precond_dstr_ilu0 / _ilu1 stay inside their arrays


# ---- host cases (tests/test_str_ilu_host.py, recorded in tests/golden/str_ilu.npz) ----------------------------------------------------
HOST_GRIDS = ((5, 4, 3), (7, 6, 5), (9, 7, 1), (1, 8, 6))
HOST_NC = (1, 2, 3, 4, 5, 6, 7)
SWAPPED = [1, 0, 2, 3, 4, 5]   # +1 stored before -1: setup0 only (setup1 refuses it, the reference's setup1 would misread it)
WHOLE = 2000                   # factors of at most this many doubles are recorded whole, larger ones as SHA-256


def host_cases():
    """(key, case, lfils)"""
    out = []
    for grid in HOST_GRIDS:
        for nc in HOST_NC:
            c = grid_case(grid, nc)
            out.append((c["name"], c, (0, 1)))
    for grid in ((5, 4, 3), (9, 7, 1)):
        for nc in (1, 3):
            nband = 6 if grid[2] > 1 else 4
            c = grid_case(grid, nc, order=SWAPPED[:nband], tag="_swap")
            out.append((c["name"], c, (0,)))
    return out


APPLY_GRIDS = ((5, 4, 3), (9, 7, 1))   # fasp_precond_dstr_ilu0 / _ilu1 on host vectors, every nc


def model_setup0_nc1(case, quirk=True):
    """fasp_ilu_dstr_setup0 for nc = 1 in numpy scalars (canonical storage order).  quirk: the -nplane band of L is formed from the -1
    band of A, as BlaILUSetupSTR.c:144 has it; False: from the -nplane band, as one would expect."""
    nline, nplane = lines(case["nx"], case["ny"], case["nz"])
    ngrid = case["nx"] * case["ny"] * case["nz"]
    a = {o: b for o, b in zip(case["offsets"], case["bands"])}
    o = {k: a[k].copy() for k in a}
    diag = case["diag"]
    d = diag.copy()
    has_plane = -nplane in a and nplane < ngrid
    d[0] = np.float64(1.0) / d[0]
    for i in range(1, ngrid):
        o[-1][i - 1] = a[-1][i - 1] * d[i - 1]
        if i >= nline:
            o[-nline][i - nline] = a[-nline][i - nline] * d[i - nline]
        if has_plane and i >= nplane:
            o[-nplane][i - nplane] = (a[-1] if quirk else a[-nplane])[i - nplane] * d[i - nplane]
        d[i] = diag[i] - o[-1][i - 1] * o[1][i - 1]
        if i >= nline:
            d[i] = d[i] - o[-nline][i - nline] * o[nline][i - nline]
        if has_plane and i >= nplane:
            d[i] = d[i] - o[-nplane][i - nplane] * o[nplane][i - nplane]
        d[i] = np.float64(1.0) / d[i]
    return d, [o[k] for k in canonical_offsets(case["nx"], case["ny"], case["nz"], len(a))]


# ---- solve systems --------------------------------------------------------------------------------------------------------------------
TOL = S.TOL
SCALAR_SOLVES = S.SCALAR_SOLVES   # (key, symmetric system, method, restart): CG on the symmetric system, BiCGstab, GMRES, VGMRES on the other
BLOCK_SOLVES = S.BLOCK_SOLVES
BLOCK_NC = (2, 3, 5)
BLOCK_COUNT_NC = (2, 3)   # where the reference's BSR ILU(0) of the converted matrix is the structured ILU(0) to rounding (checked by the generator); nc = 5: setup0 inverts its pivots with fasp_smat_inv_nc5, whose closed form is not the inverse -- another factor
MARGIN = 1.05   # the reference's true relative residual is this factor away from tol at its last step and at the one before


def _canonical(case, diag, bands, b):
    canon = canonical_offsets(case["nx"], case["ny"], case["nz"], len(case["offsets"]))
    by = dict(zip(case["offsets"], bands))
    return dict(name=case["name"] + "_ilu", nx=case["nx"], ny=case["ny"], nz=case["nz"], nc=case["nc"], offsets=canon,
                diag=np.ascontiguousarray(diag), bands=[np.ascontiguousarray(by[o]) for o in canon]), b


SYM_GRID = (13, 11, 1)
SYM_REACTION = 0.05


def scalar_system(sym):
    """not sym: the 9 x 8 x 7 convection-diffusion system of _str_cases.scalar_system with its bands in canonical order
    (fasp_ilu_dstr_setup1 takes no other).  sym: a variable-coefficient diffusion operator (SPD) on the 2-D grid 13 x 11 -- on a 3-D grid
    the reference's scalar ILU(0) forms L's plane band from the -1 band of A (BlaILUSetupSTR.c:144), the preconditioner is then far from
    symmetric and the reference's own CG does not converge with it (checked on the CPU: 500 iterations, relative residual 1.7e-2, also
    for a constant-coefficient operator), so CG is held to a grid without plane bands."""
    if not sym:
        return _canonical(*S.scalar_system(False))
    nx, ny, nz = SYM_GRID
    ngrid = nx * ny
    r = _rng("solve/sym2d")
    i = np.arange(ngrid)
    diag = np.full(ngrid, SYM_REACTION)
    bands = {}
    for d, inside in ((1, i % nx < nx - 1), (nx, i // nx < ny - 1)):
        k = np.where(inside, np.exp(r.uniform(-1.0, 1.0, ngrid)), 0.0)[:ngrid - d]
        diag[:ngrid - d] += k
        diag[d:] += k
        bands[d], bands[-d] = -k, -k.copy()
    canon = canonical_offsets(nx, ny, nz, 4)
    return dict(name="solve_sym2d_ilu", nx=nx, ny=ny, nz=nz, nc=1, offsets=canon, diag=diag, bands=[bands[o] for o in canon]), r.standard_normal(ngrid)


def block_system(nc, sym):
    return _canonical(*S.block_system(nc, sym))


def ilu_param(lfil):
    p = T.ILU_param()
    p.print_level = 0; p.ILU_type = 1; p.ILU_lfil = lfil; p.ILU_droptol = 0.001; p.ILU_relax = 0.0; p.ILU_permtol = 0.0
    return p


def solve_ilu(L, case, b, method, restart, lfil, maxit=500):
    """fasp_solver_dstr_krylov_ilu of L (the library or the reference) from a zero guess -> (status, x)."""
    A, keep = as_str(case)
    x = np.zeros_like(b)
    bv, kb = T.as_vec(b)
    xv = T.dvector(x.size, T.dp(x))
    p = S.its_param(method, restart, maxit)
    ip = ilu_param(lfil)
    return L.fasp_solver_dstr_krylov_ilu(C.byref(A), C.byref(bv), C.byref(xv), C.byref(p), C.byref(ip)), x


def true_relres(case, b, x):
    return S.true_relres(dict(case, form=0), case["diag"], case["bands"], b, x)
