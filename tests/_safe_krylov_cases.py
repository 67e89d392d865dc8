"""The cases of the safe-net Krylov solvers (fasp_solver_d{csr,bsr,str}_sp*, fasp_solver_dcsr_itsolver_s), shared by
tools/gen_golden_safe_krylov.py (which runs them through the compiled reference and records what qualifies) and the tests.

Matrices are built in numpy and are deterministic.  A case is a dict(key, fmt, method, matrix, pc, stop, tol, maxit, restart, kind):
  kind "conv"     a converged solve (the recorded return code is an iteration count)
       "maxit"    an exit at MaxIt (ERROR_SOLVER_MAXIT), where the RESTORE_BESTSOL block decides between the last and the best iterate
       "nan"      the diagonal preconditioner writes a NaN into one entry of z at its ninth call
  pc   None, "diag" (a host callback z = r / diag(A), block-wise for the block formats) or "nan" (the same with the NaN)
The right-hand side of a case is seeded by its matrix's name; perturbed(b, key) is the second right-hand side `sens` is measured with."""
import ctypes as C
import functools
import os
import zlib

import numpy as np

from _libs import ROOT, T, B3

GOLDEN = os.path.join(ROOT, "tests", "golden", "safe_krylov.npz")
TOL = 1e-8
SENS_MAX = 1e-8            # a case qualifies only if the reference's own x moves by no more than this under perturbed(b)
NAN_CALL = 9               # the preconditioner call that writes the NaN ...
NAN_ENTRY = 3              # ... into this entry of z
METHODS = {"spcg": T.SOLVER_CG, "spbcgs": T.SOLVER_BiCGstab, "spminres": T.SOLVER_MinRes, "spgmres": T.SOLVER_GMRES,
           "spvgmres": T.SOLVER_VGMRES}
FORMATS = {"csr": tuple(METHODS), "bsr": ("spbcgs", "spgmres", "spvgmres"), "str": tuple(METHODS)}   # what the reference has
SYMMETRIC = ("spcg", "spminres")   # methods that need a symmetric matrix


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ---- matrices ---------------------------------------------------------------------------------------------------------------
def stencil7(n, kx=1.0, ky=1.0, kz=1.0, shift=0.0, scale=0.0, name=""):
    """7-point operator on an n^3 grid with Dirichlet walls as (diag[n^3], {offset: band}) in the layout of a dSTRmat (a lower band is
    indexed by its column; entries across a grid line are stored zeros): -k between neighbours, 2 (kx + ky + kz) on the diagonal;
    shift > 0 adds first-order upwinded convection in +x (the Peclet shift: `shift` more on the diagonal and on the west neighbour);
    scale > 0 applies the symmetric scaling D A D, D = 10^(scale xi), xi uniform in [-1, 1] and seeded by `name`."""
    N = n * n * n
    i = np.arange(N)
    inside = {1: i % n < n - 1, n: (i // n) % n < n - 1, n * n: i // (n * n) < n - 1}
    diag = np.full(N, 2.0 * (kx + ky + kz))
    bands = {}
    for d, k in ((1, kx), (n, ky), (n * n, kz)):
        up = np.where(inside[d], -k, 0.0)[:N - d]     # A(i, i + d)
        lo = up.copy()                                # A(i + d, i)
        if d == 1 and shift:
            lo = lo - np.where(up != 0.0, shift, 0.0)
            diag[1:] += np.where(up != 0.0, shift, 0.0)
        bands[d], bands[-d] = up, lo
    if scale:
        D = 10.0 ** (scale * _rng(name + "/scale").uniform(-1.0, 1.0, N))
        diag = diag * D * D
        for d in (1, n, n * n):
            bands[d] = bands[d] * D[:N - d] * D[d:]
            bands[-d] = bands[-d] * D[d:] * D[:N - d]
    return diag, bands


def bands_to_csr(n, diag, bands):
    """CSR (sorted columns, no stored zeros) of a stencil7 operator."""
    N = len(diag)
    rows, cols, vals = [np.arange(N)], [np.arange(N)], [diag]
    for d in (1, n, n * n):
        k = np.flatnonzero(bands[d] != 0.0)
        rows += [k, k + d]; cols += [k + d, k]; vals += [bands[d][k], bands[-d][k]]
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    ia = np.zeros(N + 1, dtype=np.int32)
    ia[1:] = np.cumsum(np.bincount(rows, minlength=N))
    return ia, cols[order].astype(np.int32), vals[order]


# name: (n, stencil7 keywords, seed of the scaling and of the right-hand side).  The seeds and the scaling exponents of the three operators
# the MaxIt exits run on were chosen on the CPU, from the reference alone: with them its safe CG restores iteration 1 of 5, its safe
# BiCGstab iteration 8 of 10 and its safe MinRes (diagonal preconditioner: without one its residual norm falls monotonically)
# iteration 14 of 15, and keeps doing so when b is perturbed in its last bits.
MATRICES = {
    "p7_5": (5, {}, "p7_5"), "p7_6": (6, {}, "p7_6"), "p7_11": (11, {}, "p7_11"),
    "aniso8": (8, dict(ky=0.1, kz=0.01, scale=1.0), "aniso8"), "aniso6": (6, dict(ky=0.1, kz=0.01, scale=2.0), "aniso6a"),
    "convdiff6": (6, dict(shift=4.0), "convdiff6n"),
}


@functools.lru_cache(maxsize=None)
def system(fmt, matrix):
    """The operator of a case and its right-hand side, read-only: dict(fmt, n (unknowns), b, dinv (inverse diagonal, blocks row-major),
    nb, and the arrays of the format: ia, ja, val (csr, bsr) or grid, offsets, diag, bands (str)).  bsr: the scalar matrix (x) B3;
    str with nc = 3 (matrix name + "_nc3"): the same blocks as bands; csr of such a name: the block matrix written out entry by entry
    (what the reference is given for it: its structured product overruns its output for nc > 1, BlaSpmvSTR.c:135)."""
    nc = 1
    base = matrix
    if matrix.endswith("_nc3"):
        base, nc = matrix[:-4], 3
    n, kw, seed = MATRICES[base]
    diag, bands = stencil7(n, name=seed, **kw)
    nb = 3 if fmt == "bsr" else nc
    S = dict(fmt=fmt, matrix=matrix, nb=nb)
    blk = B3 if nb == 3 else np.ones((1, 1))
    if fmt == "str":
        offsets = [-1, 1, -n, n, -n * n, n * n]
        S.update(grid=n, offsets=offsets, diag=(diag[:, None, None] * blk).reshape(-1),
                 bands=[(bands[o][:, None, None] * blk).reshape(-1) for o in offsets])
    else:
        ia, ja, val = bands_to_csr(n, diag, bands)
        val = (val[:, None, None] * blk).reshape(-1)
        if fmt == "csr" and nb > 1:   # scalar row i nb + r: the blocks of block row i, their rows r
            cnt = np.diff(ia)
            cols = ja[:, None] * nb + np.arange(nb)[None, :]   # the nb scalar columns of every block
            ja = np.concatenate([cols[ia[i]:ia[i + 1]].reshape(-1) for i in range(len(cnt)) for _ in range(nb)]).astype(np.int32)
            v3 = val.reshape(-1, nb, nb)
            val = np.concatenate([v3[ia[i]:ia[i + 1], r, :].reshape(-1) for i in range(len(cnt)) for r in range(nb)])
            ia = np.concatenate([[0], np.cumsum(np.repeat(cnt * nb, nb))]).astype(np.int32)
        S.update(ia=ia, ja=ja, val=val)
    S["n"] = len(diag) * nb
    S["dinv"] = (np.linalg.inv(blk)[None] / diag[:, None, None]).reshape(-1)
    S["b"] = _rng(seed + matrix[len(base):] + "/" + ("bsr" if fmt == "bsr" else "b")).standard_normal(S["n"])
    for v in S.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return S


def perturbed(b, key):
    """b with every entry multiplied by 1 + 1e-14 xi, xi uniform in [-1, 1], seeded by the case's key."""
    return b * (1.0 + 1e-14 * _rng(key + "/perturb").uniform(-1.0, 1.0, len(b)))


def as_matrix(S):
    """The ctypes struct of a system -> (struct, keepalive)."""
    if S["fmt"] == "csr":
        return T.as_csr(S["ia"].copy(), S["ja"].copy(), S["val"].copy())
    if S["fmt"] == "bsr":
        return T.as_bsr(S["ia"].copy(), S["ja"].copy(), S["val"].copy(), S["nb"])
    g = S["grid"]
    return T.as_str(g, g, g, S["nb"], list(S["offsets"]), S["diag"].copy(), [b.copy() for b in S["bands"]])


class DiagPrecond:
    """z = D^-1 r (block-wise) behind a ctypes callback: a precond whose fct no library recognises, so the product calls it on the host.
    nan_call > 0: call number nan_call (counted from 1) writes a NaN into entry NAN_ENTRY of z."""

    def __init__(self, S, nan_call=0):
        nb, n = S["nb"], S["n"]
        dinv = S["dinv"].reshape(-1, nb, nb)
        self.calls = 0

        def fct(r, z, data):
            self.calls += 1
            rv = np.ctypeslib.as_array(r, (n,)).reshape(-1, nb)
            zv = np.ctypeslib.as_array(z, (n,))
            zv[:] = np.einsum("ijk,ik->ij", dinv, rv).reshape(-1)
            if self.calls == nan_call:
                zv[NAN_ENTRY] = np.nan

        self._fct = T.PRECOND_FCT(fct)
        self.pc = T.precond(None, self._fct)


# ---- the case table ---------------------------------------------------------------------------------------------------------
def _matrix_for(fmt, method, kind):
    sym = method in SYMMETRIC
    if kind == "maxit":   # the exits of the issue's list, and the same operators in the other formats
        return {"spcg": "aniso8", "spbcgs": "convdiff6", "spminres": "aniso6"}.get(method)
    if fmt == "bsr":
        return "p7_6" if kind == "nan" else "convdiff6"
    if fmt == "str":
        return "p7_6" if sym else "convdiff6"
    return "p7_6" if sym else "convdiff6"


def _case(fmt, method, matrix, pc, stop, kind, maxit=500, tol=TOL, restart=20):
    key = f"{fmt}/{method}/{matrix}/{pc or 'none'}/stop{stop}/{kind}"
    return dict(key=key, fmt=fmt, method=method, matrix=matrix, pc=pc, stop=stop, tol=tol, maxit=maxit, restart=restart, kind=kind)


MAXIT_EXITS = {"spcg": 5, "spbcgs": 10, "spminres": 15}   # MaxIt of the kind "maxit" cases


def cases():
    out = []
    for fmt, methods in FORMATS.items():
        for method in methods:
            m = _matrix_for(fmt, method, "conv")
            for pc in (None, "diag"):
                for stop in (1, 2, 3):
                    out.append(_case(fmt, method, m, pc, stop, "conv"))
            if method in MAXIT_EXITS:
                out.append(_case(fmt, method, _matrix_for(fmt, method, "maxit"), "diag" if method == "spminres" else None, 1, "maxit",
                                 maxit=MAXIT_EXITS[method]))
            out.append(_case(fmt, method, _matrix_for(fmt, method, "nan"), "nan", 1, "nan", maxit=60))
    # the sizes: odd and under one block (125 rows), odd and several blocks (1331), and the block structured form
    for method in METHODS:
        sym = method in SYMMETRIC
        out.append(_case("csr", method, "p7_5", None, 1, "conv"))
        out.append(_case("csr", method, "p7_11", "diag", 1, "conv"))
        out.append(_case("str", method, "p7_6_nc3" if sym else "convdiff6_nc3", "diag", 1, "conv"))
    return out


# what the issue pins on the CPU: (key of the case, the restore line's iteration)
PINNED_RESTORES = {"csr/spcg/aniso8/none/stop1/maxit": 1, "csr/spbcgs/convdiff6/none/stop1/maxit": 8,
                   "csr/spminres/aniso6/diag/stop1/maxit": 14}
UNKNOWN_TYPES = (6, 7, 8, 13)   # itsolver_types fasp_solver_dcsr_itsolver_s refuses (VFGMRES, GCG, GCR, SMinRes)


def set_protos(L):
    """argtypes of the safe entries on a library that exports them (the product, or the compiled reference)."""
    P = C.POINTER
    V = P(T.dvector)
    for fmt, mat in (("csr", T.dCSRmat), ("bsr", T.dBSRmat), ("str", T.dSTRmat)):
        for m in FORMATS[fmt]:
            rs = [C.c_short] if m.endswith("gmres") else []
            getattr(L, f"fasp_solver_d{fmt}_{m}").argtypes = [P(mat), V, V, P(T.precond), C.c_double, C.c_int] + rs + [C.c_short, C.c_short]
    L.fasp_solver_dcsr_itsolver_s.argtypes = [P(T.dCSRmat), V, V, P(T.precond), P(T.ITS_param)]


def reference_case(case):
    """The case as the reference is given it: a structured matrix with nc > 1 goes as the scalar CSR matrix of the same entries."""
    if case["fmt"] == "str" and case["matrix"].endswith("_nc3"):
        return dict(case, fmt="csr")
    return case


def run(L, case, b=None, print_level=T.PRINT_MIN, via_itsolver=False):
    """The case through library L (set_protos applied) from a zero guess -> (return code, x, preconditioner calls).
    via_itsolver (csr only): through fasp_solver_dcsr_itsolver_s."""
    S = system(case["fmt"], case["matrix"])
    A, keep = as_matrix(S)
    b = np.array(S["b"] if b is None else b)
    x = np.zeros(S["n"])
    bv, _ = T.as_vec(b)
    xv = T.dvector(len(x), T.dp(x))
    D = DiagPrecond(S, NAN_CALL if case["pc"] == "nan" else 0) if case["pc"] else None
    pc = C.byref(D.pc) if D else None
    if via_itsolver:
        it = T.ITS_param()
        it.print_level = print_level; it.itsolver_type = METHODS[case["method"]]; it.stop_type = case["stop"]
        it.restart = case["restart"]; it.maxit = case["maxit"]; it.tol = case["tol"]; it.abstol = 0.0
        st = L.fasp_solver_dcsr_itsolver_s(C.byref(A), C.byref(bv), C.byref(xv), pc, C.byref(it))
    else:
        args = [C.byref(A), C.byref(bv), C.byref(xv), pc, case["tol"], case["maxit"]]
        if case["method"].endswith("gmres"):
            args.append(case["restart"])
        st = getattr(L, f"fasp_solver_d{case['fmt']}_{case['method']}")(*args, case["stop"], print_level)
    return st, x, (D.calls if D else 0)


def restore_iteration(text):
    """The iteration of the "Restore iteration" line in a library's output, or -1 when there is none."""
    import re
    m = re.search(r"Discard current iteration\. Restore iteration (\d+)!", text)
    return int(m.group(1)) if m else -1


class Captured:
    """What a C library prints on stdout while the block runs."""

    def __enter__(self):
        import sys
        import tempfile
        sys.stdout.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(1)
        os.dup2(self.tmp.fileno(), 1)
        return self

    def __exit__(self, *exc):
        C.CDLL(None).fflush(None)
        os.dup2(self.saved, 1); os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
