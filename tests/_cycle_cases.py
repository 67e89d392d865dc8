"""Inputs, configurations and tolerance rules shared by test_cycle_cases.py (CPU), test_gpu_level_smooth.py and
test_gpu_cycle_forms.py: the smoothers and cycle forms of the AMG preconditioner on levels P7(n) cannot stand in for.

Inputs (numpy only, seeded).  An 11 x 12 x 13 grid graph with random power-of-two edge weights, 2 % random long-range edges and a
small mass term, as a weighted graph Laplacian L.
  spd_scaled    S L S with S = random powers of two in [1/8, 8]: symmetric positive definite, the diagonal varies by
                three orders of magnitude, so D^-1 does not commute with A
  unsym_scaled  S (L + C) S with C a first-order upwind convection part: the same, and A != A^T by a good margin
  fe            the recorded csrmat_FE.dat
What each input is for is asserted where it is built (check_matrix) and, for the hierarchy the setup makes of it with
coarse_dof = 20, by check_hierarchy: at least five levels, no level size a multiple of 64.

Tolerances.  A device result is compared with the oracle's on the same level matrices.  The bar of a case is
max(floor, 8 x probe) relative to the largest entry of the oracle's result, where
  floor  1e-13 for a smoother application (the bar of test_jacobi_sweeps), 1e-9 for a cycle application or a short solve
         (the bar of test_precond_apply, which already absorbs the coarse CG's stop at 1e-10)
  probe  the largest relative change of the ORACLE's result, over three seeds, when every entry of its input vectors is
         moved by one relative 2^-52 step in a random direction: what the problem itself makes of one rounding.  The
         factor 8: the device sums a row of up to about 40 entries in another order, which a one-ulp change of the input
         under-models.
The caps are conditions on the case, not measurements: a smoother bar above 1e-10 or a cycle / solve bar above 1e-7 fails
the case whatever the device computes -- it then needs another seed or input, never a looser bar."""
import ctypes as C
import functools

import numpy as np

from _libs import T

GRID = (11, 12, 13)   # 1716 rows: a 12^3 grid would have 1728 = 27 x 64 of them, and no level is to be a multiple of the 64-row tile
N_ROWS = GRID[0] * GRID[1] * GRID[2]
SMOOTH_FLOOR, SMOOTH_CAP = 1e-13, 1e-10
CYCLE_FLOOR, CYCLE_CAP = 1e-9, 1e-7
PROBE_SEEDS = (1, 2, 3)
PROBE_FACTOR = 8.0


# --- the matrices ------------------------------------------------------------------------------------------------------
def _coo_to_csr(n, rows, cols, vals):
    """Sum duplicates, sort by (row, column) -> (ia, ja, a)."""
    key = rows.astype(np.int64) * n + cols.astype(np.int64)
    uniq, inv = np.unique(key, return_inverse=True)
    a = np.zeros(len(uniq))
    np.add.at(a, inv, vals)
    r = (uniq // n).astype(np.int32)
    ja = (uniq % n).astype(np.int32)
    ia = np.zeros(n + 1, dtype=np.int32)
    ia[1:] = np.cumsum(np.bincount(r, minlength=n))
    return ia, ja, a


def _graph(seed):
    """Edges (lo, hi, weight, axis) of the weighted grid graph; axis 3 marks the long-range edges."""
    rng = np.random.default_rng(seed)
    N = N_ROWS
    idx = np.arange(N).reshape(GRID)
    lo, hi, ax = [], [], []
    for axis in range(3):
        g = np.moveaxis(idx, axis, 0)
        lo.append(g[:-1].ravel()); hi.append(g[1:].ravel()); ax.append(np.full(g[:-1].size, axis))
    lo = np.concatenate(lo); hi = np.concatenate(hi); ax = np.concatenate(ax)
    w = 2.0 ** rng.integers(-2, 3, size=len(lo))
    m = int(round(0.02 * len(lo)))
    p = rng.integers(0, N, size=m)
    q = (p + 1 + rng.integers(0, N - 1, size=m)) % N          # q != p
    lo = np.concatenate([lo, np.minimum(p, q)]); hi = np.concatenate([hi, np.maximum(p, q)])
    ax = np.concatenate([ax, np.full(m, 3)]); w = np.concatenate([w, 2.0 ** rng.integers(-3, 0, size=m)])
    scale = 2.0 ** rng.integers(-3, 4, size=N)
    return lo, hi, w, ax, scale


def _build(name, seed):
    n = N_ROWS
    lo, hi, w, ax, s = _graph(seed)
    dg = np.arange(n)
    rows = [lo, hi, lo, hi, dg]; cols = [lo, hi, hi, lo, dg]; vals = [w, w, -w, -w, np.full(n, 2.0 ** -4)]
    if name == "unsym_scaled":   # upwind differences of a flow along +x, +y, +z: the row of the downstream point couples to the upstream one
        g = ax < 3
        c = np.array([1.0, 0.5, 0.25])[ax[g]]
        rows += [hi[g], hi[g]]; cols += [hi[g], lo[g]]; vals += [c, -c]
    rows = np.concatenate(rows); cols = np.concatenate(cols); vals = np.concatenate(vals)
    vals = vals * s[rows] * s[cols]   # rows and columns scaled by powers of two: exact (scaling the rows alone makes the Galerkin
    # operators of the unsymmetric input so dense that the setup stops after four levels)
    return _coo_to_csr(n, rows, cols, vals)


def _dense_abs_rowsum_of_skew(ia, ja, a):
    """(||A - A^T||_inf, ||A||_inf) without forming a dense matrix."""
    n = len(ia) - 1
    rows = np.repeat(np.arange(n), np.diff(ia))
    ib, jb, d = _coo_to_csr(n, np.concatenate([rows, ja]), np.concatenate([ja, rows]), np.concatenate([a, -a]))
    skew = np.zeros(n); np.add.at(skew, np.repeat(np.arange(n), np.diff(ib)), np.abs(d))
    full = np.zeros(n); np.add.at(full, rows, np.abs(a))
    return skew.max(), full.max()


def check_matrix(name, ia, ja, a):
    """What the input is for, asserted: a later edit of the generator cannot quietly lose it."""
    n = len(ia) - 1
    rows = np.repeat(np.arange(n), np.diff(ia))
    d = a[ja == rows]
    assert len(d) == n and np.all(d > 0)
    lens = np.diff(ia)
    assert lens.min() != lens.max(), "row lengths vary"
    skew, full = _dense_abs_rowsum_of_skew(ia, ja, a)
    if name == "fe":
        return
    assert d.max() >= 64 * d.min(), "the diagonal varies by at least 64x"
    if name == "unsym_scaled":
        assert skew >= 0.05 * full, (skew, full)
    else:
        assert skew == 0.0


SEEDS = {"spd_scaled": 2024, "unsym_scaled": 2025}
INPUTS = ("spd_scaled", "unsym_scaled", "fe")


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(ia, ja, a) of an input, read-only, built once per session."""
    if name == "fe":
        from _libs import DATA, read_csr
        ia, ja, a = read_csr(DATA + "/csrmat_FE.dat")
    else:
        ia, ja, a = _build(name, SEEDS[name])
    check_matrix(name, ia, ja, a)
    for v in (ia, ja, a):
        v.setflags(write=False)
    return ia, ja, a


def check_hierarchy(name, sizes):
    """The hierarchy a setup with coarse_dof = 20 makes of an input: deep enough to tell the hybrid cycles apart, ragged."""
    assert len(sizes) >= 5, (name, sizes)
    assert all(s % 64 for s in sizes), (name, sizes)
    assert all(x > y for x, y in zip(sizes, sizes[1:])), (name, sizes)


def vectors(name, seed, k=1):
    """k standard-normal vectors of an input's row count."""
    n = len(matrix(name)[0]) - 1
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n) for _ in range(k)]


# --- the configurations: functions on (ITS_param, AMG_param), as in test_gpu_parity.py ------------------------------------
def _base(i, a): i.tol = 1e-8; a.coarse_dof = 20
def _jac(i, a): _base(i, a); a.smoother = T.SMOOTHER_JACOBI; a.relaxation = 0.6667
def _jac_w(i, a): _jac(i, a); a.cycle_type = T.W_CYCLE
def _jac_12(i, a): _jac(i, a); a.cycle_type = T.VW_CYCLE
def _jac_21(i, a): _jac(i, a); a.cycle_type = T.WV_CYCLE
def _jac_maxit2(i, a): _jac(i, a); a.maxit = 2
def _jac_cs(i, a): _jac(i, a); a.coarse_scaling = 1
def _jac23(i, a): _jac(i, a); a.presmooth_iter = 2; a.postsmooth_iter = 3
def _l1(i, a): _base(i, a); a.smoother = T.SMOOTHER_L1DIAG
def _poly3(i, a): _base(i, a); a.smoother = T.SMOOTHER_POLY; a.polynomial_degree = 3
def _poly5w21(i, a): _base(i, a); a.smoother = T.SMOOTHER_POLY; a.polynomial_degree = 5; a.cycle_type = T.W_CYCLE; a.presmooth_iter = 2; a.postsmooth_iter = 1
def _gs_cf(i, a): _base(i, a); a.smoother = T.SMOOTHER_GS; a.smooth_order = T.CF_ORDER
def _gs_nat(i, a): _base(i, a); a.smoother = T.SMOOTHER_GS; a.smooth_order = T.NO_ORDER
def _sgs(i, a): _base(i, a); a.smoother = T.SMOOTHER_SGS
def _sor(i, a): _base(i, a); a.smoother = T.SMOOTHER_SOR; a.relaxation = 1.2
def _ssor(i, a): _base(i, a); a.smoother = T.SMOOTHER_SSOR; a.relaxation = 1.2
def _gsor(i, a): _base(i, a); a.smoother = T.SMOOTHER_GSOR; a.relaxation = 0.9
def _sgsor(i, a): _base(i, a); a.smoother = T.SMOOTHER_SGSOR; a.relaxation = 1.05
def _jacf(i, a): _base(i, a); a.smoother = T.SMOOTHER_JACOBIF; a.relaxation = 0.8
def _gsf(i, a): _base(i, a); a.smoother = T.SMOOTHER_GSF
def _cg33(i, a): _base(i, a); a.smoother = T.SMOOTHER_CG; a.presmooth_iter = 3; a.postsmooth_iter = 3
def _amli1(i, a): _jac(i, a); a.cycle_type = T.AMLI_CYCLE; a.amli_degree = 1
def _amli2cs(i, a): _jac(i, a); a.cycle_type = T.AMLI_CYCLE; a.amli_degree = 2; a.coarse_scaling = 1
def _amli3gs(i, a): _gs_cf(i, a); a.cycle_type = T.AMLI_CYCLE; a.amli_degree = 3
def _kcycle_gcg(i, a): _jac(i, a); a.cycle_type = T.NL_AMLI_CYCLE; a.nl_amli_krylov_type = T.SOLVER_GCG
def _kcycle_gcr_gs(i, a): _gs_cf(i, a); a.cycle_type = T.NL_AMLI_CYCLE; a.nl_amli_krylov_type = T.SOLVER_GCR


CONFIGS = {
    "jacobi-V": _jac, "jacobi-W": _jac_w, "jacobi-12": _jac_12, "jacobi-21": _jac_21, "jacobi-V-maxit2": _jac_maxit2,
    "jacobi-V-coarse-scaling": _jac_cs, "jacobi-V23": _jac23, "l1diag": _l1, "poly3": _poly3, "poly5-W21": _poly5w21,
    "gs-cf": _gs_cf, "gs-natural": _gs_nat, "sgs": _sgs, "sor1.2": _sor, "ssor": _ssor, "gsor": _gsor, "sgsor": _sgsor,
    "jacobiF0.8": _jacf, "gsF": _gsf, "cg33": _cg33, "amli1": _amli1, "amli2-coarse-scaling": _amli2cs, "amli3-gs": _amli3gs,
    "kcycle-gcg": _kcycle_gcg, "kcycle-gcr-gs": _kcycle_gcr_gs,
}

# the smoothers of the table: name -> (smoother, smooth_order, relaxation, polynomial_degree, sweep counts to try)
PAR, SEQ = (1, 3), (1,)
SMOOTHERS = {
    "jacobi": (T.SMOOTHER_JACOBI, T.CF_ORDER, 0.6667, 3, PAR), "l1diag": (T.SMOOTHER_L1DIAG, T.CF_ORDER, 1.0, 3, PAR),
    "poly3": (T.SMOOTHER_POLY, T.CF_ORDER, 1.0, 3, PAR), "poly5": (T.SMOOTHER_POLY, T.CF_ORDER, 1.0, 5, PAR),
    "jacobiF0.8": (T.SMOOTHER_JACOBIF, T.CF_ORDER, 0.8, 3, PAR), "cg": (T.SMOOTHER_CG, T.CF_ORDER, 1.0, 3, PAR),
    "gs-cf": (T.SMOOTHER_GS, T.CF_ORDER, 1.0, 3, SEQ), "gs-natural": (T.SMOOTHER_GS, T.NO_ORDER, 1.0, 3, SEQ),
    "sgs": (T.SMOOTHER_SGS, T.CF_ORDER, 1.0, 3, SEQ), "sor1.2": (T.SMOOTHER_SOR, T.CF_ORDER, 1.2, 3, SEQ),
    "ssor": (T.SMOOTHER_SSOR, T.CF_ORDER, 1.2, 3, SEQ), "gsor": (T.SMOOTHER_GSOR, T.CF_ORDER, 0.9, 3, SEQ),
    "sgsor": (T.SMOOTHER_SGSOR, T.CF_ORDER, 1.05, 3, SEQ), "gsF": (T.SMOOTHER_GSF, T.CF_ORDER, 1.0, 3, SEQ),
}


def params(cfg):
    """Fresh (ITS_param, AMG_param) of a configuration (a name of CONFIGS or a function)."""
    from _libs import default_params
    itp, amgp = default_params()
    (CONFIGS[cfg] if isinstance(cfg, str) else cfg)(itp, amgp)
    return itp, amgp


# --- the oracle on a hierarchy -------------------------------------------------------------------------------------------
def _protos():
    from _libs import oracle
    O = oracle()
    P = C.POINTER
    O.orc_precond_famg.argtypes = O.orc_precond_amg.argtypes
    O.orc_smoothing.argtypes = [C.c_int, C.c_int, P(T.dCSRmat), T.c_double_p, T.c_double_p, C.c_int, C.c_double, C.c_int,
                                T.c_int_p, C.c_int]
    O.orc_amg_borrow_begin.argtypes = [C.c_void_p, C.c_int]
    O.orc_amg_borrow_level.argtypes = [C.c_void_p, C.c_int, P(T.dCSRmat), P(T.dCSRmat), P(T.dCSRmat), T.c_int_p]
    O.orc_amg_borrow_end.argtypes = [C.c_void_p]
    O.orc_amg_borrow_cycles.argtypes = [C.c_void_p, P(T.AMG_param)]
    O.orc_amg_borrow_free.argtypes = [C.c_void_p]
    O.orc_solve_with_hierarchy.argtypes = [C.c_void_p, P(T.dCSRmat), P(T.dvector), P(T.dvector), P(T.ITS_param),
                                           P(T.AMG_param), T.c_double_p, C.c_int, P(C.c_int), P(C.c_double)]
    return O


class _Lvl(C.Structure):
    """struct orc_level of oracle/fasp_oracle.h."""
    _fields_ = [("A", T.dCSRmat), ("P", T.dCSRmat), ("R", T.dCSRmat), ("cfmark", T.ivector), ("b", T.dvector), ("x", T.dvector),
                ("w", T.dvector)]


class Cycler:
    """Cycles and solves of the oracle on a hierarchy: its own (OrcAMG) or one borrowed from a product handle."""

    def __init__(self, buf, amgp):
        self.O = _protos(); self.buf = buf; self.amgp = amgp

    def reset(self):
        """Every level's iterate back to zero, as a setup leaves it: the full-multigrid cycle adds to what the last one left there."""
        for l in range(C.cast(self.buf, T.c_int_p)[0]):
            L = _Lvl.from_address(C.addressof(self.buf) + 8 + l * C.sizeof(_Lvl))
            C.memset(L.x.val, 0, 8 * L.x.row)

    def precond(self, r, fmg=False):
        """z = B r; as full multigrid (fmg) from a hierarchy whose iterates are zero, so that every call computes the same."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.zeros_like(r)
        if fmg:
            self.reset()
        (self.O.orc_precond_famg if fmg else self.O.orc_precond_amg)(self.buf, C.byref(self.amgp), T.dp(r), T.dp(z))
        return z

    def solve(self, ia, ja, a, f, itp, cap=600):
        """orc_solve_with_hierarchy -> (status, x, hist, relres)."""
        A, keep = T.as_csr(ia, ja, a)
        bv, fk = T.as_vec(f)
        xv, x = T.as_vec(np.zeros(len(f)))
        hist = np.zeros(cap); nh = C.c_int(0); rr = C.c_double(0)
        st = self.O.orc_solve_with_hierarchy(self.buf, C.byref(A), C.byref(bv), C.byref(xv), C.byref(itp), C.byref(self.amgp),
                                             T.dp(hist), cap, C.byref(nh), C.byref(rr))
        return st, x, hist[:nh.value].copy(), rr.value


class Borrowed(Cycler):
    """The oracle on the level matrices of a product handle H (host-only or uploaded), as bench.py borrows them: both sides
    then cycle the same levels.  amgp: the parameters the cycles run with (AMLI coefficients, cycle types per level)."""

    def __init__(self, H, amgp):
        import faspsolver_amd as fa
        O = _protos()
        nl = H.num_levels
        buf = C.create_string_buffer(O.orc_sizeof_amg())
        O.orc_amg_borrow_begin(buf, nl)
        self.keep = []; self.sizes = []
        for l in range(nl):
            vA = T.dCSRmat(); fa.lib().fasp_hip_amg_get_matrix(H.h, l, 0, C.byref(vA))
            self.sizes.append(vA.row)
            if l < nl - 1:
                vP = T.dCSRmat(); vR = T.dCSRmat(); cf = T.ivector()
                fa.lib().fasp_hip_amg_get_matrix(H.h, l, 1, C.byref(vP))
                fa.lib().fasp_hip_amg_get_matrix(H.h, l, 2, C.byref(vR))
                fa.lib().fasp_hip_amg_get_cfmark(H.h, l, C.byref(cf))
                O.orc_amg_borrow_level(buf, l, C.byref(vA), C.byref(vP), C.byref(vR), cf.val if cf.row == vA.row else None)
                self.keep += [vA, vP, vR, cf]
            else:
                O.orc_amg_borrow_level(buf, l, C.byref(vA), None, None, None)
                self.keep += [vA]
        O.orc_amg_borrow_end(buf)
        O.orc_amg_borrow_cycles(buf, C.byref(amgp))
        super().__init__(buf, amgp)

    def close(self):
        if self.buf is not None:
            self.O.orc_amg_borrow_free(self.buf)
            self.buf = None


def ref_precond(R, hr, amgp, r, fmg=False):
    """z = B r through the preconditioner the compiled reference's fasp_solver_dcsr_krylov_amg would install for amgp (SolCSR.c:537-549)
    on the reference hierarchy hr (ref_amg_setup_rs): fasp_precond_famg when fmg is set, else by cycle type fasp_precond_amli / _namli /
    _amg.  The precond_data is filled by the reference's own fasp_param_amg_to_prec, then max_levels and mgl_data as SolCSR.c:531-532 does."""
    import struct
    pc = C.create_string_buffer(R.ref_sizeof(5))
    R.fasp_param_amg_to_prec.argtypes = [C.c_void_p, C.POINTER(T.AMG_param)]
    R.fasp_param_amg_to_prec.restype = None
    R.fasp_param_amg_to_prec(pc, C.byref(amgp))
    struct.pack_into("h", pc, R.ref_offsetof_precdata(3), R.ref_amg_num_levels(hr))
    struct.pack_into("P", pc, R.ref_offsetof_precdata(19), hr)
    fct = (R.fasp_precond_famg if fmg else R.fasp_precond_amli if amgp.cycle_type == T.AMLI_CYCLE else
           R.fasp_precond_namli if amgp.cycle_type == T.NL_AMLI_CYCLE else R.fasp_precond_amg)
    fct.argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
    fct.restype = None
    rr = np.array(r, dtype=np.float64)
    z = np.zeros_like(rr)
    fct(T.dp(rr), T.dp(z), pc)
    assert np.array_equal(rr, r)
    return z


def orc_smooth(A, cf, post, spec, nsweeps, b, x):
    """orc_smoothing of smoother spec (an entry of SMOOTHERS) on the level matrix A (a dCSRmat) with C/F marker cf (int32
    array or None), from the iterate x -> the new iterate."""
    O = _protos()
    sm, order, relax, ndeg, _ = spec
    u = np.array(x, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    st = O.orc_smoothing(int(post), sm, C.byref(A), T.dp(b), T.dp(u), nsweeps, relax, order, None if cf is None else T.ip(cf), ndeg)
    assert st == 0, st
    return u


# --- the tolerance rule --------------------------------------------------------------------------------------------------
def nudge(v, seed):
    """Every entry moved by one relative 2^-52 step in a random direction."""
    s = np.random.default_rng(seed).choice([-1.0, 1.0], size=v.shape)
    return v * (1.0 + s * 2.0 ** -52)


def rel_diff(got, ref):
    got = np.asarray(got); ref = np.asarray(ref)
    if not (np.all(np.isfinite(got)) and np.all(np.isfinite(ref))):
        return float("inf")
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def probe(fn, vecs, ref=None):
    """Largest relative response of fn(*vecs) -- one array or a tuple of arrays, each measured by itself -- to nudge() of
    every input vector, over PROBE_SEEDS.  -> (reference result, probe)."""
    ref = fn(*vecs) if ref is None else ref
    worst = 0.0
    for s in PROBE_SEEDS:
        out = fn(*[nudge(v, 97 * s + k) for k, v in enumerate(vecs)])
        if isinstance(ref, tuple):
            worst = max([worst] + [rel_diff(o, r) for o, r in zip(out, ref)])
        else:
            worst = max(worst, rel_diff(out, ref))
    return ref, worst


def bar(probe_value, floor, cap, what):
    """max(floor, 8 x probe); a bar beyond its cap fails the case itself."""
    b = max(floor, PROBE_FACTOR * probe_value)
    assert b <= cap, f"{what}: probe {probe_value:.3e} puts the bar at {b:.3e}, beyond the cap {cap:.0e}: the case needs another seed or input"
    return b


class Ledger:
    """The largest probe and bar a test file has met, for its last test to print."""

    def __init__(self):
        self.rows = {}

    def note(self, kind, what, probe_value, bar_value, err=None):
        p = self.rows.get(kind)
        if p is None or probe_value > p[1]:
            self.rows[kind] = (what, probe_value, bar_value, err)

    def report(self, title):
        for kind, (what, p, b, e) in sorted(self.rows.items()):
            print(f"[{title}] largest {kind} probe {p:.3e} -> bar {b:.3e}" + ("" if e is None else f", error there {e:.3e}") + f" ({what})")
