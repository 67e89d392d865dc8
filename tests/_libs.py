"""Loaders for the checker libraries used by the tests (oracle, reference build)."""
import ctypes as C
import functools
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from faspsolver_amd import _types as T  # noqa: E402

ORACLE_SO = os.path.join(ROOT, "oracle", "liboracle.so")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libfasp_ref.so")
REF_TREE = "/root/reference"

_oracle = None
_ref = None


def build_oracle():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "all"], check=True)


def oracle():
    """liboracle.so (CPU restatement).  Built on demand (gcc only)."""
    global _oracle
    if _oracle is None:
        src = os.path.join(ROOT, "oracle", "fasp_oracle.c")
        if (not os.path.exists(ORACLE_SO)
                or os.path.getmtime(ORACLE_SO) < os.path.getmtime(src)):
            build_oracle()
        lib = C.CDLL(ORACLE_SO)
        lib.orc_dotprod.restype = C.c_double
        lib.orc_norm2.restype = C.c_double
        lib.orc_norminf.restype = C.c_double
        lib.orc_dotprod.argtypes = [C.c_int, T.c_double_p, T.c_double_p]
        lib.orc_norm2.argtypes = [C.c_int, T.c_double_p]
        lib.orc_norminf.argtypes = [C.c_int, T.c_double_p]
        lib.orc_axpy.argtypes = [C.c_int, C.c_double, T.c_double_p, T.c_double_p]
        lib.orc_axpby.argtypes = [C.c_int, C.c_double, T.c_double_p, C.c_double, T.c_double_p]
        lib.orc_aAxpy.argtypes = [C.c_double, C.POINTER(T.dCSRmat), T.c_double_p, T.c_double_p]
        lib.orc_mxv.argtypes = [C.POINTER(T.dCSRmat), T.c_double_p, T.c_double_p]
        lib.orc_smoother_jacobi.argtypes = [T.c_double_p, C.c_int, C.c_int, C.c_int,
                                            C.POINTER(T.dCSRmat), T.c_double_p, C.c_int,
                                            C.c_double]
        lib.orc_smoother_sor.argtypes = lib.orc_smoother_jacobi.argtypes
        lib.orc_smoother_gs.argtypes = [T.c_double_p, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(T.dCSRmat), T.c_double_p, C.c_int]
        lib.orc_smoother_l1diag.argtypes = lib.orc_smoother_gs.argtypes
        lib.orc_smoother_gs_cf.argtypes = [T.c_double_p, C.POINTER(T.dCSRmat), T.c_double_p,
                                           C.c_int, T.c_int_p, C.c_int]
        lib.orc_smoother_sgs.argtypes = [T.c_double_p, C.POINTER(T.dCSRmat), T.c_double_p,
                                         C.c_int]
        lib.orc_spcg.argtypes = [C.POINTER(T.dCSRmat), C.POINTER(T.dvector),
                                 C.POINTER(T.dvector), C.c_double, C.c_int, C.c_int, C.c_int]
        lib.orc_precond_amg.argtypes = [C.c_void_p, C.POINTER(T.AMG_param), T.c_double_p,
                                        T.c_double_p]
        lib.orc_amg_setup_rs.argtypes = [C.c_void_p, C.POINTER(T.dCSRmat),
                                         C.POINTER(T.AMG_param)]
        lib.orc_amg_free.argtypes = [C.c_void_p]
        _oracle = lib
    return _oracle


def have_ref():
    return os.path.exists(REF_SO)


def ref():
    """The reference compiled from its own sources (oracle/_ref), or None."""
    global _ref
    if _ref is None:
        if not have_ref():
            if os.path.isdir(REF_TREE):
                build_oracle()
            if not have_ref():
                return None
        lib = C.CDLL(REF_SO)
        lib.ref_amg_setup_rs.restype = C.c_void_p
        lib.ref_amg_setup_rs.argtypes = [C.POINTER(T.dCSRmat), C.POINTER(T.AMG_param)]
        lib.ref_amg_num_levels.argtypes = [C.c_void_p]
        lib.ref_amg_get_matrix.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(T.dCSRmat)]
        lib.ref_amg_get_cfmark.restype = T.c_int_p
        lib.ref_amg_get_cfmark.argtypes = [C.c_void_p, C.c_int]
        lib.ref_amg_free.argtypes = [C.c_void_p, C.POINTER(T.AMG_param)]
        lib.ref_precond_amg.argtypes = [C.c_void_p, C.POINTER(T.AMG_param), T.c_double_p,
                                        T.c_double_p]
        lib.ref_coarse_spcg.argtypes = [C.POINTER(T.dCSRmat), C.POINTER(T.dvector),
                                        C.POINTER(T.dvector), C.c_double]
        lib.fasp_blas_darray_dotprod.restype = C.c_double
        lib.fasp_blas_darray_norm2.restype = C.c_double
        lib.fasp_blas_darray_norminf.restype = C.c_double
        _ref = lib
    return _ref


class OrcAMG:
    """Owns an orc_amg hierarchy built by the oracle."""

    def __init__(self, A, param):
        lib = oracle()
        self.lib = lib
        self.buf = C.create_string_buffer(lib.orc_sizeof_amg())
        self.status = lib.orc_amg_setup_rs(self.buf, C.byref(A), C.byref(param))
        # struct orc_amg { int num_levels; orc_level L[20]; ... }
        self.num_levels = C.cast(self.buf, T.c_int_p)[0]

    def level(self, l):
        """(A, P, R, cfmark) of level l as struct views."""
        class Lvl(C.Structure):
            _fields_ = [("A", T.dCSRmat), ("P", T.dCSRmat), ("R", T.dCSRmat),
                        ("cfmark", T.ivector), ("b", T.dvector), ("x", T.dvector),
                        ("w", T.dvector)]
        base = C.addressof(self.buf) + 8  # int + padding
        return Lvl.from_address(base + l * C.sizeof(Lvl))

    def free(self):
        if self.buf is not None:
            self.lib.orc_amg_free(self.buf)
            self.buf = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# --- data readers (formats of base/src/BlaIO.c:146-157: 1-based ASCII CSR) ----
import numpy as np  # noqa: E402

DATA = os.path.join(ROOT, "tests", "golden", "data")


def read_csr(path):
    """fasp_dcsrvec_read2 matrix format: n, ia(n+1), ja(nnz), a(nnz), 1-based."""
    tok = open(path).read().split()
    n = int(tok[0])
    ia = np.array(tok[1:n + 2], dtype=np.int64)
    nnz = int(ia[-1] - ia[0])
    ja = np.array(tok[n + 2:n + 2 + nnz], dtype=np.int64)
    a = np.array(tok[n + 2 + nnz:n + 2 + 2 * nnz], dtype=np.float64)
    return (ia - ia[0]).astype(np.int32), (ja - 1).astype(np.int32), a


def read_vec(path):
    tok = open(path).read().split()
    n = int(tok[0])
    return np.array(tok[1:n + 1], dtype=np.float64)


def read_vecind(path):
    """fasp_dvecind_read format (BlaIO.c:887): n, then `index value` pairs."""
    tok = open(path).read().split()
    n = int(tok[0])
    v = np.zeros(n)
    for k in range(n):
        v[int(tok[1 + 2 * k])] = float(tok[2 + 2 * k])
    return v


def poisson7pt(n, lib=None):
    """P7(n) through the oracle's generator; returns numpy (ia, ja, a, f, u)."""
    lib = lib or oracle()
    A = T.dCSRmat(); b = T.dvector(); u = T.dvector()
    lib.orc_poisson7pt(n, n, n, C.byref(A), C.byref(b), C.byref(u))
    ia, ja, a = T.csr_arrays(A)
    f = np.ctypeslib.as_array(b.val, (b.row,)).copy()
    ue = np.ctypeslib.as_array(u.val, (u.row,)).copy()
    lib.orc_free_csr(C.byref(A)); lib.orc_free_vec(C.byref(b)); lib.orc_free_vec(C.byref(u))
    return ia, ja, a, f, ue


def orc_solve(ia, ja, a, f, itp, amgp, x0=None, cap=600):
    """oracle fasp_solver_dcsr_krylov_amg; returns (status, x, hist, relres)."""
    lib = oracle()
    A, keep = T.as_csr(ia, ja, a)
    x = np.zeros(len(f)) if x0 is None else x0.copy()
    bv, fk = T.as_vec(f)
    xv, x = T.as_vec(x)
    hist = np.zeros(cap); nh = C.c_int(0); rr = C.c_double(0)
    st = lib.orc_solver_dcsr_krylov_amg(C.byref(A), C.byref(bv), C.byref(xv), C.byref(itp),
                                        C.byref(amgp), T.dp(hist), cap, C.byref(nh),
                                        C.byref(rr))
    return st, x, hist[:nh.value].copy(), rr.value


def ref_solve(ia, ja, a, f, itp, amgp, x0=None, cap=600):
    """reference fasp_solver_dcsr_krylov_amg with recorded history."""
    lib = ref()
    A, keep = T.as_csr(ia, ja, a)
    x = np.zeros(len(f)) if x0 is None else x0.copy()
    bv, fk = T.as_vec(f)
    xv, x = T.as_vec(x)
    hist = np.zeros(cap); nh = C.c_int(0)
    st = lib.ref_krylov_amg_hist(C.byref(A), C.byref(bv), C.byref(xv), C.byref(itp),
                                 C.byref(amgp), T.dp(hist), cap, C.byref(nh))
    return st, x, hist[:nh.value].copy()


def default_params(lib=None):
    lib = lib or oracle()
    itp = T.ITS_param(); amgp = T.AMG_param()
    lib.orc_param_solver_init(C.byref(itp)); lib.orc_param_amg_init(C.byref(amgp))
    return itp, amgp


def read_bsr(path):
    """fasp_dbsr_read format (BlaIO.c:807): ROW COL NNZ / nb / storage_manner / n, IA / n, JA / n, val."""
    tok = open(path).read().split()
    ROW, COL, NNZ, nb, sm = (int(t) for t in tok[:5])
    p = 5
    n = int(tok[p]); ia = np.array(tok[p + 1:p + 1 + n], dtype=np.int32); p += 1 + n
    n = int(tok[p]); ja = np.array(tok[p + 1:p + 1 + n], dtype=np.int32); p += 1 + n
    n = int(tok[p]); val = np.array(tok[p + 1:p + 1 + n], dtype=np.float64)
    assert sm == 0 and len(ia) == ROW + 1 and len(ja) == NNZ and len(val) == NNZ * nb * nb
    return ia, ja, val, nb


B3 = np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 2.0]])


def poisson7pt_bsr(n, block=B3):
    """Synthetic multi-block system P7(n) (x) B: every scalar entry a_ij becomes a_ij * B."""
    ia, ja, a, f, ue = poisson7pt(n)
    nb = block.shape[0]
    val = (a[:, None, None] * block[None, :, :]).reshape(-1)
    return ia, ja, val, nb


# --- BSR AMG (config 3) helpers ----------------------------------------------------------
class BsrLvl(C.Structure):
    """struct orc_bsr_level of oracle/fasp_oracle.h."""
    _fields_ = [("A", T.dBSRmat), ("P", T.dBSRmat), ("R", T.dBSRmat), ("diaginv", T.c_double_p),
                ("b", T.dvector), ("x", T.dvector), ("w", T.dvector)]


def bsr_arrays(M):
    ia = np.ctypeslib.as_array(M.IA, (M.ROW + 1,)).copy()
    ja = np.ctypeslib.as_array(M.JA, (max(M.NNZ, 1),))[:M.NNZ].copy()
    nv = M.NNZ * M.nb * M.nb
    v = np.ctypeslib.as_array(M.val, (max(nv, 1),))[:nv].copy()
    return ia, ja, v


def bsr_protos():
    o = oracle()
    o.orc_amg_setup_ua_bsr.argtypes = [C.c_void_p, C.POINTER(T.dBSRmat), C.POINTER(T.AMG_param)]
    o.orc_solver_dbsr_krylov_amg.argtypes = [
        C.POINTER(T.dBSRmat), C.POINTER(T.dvector), C.POINTER(T.dvector), C.POINTER(T.ITS_param),
        C.POINTER(T.AMG_param), T.c_int_p, T.c_double_p]
    R = ref()
    if R is not None:
        R.ref_bsr_setup_ua.restype = C.c_void_p
        R.ref_bsr_setup_ua.argtypes = [C.POINTER(T.dBSRmat), C.POINTER(T.AMG_param)]
        R.ref_bsr_num_levels.argtypes = [C.c_void_p]
        R.ref_bsr_get_matrix.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(T.dBSRmat)]
        R.ref_bsr_get_diaginv.argtypes = [C.c_void_p, C.c_int]
        R.ref_bsr_get_diaginv.restype = T.c_double_p
        R.ref_bsr_free.argtypes = [C.c_void_p]
        R.fasp_solver_dbsr_krylov_amg.argtypes = [
            C.POINTER(T.dBSRmat), C.POINTER(T.dvector), C.POINTER(T.dvector),
            C.POINTER(T.ITS_param), C.POINTER(T.AMG_param)]
    return o, R


def bsr_params(solver=5, cycle=1, agg=2):
    """Config 3 of BASELINE.json: UA-AMG (agg 2 = VMB; 1 = the reference's default, symmetric
    pairwise matching), block Jacobi, VGMRES(30), tol 1e-8."""
    itp, amgp = default_params()
    amgp.AMG_type = T.UA_AMG; amgp.aggregation_type = agg; amgp.smoother = T.SMOOTHER_JACOBI
    amgp.cycle_type = cycle
    itp.tol = 1e-8; itp.itsolver_type = solver; itp.restart = 30
    return itp, amgp


def orc_bsr_solve(ia, ja, val, nb, f, itp, amgp):
    o, _ = bsr_protos()
    A, keep = T.as_bsr(ia, ja, val, nb)
    n = A.ROW * nb
    x = np.zeros(n); bv, fk = T.as_vec(f); xv = T.dvector(n, T.dp(x))
    nl = C.c_int(0); rr = C.c_double(0)
    st = o.orc_solver_dbsr_krylov_amg(C.byref(A), C.byref(bv), C.byref(xv), C.byref(itp),
                                      C.byref(amgp), C.byref(nl), C.byref(rr))
    return st, x, nl.value, rr.value


def ref_bsr_solve(ia, ja, val, nb, f, itp, amgp):
    _, R = bsr_protos()
    A, keep = T.as_bsr(ia, ja, val, nb)
    n = A.ROW * nb
    x = np.zeros(n); bv, fk = T.as_vec(f); xv = T.dvector(n, T.dp(x))
    st = R.fasp_solver_dbsr_krylov_amg(C.byref(A), C.byref(bv), C.byref(xv), C.byref(itp),
                                       C.byref(amgp))
    return st, x


class OrcBSR:
    """UA-BSR hierarchy built by the oracle: list of (A, P, R, diaginv) numpy tuples per level."""

    def __init__(self, ia, ja, val, nb, amgp):
        o, _ = bsr_protos()
        A, keep = T.as_bsr(ia, ja, val, nb)
        buf = C.create_string_buffer(o.orc_sizeof_amg_bsr())
        self.status = o.orc_amg_setup_ua_bsr(buf, C.byref(A), C.byref(amgp))
        self.num_levels = C.cast(buf, T.c_int_p)[0]
        self.levels = []
        for l in range(self.num_levels):
            L = BsrLvl.from_address(C.addressof(buf) + 8 + l * C.sizeof(BsrLvl))
            last = l == self.num_levels - 1
            d = None
            if L.diaginv:
                d = np.ctypeslib.as_array(L.diaginv, (L.A.ROW * nb * nb,)).copy()
            self.levels.append(dict(
                A=(L.A.ROW, L.A.COL, L.A.NNZ) + bsr_arrays(L.A),
                P=None if last else (L.P.ROW, L.P.COL, L.P.NNZ) + bsr_arrays(L.P),
                R=None if last else (L.R.ROW, L.R.COL, L.R.NNZ) + bsr_arrays(L.R),
                diaginv=d))
        self._buf = buf  # hierarchy memory is leaked with the buffer (test process only)


def orc_bsr_ops():
    """The oracle with the prototypes of its block operators set."""
    o = oracle()
    o.orc_bsr_mxv.argtypes = [C.POINTER(T.dBSRmat), T.c_double_p, T.c_double_p]
    o.orc_bsr_aAxpy.argtypes = [C.c_double, C.POINTER(T.dBSRmat), T.c_double_p, T.c_double_p]
    o.orc_bsr_getdiaginv.argtypes = [C.POINTER(T.dBSRmat)]
    o.orc_bsr_getdiaginv.restype = T.c_double_p
    o.orc_bsr_jacobi1.argtypes = [C.POINTER(T.dBSRmat), T.c_double_p, T.c_double_p, T.c_double_p]
    o.orc_bsr_gs_sor.argtypes = [C.POINTER(T.dBSRmat), T.c_double_p, T.c_double_p, T.c_double_p, C.c_int, C.c_int, C.c_double]
    o.orc_free.argtypes = [C.c_void_p]
    return o


def orc_diaginv(o, A):
    """orc_bsr_getdiaginv as a numpy array."""
    dp_ = o.orc_bsr_getdiaginv(C.byref(A))
    d = np.ctypeslib.as_array(dp_, (A.ROW * A.nb * A.nb,)).copy()
    o.orc_free(dp_)
    return d


SOR_WEIGHTS = (1.1, 1.0, 0.5)   # the block SOR weights the sweeps are compared at


# --- irregular BSR matrices for the block row kernel (k_bsr_wstream) and the block sweeps ---------
def bsr_tile(nb):
    """(RW, CAPB, U) of k_bsr_wstream<nb, .>: block rows per wave tile, blocks per LDS chunk, blocks per round trip."""
    return 64 // nb, 1536 // (nb * nb), 8 if nb <= 3 else 4


def ragged_bsr(nb, seed, square=True, extra_cols=0):
    """An irregular BSR matrix that reaches the edges of k_bsr_wstream<nb, .> a stencil never touches
    -> (ROW, COL, ia, ja, val, lens); deterministic in (nb, seed, square, extra_cols).

    ROW = max(13 RW + 1, 2 CAPB + 67), COL = ROW + extra_cols (extra_cols >= -50).  Values are standard normal.  Rows hold
    1 .. 2U + 2 blocks (capped at COL) in distinct, unsorted columns, except row 0 (2 CAPB + 3 blocks: three LDS chunks),
    rows RW - 1 and RW (empty: end of one wave tile, start of the next), rows 2 RW .. 3 RW - 1 (empty: a tile without
    blocks), row 3 RW + 1 (one block) and the last row (CAPB + 1 blocks).  square: every row holds its diagonal block at a
    random position, the empty rows become diagonal-only (the sweeps need a diagonal) and the diagonal block gets
    I * 3 sqrt(4 nb len) added, which keeps one Gauss-Seidel / SOR sweep bounded.  Otherwise the empty rows stay empty and
    the diagonal is nothing special."""
    RW, CAPB, U = bsr_tile(nb)
    nb2 = nb * nb
    rng = np.random.default_rng(seed)
    ROW = max(13 * RW + 1, 2 * CAPB + 67)
    COL = ROW + extra_cols
    assert not (square and extra_cols), "the square form has COL == ROW"
    lens = np.minimum(rng.integers(1, 2 * U + 3, size=ROW), COL)
    lens[0] = 2 * CAPB + 3
    empty = np.r_[RW - 1, RW, 2 * RW:3 * RW]
    lens[empty] = 1 if square else 0
    lens[3 * RW + 1] = 1
    lens[ROW - 1] = CAPB + 1
    assert lens.max() <= COL
    ia = np.zeros(ROW + 1, dtype=np.int32)
    ia[1:] = np.cumsum(lens)
    ja = np.empty(int(ia[-1]), dtype=np.int32)
    for i in range(ROW):   # (the one per-row loop: a draw without replacement per row)
        k = int(lens[i])
        if square:
            c = rng.choice(COL - 1, size=k - 1, replace=False)
            c = np.append(c + (c >= i), i)
        else:
            c = rng.choice(COL, size=k, replace=False)
        rng.shuffle(c)
        ja[ia[i]:ia[i + 1]] = c
    val = rng.standard_normal(int(ia[-1]) * nb2)
    if square:
        rows = np.repeat(np.arange(ROW), lens)
        kd = np.flatnonzero(ja == rows)
        assert len(kd) == ROW
        boost = 3.0 * np.sqrt(4.0 * nb * lens)
        val.reshape(-1, nb, nb)[kd[:, None], np.arange(nb), np.arange(nb)] += boost[:, None]
    # the edges this matrix exists for: a later edit cannot quietly lose one
    assert lens.max() > 2 * CAPB                                   # one block row alone spans three LDS chunks
    assert ROW % RW != 0 and ROW % (4 * RW) != 0                   # last wave tile with nbr < RW, last workgroup partial
    tiles = ia[np.minimum(np.arange(0, ROW + RW, RW), ROW)]        # block offsets of the wave tiles
    per_tile = np.diff(tiles)
    assert (per_tile > CAPB).sum() >= 2                            # multi-chunk tiles at both ends
    if not square:
        assert (per_tile[:-1] == 0).any() and lens[RW - 1] == 0 and lens[RW] == 0   # a whole empty tile; empty rows at a tile's end and start
    if nb % 2:
        tail = per_tile % CAPB                                     # blocks of a tile's last chunk (0: it is a full one)
        assert ((tail % 2 == 1) | ((per_tile >= CAPB) & (CAPB % 2 == 1))).any()     # a chunk of an odd number of doubles
    first = np.flatnonzero(lens > 1)
    assert all(len(set(ja[ia[i]:ia[i + 1]])) == lens[i] for i in (0, ROW - 1, int(first[0])))   # distinct columns
    assert (np.diff(ja[ia[0]:ia[1]]) < 0).any()                    # unsorted
    return ROW, COL, ia, ja, val, lens


RAGGED_SHAPES = {"square": (True, 0), "wide": (False, 37), "tall": (False, -50)}   # COL = ROW, ROW + 37, ROW - 50


@functools.lru_cache(maxsize=None)
def ragged_case(nb, shape):
    """ragged_bsr(nb, .) in one of RAGGED_SHAPES with the vectors the tests share (read-only: built once per session):
    dict(ROW, COL, nb, ia, ja, val, lens, x (COL nb), y0, b, u0 (ROW nb))."""
    square, extra = RAGGED_SHAPES[shape]
    seed = 100 * nb + list(RAGGED_SHAPES).index(shape)
    ROW, COL, ia, ja, val, lens = ragged_bsr(nb, seed, square, extra)
    rng = np.random.default_rng(seed + 7)
    c = dict(ROW=ROW, COL=COL, nb=nb, ia=ia, ja=ja, val=val, lens=lens, x=rng.standard_normal(COL * nb),
             y0=rng.standard_normal(ROW * nb), b=rng.standard_normal(ROW * nb), u0=rng.standard_normal(ROW * nb))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


BSR_MAXGRID = 2048   # MAXGRID of csrc/solver.hip: the largest grid launch_bsr asks for


def wide_bsr(nb):
    """BSR matrix of 2048 * 4 RW + 5 block rows of two blocks, the diagonal (boosted as in ragged_bsr) and column
    (7 i + 3) mod ROW (dropped where that is the diagonal): more 4-wave tiles than the largest grid, so whatever the
    occupancy cap is, a workgroup of k_bsr_wstream takes a second tile.  -> (ROW, COL, ia, ja, val, lens)."""
    RW, _, _ = bsr_tile(nb)
    ROW = BSR_MAXGRID * 4 * RW + 5
    i = np.arange(ROW, dtype=np.int64)
    j2 = (7 * i + 3) % ROW
    lens = np.where(j2 == i, 1, 2)
    ia = np.zeros(ROW + 1, dtype=np.int32)
    ia[1:] = np.cumsum(lens)
    ja = np.empty(int(ia[-1]), dtype=np.int32)
    ja[ia[:-1]] = i
    two = lens == 2
    ja[ia[:-1][two] + 1] = j2[two]
    val = np.random.default_rng(100 + nb).standard_normal(len(ja) * nb * nb)
    val.reshape(-1, nb, nb)[ia[:-1, None], np.arange(nb), np.arange(nb)] += (3.0 * np.sqrt(4.0 * nb * lens))[:, None]
    assert (ROW + 4 * RW - 1) // (4 * RW) > BSR_MAXGRID
    return ROW, ROW, ia, ja, val, lens


def bsr_mxv_longdouble(ROW, nb, ia, ja, val, x):
    """y = A x and s = |A| |x| per scalar row in np.longdouble, independent of the oracle -> (y, s, m): m = products per row."""
    NNZ = len(ja)
    ld = np.longdouble
    xg = x.astype(ld)[(ja.astype(np.int64) * nb)[:, None] + np.arange(nb)]          # NNZ x nb
    prod = val.reshape(NNZ, nb, nb).astype(ld) * xg[:, None, :]                     # NNZ x nb x nb
    y = np.zeros((ROW, nb), dtype=ld); s = np.zeros((ROW, nb), dtype=ld)
    lens = np.diff(ia)
    rows = np.flatnonzero(lens > 0)
    if len(rows):
        y[rows] = np.add.reduceat(prod.sum(axis=2), ia[:-1][rows], axis=0)
        s[rows] = np.add.reduceat(np.abs(prod).sum(axis=2), ia[:-1][rows], axis=0)
    return y.reshape(-1), s.reshape(-1), np.repeat(lens * nb, nb)


def sum_bound_ratio(got, exact, sabs, m):
    """Worst |got - exact| / bound over the entries of a vector whose entry i is a sum of m[i] rounded terms (products, or a
    handful of elementwise operations on top of them) of absolute sum sabs[i], evaluated in double precision in ANY order, against its
    np.longdouble evaluation `exact`: the a-priori bound (m + 1) u / (1 - (m + 1) u) * sabs with u = 2^-53, plus 2^-63 |exact| for the
    80-bit side.  A ratio <= 1 passes.  Entries without terms (m == 0) must be exact; a non-finite result fails."""
    ld = np.longdouble
    m = np.asarray(m)
    u = ld(2.0) ** -53
    g = (m + 1) * u / (1 - (m + 1) * u)
    bound = g * np.asarray(sabs, dtype=ld) + ld(2.0) ** -63 * np.abs(exact)
    err = np.abs(np.asarray(got).astype(ld) - exact)
    if np.any(err[m == 0] != 0) or not np.all(np.isfinite(got)):
        return float("inf")
    nz = (m > 0) & (err > 0)
    return float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0


def csr_mxv_longdouble(ia, ja, val, x):
    """y = A x and s = |A| |x| per row of a CSR matrix in np.longdouble, independent of the oracle -> (y, s, m): m = products per row."""
    return bsr_mxv_longdouble(len(ia) - 1, 1, ia, ja, val, x)


def bsr_mxv_bound_ratio(ROW, nb, ia, ja, val, x, y):
    """Worst |y - A x| / bound over the scalar rows, with the a-priori bound of any order of double-precision evaluation of
    a row of m products, (m + 1) u / (1 - (m + 1) u) * sum |a| |x| with u = 2^-53, plus 2^-63 |y| for the 80-bit
    evaluation it is measured against (sum_bound_ratio; nb = 1 is a CSR matrix).  A ratio <= 1 passes.  Rows without blocks
    must be exact zeros."""
    yl, s, m = bsr_mxv_longdouble(ROW, nb, ia, ja, val, x)
    return sum_bound_ratio(y, yl, s, m)
