"""ILU factorisation on the host (csrc/ilu_setup.cpp) against the compiled reference: fasp_ilu_dcsr_setup for ILUk / ILUt /
ILUtp over a grid of matrices and parameters must give the same bytes (ijlu, luval, nzlu, iperm, work, status, and the
caller's A after the call -- ILUtp renumbers its columns), the same failures, and fasp_param_ilu_init the same struct.
No GPU needed; without one the ILU compute entry points refuse to run."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _libs
from _libs import DATA, ROOT, T, poisson7pt, read_csr

P = C.POINTER
ref_needed = pytest.mark.skipif(not _libs.have_ref() and not os.path.isdir(_libs.REF_TREE),
                                reason="oracle/_ref/libfasp_ref.so (the reference build) is absent")


def ilu_protos(L):
    """argtypes of the ILU entry points on a library (ours or the reference build)."""
    L.fasp_param_ilu_init.argtypes = [P(T.ILU_param)]
    L.fasp_param_ilu_init.restype = None
    L.fasp_ilu_dcsr_setup.argtypes = [P(T.dCSRmat), P(T.ILU_data), P(T.ILU_param)]
    L.fasp_ilu_dcsr_setup.restype = C.c_short
    L.fasp_ilu_data_free.argtypes = [P(T.ILU_data)]
    L.fasp_ilu_data_free.restype = None
    for f in ("fasp_precond_ilu", "fasp_precond_ilu_forward", "fasp_precond_ilu_backward"):
        getattr(L, f).argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
        getattr(L, f).restype = None
    L.fasp_smoother_dcsr_ilu.argtypes = [P(T.dCSRmat), P(T.dvector), P(T.dvector), C.c_void_p]
    L.fasp_smoother_dcsr_ilu.restype = None
    L.fasp_solver_dcsr_krylov_ilu.argtypes = [P(T.dCSRmat), P(T.dvector), P(T.dvector), P(T.ITS_param), P(T.ILU_param)]
    L.fasp_solver_dcsr_krylov_ilu.restype = C.c_int
    L.fasp_param_solver_init.argtypes = [P(T.ITS_param)]
    L.fasp_param_solver_init.restype = None
    L.fasp_dmtxsym_read.argtypes = [C.c_char_p, P(T.dCSRmat)]
    return L


class Csr:
    """A dCSRmat over numpy arrays owned by this object (the library may renumber JA in place)."""
    def __init__(self, ia, ja, a):
        self.ia = np.ascontiguousarray(ia, dtype=np.int32).copy()
        self.ja = np.ascontiguousarray(ja, dtype=np.int32).copy()
        self.a = np.ascontiguousarray(a, dtype=np.float64).copy()
        n = len(self.ia) - 1
        self.M = T.dCSRmat(n, n, len(self.a), self.ia.ctypes.data_as(T.c_int_p), self.ja.ctypes.data_as(T.c_int_p),
                           self.a.ctypes.data_as(T.c_double_p))


def nos7():
    L = ilu_protos(_libs.ref() if _libs.have_ref() else __import__("faspsolver_amd").lib())
    A = T.dCSRmat()
    assert L.fasp_dmtxsym_read((DATA + "/nos7.mtx").encode(), C.byref(A)) == 0
    ia, ja, a = T.csr_arrays(A)
    return ia.copy(), ja.copy(), a.copy()


def nonsym_unsorted(n=300, per_row=6, seed=7):
    """nonsymmetric, banded, diagonally dominant but for every seventh row (a weak pivot), columns in random order inside each row"""
    rng = np.random.default_rng(seed)
    ia, ja, a = [0], [], []
    for i in range(n):
        near = np.arange(max(0, i - 12), min(n, i + 13))   # a band: the fill of ILUk(3) stays inside the allocated entries
        cols = set(rng.choice(near, size=per_row, replace=False).tolist()) - {i}
        ent = [(c, rng.uniform(-1.0, 1.0)) for c in cols] + [(i, 0.1 if i % 7 == 3 else 2.0 * per_row)]  # weak pivots: ILUtp swaps
        rng.shuffle(ent)
        ja += [c for c, _ in ent]; a += [v for _, v in ent]; ia.append(len(ja))
    return np.array(ia, np.int32), np.array(ja, np.int32), np.array(a)


def matrices():
    out = {}
    out["FD"] = read_csr(DATA + "/csrmat_FD.dat")
    out["FE"] = read_csr(DATA + "/csrmat_FE.dat")
    out["NOS7"] = nos7()
    for n in (8, 16):
        ia, ja, a, _, _ = poisson7pt(n)
        out[f"P7_{n}"] = (ia, ja, a)
    out["nonsym"] = nonsym_unsorted()
    return out


PARAMS = [("ILUk", T.ILUk, lf, 1e-3, 0.01) for lf in (0, 1, 2, 3)] + \
         [("ILUt", T.ILUt, 2, dt, 0.01) for dt in (1e-3, 1e-2)] + \
         [("ILUtp", T.ILUtp, 2, 1e-3, pt) for pt in (0.01, 0.5)]


def ilu_param(L, typ, lfil, droptol, permtol):
    p = T.ILU_param()
    L.fasp_param_ilu_init(C.byref(p))
    p.ILU_type, p.ILU_lfil, p.ILU_droptol, p.ILU_permtol = typ, lfil, droptol, permtol
    return p


def setup(L, arrays, prm):
    """run fasp_ilu_dcsr_setup of library L on a fresh copy of the matrix; returns (status, data, csr) -- free with L."""
    A = Csr(*arrays)
    d = T.ILU_data()
    st = L.fasp_ilu_dcsr_setup(C.byref(A.M), C.byref(d), C.byref(prm))
    return st, d, A


def snapshot(st, d, A):
    """the bytes a caller sees after the setup"""
    out = {"status": int(st), "IA": A.ia.tobytes(), "JA": A.ja.tobytes(), "val": A.a.tobytes()}
    if st == 0:
        nz = d.nzlu
        out["nzlu"] = nz
        out["ijlu"] = np.ctypeslib.as_array(d.ijlu, (nz,)).tobytes()
        out["luval"] = np.ctypeslib.as_array(d.luval, (nz,)).tobytes()
        out["nwork"] = d.nwork
        out["work"] = np.ctypeslib.as_array(d.work, (d.nwork,)).tobytes()
        out["rowcol"] = (d.row, d.col, d.type)
        if d.type == T.ILUtp:
            out["iperm"] = np.ctypeslib.as_array(d.iperm, (2 * d.row,)).tobytes()
    return out


@pytest.fixture(scope="module")
def libs(fa):
    ref = _libs.ref()
    if ref is None:
        pytest.skip("reference build absent")
    return ilu_protos(fa.lib()), ilu_protos(ref)


@pytest.fixture(scope="module")
def mats():
    return matrices()


@pytest.mark.ref
@ref_needed
@pytest.mark.parametrize("mname", ["FD", "FE", "NOS7", "P7_8", "P7_16", "nonsym"])
@pytest.mark.parametrize("pname,typ,lfil,droptol,permtol", PARAMS)
def test_setup_matches_reference(libs, mats, mname, pname, typ, lfil, droptol, permtol):
    ours, ref = libs
    arrays = mats[mname]
    res = []
    for L in (ours, ref):
        st, d, A = setup(L, arrays, ilu_param(L, typ, lfil, droptol, permtol))
        res.append(snapshot(st, d, A))
        L.fasp_ilu_data_free(C.byref(d))
        if typ == T.ILUtp and st == 0:   # fasp_ilu_data_free numbers the columns back
            assert A.ja.tobytes() == np.ascontiguousarray(arrays[1], dtype=np.int32).tobytes()
    assert res[0]["status"] == 0 == res[1]["status"]
    assert res[0].keys() == res[1].keys()
    for k in res[1]:
        assert res[0][k] == res[1][k], (mname, pname, k)
    if typ == T.ILUtp and permtol == 0.5 and mname == "nonsym":
        assert res[0]["JA"] != np.ascontiguousarray(arrays[1], dtype=np.int32).tobytes()  # pivoting happened: A renumbered


def _arrow(n=200):
    """dense first row and column: ILU(1) fills the whole matrix -- more than the entries the setup allocates"""
    ia, ja, a = [0], [], []
    for i in range(n):
        cols = list(range(n)) if i == 0 else [0, i]
        ja += cols; a += [float(n) if c == i else -1.0 for c in cols]; ia.append(len(ja))
    return np.array(ia, np.int32), np.array(ja, np.int32), np.array(a)


FAILING = [
    ("negative lfil", T.ILUk, -1, lambda: read_csr(DATA + "/csrmat_FD.dat")),
    ("ILUk zero pivot", T.ILUk, 0, lambda: (np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.array([1.0, 1.0]))),
    ("ILUtp zero row", T.ILUtp, 2, lambda: (np.array([0, 1, 1, 2], np.int32), np.array([0, 2], np.int32), np.array([1.0, 1.0]))),
    ("ILUk storage", T.ILUk, 1, _arrow),
    ("ILUt storage", T.ILUt, 2, lambda: _arrow(1000)),
]


@pytest.mark.ref
@ref_needed
@pytest.mark.parametrize("case,typ,lfil,make", FAILING, ids=[c[0] for c in FAILING])
def test_failing_setup_matches_reference(libs, case, typ, lfil, make):
    ours, ref = libs
    arrays = make()
    res = []
    for L in (ours, ref):
        prm = ilu_param(L, typ, lfil, 0.0 if case == "ILUt storage" else 1e-3, 0.01)
        st, d, A = setup(L, arrays, prm)
        res.append(snapshot(st, d, A))
        L.fasp_ilu_data_free(C.byref(d))
    assert res[0]["status"] == T.ERROR_SOLVER_ILUSETUP == res[1]["status"]
    assert res[0] == res[1]


@pytest.mark.ref
@ref_needed
def test_param_ilu_init_matches_reference(libs):
    ours, ref = libs
    a, b = T.ILU_param(), T.ILU_param()
    C.memset(C.byref(a), 0x5A, C.sizeof(a)); C.memset(C.byref(b), 0x5A, C.sizeof(b))
    ours.fasp_param_ilu_init(C.byref(a)); ref.fasp_param_ilu_init(C.byref(b))
    assert bytes(a) == bytes(b)
    assert (a.ILU_type, a.ILU_lfil) == (T.ILUk, 2)


def test_ilu_abi_layout():
    assert C.sizeof(T.ILU_param) == 32
    assert C.sizeof(T.ILU_data) == 136


_REFUSE = r"""
import ctypes as C, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import faspsolver_amd as fa
from faspsolver_amd import _types as T
from test_ilu_setup import Csr, ilu_protos, ilu_param
L = ilu_protos(fa.lib())
ia, ja, a, f, ue = fa.poisson7pt(4)
A = Csr(ia, ja, a)
d = T.ILU_data()
assert L.fasp_ilu_dcsr_setup(C.byref(A.M), C.byref(d), C.byref(ilu_param(L, T.ILUk, 0, 1e-3, 0.01))) == 0
if sys.argv[1] == "solver":
    x = np.zeros(len(f)); b = np.array(f)
    it = T.ITS_param(); L.fasp_param_solver_init(C.byref(it))
    bv = T.dvector(len(f), b.ctypes.data_as(T.c_double_p)); xv = T.dvector(len(f), x.ctypes.data_as(T.c_double_p))
    st = L.fasp_solver_dcsr_krylov_ilu(C.byref(A.M), C.byref(bv), C.byref(xv), C.byref(it), C.byref(ilu_param(L, T.ILUk, 0, 1e-3, 0.01)))
    print("status", st, "x untouched", bool(np.all(x == 0.0)))
else:
    r = np.ones(len(f)); z = np.zeros(len(f))
    L.fasp_precond_ilu(r.ctypes.data_as(T.c_double_p), z.ctypes.data_as(T.c_double_p), C.cast(C.byref(d), C.c_void_p))
    print("returned")
"""


def test_ilu_apply_refuses_without_gpu(fa, tmp_path):
    if fa.available():
        pytest.skip("a GPU is present")
    script = tmp_path / "refuse.py"
    script.write_text(_REFUSE.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    out = subprocess.run([sys.executable, str(script), "solver"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert f"status {T.ERROR_MISC} x untouched True" in out.stdout
    out = subprocess.run([sys.executable, str(script), "precond"], capture_output=True, text=True)
    assert out.returncode == (T.ERROR_MISC & 0xFF) and "returned" not in out.stdout
    assert "no CPU fallback" in out.stderr
