"""Structured matrices (dSTRmat), the part that needs no GPU: struct layouts, create / alloc / cp / free, fasp_format_dstr_dcsr,
fasp_dstr_read, fasp_hip_str_form, the host preconditioner fasp_precond_dstr_diag, the numpy restatement of the four arithmetic forms
against the recorded (and, where oracle/_ref is built, the live) reference, and the refusal to compute without a device."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _libs
import _str_cases as S
from _libs import ROOT, T


@pytest.fixture(scope="module")
def G():
    return np.load(S.GOLDEN)


@pytest.fixture(scope="module")
def R():
    lib = _libs.ref()
    return S.ref_protos(lib) if lib is not None else None


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_struct_layouts_match_the_reference(G, tmp_path):
    lay = [int(v) for v in G["layout"]]
    D, Pd = T.dSTRmat, T.precond_diag_str
    mine = [C.sizeof(D)] + [getattr(D, f).offset for f in ("nx", "ny", "nz", "nxy", "nc", "ngrid", "diag", "nband", "offsets", "offdiag")]
    mine += [C.sizeof(Pd), Pd.nc.offset, Pd.diag.offset, T.MAT_STR]
    assert mine == lay
    names = ("nx", "ny", "nz", "nxy", "nc", "ngrid", "diag", "nband", "offsets", "offdiag")
    checks = [f'_Static_assert(sizeof(dSTRmat)=={lay[0]},"size");']
    checks += [f'_Static_assert(offsetof(dSTRmat,{m})=={o},"{m}");' for m, o in zip(names, lay[1:11])]
    checks += [f'_Static_assert(sizeof(precond_diag_str)=={lay[11]},"size");', f'_Static_assert(offsetof(precond_diag_str,nc)=={lay[12]},"nc");',
               f'_Static_assert(offsetof(precond_diag_str,diag)=={lay[13]},"diag");', f'_Static_assert(MAT_STR=={lay[14]},"MAT_STR");']
    src = tmp_path / "l.c"
    src.write_text('#include <stddef.h>\n#include "fasp_hip.h"\n' + "\n".join(checks) + "\nint main(void){return 0;}\n")
    subprocess.run(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_create_alloc_cp_free(fa):
    L = fa.lib()
    offs = np.array([-1, 1, -5, 5, -20, 20, 75], dtype=np.int32)
    A = L.fasp_dstr_create(5, 4, 3, 2, 7, T.ip(offs))
    assert (A.nx, A.ny, A.nz, A.nxy, A.ngrid, A.nc, A.nband) == (5, 4, 3, 20, 60, 2, 7)
    assert [A.offsets[b] for b in range(7)] == list(offs)
    assert np.all(np.ctypeslib.as_array(A.diag, shape=(240,)) == 0.0)
    for b in range(6):
        assert np.all(np.ctypeslib.as_array(A.offdiag[b], shape=((60 - abs(int(offs[b]))) * 4,)) == 0.0)
    assert not A.offdiag[6]   # |offset| >= ngrid: a legal band without entries
    r = np.random.default_rng(5)
    np.ctypeslib.as_array(A.diag, shape=(240,))[:] = r.standard_normal(240)
    for b in range(6):
        m = (60 - abs(int(offs[b]))) * 4
        np.ctypeslib.as_array(A.offdiag[b], shape=(m,))[:] = r.standard_normal(m)
    B = T.dSTRmat()
    L.fasp_dstr_alloc(5, 4, 3, 20, 60, 7, 2, T.ip(offs), C.byref(B))
    assert (B.nx, B.ny, B.nz, B.nxy, B.ngrid, B.nc, B.nband) == (5, 4, 3, 20, 60, 2, 7)
    B.offsets[0] = 99
    L.fasp_dstr_cp(C.byref(A), C.byref(B))
    assert [B.offsets[b] for b in range(7)] == list(offs)
    assert np.array_equal(np.ctypeslib.as_array(B.diag, shape=(240,)), np.ctypeslib.as_array(A.diag, shape=(240,)))
    for b in range(6):
        m = (60 - abs(int(offs[b]))) * 4
        assert np.array_equal(np.ctypeslib.as_array(B.offdiag[b], shape=(m,)), np.ctypeslib.as_array(A.offdiag[b], shape=(m,)))
    assert L.fasp_hip_str_form(C.byref(B)) == S.FORM_G
    for M in (A, B):
        L.fasp_dstr_free(C.byref(M))
        assert (M.nx, M.ny, M.nz, M.nxy, M.ngrid, M.nc, M.nband) == (0,) * 7 and not M.diag and not M.offsets
    Z = L.fasp_dstr_create(3, 1, 1, 1, 0, None)   # no bands at all
    assert Z.ngrid == 3 and Z.nband == 0 and L.fasp_hip_str_form(C.byref(Z)) == S.FORM_G
    L.fasp_dstr_free(C.byref(Z))


@pytest.mark.parametrize("case", S.op_cases(), ids=lambda c: c["name"])
def test_format_dstr_dcsr_bytes(fa, G, R, case):
    L = fa.lib()
    diag, bands = S.build(case)
    A, keep = S.as_str(case, diag, bands)
    B = T.dCSRmat()
    assert L.fasp_format_dstr_dcsr(C.byref(A), C.byref(B)) == 0
    ngrid, nc = A.ngrid, A.nc
    assert B.row == B.col == ngrid * nc
    ia, ja, val = T.csr_arrays(B)
    sha = np.frombuffer(hashlib.sha256(ia.tobytes() + ja.tobytes() + val.tobytes()).digest(), dtype=np.uint8)
    k = list(G["csr_names"]).index(case["name"])
    assert np.array_equal(sha, G["csr_sha"][k])
    if R is not None:
        Br = T.dCSRmat()
        R.fasp_format_dstr_dcsr(C.byref(A), C.byref(Br))
        for mine, theirs in zip((ia, ja, val), T.csr_arrays(Br)):
            assert mine.tobytes() == theirs.tobytes()
    # the product of the converted matrix is the product of A (to rounding), and every row starts with its diagonal entry
    x, y0 = S.vectors(case)
    y = np.array([np.dot(val[ia[i]:ia[i + 1]], x[ja[ia[i]:ia[i + 1]]]) for i in range(B.row)])
    yl = S.mxv_longdouble(case, diag, bands, x)
    assert np.max(np.abs(y - yl.astype(np.float64))) <= 1e-12 * max(1.0, float(np.max(np.abs(yl))))
    assert np.array_equal(ja[ia[:-1]], np.arange(B.row))
    L.fasp_dcsr_free(C.byref(B))


def test_format_dstr_dcsr_refuses(fa):
    L = fa.lib()
    A, keep = T.as_str(3, 2, 1, 1, [1, 1], np.ones(6), [np.ones(5), np.ones(5)])   # a repeated offset
    B = T.dCSRmat()
    assert L.fasp_format_dstr_dcsr(C.byref(A), C.byref(B)) == T.ERROR_INPUT_PAR and not B.IA
    assert L.fasp_format_dstr_dcsr(C.byref(A), None) == T.ERROR_INPUT_PAR


def test_dstr_read(fa, tmp_path):
    L = fa.lib()
    tok = open(S.DATA_FILE).read().split()
    A = T.dSTRmat()
    assert L.fasp_dstr_read(S.DATA_FILE.encode(), C.byref(A)) == 0
    assert (A.nx, A.ny, A.nz, A.nxy, A.ngrid, A.nc, A.nband) == (5, 4, 3, 20, 60, 2, 6) == tuple(
        [int(tok[0]), int(tok[1]), int(tok[2]), 20, 60, int(tok[3]), int(tok[4])])
    at = 5
    n = int(tok[at]); at += 1
    assert n == 240
    assert np.array_equal(np.ctypeslib.as_array(A.diag, shape=(n,)), np.array([float(t) for t in tok[at:at + n]])); at += n
    case = [c for c in S.op_cases() if c["name"] == "c3d_5x4x3_nc2"][0]
    diag, bands = S.build(case)
    assert np.allclose(np.ctypeslib.as_array(A.diag, shape=(240,)), diag, rtol=1e-6, atol=0)   # the writer keeps seven digits
    for b in range(6):
        off, n = int(tok[at]), int(tok[at + 1]); at += 2
        assert A.offsets[b] == off == case["offsets"][b] and n == (60 - abs(off)) * 4
        assert np.array_equal(np.ctypeslib.as_array(A.offdiag[b], shape=(n,)), np.array([float(t) for t in tok[at:at + n]])); at += n
    assert at == len(tok)
    assert L.fasp_hip_str_form(C.byref(A)) == S.FORM_N
    L.fasp_dstr_free(C.byref(A))
    # comment lines at the head are skipped; a missing file, a short file and a wrong band length are refused
    text = open(S.DATA_FILE).read()
    p = tmp_path / "c.dat"; p.write_text("% a comment\n" + text)
    assert L.fasp_dstr_read(str(p).encode(), C.byref(A)) == 0 and A.ngrid == 60
    L.fasp_dstr_free(C.byref(A))
    assert L.fasp_dstr_read(str(tmp_path / "none.dat").encode(), C.byref(A)) == -10   # ERROR_OPEN_FILE
    p = tmp_path / "short.dat"; p.write_text(" ".join(tok[:-3]))
    assert L.fasp_dstr_read(str(p).encode(), C.byref(A)) == -11 and not A.diag        # ERROR_WRONG_FILE
    bad = list(tok); bad[5] = "239"
    p = tmp_path / "len.dat"; p.write_text(" ".join(bad))
    assert L.fasp_dstr_read(str(p).encode(), C.byref(A)) == -11
    assert L.fasp_dstr_read(None, C.byref(A)) == T.ERROR_INPUT_PAR


@pytest.mark.parametrize("case", S.op_cases() + S.form_only_cases(), ids=lambda c: c["name"])
def test_str_form(fa, case):
    diag, bands = S.build(case)
    A, keep = S.as_str(case, diag, bands)
    assert fa.lib().fasp_hip_str_form(C.byref(A)) == case["form"]


def test_str_form_solve_systems(fa):
    L = fa.lib()
    for sym in (True, False):
        c, diag, bands, b = S.scalar_system(sym)
        A, keep = S.as_str(c, diag, bands)
        assert L.fasp_hip_str_form(C.byref(A)) == S.FORM_S
        for nc in S.BLOCK_NC:
            c, diag, bands, b = S.block_system(nc, sym)
            A, keep = S.as_str(c, diag, bands)
            assert L.fasp_hip_str_form(C.byref(A)) == c["form"]


def test_str_form_refusals(fa):
    L = fa.lib()
    ok = dict(name="ok", nx=5, ny=4, nz=3, nc=2, offsets=[-1, 1, -5, 5, -20, 20])
    diag, bands = S.build(ok)
    A, keep = S.as_str(ok, diag, bands)
    assert L.fasp_hip_str_form(C.byref(A)) == S.FORM_N
    assert L.fasp_hip_str_form(None) == T.ERROR_INPUT_PAR
    for field, value in (("nc", 0), ("nc", 8), ("nc", -1), ("nband", -1)):
        A, keep = S.as_str(ok, diag, bands)
        setattr(A, field, value)
        assert L.fasp_hip_str_form(C.byref(A)) == T.ERROR_INPUT_PAR, (field, value)
    for offsets in ([-1, 1, 0, 5, -20, 20], [-1, 1, -5, 5, 5, 20], [3, 3]):
        c = dict(ok, offsets=offsets)
        d2, b2 = S.build(c)
        A, keep = S.as_str(c, d2, b2)
        assert L.fasp_hip_str_form(C.byref(A)) == T.ERROR_INPUT_PAR, offsets
    A, keep = S.as_str(ok, diag, bands)
    A.diag = None
    assert L.fasp_hip_str_form(C.byref(A)) == T.ERROR_INPUT_PAR
    A, keep = S.as_str(ok, diag, bands)
    A.offsets = None
    assert L.fasp_hip_str_form(C.byref(A)) == T.ERROR_INPUT_PAR
    A, keep = S.as_str(ok, diag, bands)
    A.offdiag[2] = None
    assert L.fasp_hip_str_form(C.byref(A)) == T.ERROR_INPUT_PAR


@pytest.mark.parametrize("case", S.op_cases(), ids=lambda c: c["name"])
def test_restated_forms_are_the_reference(G, R, case):
    """The four forms as DESIGN.md section 3.6 states them (model_aAxpy), bit for bit the recorded reference results -- and the live
    reference's where it is built."""
    diag, bands = S.build(case)
    x, y0 = S.vectors(case)
    keys = list(G["op_keys"])
    for alpha in S.ALPHAS:
        y = S.model_aAxpy(case, diag, bands, alpha, x, y0)
        k = keys.index(f"{case['name']}/{alpha}")
        assert np.array_equal(S.digest(y), G["op_sha"][k]), alpha
        lo, hi = G["op_small_off"][k], G["op_small_off"][k + 1]
        assert hi - lo == (y.size if y.size <= 420 else 0)
        if hi > lo:
            assert np.array_equal(_bits(y), _bits(G["op_small"][lo:hi])), alpha
        if R is not None and case["ref_ok"]:
            assert np.array_equal(_bits(y), _bits(S.ref_aAxpy(R, case, diag, bands, alpha, x, y0))), alpha
        if alpha == 0.0 and case["form"] == S.FORM_G:
            assert np.array_equal(_bits(y), _bits(y0))


@pytest.mark.parametrize("nc", S.DINV_NC)
def test_precond_dstr_diag_host(fa, G, R, nc):
    L = fa.lib()
    diag, r = S.dinv_inputs(nc)
    dinv = np.array(G[f"dinv_{nc}"])
    z = np.full_like(r, np.nan)
    dd = T.precond_diag_str(nc, T.dvector(dinv.size, T.dp(dinv)))
    L.fasp_precond_dstr_diag(T.dp(r), T.dp(z), C.byref(dd))
    assert np.array_equal(_bits(z), _bits(G[f"dinv_z_{nc}"]))
    if R is not None:
        assert np.array_equal(_bits(dinv), _bits(S.ref_dinv(R, nc, diag)))
        zr = np.zeros_like(r)
        R.fasp_precond_dstr_diag(T.dp(r), T.dp(zr), C.byref(dd))
        assert np.array_equal(_bits(z), _bits(zr))


def test_precond_dstr_diag_sums_from_zero_where_the_reference_does(fa):
    """nc = 1 and 6 run the general text of fasp_blas_smat_mxv, which starts from 0.0: a product of -0.0 comes out +0.0."""
    L = fa.lib()
    for nc, want_negative_zero in ((1, False), (6, False), (2, True), (7, True)):
        dinv = np.full(nc * nc, -1.0)   # every product is -0.0
        r = np.zeros(nc)
        z = np.full(nc, np.nan)
        dd = T.precond_diag_str(nc, T.dvector(dinv.size, T.dp(dinv)))
        L.fasp_precond_dstr_diag(T.dp(r), T.dp(z), C.byref(dd))
        assert np.all(z == 0.0) and np.all(np.signbit(z) == want_negative_zero), (nc, z)


_REFUSE = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import ctypes as C
import numpy as np
import faspsolver_amd as fa
import _str_cases as S
from _libs import T
L = fa.lib()
c, diag, bands, b = S.scalar_system(True)
A, keep = S.as_str(c, diag, bands)
x = np.zeros_like(b)
if sys.argv[1] == "mxv":
    L.fasp_blas_dstr_mxv(C.byref(A), T.dp(b), T.dp(x))
elif sys.argv[1] == "time":
    print("time", L.fasp_hip_time_str_mxv(C.byref(A), 3))
    sys.exit(0)
else:
    print("status", S.solve_with(L, "fasp_solver_dstr_" + sys.argv[1], c, diag, bands, b, T.SOLVER_CG, 25)[0])
print("returned")
"""


def test_str_entries_refuse_without_gpu(fa, tmp_path):
    """As their CSR siblings: the products and the Krylov entries end the process with the no-device message, the timer returns -1."""
    if fa.available():
        pytest.skip("a GPU is present")
    script = tmp_path / "refuse.py"
    script.write_text(_REFUSE.format(root=ROOT, tests=os.path.join(ROOT, "tests")))
    for what in ("mxv", "krylov", "krylov_diag"):
        out = subprocess.run([sys.executable, str(script), what], capture_output=True, text=True)
        assert out.returncode == (T.ERROR_MISC & 0xFF) and "returned" not in out.stdout, (what, out.stdout, out.stderr)
        assert "no CPU fallback" in out.stderr
    out = subprocess.run([sys.executable, str(script), "time"], capture_output=True, text=True)
    assert out.returncode == 0 and "time -1.0" in out.stdout, out.stdout + out.stderr
