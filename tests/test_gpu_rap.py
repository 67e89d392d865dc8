"""The Galerkin product on the device (fasp_blas_dcsr_rap, BlaSpmvCSR.c:999; csrc/rap.hip.h): both forms give the reference's bytes --
IA, JA and val -- on the pinned random operands, on the levels of the three AMG setups, in row batches of a tiny arena; the setups'
opt-in switch changes no byte of a hierarchy or a solve; repeated products leave no device memory behind."""
import ctypes as C

import numpy as np
import pytest

import _libs
import _rap_cases as rc
from _libs import T, poisson7pt

pytestmark = pytest.mark.gpu
FORMS = (-1, 0, 1)


def _tune(L, key, value):
    assert L.fasp_hip_tune(key.encode(), value) == 0, key


def _product(gpu, name_or_ops):
    ops = rc.operands(name_or_ops) if isinstance(name_or_ops, str) else name_or_ops
    r, a, p, _keep = rc.as_mats(*ops)
    out = T.dCSRmat()
    st = gpu.lib().fasp_hip_dcsr_rap(C.byref(r), C.byref(a), C.byref(p), C.byref(out))
    assert st == 0, st
    assert (out.row, out.col) == (ops[4], ops[4])
    return rc.take(out, gpu.lib().fasp_dcsr_free)


@pytest.mark.parametrize("name", rc.CASES)
def test_bytes_of_the_restatement(gpu, name):
    L = gpu.lib()
    want = rc.expected(name)
    try:
        for form in FORMS:
            _tune(L, "rap_form", form)
            got = _product(gpu, name)
            info = gpu.rap_info()
            print(name, "form", form, info, "nnz", len(got[1]) // 4)
            assert got[0] == want[0], (name, form, "IA")
            assert got[1] == want[1], (name, form, "JA")
            assert got[2] == want[2], (name, form, "val")
            assert info["rows"] == rc.operands(name)[4]
            if form >= 0:   # the forced form -- but a P with a repeated column inside a row always takes form 0
                assert info["form"] == (0 if name == "repeated" else form), info
            if name == "wide" and form == 1:
                assert info["lds"] == 1   # (the short rows; the two long ones cannot fit any LDS table)
    finally:
        _tune(L, "rap_form", -1)


@pytest.mark.ref
@pytest.mark.parametrize("name", rc.CASES)
def test_bytes_of_the_compiled_reference(gpu, name):
    ref = _libs.ref()
    if ref is None:
        pytest.fail("the reference build (oracle/_ref/libfasp_ref.so) is missing")
    P = C.POINTER
    ref.fasp_blas_dcsr_rap.argtypes = [P(T.dCSRmat)] * 4; ref.fasp_blas_dcsr_rap.restype = None
    ref.fasp_dcsr_free.argtypes = [P(T.dCSRmat)]; ref.fasp_dcsr_free.restype = None
    r, a, p, _keep = rc.as_mats(*rc.operands(name))
    out = T.dCSRmat()
    ref.fasp_blas_dcsr_rap(C.byref(r), C.byref(a), C.byref(p), C.byref(out))
    want = rc.take(out, ref.fasp_dcsr_free)
    L = gpu.lib()
    try:
        for form in FORMS:
            _tune(L, "rap_form", form)
            assert _product(gpu, name) == want, (name, form)
    finally:
        _tune(L, "rap_form", -1)
    # the public void entry: the same bytes, arrays the caller releases with fasp_dcsr_free
    out = T.dCSRmat()
    L.fasp_blas_dcsr_rap(C.byref(r), C.byref(a), C.byref(p), C.byref(out))
    assert rc.take(out, L.fasp_dcsr_free) == want


@pytest.mark.parametrize("name", ["seed0", "wide"])
def test_row_batches_of_a_tiny_arena(gpu, name):
    """rap_arena_kb = 8: seed 0's tables (up to 2 KiB a row, 97 rows) need many batches in form 0; the wide case's two long rows
    (tables of 64 KiB) exceed the budget alone in either form -- a batch of one row is always allowed."""
    L = gpu.lib()
    want = rc.expected(name)
    try:
        _tune(L, "rap_arena_kb", 8)
        for form in (0, 1):
            _tune(L, "rap_form", form)
            got = _product(gpu, name)
            info = gpu.rap_info()
            print(name, "form", form, info)
            assert got == want, (name, form)
            assert info["form"] == form
            if form == 0:
                assert info["batches"] >= 3, info
            elif name == "wide":   # form 1: the short rows keep their tables in LDS, the two long ones go through the arena one by one
                assert info["batches"] == 2 and info["lds"] == 1, info
    finally:
        _tune(L, "rap_arena_kb", 262144)
        _tune(L, "rap_form", -1)


def _amg_param(gpu, amg_type, coarse_dof=None):
    amgp = gpu.param_amg_init()
    amgp.AMG_type = amg_type; amgp.smoother = T.SMOOTHER_JACOBI; amgp.relaxation = 0.6667
    if coarse_dof:
        amgp.coarse_dof = coarse_dof
    return amgp


@pytest.mark.parametrize("amg_type,levels", [(T.CLASSIC_AMG, 3), (T.SA_AMG, 3), (T.UA_AMG, 2)])
def test_levels_of_the_host_hierarchies(gpu, amg_type, levels):
    """P7(8), coarse_dof = 50: the device product of (R_l, A_l, P_l) of the host hierarchy is A_{l+1} of that hierarchy, byte for
    byte, at every level and in both forms (UA: the boolean P too)."""
    L = gpu.lib()
    ia, ja, a, f, ue = poisson7pt(8)
    H = gpu.AMG(ia, ja, a, _amg_param(gpu, amg_type, 50), host_only=True)
    try:
        assert H.num_levels == levels
        for l in range(levels - 1):
            nf, _, Aia, Aja, Av = H.matrix(l, 0)
            _, nc, Pia, Pja, Pv = H.matrix(l, 1)
            _, _, Ria, Rja, Rv = H.matrix(l, 2)
            _, _, Cia, Cja, Cv = H.matrix(l + 1, 0)
            want = (Cia.tobytes(), Cja.tobytes(), Cv.tobytes())
            for form in (0, 1):
                _tune(L, "rap_form", form)
                got = _product(gpu, ((Ria, Rja, Rv), (Aia, Aja, Av), (Pia, Pja, Pv), nf, nc))
                assert got == want, (amg_type, l, form)
                assert gpu.rap_info()["form"] == form
    finally:
        _tune(L, "rap_form", -1)
        H.close()


def _hierarchy_and_solves(gpu, ia, ja, a, f, amg_type):
    """(levels, every level's A, P, R bytes, PCG iterations and x of a resident solve, the same of the one-shot entry)"""
    H = gpu.AMG(ia, ja, a, _amg_param(gpu, amg_type))
    try:
        nl = H.num_levels
        mats = [tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in H.matrix(l, w))
                for l in range(nl) for w in range(3 if l + 1 < nl else 1)]
        itp = gpu.param_solver_init(); itp.tol = 1e-8
        st, x, hist, stats = H.solve(f, itp)
    finally:
        H.close()
    x1 = np.zeros(len(f))
    itp = gpu.param_solver_init(); itp.tol = 1e-8
    st1 = gpu.solver_dcsr_krylov_amg(ia, ja, a, f, x1, itp, _amg_param(gpu, amg_type))
    return nl, mats, (st, x.tobytes()), (st1, x1.tobytes())


@pytest.mark.parametrize("amg_type", [T.CLASSIC_AMG, T.SA_AMG, T.UA_AMG])
def test_device_rap_inside_the_setups(gpu, amg_type):
    L = gpu.lib()
    ia, ja, a, f, ue = poisson7pt(12)
    host = _hierarchy_and_solves(gpu, ia, ja, a, f, amg_type)
    assert host[2][0] > 0 and host[3][0] > 0
    count = L.fasp_hip_rap_device_count()
    try:
        _tune(L, "device_rap", 1)
        dev = _hierarchy_and_solves(gpu, ia, ja, a, f, amg_type)
    finally:
        _tune(L, "device_rap", 0)
    assert L.fasp_hip_rap_device_count() - count >= 2 * (host[0] - 1) > 0   # the resident and the one-shot setup: the switch acts
    assert dev[0] == host[0]
    assert dev[1] == host[1]
    assert dev[2] == host[2]
    assert dev[3] == host[3]
    count = L.fasp_hip_rap_device_count()
    gpu.AMG(ia, ja, a, _amg_param(gpu, amg_type)).close()
    assert L.fasp_hip_rap_device_count() == count   # off again: the host product


def _hip_runtime():
    """the HIP runtime this process has loaded (libfasp_hip.so links it)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    pytest.fail("libamdhip64 is not loaded")


def _free_bytes(hip):
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_lifetime(gpu):
    want = rc.expected("seed3")
    hip = _hip_runtime()
    assert _product(gpu, "seed3") == want   # (what the library keeps for the process is allocated by now)
    start = _free_bytes(hip)
    for i in range(20):
        gpu.lib().fasp_hip_tune(b"rap_form", i % 2)
        assert _product(gpu, "seed3") == want
    gpu.lib().fasp_hip_tune(b"rap_form", -1)
    assert _free_bytes(hip) == start
