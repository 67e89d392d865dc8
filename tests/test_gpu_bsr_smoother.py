"""The block smoother entries on the device (csrc/bsr_sweep.hip.h) against tests/golden/bsr_smoothers.npz, the compiled reference's results:
every case through its public entry and through the resident handle, with one launch per level and with the single launch, EQUAL BIT FOR BIT
(the reference's loops are deterministic, every row is summed in its own lane in storage order, nothing is fused).  Then the form the depth
selects, the handle's lifetime, the block AMG cycle with fasp_hip_tune("bsr_cycle_sweep", 1) against the default sweeps, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import _bsr_smoother_cases as S
from _libs import T, bsr_params, poisson7pt_bsr

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def golden():
    return np.load(S.GOLDEN)


@pytest.fixture(scope="module")
def lib(gpu):
    L = S.protos(gpu.lib())
    yield L
    L.fasp_hip_tune(b"bsr_sweep_form", -1)
    L.fasp_hip_tune(b"bsr_cycle_sweep", 0)


def handle_of(gpu, case):
    ia, ja, val, nb = S.matrix(case["mat"])
    order, mark = S.order_args(case)
    fixed = S.ENTRIES[case["entry"]][2]
    if fixed:
        order, mark = (S.ASCEND if fixed == "asc" else S.DESCEND), None
    d = None if case["entry"] in S.SELF_INVERTING or S.ENTRIES[case["entry"]][0] == S.IDENT else S.given_diaginv(case)
    return gpu.BSRSmoother(ia, ja, val, nb, order, mark, d)


@pytest.mark.parametrize("cid", [c["id"] for c in S.CASES])
def test_every_case_equals_the_reference_bit_for_bit(gpu, lib, golden, cid):
    case = S.BY_ID[cid]
    want = bits(golden[cid + "/out"])
    kind = S.ENTRIES[case["entry"]][0]
    swept = S.sequence(case) is not None
    try:
        for form in (0, 1):
            lib.fasp_hip_tune(b"bsr_sweep_form", form)
            assert np.array_equal(bits(S.call_entry(lib, case)), want), ("entry", form)
            if kind == S.JACOBI:
                continue
            H = handle_of(gpu, case)
            try:
                b, u = S.start_of(case)
                assert H.apply(b, u, kind, case["w"]) == 0
                assert np.array_equal(bits(u), want), ("handle", form)
                if swept:
                    assert H.info()["last_form"] == form
            finally:
                H.free()
    finally:
        lib.fasp_hip_tune(b"bsr_sweep_form", -1)


# the auto form: the single launch for plans deeper than 64 levels of at most 8 chunks on average (csrc/bsr_sweep.hip.h)
@pytest.mark.parametrize("mat,order,levels,single", [("p7:6:3", "asc", 16, 0), ("p7:6:3", "rb", 2, 0), ("p7:10:3", "asc", 28, 0),
                                                     ("chain:64", "asc", 64, 0), ("chain:65", "asc", 65, 1), ("chain:129", "desc", 129, 1)])
def test_auto_form_follows_the_depth(gpu, lib, mat, order, levels, single):
    lib.fasp_hip_tune(b"bsr_sweep_form", -1)
    case = dict(mat=mat, entry="gs1", order=order, w=1.0, u0="rand")
    H = handle_of(gpu, case)
    try:
        i = H.info()
        assert (i["levels"], i["auto_form"], i["last_form"]) == (levels, single, -1)
        assert i["chunks"] >= -(-(len(S.matrix(mat)[0]) - 1) // 64) and i["nent"] >= 0 and i["padded"] >= 0
        b, u = S.start_of(case)
        assert H.apply(b, u, S.GS, 1.0) == 0 and H.info()["last_form"] == single
        assert np.array_equal(bits(u), bits(S.restated(case)))
    finally:
        H.free()


def test_two_applies_on_one_handle_equal_two_one_shot_calls(gpu, lib):
    case = S.BY_ID["p7:6:3|sor_order|perm|1.3|rand"]
    ia, ja, val, nb = S.matrix(case["mat"])
    A, keep = T.as_bsr(ia.copy(), ja.copy(), val.copy(), nb)
    b, u1 = S.start_of(case)
    d = S.given_diaginv(case)
    mark = S.mark_of(case["mat"], "perm")
    bv, bk = T.as_vec(b.copy())
    uv = T.dvector(len(u1), T.dp(u1))
    for _ in range(2):
        lib.fasp_smoother_dbsr_sor_order(C.byref(A), C.byref(bv), C.byref(uv), T.dp(d), mark.ctypes.data_as(T.c_int_p), 1.3)
    H = handle_of(gpu, case)
    try:
        _, u2 = S.start_of(case)
        assert H.apply(b, u2, S.SOR, 1.3) == 0 and H.apply(b, u2, S.SOR, 1.3) == 0
    finally:
        H.free()
    assert np.array_equal(bits(u1), bits(u2)) and not np.array_equal(bits(u1), bits(S.start_of(case)[1]))


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


def test_lifetime(gpu, lib):
    case = S.BY_ID["p7:10:3|sor_order|perm|1.3|rand"]

    def one_round():
        H = handle_of(gpu, case)
        b, u = S.start_of(case)
        assert H.apply(b, u, S.SOR, 1.3) == 0
        H.free()
        return u.tobytes()

    hip = _hip_runtime()
    first = one_round()   # (work space the library keeps for the process is allocated by now)
    start = _free_bytes(hip)
    for _ in range(20):
        assert one_round() == first
    assert _free_bytes(hip) == start


def _block_params(smoother, ilu_levels):
    _, p = bsr_params()
    p.coarse_dof = 50
    p.ILU_levels, p.ILU_lfil = ilu_levels, 0
    p.presmooth_iter = p.postsmooth_iter = 1
    p.smoother = smoother
    p.relaxation = 1.1 if smoother in (T.SMOOTHER_SOR, T.SMOOTHER_SSOR) else 1.0
    return p


@pytest.mark.parametrize("ilu_levels", [0, 1])
@pytest.mark.parametrize("smoother", [T.SMOOTHER_GS, T.SMOOTHER_SGS, T.SMOOTHER_SOR, T.SMOOTHER_SSOR])
@pytest.mark.parametrize("nb", [1, 3, 5])
def test_cycle_sweeps_through_the_plan_equal_the_default_sweeps(gpu, lib, nb, smoother, ilu_levels):
    ia, ja, val, nb = poisson7pt_bsr(6, S.block(nb))
    r = np.random.default_rng(40 + nb).uniform(-1.0, 1.0, (len(ia) - 1) * nb)
    z = {}
    try:
        for key in (0, 1):
            lib.fasp_hip_tune(b"bsr_cycle_sweep", key)
            G = gpu.BSRAMG(ia, ja, val, nb, _block_params(smoother, ilu_levels))
            try:
                assert G.num_levels >= 2
                z[key] = G.precond(r)
            finally:
                G.free()
    finally:
        lib.fasp_hip_tune(b"bsr_cycle_sweep", 0)
    assert np.any(z[0] != 0.0) and np.all(np.isfinite(z[0]))
    assert np.array_equal(bits(z[0]), bits(z[1]))


def test_refusals(gpu, lib):
    ia, ja, val, nb = S.matrix("p7:6:3")
    ROW = len(ia) - 1
    h = C.c_void_p()
    A, keep = T.as_bsr(ia, ja, val, nb)
    bad = np.arange(ROW, dtype=np.int32); bad[7] = 8
    assert lib.fasp_hip_bsr_smoother_create(C.byref(h), C.byref(A), None, 0, bad.ctypes.data_as(T.c_int_p)) == T.ERROR_INPUT_PAR and not h
    A8, keep8 = T.as_bsr(ia, ja, np.zeros(len(ja) * 64), 8)
    assert lib.fasp_hip_bsr_smoother_create(C.byref(h), C.byref(A8), None, S.ASCEND, None) == gpu.ERROR_NUM_BLOCKS and not h
    H = gpu.BSRSmoother(ia, ja, val, nb)
    try:
        b, u0 = S.inputs("p7:6:3")
        u = u0.copy()
        assert H.apply(b[:-1], u, S.GS, 1.0) == T.ERROR_INPUT_PAR            # b shorter than ROW nb
        assert H.apply(b, u[:-1].copy(), S.GS, 1.0) == T.ERROR_INPUT_PAR
        assert H.apply(b, u, 3, 1.0) == T.ERROR_INPUT_PAR
        assert np.array_equal(bits(u), bits(u0))
        assert H.apply(b, u, S.GS, 1.0) == 0 and not np.array_equal(bits(u), bits(u0))
    finally:
        H.free()
