"""The safe-net Krylov solvers on the device against the recorded reference (tests/golden/safe_krylov.npz, written by
tools/gen_golden_safe_krylov.py): the return code, x within max(1e-10, 100 sens) max|x_ref|, the restore line exactly when the
reference printed one and with its iteration, a finite x in every NaN case -- in the fused form and over the unfused BLAS-1 launches
(fasp_hip_tune("safe_fused", 0)) -- and, with an AMG handle as the preconditioner, agreement with the non-safe entries.

The floor 1e-10 is the convention of tests/test_plugin_krylov.py; the factor 100 is there because the device's tree reductions perturb
every iteration, where the recorded perturbation of b acts once."""
import ctypes as C
import functools

import numpy as np
import pytest

import _safe_krylov_cases as K
from _libs import T

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    G = np.load(K.GOLDEN)
    keys = [str(k) for k in G["keys"]]
    return {k: (int(G["code"][j]), int(G["restore"][j]), float(G["sens"][j]), G[f"x_{j}"]) for j, k in enumerate(keys)}


CASES = {c["key"]: c for c in K.cases()}
KEYS = [str(k) for k in np.load(K.GOLDEN)["keys"]]


@pytest.fixture(scope="module")
def L(gpu):
    lib = gpu.lib()
    yield lib
    lib.fasp_hip_tune(b"safe_fused", 1)


@pytest.mark.parametrize("fused", (1, 0))
@pytest.mark.parametrize("key", KEYS)
def test_case_against_the_reference(L, key, fused):
    code, restore, sens, x_ref = golden()[key]
    case = CASES[key]
    assert L.fasp_hip_tune(b"safe_fused", fused) == 0
    try:
        with K.Captured() as cap:
            st, x, calls = K.run(L, case)
    finally:
        L.fasp_hip_tune(b"safe_fused", 1)
    got = K.restore_iteration(cap.text)
    scale = float(np.max(np.abs(x_ref)))
    err = float(np.max(np.abs(x - x_ref))) if np.all(np.isfinite(x)) else float("inf")
    bound = max(1e-10, 100.0 * sens) * scale
    print(f"{key} fused={fused}: code {st} (reference {code}), restore {got} ({restore}), max|x - x_ref| = {err:.3e}, bound {bound:.3e}")
    assert np.all(np.isfinite(x))
    assert st == code
    assert got == restore
    assert err <= bound


@pytest.mark.parametrize("key", [k for k in KEYS if CASES[k]["fmt"] == "csr" and CASES[k]["kind"] != "conv"])
def test_itsolver_s_reaches_the_same_solver(L, key):
    code, restore, sens, x_ref = golden()[key]
    with K.Captured() as cap:
        st, x, _ = K.run(L, CASES[key], via_itsolver=True)
    assert st == code and K.restore_iteration(cap.text) == restore
    assert np.max(np.abs(x - x_ref)) <= max(1e-10, 100.0 * sens) * np.max(np.abs(x_ref))


def test_krylov_s_prints_its_timing_line(gpu, L):
    S = K.system("csr", "p7_5")
    it = gpu.param_solver_init(); it.print_level = T.PRINT_MIN; it.itsolver_type = T.SOLVER_BiCGstab; it.tol = K.TOL
    x = np.zeros(S["n"])
    with K.Captured() as cap:
        st = gpu.solver_dcsr_krylov_s(S["ia"], S["ja"], S["val"], np.array(S["b"]), x, it)
    code, _, sens, x_ref = golden()["csr/spbcgs/p7_5/none/stop1/conv"]
    assert st == code and np.max(np.abs(x - x_ref)) <= max(1e-10, 100.0 * sens) * np.max(np.abs(x_ref))
    assert "Calling Safe BiCGstab solver (CSR) ..." in cap.text and "Krylov method totally costs" in cap.text


@pytest.mark.parametrize("safe, plain, restart", (("spcg", "pcg", None), ("spvgmres", "pvgmres", 20)))
def test_amg_handle_agrees_with_the_non_safe_entry(gpu, L, safe, plain, restart):
    """A device AMG handle as the preconditioner (it stays in HBM) on P7(11), tol 1e-8: the safe method takes the iterations of its
    non-safe twin, gives its x to 1e-10, and restores nothing."""
    S = K.system("csr", "p7_11")
    A, keep = K.as_matrix(S)
    amgp = gpu.param_amg_init(); amgp.smoother = T.SMOOTHER_JACOBI; amgp.relaxation = 0.6667; amgp.print_level = 0
    pc = L.fasp_hip_precond_setup(C.byref(A), C.byref(amgp))
    assert pc
    try:
        b = np.array(S["b"])
        bv, _ = T.as_vec(b)
        out = {}
        for name, extra in ((safe, ()), (plain, (0.0,))):   # the non-safe prototypes have abstol
            x = np.zeros(S["n"])
            xv = T.dvector(len(x), T.dp(x))
            args = [C.byref(A), C.byref(bv), C.byref(xv), pc, 1e-8, *extra, 500] + ([restart] if restart else []) + [T.STOP_REL_RES, T.PRINT_MIN]
            with K.Captured() as cap:
                st = getattr(L, "fasp_solver_dcsr_" + name)(*args)
            out[name] = (st, x, cap.text)
    finally:
        L.fasp_hip_precond_free(pc)
    (s1, x1, t1), (s0, x0, _) = out[safe], out[plain]
    print(f"{safe}: {s1} iterations, {plain}: {s0}; max|dx| / max|x| = {np.max(np.abs(x1 - x0)) / np.max(np.abs(x0)):.3e}")
    assert s1 == s0 and s1 > 0
    assert np.max(np.abs(x1 - x0)) <= 1e-10 * np.max(np.abs(x0))
    assert K.restore_iteration(t1) == -1
