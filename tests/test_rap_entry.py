"""The Galerkin product's entries (fasp_blas_dcsr_rap, BlaSpmvCSR.c:999; csrc/rap.hip.h) as far as they go without a GPU: the names
are exported, bad arguments are refused before anything touches a device, and fasp_hip_tune("device_rap", 1) leaves a host-only
setup what it was."""
import ctypes as C

import numpy as np

import _rap_cases as rc
from _libs import T, poisson7pt

NAMES = ["fasp_blas_dcsr_rap", "fasp_hip_dcsr_rap", "fasp_hip_rap_info", "fasp_hip_rap_device_count", "fasp_hip_rap_time"]


def test_names_are_exported(fa):
    L = fa.lib()
    for n in NAMES:
        assert n in fa.EXPORTS and hasattr(L, n), n
    for key in ("rap_form", "rap_arena_kb", "device_rap"):
        assert L.fasp_hip_tune(key.encode(), -1 if key == "rap_form" else 262144 if key == "rap_arena_kb" else 0) == 0, key
    assert callable(fa.rap) and callable(fa.rap_info) and callable(fa.rap_time)


def _all_zero(M):
    return bytes(M) == bytes(C.sizeof(M))


def test_bad_arguments_are_refused_before_the_device(fa):
    L = fa.lib()
    count = L.fasp_hip_rap_device_count()
    R, A, P, nf, nc = rc.operands("seed0")
    r, a, p, _keep = rc.as_mats(R, A, P, nf, nc)
    for args in ((None, a, p), (r, None, p), (r, a, None)):
        out = T.dCSRmat(7, 7, 7, None, None, None)
        assert L.fasp_hip_dcsr_rap(*[C.byref(m) if m is not None else None for m in args], C.byref(out)) == T.ERROR_INPUT_PAR
        assert _all_zero(out)
    assert L.fasp_hip_dcsr_rap(C.byref(r), C.byref(a), C.byref(p), None) == T.ERROR_INPUT_PAR
    # dimensions that do not chain: R->col != A->row, A->row != A->col, A->col != P->row, P->col != R->row
    for which, field, value in ((0, "col", nf + 1), (1, "col", nf - 1), (2, "row", nf - 1), (2, "col", nc + 1)):
        r, a, p, _keep = rc.as_mats(R, A, P, nf, nc)
        setattr((r, a, p)[which], field, value)
        out = T.dCSRmat(7, 7, 7, None, None, None)
        assert L.fasp_hip_dcsr_rap(C.byref(r), C.byref(a), C.byref(p), C.byref(out)) == T.ERROR_INPUT_PAR, (which, field)
        assert _all_zero(out)
        assert L.fasp_hip_rap_time(C.byref(r), C.byref(a), C.byref(p), 0, 1) < 0
    assert L.fasp_hip_rap_device_count() == count
    assert L.fasp_hip_rap_info(None) == T.ERROR_INPUT_PAR


def _host_hierarchy(fa, ia, ja, a, amg_type):
    amgp = fa.param_amg_init(); amgp.AMG_type = amg_type; amgp.smoother = T.SMOOTHER_JACOBI; amgp.coarse_dof = 50
    H = fa.AMG(ia, ja, a, amgp, host_only=True)
    out = []
    for l in range(H.num_levels):
        for w in range(3 if l + 1 < H.num_levels else 1):
            out.append(tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in H.matrix(l, w)))
    H.close()
    return out


def test_device_rap_switch_keeps_the_host_setup(fa):
    """With the switch on, a host-only setup takes the device product where a device is usable and the host product where none
    is: the hierarchy is the same bytes either way (on a machine without a GPU this is the host product, silently)."""
    L = fa.lib()
    ia, ja, a, f, ue = poisson7pt(8)
    for amg_type in (T.CLASSIC_AMG, T.SA_AMG, T.UA_AMG):
        base = _host_hierarchy(fa, ia, ja, a, amg_type)
        assert len(base) >= 4
        try:
            assert L.fasp_hip_tune(b"device_rap", 1) == 0
            assert _host_hierarchy(fa, ia, ja, a, amg_type) == base
        finally:
            L.fasp_hip_tune(b"device_rap", 0)


def test_host_product_timer_runs(fa):
    """fasp_hip_rap_time(where = 0) runs the setups' host product on the pinned cases without complaint (its bytes are compared
    in test_device_rap_switch_keeps_the_host_setup and, on the GPU, against every device product)."""
    for name in ("seed0", "repeated"):
        R, A, P, nf, nc = rc.operands(name)
        assert fa.rap_time(R + (nf,), A + (nf,), P + (nc,), 0, 1) >= 0.0
