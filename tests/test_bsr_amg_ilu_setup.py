"""ILU levels of the block UA-AMG setup on the host (csrc/host_setup.cpp, host_setup_ua_bsr) against the compiled reference
(fasp_amg_setup_ua_bsr, PreAMGSetupUABSR.c:149-179 and :351): with AMG_param.ILU_levels > 0 every level below
min(ILU_levels, levels - 1) carries a block ILUk(ILU_lfil) factor of its own matrix, equal byte for byte to the reference's
fasp_ilu_dbsr_setup on the reference's matrix of that level; the levels beyond carry none; A / P / R of every level are the
bytes of the hierarchy built without ILU; AMG_param.ILU_levels comes back as the reference leaves it.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import faspsolver_amd as fa

import _libs
from _libs import T, bsr_arrays, bsr_params, bsr_protos, poisson7pt_bsr
from test_bilu_setup import bilu_protos, ref_needed

pytestmark = [pytest.mark.ref, ref_needed]
P = C.POINTER

# (n of P7(n) (x) B3, aggregation, levels with coarse_dof = 50)
CASES = {"p6_vmb": (6, 2, 2), "p12_vmb": (12, 2, 3), "p10_pair": (10, 1, 3)}


def _params(agg, ilu_levels, lfil):
    _, amgp = bsr_params(agg=agg)
    amgp.coarse_dof = 50
    amgp.ILU_levels = ilu_levels
    amgp.ILU_lfil = lfil
    return amgp


_plain = {}


def plain_hierarchy(case):
    """A / P / R of every level of the product's hierarchy with ILU_levels = 0 (built once per case)."""
    if case not in _plain:
        n, agg, _ = CASES[case]
        ia, ja, val, nb = poisson7pt_bsr(n)
        G = fa.BSRAMG(ia, ja, val, nb, _params(agg, 0, 0), host_only=True)
        nl = G.num_levels
        _plain[case] = [[G.matrix(l, w) if (w == 0 or l < nl - 1) else None for w in range(3)] for l in range(nl)]
        G.free()
    return _plain[case]


def _same(a, b):
    return a[:3] == b[:3] and all(x.tobytes() == y.tobytes() for x, y in zip(a[3:], b[3:]))


@pytest.mark.parametrize("lfil", [0, 1])
@pytest.mark.parametrize("ilu_levels", [1, 2, 9])
@pytest.mark.parametrize("case", sorted(CASES))
def test_factors_and_hierarchy_equal_reference(case, ilu_levels, lfil):
    n, agg, levels = CASES[case]
    ia, ja, val, nb = poisson7pt_bsr(n)
    _, R = bsr_protos()
    R = bilu_protos(R)
    ref_free = C.CFUNCTYPE(None, C.c_void_p, P(T.AMG_param))(("ref_bsr_free", R))

    p_ours, p_ref = _params(agg, ilu_levels, lfil), _params(agg, ilu_levels, lfil)
    G = fa.BSRAMG(ia, ja, val, nb, p_ours, host_only=True)
    A, keep = T.as_bsr(ia, ja, val, nb)
    h = R.ref_bsr_setup_ua(C.byref(A), C.byref(p_ref))
    assert h
    try:
        assert G.num_levels == levels == R.ref_bsr_num_levels(h)   # (a degenerate hierarchy must not pass silently)
        assert p_ours.ILU_levels == p_ref.ILU_levels == ilu_levels  # 9 stays 9
        assert bytes(p_ours) == bytes(p_ref)
        plain = plain_hierarchy(case)
        assert len(plain) == levels
        for l in range(levels):
            for w in range(3):
                if plain[l][w] is not None:
                    assert _same(G.matrix(l, w), plain[l][w]), (l, w)
        for l in range(levels):
            f = G.ilu(l)
            if l >= min(ilu_levels, levels - 1):
                assert f is None, l
                continue
            assert f is not None, l
            v = T.dBSRmat()
            R.ref_bsr_get_matrix(h, l, 0, C.byref(v))
            assert _same(G.matrix(l, 0), (v.ROW, v.COL, v.NNZ) + bsr_arrays(v))
            prm = T.ILU_param()
            R.fasp_param_ilu_init(C.byref(prm))
            prm.ILU_type, prm.ILU_lfil = p_ref.ILU_type, lfil
            d = T.ILU_data()
            assert R.fasp_ilu_dbsr_setup(C.byref(v), C.byref(d), C.byref(prm)) == 0
            try:
                assert (f["nb"], f["row"], f["nzlu"]) == (d.nb, d.row, d.nzlu) == (nb, v.ROW, d.nzlu)
                assert f["ijlu"].tobytes() == np.ctypeslib.as_array(d.ijlu, (d.nzlu,)).tobytes()
                assert f["luval"].tobytes() == np.ctypeslib.as_array(d.luval, (d.nzlu * nb * nb,)).tobytes()
            finally:
                R.fasp_ilu_data_free(C.byref(d))
    finally:
        G.free()
        ref_free(h, C.byref(p_ref))


def test_ilu_levels_below_zero_mean_none():
    ia, ja, val, nb = poisson7pt_bsr(6)
    p = _params(2, -1, 0)
    G = fa.BSRAMG(ia, ja, val, nb, p, host_only=True)
    assert G.num_levels == 2 and G.ilu(0) is None and G.ilu(1) is None and p.ILU_levels == -1
    G.free()


def test_schwarz_levels_are_still_refused():
    ia, ja, val, nb = poisson7pt_bsr(6)
    p = _params(2, 1, 0)
    p.SWZ_levels = 1
    h = C.c_void_p()
    A, keep = T.as_bsr(ia, ja, val, nb)
    assert fa.lib().fasp_hip_bsr_amg_create_host(C.byref(h), C.byref(A), C.byref(p)) == T.ERROR_INPUT_PAR
    assert not h
