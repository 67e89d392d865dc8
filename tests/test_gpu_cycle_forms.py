"""The cycle forms of csrc/cycles.hip.h -- V, W, the hybrid 12 / 21, AMLI, the K-cycle, maxit > 1, coarse scaling, every smoother --
through the resident preconditioner against the oracle cycling THE SAME levels (the handle's hierarchy, borrowed), on spd_scaled,
unsym_scaled and csrmat_FE (_cycle_cases.py): inputs whose diagonal varies, whose A is not A^T and whose levels have ragged sizes.

Bar of an application: max(1e-9, 8 x probe) of max|z|, at most 1e-7 (_cycle_cases.py).  Repeat applications are compared bit for bit."""
import numpy as np
import pytest

import _cycle_cases as K
from _libs import T

pytestmark = pytest.mark.gpu

LEDGER = K.Ledger()


class Pair:
    """A resident hierarchy of an input under a configuration and the oracle on its levels."""

    def __init__(self, gpu, name, cfg):
        ia, ja, a = K.matrix(name)
        self.H = gpu.AMG(ia, ja, a, K.params(cfg)[1])
        self.B = K.Borrowed(self.H, K.params(cfg)[1])
        K.check_hierarchy(name, self.B.sizes)

    def close(self):
        self.B.close(); self.H.close()


@pytest.mark.parametrize("name", K.INPUTS)
@pytest.mark.parametrize("cfg", list(K.CONFIGS))
def test_one_application_and_its_repeat(gpu, cfg, name):
    """z = B r of the device equals the oracle's on the same levels; a second application of the same r on the same handle -- which
    starts from the level vectors, swapped buffers and lazy flags the first one left -- returns the first one's bits."""
    P = Pair(gpu, name, cfg)
    try:
        r, = K.vectors(name, 11)
        z_ref, p = K.probe(P.B.precond, [r])
        what = f"{cfg} on {name}"
        bar = K.bar(p, K.CYCLE_FLOOR, K.CYCLE_CAP, what)
        z = P.H.precond(r)
        err = K.rel_diff(z, z_ref)
        print(f"{what}: error {err:.3e}, probe {p:.3e}, bar {bar:.3e}")
        LEDGER.note("cycle", what, p, bar, err)
        assert err <= bar, f"{what}: error {err:.3e} > bar {bar:.3e} (probe {p:.3e})"
        z2 = P.H.precond(r)
        assert np.array_equal(z2, z), f"{what}: the repeat differs by {K.rel_diff(z2, z):.3e}"
    finally:
        P.close()


@pytest.mark.parametrize("name", K.INPUTS)
def test_hybrid_cycles_are_told_apart(gpu, name):
    """Cycle types 12 and 21 differ from V, from W and from each other by far more than the bar (here: a thousand times), on the
    device as in the oracle: with fewer than four levels 12 would equal V and 21 would equal W bit for bit, and the comparison
    above would say nothing about the ncycles[] table."""
    forms = ("jacobi-V", "jacobi-W", "jacobi-12", "jacobi-21")
    r, = K.vectors(name, 11)
    dev, orc, bars = {}, {}, []
    for cfg in forms:
        P = Pair(gpu, name, cfg)
        try:
            assert len(P.B.sizes) >= 5
            orc[cfg], p = K.probe(P.B.precond, [r])
            bars.append(K.bar(p, K.CYCLE_FLOOR, K.CYCLE_CAP, f"{cfg} on {name}"))
            dev[cfg] = P.H.precond(r)
        finally:
            P.close()
    for i, c1 in enumerate(forms):
        for c2 in forms[i + 1:]:
            d_dev, d_orc = K.rel_diff(dev[c1], dev[c2]), K.rel_diff(orc[c1], orc[c2])
            print(f"{name}: {c1} against {c2}: device {d_dev:.3e}, oracle {d_orc:.3e}")
            assert d_dev >= 1000 * max(bars) and d_orc >= 1000 * max(bars), (c1, c2, d_dev, d_orc)


def _pcg(i, a): i.itsolver_type = T.SOLVER_CG
def _jac_pcg(i, a): K.CONFIGS["jacobi-V"](i, a); _pcg(i, a)
def _gs_pcg(i, a): K.CONFIGS["gs-cf"](i, a); _pcg(i, a)
def _kcycle_vfgmres(i, a): K.CONFIGS["kcycle-gcg"](i, a); i.itsolver_type = T.SOLVER_VFGMRES; i.restart = 30
def _fmg_pcg(i, a): K.CONFIGS["jacobi-V"](i, a); _pcg(i, a); i.precond_type = T.PREC_FMG


SOLVES = {"pcg-jacobi-V-fuse_zr": (_jac_pcg, 1), "pcg-jacobi-V-no-fuse_zr": (_jac_pcg, 0), "pcg-gs": (_gs_pcg, 1),
          "vfgmres30-kcycle-gcg": (_kcycle_vfgmres, 1), "pcg-fmg": (_fmg_pcg, 1)}


@pytest.mark.parametrize("name", K.INPUTS)
@pytest.mark.parametrize("solve", list(SOLVES))
def test_short_solves(gpu, solve, name):
    """Four iterations of a Krylov method around the preconditioner against orc_solve_with_hierarchy on the same levels, compared as
    _cmp_solve of test_gpu_parity.py does: equal status and history length, history to 1e-8, final relative residual to 1e-10, x to
    max(1e-8, 8 x probe) of max|x|, at most 1e-7.  Here the first Jacobi sweep and the (z, r) partials fused into the PCG update
    (pre_marked, want_zr; fasp_hip_tune("fuse_zr") both ways) meet a diagonal that varies."""
    mod, fuse_zr = SOLVES[solve]

    def mod4(i, a):
        mod(i, a); i.maxit = 4
    ia, ja, a = K.matrix(name)
    f, = K.vectors(name, 21)
    P = Pair(gpu, name, mod4)
    L = gpu.lib()
    try:
        def orc(ff):
            P.B.reset()   # (full multigrid carries the levels' iterates from one application to the next: every solve starts from zeros)
            s, x, h, rr = P.B.solve(ia, ja, a, ff, K.params(mod4)[0])
            return x, s, h, rr
        x_ref, s_ref, h_ref, rr_ref = orc(f)
        _, p = K.probe(lambda ff: orc(ff)[0], [f], ref=x_ref)
        what = f"{solve} on {name}"
        bar = K.bar(p, 1e-8, K.CYCLE_CAP, what)
        L.fasp_hip_tune(b"fuse_zr", fuse_zr)
        s, x, h, stats = P.H.solve(f, K.params(mod4)[0])
        err = K.rel_diff(x, x_ref)
        print(f"{what}: status {s} (oracle {s_ref}), error of x {err:.3e}, probe {p:.3e}, bar {bar:.3e}, relres {stats.relres:.6e} (oracle {rr_ref:.6e})")
        LEDGER.note("solve", what, p, bar, err)
        assert s == s_ref, (s, s_ref)
        if len(h_ref):   # the oracle records the residual history of CG only
            assert len(h) == len(h_ref)
            assert np.allclose(h, h_ref, rtol=1e-8, atol=1e-12 * h_ref[0]), np.max(np.abs(h - h_ref) / h_ref)
        assert abs(stats.relres - rr_ref) <= 1e-10
        assert err <= bar, f"{what}: error {err:.3e} > bar {bar:.3e} (probe {p:.3e})"
    finally:
        L.fasp_hip_tune(b"fuse_zr", 1)
        P.close()


def test_report_largest_probes():
    """Not a check: prints the largest probe and bar met above (pytest -s), for the record."""
    LEDGER.report("test_gpu_cycle_forms")
