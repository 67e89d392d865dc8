"""smooth() of csrc/smoothers.hip.h through fasp_hip_level_smooth against the oracle's smoothing step (orc_smoothing) on levels
0, 2 and the last but one of the hierarchies of spd_scaled and unsym_scaled (_cycle_cases.py): every smoother of the table, before
and after the coarse correction, from the lazily zero iterate and from a random one, one sweep and three.  The varying diagonal and
A != A^T are what P7 cannot offer: dinv taken by column, D^-1 on the wrong operand, an A / A^T mix-up all show here.

Bar of a case: max(1e-13, 8 x probe) of max|u|, at most 1e-10 (_cycle_cases.py)."""
import numpy as np
import pytest

import _cycle_cases as K
from _libs import T

pytestmark = pytest.mark.gpu

LEDGER = K.Ledger()
NAMES = ("spd_scaled", "unsym_scaled")
LEVELS = ("0", "2", "last-but-one")


def _make(gpu, name, cfg="gs-cf"):
    ia, ja, a = K.matrix(name)
    return gpu.AMG(ia, ja, a, K.params(cfg)[1])


@pytest.fixture(scope="module")
def handles(gpu):
    """One resident hierarchy per input (the reference's default smoother, coarse_dof = 20), shared by every case: smooth() takes the
    smoother as an argument, and what a case leaves on a level (polynomial tables, schedules, swapped buffers) is part of the test."""
    made = {}

    def get(name):
        if name not in made:
            H = _make(gpu, name)
            K.check_hierarchy(name, [H.matrix(l, 0)[0] for l in range(H.num_levels)])
            made[name] = H
        return made[name]
    yield get
    for H in made.values():
        H.close()


def _level(H, key):
    return H.num_levels - 2 if key == "last-but-one" else int(key)


def _operands(H, level):
    """(dCSRmat of the level's A, keepalive, C/F marker, b, x) -- the matrices through fasp_hip_amg_get_matrix / _get_cfmark."""
    n, m, ia, ja, a = H.matrix(level, 0)
    A, keep = T.as_csr(ia, ja, a)
    cf = H.cfmark(level).astype(np.int32)
    assert len(cf) == n
    rng = np.random.default_rng(1000 + level)
    return A, keep, cf, rng.standard_normal(n), rng.standard_normal(n)


def _dev(H, level, post, spec, ns, b, x):
    sm, order, relax, ndeg, _ = spec
    return H.level_smooth(level, post, sm, order, ns, relax, ndeg, b, x)


@pytest.mark.parametrize("sname", list(K.SMOOTHERS))
@pytest.mark.parametrize("lkey", LEVELS)
@pytest.mark.parametrize("name", NAMES)
def test_level_smooth_equals_oracle(handles, name, lkey, sname):
    H = handles(name)
    level = _level(H, lkey)
    spec = K.SMOOTHERS[sname]
    A, keep, cf, b, x0 = _operands(H, level)
    n = len(b)
    for post in (0, 1):
        for zero in (0, 1):
            for ns in spec[4]:
                what = f"{sname} post={post} zero_start={zero} sweeps={ns} level {level} ({n} rows) of {name}"
                if zero:
                    u_ref, p = K.probe(lambda bb: K.orc_smooth(A, cf, post, spec, ns, bb, np.zeros(n)), [b])
                else:
                    u_ref, p = K.probe(lambda bb, xx: K.orc_smooth(A, cf, post, spec, ns, bb, xx), [b, x0])
                bar = K.bar(p, K.SMOOTH_FLOOR, K.SMOOTH_CAP, what)
                st, u = _dev(H, level, post, spec, ns, b, None if zero else x0)   # (zero_start: the buffer handed over is all NaN)
                assert st == 0, (what, st)
                err = K.rel_diff(u, u_ref)
                print(f"{what}: error {err:.3e}, probe {p:.3e}, bar {bar:.3e}")
                LEDGER.note("smoother", what, p, bar, err)
                assert err <= bar, f"{what}: error {err:.3e} > bar {bar:.3e} (probe {p:.3e})"


@pytest.mark.parametrize("sname", list(K.SMOOTHERS))
@pytest.mark.parametrize("name", NAMES)
def test_calls_in_a_row_equal_fresh_handles(gpu, name, sname):
    """What a call leaves behind on a level -- polynomial tables, sweep schedules, the C/F marker, swapped iterate buffers, a stale
    iterate -- changes nothing: calls A (before, from zero) and B (after, from a random iterate, the other sweep count) in a row on one
    handle, on levels 0 and 2, give the bits each gives as the first call on a level of a fresh handle."""
    spec = K.SMOOTHERS[sname]
    Hs, Ha, Hb = (_make(gpu, name) for _ in range(3))
    try:
        for level in (0, 2):
            A, keep, cf, b, x0 = _operands(Hs, level)
            call_a = lambda H: _dev(H, level, 0, spec, spec[4][-1], b, None)
            call_b = lambda H: _dev(H, level, 1, spec, spec[4][0], b[::-1].copy(), x0)
            fresh_a, fresh_b = call_a(Ha), call_b(Hb)
            for (st, u), (st1, u1) in zip([call_a(Hs), call_b(Hs), call_a(Hs)], [fresh_a, fresh_b, fresh_a]):
                assert st == 0 and st1 == 0
                assert np.all(np.isfinite(u)) and np.array_equal(u, u1), (sname, name, level, K.rel_diff(u, u1))
    finally:
        for H in (Hs, Ha, Hb):
            H.close()


def test_f_smoothers_need_a_cf_marker(gpu):
    """Jacobi-F and GS-F on an unsmoothed-aggregation hierarchy, which has no C/F marker: ERROR_AMG_SMOOTH_TYPE, x left alone;
    a smoother that needs none runs there."""
    ia, ja, a = K.matrix("spd_scaled")
    itp, amgp = K.params("jacobi-V"); amgp.AMG_type = T.UA_AMG
    H = gpu.AMG(ia, ja, a, amgp)
    try:
        assert H.num_levels >= 2
        n = H.matrix(0, 0)[0]
        b = np.random.default_rng(5).standard_normal(n)
        for sname in ("jacobiF0.8", "gsF"):
            for zero in (0, 1):
                x = np.full(n, 7.0)
                st, u = _dev(H, 0, 0, K.SMOOTHERS[sname], 1, b, None if zero else x)
                assert st == T.ERROR_AMG_SMOOTH_TYPE, (sname, st)
                assert np.all(np.isnan(u)) if zero else np.array_equal(u, x)
        st, u = _dev(H, 0, 0, K.SMOOTHERS["jacobi"], 1, b, None)
        assert st == 0 and np.all(np.isfinite(u))
    finally:
        H.close()


def test_bad_arguments_touch_nothing(handles, gpu):
    H = handles("spd_scaled")
    L = gpu.lib()
    n = H.matrix(0, 0)[0]
    b = np.ones(n); x = np.full(n, 3.0)
    sm, order, relax, ndeg, _ = K.SMOOTHERS["jacobi"]
    good = dict(h=H.h, level=0, post=0, smoother=sm, order=order, nsweeps=1, relax=relax, ndeg=ndeg, zero_start=0, b=T.dp(b), x=T.dp(x))
    for key, val in (("h", None), ("level", -1), ("level", H.num_levels), ("post", 2), ("post", -1), ("zero_start", 2), ("nsweeps", -1),
                     ("ndeg", -1), ("b", None), ("x", None)):
        args = dict(good); args[key] = val
        st = L.fasp_hip_level_smooth(*[args[k] for k in ("h", "level", "post", "smoother", "order", "nsweeps", "relax", "ndeg", "zero_start", "b", "x")])
        assert st == T.ERROR_INPUT_PAR, (key, val, st)
        assert np.all(x == 3.0) and np.all(b == 1.0)
    x2 = x.copy()
    assert L.fasp_hip_level_smooth(H.h, 0, 0, 99, order, 1, relax, ndeg, 0, T.dp(b), T.dp(x2)) == T.ERROR_AMG_SMOOTH_TYPE   # an unknown smoother
    assert np.array_equal(x2, x)
    # ... and the level still works, its right-hand side pointer and lazy flags as they were: a cycle through the handle
    r = np.random.default_rng(3).standard_normal(n)
    z1 = H.precond(r)
    st, u = _dev(H, 0, 1, K.SMOOTHERS["poly3"], 1, b, x)
    assert st == 0
    assert np.array_equal(H.precond(r), z1)


def test_report_largest_probes():
    """Not a check: prints the largest probe and bar met above (pytest -s), for the record."""
    LEDGER.report("test_gpu_level_smooth")
