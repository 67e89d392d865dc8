"""CPU side of the cycle-form tests (_cycle_cases.py): the inputs are what they are meant to be, the oracle's cycle of every
configuration equals the compiled reference's on the reference's own hierarchy, every case's perturbation probe leaves its
bar under the cap, and a host-only hierarchy of the product can be borrowed into the oracle and cycled."""
import ctypes as C
import functools

import numpy as np
import pytest

import _cycle_cases as K
from _libs import OrcAMG, T, ref

LEDGER = K.Ledger()
# csrmat_FE: test_oracle_vs_ref.py shows the oracle's hierarchy bit-equal to the reference's; the generated inputs are compared as they come
BIT_EQUAL_HIERARCHY = ("fe",)
FORMS = [(c, False) for c in K.CONFIGS] + [("jacobi-V", True), ("gs-cf", True)]   # (configuration, as full multigrid)
FORM_IDS = [c + ("-FMG" if f else "") for c, f in FORMS]


def _own(name, cfg):
    """The oracle's own hierarchy of an input under a configuration -> (OrcAMG, Cycler, AMG_param)."""
    ia, ja, a = K.matrix(name)
    itp, amgp = K.params(cfg)
    A, keep = T.as_csr(ia, ja, a)
    O = OrcAMG(A, amgp)
    assert O.status >= 0
    return O, K.Cycler(O.buf, amgp), amgp


@functools.lru_cache(maxsize=None)
def _probed(name, cfg, fmg=False):
    """(z, probe) of one application of a configuration by the oracle on its own hierarchy; computed once, shared, read-only."""
    O, cyc, amgp = _own(name, cfg)
    r, = K.vectors(name, 11)
    z, p = K.probe(lambda v: cyc.precond(v, fmg), [r])
    O.free()
    z.setflags(write=False)
    return z, p


@pytest.mark.parametrize("name", K.INPUTS)
def test_inputs_are_what_they_are_for(name):
    ia, ja, a = K.matrix(name)          # check_matrix ran when it was built; once more on the cached arrays
    K.check_matrix(name, ia, ja, a)
    O, cyc, amgp = _own(name, "jacobi-V")
    sizes = [O.level(l).A.row for l in range(O.num_levels)]
    print(name, "levels", sizes)
    K.check_hierarchy(name, sizes)
    if name != "fe":
        assert len(ia) - 1 == K.N_ROWS
        again = K._build(name, K.SEEDS[name])
        assert all(np.array_equal(x, y) for x, y in zip(again, (ia, ja, a)))   # seeded: the same matrix every time
    O.free()


def _levels_equal(R, hr, O):
    nl = R.ref_amg_num_levels(hr)
    if nl != O.num_levels:
        return False
    for l in range(nl):
        for which, nm in ((0, "A"), (1, "P"), (2, "R")):
            if which and l == nl - 1:
                continue
            v = T.dCSRmat(); R.ref_amg_get_matrix(hr, l, which, C.byref(v))
            if v.row != getattr(O.level(l), nm).row or v.nnz != getattr(O.level(l), nm).nnz:
                return False
            if not all(np.array_equal(x, y) for x, y in zip(T.csr_arrays(v), T.csr_arrays(getattr(O.level(l), nm)))):
                return False
    return True


@pytest.mark.ref
@pytest.mark.parametrize("name", K.INPUTS)
@pytest.mark.parametrize("cfg,fmg", FORMS, ids=FORM_IDS)
def test_oracle_cycle_equals_reference(cfg, fmg, name):
    """One application z = B r of every configuration: the oracle on its own hierarchy against the compiled reference on its own
    (fasp_precond_amg / _amli / _namli / _famg as fasp_solver_dcsr_krylov_amg installs them).  Bit for bit where the two hierarchies are
    bit-equal -- required for csrmat_FE --, within the cycle bar otherwise."""
    R = ref()
    if R is None:
        pytest.skip("oracle/_ref/libfasp_ref.so not available")
    ia, ja, a = K.matrix(name)
    O, cyc, amgp = _own(name, cfg)
    itp2, amgp2 = K.params(cfg)
    A, keep = T.as_csr(ia, ja, a)
    hr = R.ref_amg_setup_rs(C.byref(A), C.byref(amgp2))
    assert hr
    same = _levels_equal(R, hr, O)
    r, = K.vectors(name, 11)
    z_ref = K.ref_precond(R, hr, amgp2, r, fmg)
    z, p = _probed(name, cfg, fmg)
    b = K.bar(p, K.CYCLE_FLOOR, K.CYCLE_CAP, f"{cfg} on {name}")
    err = K.rel_diff(z, z_ref)
    R.ref_amg_free(hr, C.byref(amgp2)); O.free()
    if name in BIT_EQUAL_HIERARCHY:
        assert same, "the oracle's hierarchy no longer equals the reference's"
    if same:
        assert np.array_equal(z, z_ref), f"hierarchies bit-equal, cycles not: relative difference {err:.3e}"
    else:
        assert err <= b, f"relative difference {err:.3e} > bar {b:.3e} (probe {p:.3e})"


@pytest.mark.parametrize("name", K.INPUTS)
@pytest.mark.parametrize("cfg,fmg", FORMS, ids=FORM_IDS)
def test_probe_stays_under_the_cap(cfg, fmg, name):
    """The bar max(1e-9, 8 x probe) of every cycle case stays under 1e-7, and the cycle's result is finite and of ordinary size."""
    r, = K.vectors(name, 11)
    z, p = _probed(name, cfg, fmg)
    assert np.all(np.isfinite(z)) and 0 < np.max(np.abs(z)) < 1e8 * np.max(np.abs(r))
    b = K.bar(p, K.CYCLE_FLOOR, K.CYCLE_CAP, f"{cfg} on {name}")
    LEDGER.note("cycle", f"{cfg}{'-FMG' if fmg else ''} on {name}", p, b)


@pytest.mark.parametrize("name", K.INPUTS)
def test_smoother_probes_stay_under_the_cap(name):
    """The same for every smoother of the table, before and after, from zero and from a random iterate, on levels 0 and 2 of the
    oracle's hierarchy."""
    O, cyc, amgp = _own(name, "jacobi-V")
    for level in (0, 2):
        Lv = O.level(level)
        n = Lv.A.row
        cf = np.ctypeslib.as_array(Lv.cfmark.val, (n,)).copy()
        rng = np.random.default_rng(100 + level)
        b0 = rng.standard_normal(n); x0 = rng.standard_normal(n)
        for sname, spec in K.SMOOTHERS.items():
            for post in (0, 1):
                for ns in spec[4]:
                    for zero in (0, 1):
                        fn = (lambda b: K.orc_smooth(Lv.A, cf, post, spec, ns, b, np.zeros(n))) if zero else \
                             (lambda b, x: K.orc_smooth(Lv.A, cf, post, spec, ns, b, x))
                        u, p = K.probe(fn, [b0] if zero else [b0, x0])
                        what = f"{sname} post={post} sweeps={ns} zero={zero} level {level} of {name}"
                        assert np.all(np.isfinite(u)), what
                        LEDGER.note("smoother", what, p, K.bar(p, K.SMOOTH_FLOOR, K.SMOOTH_CAP, what))
    O.free()


@pytest.mark.parametrize("name", K.INPUTS)
@pytest.mark.parametrize("cfg", ["jacobi-V", "jacobi-12", "amli2-coarse-scaling", "kcycle-gcg", "gsF"])
def test_host_only_hierarchy_borrowed_and_cycled(fa, cfg, name):
    """A host-only hierarchy of the product, borrowed into the oracle as bench.py does, cycles like the oracle's own: bit for bit
    when the two hierarchies are bit-equal, within the cycle bar otherwise."""
    ia, ja, a = K.matrix(name)
    O, cyc, amgp = _own(name, cfg)
    amgp3 = fa.param_amg_init(); K.CONFIGS[cfg](K.params(cfg)[0], amgp3)
    H = fa.AMG(ia, ja, a, amgp3, host_only=True)
    B = K.Borrowed(H, amgp3)
    K.check_hierarchy(name, B.sizes)
    same = B.sizes == [O.level(l).A.row for l in range(O.num_levels)]
    for l in range(len(B.sizes)):
        for which, nm in ((0, "A"), (1, "P"), (2, "R")):
            if same and not (which and l == len(B.sizes) - 1):
                same = all(np.array_equal(x, y) for x, y in zip(H.matrix(l, which)[2:], T.csr_arrays(getattr(O.level(l), nm))))
    r, = K.vectors(name, 11)
    z_own, p = _probed(name, cfg)
    z = B.precond(r)
    err = K.rel_diff(z, z_own)
    b = K.bar(p, K.CYCLE_FLOOR, K.CYCLE_CAP, f"{cfg} on {name}")
    B.close(); H.close(); O.free()
    if name in BIT_EQUAL_HIERARCHY:
        assert same
    if same:
        assert np.array_equal(z, z_own), err
    else:
        assert err <= b, f"relative difference {err:.3e} > bar {b:.3e} (probe {p:.3e})"


def test_report_largest_probes():
    """Not a check: prints the largest probe and bar met above (pytest -s), for the record."""
    LEDGER.report("test_cycle_cases")
