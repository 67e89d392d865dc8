"""Every coarse-level solver kernel on its own, at its size edges.

A hierarchy with AMG_param.max_levels = 1 has one level: mgcycle() goes straight to coarse_solve() (cycles.hip.h), so

* AMG.precond(r) IS the coarse solver applied to r from a zero guess (the x_zero entry of every kernel).  precond_amg() starts
  from fasp_param_amg_init and copies the fields of fasp_param_prec_to_amg only: AMG_param.tol is NOT one of them, the cycle
  sees tol = 1e-6 whatever the user set and the coarse solver receives tol = 1e-6 * 1e-4 (about 1e-10);
* AMG.amg_solve(b, amgparam, x0) with amgparam.maxit = 1 IS the coarse solver started from the iterate x0 (the initial-product
  entry); amg_solve_device() hands the caller's AMG_param to the cycle: tol = amgparam.tol * 1e-4 (here 1e-5 * 1e-4).  It runs
  no cycle at all when ||b|| <= 1e-20, so a zero right-hand side reaches the coarse solver through precond() only.

Both receive MaxIt = max(250, min(m * m, 1000)) (coarse_spcg(), PreMGUtil.inl:41).  Read off the code and confirmed with
FASP_HIP_DEBUG_COARSE=1, which prints the relative residual each coarse solve stopped at: e.g. 1.5e-11 / 5.8e-10 (64 rows),
9.2e-11 / 6.5e-10 (1000 rows), 9.9e-11 / 8.2e-10 (8001 rows) for precond / amg_solve -- the first iterates below 1e-10 and 1e-9,
at the oracle's iteration counts (assertion (c)).

The CPU counterpart is orc_spcg (oracle/fasp_oracle.h, pinned bit for bit to the compiled reference by
test_oracle_vs_ref.py::test_coarse_spcg_bit_exact) with the same A, b, x0, tol, MaxIt, and orc_gmres(mode 2, restart 20, the same
MaxIt) behind it where the safe CG gives up -- the SPVGMRES net of coarse_solve().

Assertions of section 1, for the device result u and the oracle's result alike:
 (a) the true residual, formed here in extended precision, relative to ||r0|| = ||b - A x0|| (the quantity STOP_REL_RES divides by,
     KrySPcg.c:125; ||b|| for the zero guess; the nonzero guesses are built with ||r0|| <= 0.8 ||b||, so the same figure holds
     relative to ||b|| as well) is below tol + c,  c = 2 (k + 2) eps (|| |A| |u| ||_2 + ||b||_2) / ||r0||_2,  k the
     longest row, eps = 2^-53: the rounding bound of the residual the solver itself evaluates in double before it accepts u;
 (b) ||u_dev - u_orc||_2 <= 2 (tol + c) ||r0||_2 / lambda_min(A) -- what two vectors that satisfy (a) imply.  lambda_min from
     numpy.linalg.eigvalsh for m <= 2048, from Gershgorin's bound of the strictly diagonally dominant matrix above that;
 (c) stats.coarse_iters against orc_spcg's return value: |delta| <= 0.02 its + 2 (the bar of test_gpu_coarse_small.py for
     reordered sums); small_onewave 3 and 4 give the same count and bitwise the same u;
 (d) 64 NaN doubles before and behind every vector handed over stay untouched, r / b stay bitwise unchanged, u has no NaN;
and the kernel that ran (fasp_hip_coarse_kernel_info) is the one the selection table of coarse_spcg() names for the case.

The k_spcg_dpp hazard check (no GPU) disassembles the built library: see test_dpp_wait_states_in_the_built_library.
"""
import ctypes as C
import functools
import os
import re
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import faspsolver_amd as fa
from faspsolver_amd import _types as T
import _libs
from _coarse_cases import (ARROW, DEFAULTS, FAMILY, GM_CB, GM_NE, GM_RESTART, SMALL_BLOCK, arrowhead, band_sparse, block_diag, dense_spd,
                           diagonal, dyadic, expected_block_kernel, expected_kernel, kernel_name, laplacian, max_it, persist_ne,
                           random_sparse, rows_of, scaled, sym_from_pairs, to_csr, wide_rows)

EPS = 2.0 ** -53
TOL_PRECOND = 1e-6 * 1e-4      # precond_amg(): fasp_param_amg_init's tol, times 1e-4 in the cycle
AMG_TOL = 1e-5                 # what the tests hand to amg_solve
TOL_SOLVE = AMG_TOL * 1e-4
CANARY = 64


# (the matrices and the selection table, restated: tests/_coarse_cases.py, shared with the CPU test of the plan, test_coarse_plan.py)
# ---------------------------------------------------------------------------------------------------------------------
# the cases of section 1
# ---------------------------------------------------------------------------------------------------------------------
ONEWAVE_M = [1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 95, 96, 97, 111, 112, 113, 127, 128]
EDGES = {15, 16, 17, 63, 64, 65, 95, 96, 97, 127, 128}
MID_M = [129, 500, 1000, 2048, 2049, 3700, 3800, 4096, 4097]
BIG_M = [5000, 5088, 5089, 5120, 5121, 6144, 6145, 8000, 8001, 9000]

CASES = {}


def _add(name, m, build, group):
    CASES[name] = (m, build, group)


def _fixed(f, *args):
    """A builder that draws nothing."""
    return lambda rng: f(*args)


for _k, _m in enumerate(ONEWAVE_M):
    _add(f"lap{1 + _k % 3}d-{_m}", _m, _fixed(laplacian, _m, 1 + _k % 3), "onewave")
    _add(f"rand-{_m}", _m, functools.partial(random_sparse, _m), "onewave")
    if _m in EDGES:
        _add(f"dense-{_m}", _m, functools.partial(dense_spd, _m), "onewave")
for _m in (48, 80, 113, 128):
    _add(f"blockdiag-{_m}", _m, functools.partial(block_diag, _m), "onewave")
for _m in (33, 64, 97, 128):    # (iv) in the strength the reference's safe CG still converges on: D = diag(10^+-1), entries over four decades
    _add(f"scaled10-{_m}", _m, _fixed(scaled, _m, 10.0, 0.1), "onewave")
for _m, _v, _n in ((1, [1.0], "identity"), (2, [4.0], "4I"), (3, [2.0, 8.0], "twovalues"), (64, [1.0], "identity"),
                   (65, [4.0], "4I"), (96, [2.0, 8.0], "twovalues"), (128, [2.0, 8.0, 8.0], "twovalues")):
    _add(f"{_n}-{_m}", _m, _fixed(diagonal, _m, _v), "onewave")
for _k, _m in enumerate(MID_M):
    _add(f"lap3d-{_m}", _m, _fixed(laplacian, _m, 3), "mid")
    _add(f"band-{_m}", _m, functools.partial(band_sparse, _m), "mid")
_add("wide-600", 600, functools.partial(wide_rows, 600), "big")
for _m in BIG_M:
    _add(f"lap3d-{_m}", _m, _fixed(laplacian, _m, 3), "big")
    _add(f"band-{_m}", _m, functools.partial(band_sparse, _m), "big")
for _m, _l in ARROW:
    _add(f"arrow-{_m}-" + "+".join(str(x) for x in _l), _m, functools.partial(arrowhead, _m, _l), "arrow")


def names(group):
    return [n for n, c in CASES.items() if c[2] == group]


def mxv(ia, ja, a, x, dtype=np.float64):
    y = np.zeros(len(ia) - 1, dtype=dtype)
    np.add.at(y, rows_of(ia), a.astype(dtype) * x.astype(dtype)[ja])
    return y


@functools.lru_cache(maxsize=None)
def problem(name):
    """(ia, ja, a, b, x0, lambda_min, k) of a case, seeded by its name."""
    m, build, _ = CASES[name]
    rng = np.random.default_rng(int.from_bytes(name.encode(), "little") % (2 ** 32))
    ia, ja, a = build(rng)
    assert len(ia) == m + 1
    b = rng.standard_normal(m)
    # x0 = half the solution + noise with ||A noise|| = ||b|| / 4: ||r0|| = ||b / 2 - A noise|| lies within [0.25, 0.75] ||b||, so
    # the bound relative to ||r0|| (what STOP_REL_RES divides by) implies the same bound relative to ||b||
    x0 = rng.standard_normal(m)
    x0 *= 0.25 * np.linalg.norm(b) / np.linalg.norm(mxv(ia, ja, a, x0))
    x0 += 0.5 * orc_spcg(ia, ja, a, b, np.zeros(m), TOL_PRECOND)[1]
    assert np.linalg.norm(b - mxv(ia, ja, a, x0)) <= 0.8 * np.linalg.norm(b), name
    rows = rows_of(ia)
    if m <= 2048:
        D = np.zeros((m, m)); np.add.at(D, (rows, ja), a)
        assert np.array_equal(D, D.T)
        lam = float(np.linalg.eigvalsh(D)[0])
    else:                                    # Gershgorin: min_i (a_ii - sum_j |a_ij|); stored pieces of one entry only widen the disc
        diag = np.bincount(rows, weights=np.where(ja == rows, a, 0.0), minlength=m)
        off = np.bincount(rows, weights=np.where(ja == rows, 0.0, np.abs(a)), minlength=m)
        lam = float((diag - off).min())
    assert lam > 0.0, (name, lam)
    return ia, ja, a, b, x0, lam, int(np.diff(ia).max())


def residual_check(ia, ja, a, b, x0, u, tol, k):
    """(true relative residual in extended precision, tol + c, ||r0||) -- assertion (a)."""
    L = np.longdouble
    r = b.astype(L) - mxv(ia, ja, a, u, L)
    r0 = b.astype(L) - mxv(ia, ja, a, x0, L)
    nr0 = float(np.sqrt(np.sum(r0 * r0)))
    absAu = mxv(ia, ja, np.abs(a), np.abs(u))
    c = 2.0 * (k + 2) * EPS * (np.linalg.norm(absAu) + np.linalg.norm(b)) / nr0
    return float(np.sqrt(np.sum(r * r))) / nr0, tol + c, nr0


def orc_spcg(ia, ja, a, b, x0, tol):
    A, keep = T.as_csr(ia, ja, a)
    u = np.array(x0, dtype=np.float64)
    bv, bk = T.as_vec(b); uv = T.dvector(len(u), T.dp(u))
    st = _libs.oracle().orc_spcg(C.byref(A), C.byref(bv), C.byref(uv), tol, max_it(len(b)), 1, 0)
    return st, u


def orc_coarse(ia, ja, a, b, x0, tol):
    """fasp_coarse_itsolver (PreMGUtil.inl:37-58): the safe CG, the SPVGMRES net behind it -> (CG status, net status or None, u)."""
    st, u = orc_spcg(ia, ja, a, b, x0, tol)
    net = None
    if st < 0:
        o = _libs.oracle()
        o.orc_gmres.argtypes = [C.c_int, C.POINTER(T.dCSRmat), C.POINTER(T.dvector), C.POINTER(T.dvector), C.c_void_p,
                                C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        A, keep = T.as_csr(ia, ja, a)
        bv, bk = T.as_vec(b); uv = T.dvector(len(u), T.dp(u))
        net = o.orc_gmres(2, C.byref(A), C.byref(bv), C.byref(uv), None, None, tol, 0.0, max_it(len(b)), 20, 1, 0, None)
    return st, net, u


@functools.lru_cache(maxsize=None)
def oracle_results(name):
    ia, ja, a, b, x0, lam, k = problem(name)
    return (orc_spcg(ia, ja, a, b, np.zeros_like(b), TOL_PRECOND), orc_spcg(ia, ja, a, b, x0, TOL_SOLVE))


# ---------------------------------------------------------------------------------------------------------------------
# CPU half: the oracle alone converges on every case and sits inside the bounds the device results are held to
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_alone_is_inside_every_bound(name):
    ia, ja, a, b, x0, lam, k = problem(name)
    m = len(b)
    for (st, u), start, tol in zip(oracle_results(name), (np.zeros(m), x0), (TOL_PRECOND, TOL_SOLVE)):
        assert 0 < st <= max_it(m), (name, st)
        rel, bound, nr0 = residual_check(ia, ja, a, b, start, u, tol, k)
        print(f"{name}: oracle its {st} relres {rel:.3e} bound {bound:.3e} lambda_min {lam:.3e}")
        assert rel < bound, (name, rel, bound)
        # (b) against a second, independent solution: the dense solve for small m
        if m <= 2048:
            D = np.zeros((m, m)); np.add.at(D, (rows_of(ia), ja), a)
            ux = np.linalg.solve(D, b)
            relx, boundx, _ = residual_check(ia, ja, a, b, start, ux, tol, k)
            assert np.linalg.norm(u - ux) <= (bound + boundx) * nr0 / lam, name


# ---------------------------------------------------------------------------------------------------------------------
# the two handles, with canaries
# ---------------------------------------------------------------------------------------------------------------------
def guarded(v):
    buf = np.full(len(v) + 2 * CANARY, np.nan)
    buf[CANARY:CANARY + len(v)] = v
    return buf


def canaries_intact(buf, m):
    return bool(np.isnan(buf[:CANARY]).all() and np.isnan(buf[CANARY + m:]).all())


def mid_ptr(buf):
    return C.cast(buf.ctypes.data + 8 * CANARY, T.c_double_p)


def single_level(ia, ja, a):
    amgp = fa.param_amg_init()
    amgp.max_levels = 1; amgp.maxit = 1; amgp.smoother = T.SMOOTHER_JACOBI
    H = fa.AMG(ia, ja, a, amgp)
    assert H.num_levels == 1
    return H


def apply_precond(H, r):
    """z = coarse solve of A z = r from the zero guess -> (z, canaries and r intact)."""
    m = len(r)
    rb, zb = guarded(r), guarded(np.zeros(m))
    st = fa.lib().fasp_hip_precond_amg(H.h, mid_ptr(rb), mid_ptr(zb))
    assert st >= 0, st
    ok = canaries_intact(rb, m) and canaries_intact(zb, m) and np.array_equal(rb[CANARY:CANARY + m], r, equal_nan=True)
    return zb[CANARY:CANARY + m].copy(), ok


def apply_solve(H, b, x0):
    """One cycle of amg_solve = one coarse solve from x0 -> (u, coarse iterations, canaries and b intact)."""
    m = len(b)
    bb, xb = guarded(b), guarded(x0)
    amgp = fa.param_amg_init()
    amgp.max_levels = 1; amgp.maxit = 1; amgp.smoother = T.SMOOTHER_JACOBI; amgp.tol = AMG_TOL
    bv = T.dvector(m, mid_ptr(bb)); xv = T.dvector(m, mid_ptr(xb))
    stats = T.fasp_hip_stats()
    fa.lib().fasp_hip_amg_solve(H.h, C.byref(bv), C.byref(xv), C.byref(amgp), None, 0, C.byref(stats))
    ok = canaries_intact(bb, m) and canaries_intact(xb, m) and np.array_equal(bb[CANARY:CANARY + m], b, equal_nan=True)
    return xb[CANARY:CANARY + m].copy(), int(stats.coarse_iters), ok


# fasp_hip_amg_kernel_info families of a losslessly coded operator (4 coded values, 5 / 6 / 9 row patterns): coarse_spcg() takes
# the fused and persistent kernels for plain CSR only
CODED_KINDS = (4, 5, 6, 9)
RAN = {}    # kernel instantiation -> cases that ran it (printed at the end of the module's GPU tests)


def set_tune(**kw):
    for key, v in kw.items():
        assert fa.lib().fasp_hip_tune(key.encode(), int(v)) >= 0, key



def check_case(name, H, tune, small_coarse=True):
    """Section 1 (a)-(d) + the kernel read-out for one case under the switches `tune` (already set) -> {entry: (u, iterations)}."""
    ia, ja, a, b, x0, lam, k = problem(name)
    m = len(b)
    coded = H.kernel_info(0)[0] in CODED_KINDS
    want = expected_kernel(ia, tune, H.coarse_kernel_info()[6], coded, small_coarse)
    out = {}
    for entry, start, tol, (s_orc, u_orc) in zip(("precond", "solve"), (np.zeros(m), x0), (TOL_PRECOND, TOL_SOLVE),
                                                  oracle_results(name)):
        if entry == "precond":
            u, ok = apply_precond(H, b)
            its = None
        else:
            u, its, ok = apply_solve(H, b, x0)
        info = H.coarse_kernel_info()
        tag = f"{name} {entry} {tune}"
        rel, bound, nr0 = residual_check(ia, ja, a, b, start, u, tol, k)
        diff = float(np.linalg.norm(u - u_orc))
        print(f"{tag}: ran {kernel_name(info)} cg {info[3]} net {info[4]} its {its} (oracle {s_orc}) relres {rel:.3e} "
              f"(bound {bound:.3e}) |u - u_orc| {diff:.3e} (bound {2 * bound * nr0 / lam:.3e})")
        RAN.setdefault(kernel_name(info), []).append(f"{name}/{entry}")
        assert tuple(info[:3]) == want, (tag, kernel_name(info), kernel_name(want))
        assert ok, tag                                            # (d)
        assert not np.isnan(u).any(), tag
        assert info[3] > 0 and info[4] == 0, (tag, info)          # the safe CG converged, no net
        assert rel < bound, (tag, rel, bound)                     # (a)
        assert diff <= 2 * bound * nr0 / lam, (tag, diff)         # (b)
        if its is not None:                                       # (c)
            assert its == info[3], (tag, its, info)
            assert abs(its - s_orc) <= 0.02 * s_orc + 2, (tag, its, s_orc)
        else:
            assert abs(info[3] - s_orc) <= 0.02 * s_orc + 2, (tag, info[3], s_orc)
        out[entry] = (u, info[3])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", names("onewave"))
def test_one_wavefront_forms(gpu, name):
    ia, ja, a = problem(name)[:3]
    got = {}
    H = single_level(ia, ja, a)
    try:
        for form in (4, 3, 2, 1, 0):
            set_tune(small_onewave=form)
            got[form] = check_case(name, H, dict(DEFAULTS, small_onewave=form))
    finally:
        set_tune(**DEFAULTS)
        H.close()
    for entry in ("precond", "solve"):      # forms 3 and 4: the same arithmetic with and without sending ahead
        assert got[3][entry][1] == got[4][entry][1], (name, entry)
        assert np.array_equal(got[3][entry][0], got[4][entry][0]), (name, entry)


@pytest.mark.gpu
@pytest.mark.parametrize("name", names("mid"))
def test_single_workgroup_lds_modes(gpu, name):
    ia, ja, a = problem(name)[:3]
    H = single_level(ia, ja, a)
    try:
        for lds in (1, 0):
            set_tune(small_lds=lds)
            check_case(name, H, dict(DEFAULTS, small_lds=lds))
    finally:
        set_tune(**DEFAULTS)
        H.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", names("big"))
def test_batched_fused_and_persistent_paths(gpu, name):
    ia, ja, a = problem(name)[:3]
    H = single_level(ia, ja, a)
    try:
        for fused, persist in ((1, 1), (1, 0), (0, 0)):
            for batch in (1, 8):
                tune = dict(DEFAULTS, spcg_fused=fused, spcg_persist=persist, spcg_batch=batch)
                set_tune(**tune)
                check_case(name, H, tune)
    finally:
        set_tune(**DEFAULTS)
        H.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", names("arrow"))
def test_persistent_register_budget(gpu, name):
    """Arrowhead matrices whose dense leading rows need 30, 46, 54, 61 and 66 slots of 64 entries: NE = 32, 48, 56, 64 and the
    refusal (fused path), at m = 4200 (u in LDS) and m = 5500 (u in memory)."""
    ia, ja, a = problem(name)[:3]
    m, longest = len(ia) - 1, int(np.diff(ia).max())
    want_ne = {30: 32, 46: 48, 54: 56, 61: 64, 66: 0}[(longest + 63) // 64]
    H = single_level(ia, ja, a)
    try:
        assert persist_ne(ia, H.coarse_kernel_info()[6]) == want_ne, (name, longest)
        set_tune(**DEFAULTS)
        check_case(name, H, dict(DEFAULTS))
        info = H.coarse_kernel_info()
        if want_ne:
            assert tuple(info[:3]) == (6, want_ne, 1 if m <= 5088 else 0), (name, info)
        else:
            assert info[0] == 5, (name, info)
    finally:
        set_tune(**DEFAULTS)
        H.close()


# ---------------------------------------------------------------------------------------------------------------------
# section 2: verdicts a well-posed coarse matrix never produces (integer data: which branch fires is not decided by rounding)
# ---------------------------------------------------------------------------------------------------------------------
def embed(m, ia, ja, a):
    """The small matrix in the leading rows of an m x m matrix, identity behind it."""
    m0 = len(ia) - 1
    idx = np.arange(m0, m)
    return to_csr(m, np.concatenate([rows_of(ia), idx]), np.concatenate([ja, idx]), np.concatenate([a, np.ones(m - m0)]))


def verdict_problem(kind, m):
    """(ia, ja, a, b, x0 or None) -- x0 None: the zero guess through precond()."""
    if kind in ("zero_rhs", "zero_rhs_guess"):
        ia, ja, a = laplacian(m, 1, shift=0.0)
        x0 = np.arange(m, dtype=np.float64) % 5 - 2.0
        return ia, ja, a, np.zeros(m), None if kind == "zero_rhs" else x0
    if kind == "div0":                       # A = diag(1, -1) (+) I, b = (1, 1, 0, ..): (p, A p) = 0 in the first iteration
        ia, ja, a = embed(m, *diagonal(2, [1.0, -1.0]))
        b = np.zeros(m); b[:2] = 1.0
        return ia, ja, a, b, None
    if kind == "nan_rhs":
        ia, ja, a = laplacian(m, 1, shift=1.0)
        b = np.ones(m); b[m // 2] = np.nan
        return ia, ja, a, b, None
    if kind in ("neumann_consistent", "neumann_inconsistent"):
        idx = np.arange(m - 1)
        deg = np.full(m, 2.0); deg[0] = deg[-1] = 1.0
        ia, ja, a = to_csr(m, np.concatenate([idx, idx + 1, np.arange(m)]), np.concatenate([idx + 1, idx, np.arange(m)]),
                           np.concatenate([-np.ones(2 * (m - 1)), deg]))
        b = np.zeros(m); b[0] = 3.0; b[-1] = -3.0 if kind == "neumann_consistent" else 1.0
        return ia, ja, a, b, None
    if kind in ("empty_row", "empty_row_guess"):   # row and column m // 3 hold nothing, b there is 0
        e = m // 3
        ia, ja, a = laplacian(m, 1, shift=1.0)
        rows = rows_of(ia)
        keep = (rows != e) & (ja != e)
        ia, ja, a = to_csr(m, rows[keep], ja[keep], a[keep])
        b = np.ones(m); b[e] = 0.0
        x0 = np.full(m, 0.5); x0[e] = 7.0
        return ia, ja, a, b, None if kind == "empty_row" else x0
    if kind == "scaled":
        return scaled(m) + (np.random.default_rng(m).standard_normal(m), None)
    if kind == "negative_1x1":
        return to_csr(1, [0], [0], [-2.0]) + (np.array([3.0]), None)
    if kind == "indefinite_2x2":
        return to_csr(2, [0, 0, 1, 1], [0, 1, 0, 1], [1.0, 2.0, 2.0, 1.0]) + (np.array([1.0, 0.0]), None)
    raise KeyError(kind)


VERDICT_CASES = [(k, m) for k in ("zero_rhs", "zero_rhs_guess", "div0", "nan_rhs", "neumann_consistent", "neumann_inconsistent",
                                  "empty_row", "empty_row_guess", "scaled") for m in (40, 100, 1000, 4200)] + [("negative_1x1", 1), ("indefinite_2x2", 2)]


def oracle_verdict(kind, m):
    ia, ja, a, b, x0 = verdict_problem(kind, m)
    tol = TOL_PRECOND if x0 is None else TOL_SOLVE
    return orc_coarse(ia, ja, a, b, np.zeros(m) if x0 is None else x0, tol)


@pytest.mark.parametrize("kind,m", VERDICT_CASES)
def test_oracle_verdicts_are_finite_decisions(kind, m):
    """CPU half of section 2: the oracle ends every one of these cases (no crash, a definite status); recorded for the GPU half."""
    st, net, u = oracle_verdict(kind, m)
    print(kind, m, "cg", st, "net", net, "nan in u", bool(np.isnan(u).any()))
    assert st <= max_it(m)
    assert (net is None) == (st >= 0)


def check_verdict(kind, m, H, tag, tune=None, small_coarse=True):
    ia, ja, a, b, x0 = verdict_problem(kind, m)
    s_orc, net_orc, u_orc = oracle_verdict(kind, m)
    if x0 is None:
        u, ok = apply_precond(H, b)
    else:
        u, its, ok = apply_solve(H, b, x0)
        if np.linalg.norm(b) <= 1e-20:       # amg_solve_device runs no cycle on a zero right-hand side: u = 0 (PreMGSolve.c)
            assert ok and np.array_equal(u, np.zeros(m)), tag
            return
    info = H.coarse_kernel_info()
    print(f"{tag}: ran {kernel_name(info)} cg {info[3]} net {info[4]}/{info[5]}; oracle cg {s_orc} net {net_orc}")
    RAN.setdefault(kernel_name(info), []).append(f"{kind}-{m}")
    assert ok, tag
    want = expected_kernel(ia, tune or DEFAULTS, info[6], H.kernel_info(0)[0] in CODED_KINDS, small_coarse)
    if not (kind == "zero_rhs" and want[0] == 7):                     # (the per-iteration path launches nothing for r0 = 0)
        assert tuple(info[:3]) == want, (tag, kernel_name(info), kernel_name(want))
    if kind.startswith("empty_row"):
        assert info[0] != 6, tag                                      # build_persist_plan refuses a matrix with an empty row
    assert (info[3] < 0) == (s_orc < 0), (tag, info, s_orc)           # the same verdict path: did the safe CG give up,
    assert info[4] == (0 if net_orc is None else 1), (tag, info)      # did the net run
    if s_orc < 0:
        assert info[3] == s_orc, (tag, info, s_orc)                   # ... and with which of the reference's codes
    assert np.array_equal(np.isnan(u), np.isnan(u_orc)), tag
    if kind in ("zero_rhs", "div0", "nan_rhs"):                       # u is what the guess was / a restored copy: bit for bit
        assert np.array_equal(u, u_orc, equal_nan=True), tag
    if kind.startswith("empty_row"):                                  # left as given: 0 from the zero guess, 7 from the other
        assert u[m // 3] == (0.0 if x0 is None else x0[m // 3]), tag
    if not np.isnan(u_orc).any() and np.linalg.norm(b) > 0:
        start = np.zeros(m) if x0 is None else x0
        tol = TOL_PRECOND if x0 is None else TOL_SOLVE
        k = max(int(np.diff(ia).max()), 1)
        rel_o, bound_o, _ = residual_check(ia, ja, a, b, start, u_orc, tol, k)
        if rel_o < bound_o:                                           # the oracle converged: bound (a) holds for the device too
            rel, bound, nr0 = residual_check(ia, ja, a, b, start, u, tol, k)
            assert rel < bound, (tag, rel, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,m", VERDICT_CASES)
def test_verdict_branches(gpu, kind, m):
    ia, ja, a = verdict_problem(kind, m)[:3]
    H = single_level(ia, ja, a)
    try:
        forms = (4, 3, 2, 1, 0) if m <= 128 else (4,)
        for form in forms:
            set_tune(small_onewave=form)
            check_verdict(kind, m, H, f"{kind}-{m} form {form}", dict(DEFAULTS, small_onewave=form))
        if m > 128:
            for fused, persist in ((1, 0), (0, 0)):
                set_tune(spcg_fused=fused, spcg_persist=persist)
                check_verdict(kind, m, H, f"{kind}-{m} fused {fused} persist {persist}",
                              dict(DEFAULTS, spcg_fused=fused, spcg_persist=persist))
    finally:
        set_tune(**DEFAULTS)
        H.close()


_CHILD = """
import sys, numpy as np
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import test_gpu_coarse_direct as t
for kind, m in t.VERDICT_CASES:
    if m < 40 or m > 1000:
        continue
    ia, ja, a = t.verdict_problem(kind, m)[:3]
    H = t.single_level(ia, ja, a)
    t.check_verdict(kind, m, H, f"{{kind}}-{{m}} host-batched", small_coarse=False)
    info = H.coarse_kernel_info()
    assert info[0] in (0, 5, 6, 7), info
    H.close()
for name in ("lap2d-64", "rand-97", "band-1000", "lap3d-3800"):
    ia, ja, a = t.problem(name)[:3]
    H = t.single_level(ia, ja, a)
    t.check_case(name, H, dict(t.DEFAULTS), small_coarse=False)
    H.close()
print("CHILD OK")
"""


@pytest.mark.gpu
def test_small_sizes_on_the_batched_path_in_a_child_process(gpu):
    """FASP_HIP_SMALL_COARSE=0 (read once per process): the verdict cases and four section-1 cases of at most 4096 rows through
    the host-replayed batched / fused / persistent path, in a fresh child."""
    root = _libs.ROOT
    env = dict(os.environ, FASP_HIP_SMALL_COARSE="0")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(tests=os.path.join(root, "tests"), root=root)], env=env,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:]); print(r.stderr[-3000:])
    assert r.returncode == 0 and "CHILD OK" in r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# section 4: the wait states in front of v_fmac_f64_dpp, checked in the built code object (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
LLVM_BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def gfx950_code_objects(so):
    """The gfx950 code objects of every offload bundle in the library's .hip_fatbin section."""
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([os.path.join(LLVM_BIN, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fat], check=True)
        blob = open(fat, "rb").read()
    out = []
    at = blob.find(BUNDLE_MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", blob, at + 24)
        p = at + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if triple.endswith("gfx950") and size:
                out.append(blob[at + off:at + off + size])
        at = blob.find(BUNDLE_MAGIC, at + 1)
    return out


def disassemble_dpp_kernels():
    """{mangled kernel name: [(address, mnemonic, operand text, branch target or None)]} of the k_spcg_dpp instantiations."""
    kernels = {}
    for co in gfx950_code_objects(fa.LIB_PATH):
        with tempfile.TemporaryDirectory() as d:
            fn = os.path.join(d, "co.elf")
            open(fn, "wb").write(co)
            objdump = os.path.join(LLVM_BIN, "llvm-objdump")
            syms = subprocess.run([objdump, "-t", fn], capture_output=True, text=True, check=True).stdout
            want = [l.split()[-1] for l in syms.splitlines() if "k_spcg_dpp" in l and " F " in l and not l.endswith(".kd")]
            if not want:
                continue
            txt = subprocess.run([objdump, "-d", "--disassemble-symbols=" + ",".join(want), fn], capture_output=True, text=True,
                                 check=True).stdout
        cur = None
        for line in txt.splitlines():
            h = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
            if h:
                cur = kernels.setdefault(h.group(1), [])
                continue
            q = re.match(r"^\s+(\S+)\s*(.*?)\s*// ([0-9A-F]+):((?: [0-9A-F]{8})+)(?: <\S+\+0x([0-9A-Fa-f]+)>)?", line)
            if q and cur is not None:
                cur.append((int(q.group(3), 16), q.group(1), q.group(2), q.group(5)))
    return kernels


def vregs(operand):
    """Registers a vector operand names: v7 -> {7}, v[4:5] -> {4, 5}."""
    q = re.match(r"^v\[(\d+):(\d+)\]$", operand)
    if q:
        return set(range(int(q.group(1)), int(q.group(2)) + 1))
    q = re.match(r"^v(\d+)$", operand)
    return {int(q.group(1))} if q else set()


def dpp_hazards(insts):
    """For every v_fmac_f64_dpp: a VALU write of its DPP source within the 2 preceding issue slots, or an EXEC write within the 5
    preceding (s_nop N counts N + 1) -- the wait states ADVICE.md (round 6) and the comment above dpp_col in small_solvers.hip.h
    name -- on ANY path that reaches it: straight-line predecessors and every branch that lands inside the window."""
    base = insts[0][0]
    index = {adr: i for i, (adr, *_rest) in enumerate(insts)}
    preds = {i: [] for i in range(len(insts))}
    for i, (adr, mn, ops, target) in enumerate(insts):
        ends = mn in ("s_branch", "s_endpgm", "s_setpc_b64", "s_swappc_b64")
        if not ends and i + 1 < len(insts):
            preds[i + 1].append(i)
        if target is not None and mn.startswith(("s_branch", "s_cbranch")):
            j = index.get(base + int(target, 16))
            if j is not None:
                preds[j].append(i)
    found = []

    def walk(i, slots, src, origin, seen):
        for j in preds[i]:
            adr, mn, ops, _t = insts[j]
            first = ops.split(",")[0].strip() if ops else ""
            writes_exec = first.startswith("exec") or "saveexec" in mn or mn.startswith("v_cmpx")
            dst = vregs(first)
            if mn.startswith("v_swap"):      # two destinations
                dst = set().union(*(vregs(o.strip()) for o in ops.split(",")))
            writes_src = mn.startswith("v_") and not mn.startswith(("v_cmp", "v_readlane", "v_readfirstlane")) and dst & src
            if writes_src and slots < 2:
                found.append((hex(insts[origin][0]), "VALU write of the DPP source", hex(adr), mn, ops, slots))
            if writes_exec and slots < 5:
                found.append((hex(insts[origin][0]), "EXEC write", hex(adr), mn, ops, slots))
            cost = 1
            if mn == "s_nop":
                cost = int(ops.split()[0], 0) + 1
            if slots + cost < 5 and (j, slots + cost) not in seen:
                seen.add((j, slots + cost))
                walk(j, slots + cost, src, origin, seen)

    n = 0
    for i, (adr, mn, ops, _t) in enumerate(insts):
        if mn == "v_fmac_f64_dpp":
            n += 1
            walk(i, 0, vregs(ops.split(",")[1].strip()), i, set())
    return n, found


def test_dpp_wait_states_in_the_built_library():
    kernels = disassemble_dpp_kernels()
    assert len(kernels) == 6, sorted(kernels)
    for name, insts in sorted(kernels.items()):
        n, found = dpp_hazards(insts)
        print(name, len(insts), "instructions,", n, "v_fmac_f64_dpp")
        assert n >= 16 and n % 16 == 0, (name, n)   # 16 columns x RB row blocks at every product site
        assert not found, (name, found[:8])


def test_dpp_hazard_checker_sees_a_planted_hazard():
    """The checker itself: a VALU write one slot ahead, an EXEC write three slots ahead, a branch that lands behind the s_nop."""
    fm = "v[0:1], v[4:5], v[8:9] row_newbcast:0 row_mask:0xf bank_mask:0xf"
    clean = [(0, "v_mov_b32_e32", "v4, 0", None), (4, "s_nop", "4", None), (8, "v_fmac_f64_dpp", fm, None)]
    assert dpp_hazards(clean) == (1, [])
    valu = [(0, "s_nop", "4", None), (4, "v_mov_b32_e32", "v5, 0", None), (8, "s_waitcnt", "lgkmcnt(0)", None),
            (12, "v_fmac_f64_dpp", fm, None)]
    assert [f[1] for f in dpp_hazards(valu)[1]] == ["VALU write of the DPP source"]
    ex = [(0, "s_or_b64", "exec, exec, s[2:3]", None), (4, "s_nop", "2", None), (8, "v_fmac_f64_dpp", fm, None)]
    assert [f[1] for f in dpp_hazards(ex)[1]] == ["EXEC write"]
    jump = [(0, "v_add_f64", "v[4:5], v[4:5], v[6:7]", None), (8, "s_branch", "3", "10"), (12, "s_nop", "4", None),
            (16, "v_fmac_f64_dpp", fm, None)]
    assert [f[1] for f in dpp_hazards(jump)[1]] == ["VALU write of the DPP source"]


def test_switch_defaults_are_the_library_s():
    """DEFAULTS is what the finally blocks set: it has to be what the library starts with."""
    src = open(os.path.join(_libs.ROOT, "faspsolver_amd", "csrc", "device_csr.hip.h")).read()
    tuning = src[src.index("struct Tuning"):]
    for key, v in DEFAULTS.items():
        assert int(re.search(r"\b%s = (-?\d+)" % key, tuning).group(1)) == v, key


# ---------------------------------------------------------------------------------------------------------------------
# section 3: the block coarse solver, k_gmres_small<SmallBSR, LV> (bsr.hip.h, mgcycle_bsr's coarsest level), through
# BSRAMG(max_levels = 1).precond().  precond_amg_bsr() starts from fasp_param_amg_init: the coarse GMRES receives tol = 1e-6 (no
# factor 1e-4 on this path), abstol = tol * 1e-8, MaxIt = min(n * n, 200), restart 25 -- fasp_solver_dbsr_pvgmres without
# preconditioner, the oracle's gmres_core on the block operator (orc_gmres_bsr).
# Thresholds, in scalar rows n = ROW * nb, read off bsr.hip.h and small_solvers.hip.h:
#   n <= 64 * GM_NE = 1024        the modified Gram-Schmidt sweep in one wavefront, (n + 63) / 64 elements per lane;
#   nb = 3, n <= SMALL_BLOCK = 512  the matrix on chip in registers; up to 2 * SMALL_BLOCK with cache2: the rows beyond 512 keep
#                                 GM_CB = 14 blocks of 28 bytes each in LDS, while 216 n + 392 (n - 512) <= 140 KiB, i.e. n <= 565;
#   216 n (+ the above) <= 140 KiB, n <= 663   the basis in LDS (LV), else in memory; small_lds = 0 forces the latter;
#   n <= 4096 and NNZ nb^2 <= 131072           k_gmres_small at all, else the general device GMRES.
# ---------------------------------------------------------------------------------------------------------------------
BSR_TOL = 1e-6
BSR_CASES = [(1, r, 5) for r in (1, 64, 65, 663, 664, 1023, 1024, 1025, 4095, 4096, 4097)] + \
            [(2, r, 5) for r in (1, 331, 332, 511, 512, 513, 2047, 2048, 2049)] + \
            [(3, r, 5) for r in (1, 170, 171, 188, 189, 221, 222, 341, 342, 1365, 1366)] + \
            [(5, r, 5) for r in (1, 132, 133, 204, 205, 819, 820)] + [(5, 700, 9)]   # (the last: NNZ nb^2 = 157 000 > 131072 at n = 3500)


def test_block_thresholds_are_the_kernel_s():
    src = open(os.path.join(_libs.ROOT, "faspsolver_amd", "csrc", "small_solvers.hip.h")).read()
    for key, v in (("GM_NE", GM_NE), ("GM_CB", GM_CB), ("SMALL_BLOCK", SMALL_BLOCK)):
        assert int(re.search(r"constexpr int %s = (\d+);" % key, src).group(1)) == v, key


@functools.lru_cache(maxsize=None)
def block_problem(nb, ROW, per_row):
    """Block matrix on the pattern of the 2-D Laplacian cut to ROW block rows (5 blocks per row) or of a band of half-width 4 (9
    blocks per row): random dyadic blocks,
    the diagonal of every scalar row = the sum of the moduli of the rest of that row + 1 (strictly diagonally dominant, not
    symmetric).  -> (ia, ja, val, b, scalar CSR of the same matrix)"""
    rng = np.random.default_rng(1000 * nb + ROW)
    if per_row == 5:
        ia, ja, _ = laplacian(ROW, 2)
    else:
        i = np.repeat(np.arange(ROW), 9); j = i + np.tile(np.arange(-4, 5), ROW)
        ia, ja, _ = to_csr(ROW, i[(j >= 0) & (j < ROW)], j[(j >= 0) & (j < ROW)], np.ones(int(((j >= 0) & (j < ROW)).sum())))
    val = rng.integers(-16, 17, size=(len(ja), nb, nb)).astype(np.float64) / 64.0
    rows = rows_of(ia)
    dk = np.flatnonzero(ja == rows)
    assert len(dk) == ROW
    r = np.arange(nb)
    val[dk[:, None], r, r] = 0.0
    rowsum = np.zeros((ROW, nb)); np.add.at(rowsum, rows, np.abs(val).sum(axis=2))
    val[dk[:, None], r, r] = rowsum + 1.0
    b = rng.standard_normal(ROW * nb)
    # scalar CSR: row i nb + r holds, block by block, the columns ja nb + c
    cnt = np.diff(ia)
    sia = np.zeros(ROW * nb + 1, dtype=np.int32); sia[1:] = np.cumsum(np.repeat(cnt * nb, nb))
    srows = (rows[:, None, None] * nb + r[None, :, None]) + 0 * r[None, None, :]
    scols = (ja[:, None, None] * nb + r[None, None, :]) + 0 * r[None, :, None]
    o = np.argsort(srows.ravel(), kind="stable")
    return ia, ja, val.reshape(-1), b, (sia, scols.ravel()[o].astype(np.int32), val.ravel()[o])


def orc_block_gmres(nb, ROW, per_row):
    ia, ja, val, b, _ = block_problem(nb, ROW, per_row)
    n = ROW * nb
    o = _libs.oracle()
    o.orc_gmres_bsr.argtypes = [C.c_int, C.POINTER(T.dBSRmat), C.POINTER(T.dvector), C.POINTER(T.dvector), C.c_double, C.c_double,
                                C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    A, keep = T.as_bsr(ia, ja, val, nb)
    x = np.zeros(n)
    bv, bk = T.as_vec(b); xv = T.dvector(n, T.dp(x))
    st = o.orc_gmres_bsr(0, C.byref(A), C.byref(bv), C.byref(xv), BSR_TOL, BSR_TOL * 1e-8, min(n * n, 200), GM_RESTART, 1, 0, None)
    return st, x


@pytest.mark.parametrize("nb,ROW,per_row", BSR_CASES)
def test_oracle_block_gmres_is_inside_the_bound(nb, ROW, per_row):
    """CPU half of section 3: the oracle converges on every case and its result satisfies (a)."""
    ia, ja, val, b, (sia, sja, sa) = block_problem(nb, ROW, per_row)
    n = ROW * nb
    st, x = orc_block_gmres(nb, ROW, per_row)
    if n == 1:      # MaxIt = min(n * n, 200) = 1: the reference reports MAXIT behind its one, exact, step
        assert st == T.ERROR_SOLVER_MAXIT, st
    else:
        assert 0 < st <= min(n * n, 200), st
    rel, bound, _ = residual_check(sia, sja, sa, b, np.zeros(n), x, BSR_TOL, per_row * nb)
    print(f"nb {nb} ROW {ROW}: oracle its {st} relres {rel:.3e} bound {bound:.3e}")
    assert rel < bound, (rel, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("nb,ROW,per_row", BSR_CASES)
def test_block_coarse_gmres(gpu, nb, ROW, per_row):
    ia, ja, val, b, (sia, sja, sa) = block_problem(nb, ROW, per_row)
    n = ROW * nb
    s_orc, x_orc = orc_block_gmres(nb, ROW, per_row)
    itp, amgp = _libs.bsr_params()
    amgp.max_levels = 1; amgp.maxit = 1
    H = fa.BSRAMG(ia, ja, val, nb, amgp)
    try:
        assert H.num_levels == 1
        for lds in (1, 0):
            set_tune(small_lds=lds)
            rb = guarded(b); r_in = rb[CANARY:CANARY + n]
            z = H.precond(r_in)
            info = H.coarse_kernel_info()
            tag = f"nb {nb} ROW {ROW} small_lds {lds}"
            rel, bound, _ = residual_check(sia, sja, sa, b, np.zeros(n), z, BSR_TOL, per_row * nb)
            kname = "k_gmres_small<SmallBSR,LV=%d,cache2=%d>" % info[1:3] if info[0] == 8 else "gmres_device"
            print(f"{tag}: ran {kname} status {info[3]} its {info[4]} (oracle {s_orc}) relres {rel:.3e} (bound {bound:.3e}) "
                  f"|z - z_orc| {np.linalg.norm(z - x_orc):.3e}")
            RAN.setdefault(kname, []).append(f"nb{nb}-{ROW}")
            assert tuple(info[:3]) == expected_block_kernel(nb, ROW, len(ja), lds), (tag, info)
            assert canaries_intact(rb, n) and np.array_equal(r_in, b) and not np.isnan(z).any(), tag
            assert rel < bound, (tag, rel, bound)                 # (a)
            if s_orc > 0:
                assert info[3] > 0 and info[4] == s_orc, (tag, info, s_orc)   # equal iteration count
            else:
                assert info[3] == s_orc, (tag, info, s_orc)       # (n = 1: the reference's MAXIT)
    finally:
        set_tune(**DEFAULTS)
        H.free()


@pytest.mark.gpu
def test_zz_kernel_coverage_table(gpu):
    """The last GPU test of the module: every instantiation the selection can reach was run by a test above, in this process (a
    tripwire over the whole module, not a test to select on its own); the table kernel -> cases goes to the output."""
    for kname in sorted(RAN):
        cases = RAN[kname]
        print(f"{kname}: {len(cases)} applications, e.g. {', '.join(sorted(set(cases))[:6])}")
    assert RAN, "the section-1 tests of this module fill the table: run the module as a whole"
    need = [(1, 4, 1), (1, 4, 0), (1, 6, 1), (1, 6, 0), (1, 8, 1), (1, 8, 0), (2, 32, 0), (2, 48, 0), (2, 64, 0), (3, 0, 0),
            (4, 2, 0), (4, 1, 0), (4, 0, 0), (5, 4, 0), (5, 10, 0), (5, 16, 0), (6, 32, 1), (6, 32, 0), (6, 48, 1), (6, 48, 0),
            (6, 56, 1), (6, 56, 0), (6, 64, 1), (6, 64, 0), (7, 4, 0), (7, 10, 0), (7, 0, 0)]
    missing = [kernel_name(k) for k in need if kernel_name(k) not in RAN]
    assert not missing, missing
    for k in ("k_gmres_small<SmallBSR,LV=1,cache2=0>", "k_gmres_small<SmallBSR,LV=0,cache2=0>", "k_gmres_small<SmallBSR,LV=1,cache2=1>",
              "k_gmres_small<SmallBSR,LV=0,cache2=1>", "gmres_device"):
        assert k in RAN, k
