"""The plain CSR kernels -- k_csr_lstream, k_csr_wstream2, k_csr_xtile (csrc/kernels2.hip.h), the four k_csr_wstream<OP, RW, CAPW> and the six
k_csr_rows<L, OP> (csrc/kernels.hip.h), the four k_csr_estream<L, OP> (csrc/kernels3.hip.h) -- on the irregular matrices of tests/_plain_cases.py,
every row operation, one by one through fasp_hip_matrix_op, against the CPU oracle's restatement of the reference on the same inputs.

Traits and plan.  fasp_hip_matrix_traits must report, field by field, the traits the generator restated from the upload rules;
fasp_hip_csr_plan, asked under the run's tune keys for THIS operation on those device traits, must name the instantiation the run was built for;
*kind_out must be the family of y = M x.  A matrix that misses its kernel fails.

Order-preserving kernels (k_csr_lstream, k_csr_wstream2, k_csr_xtile, k_csr_wstream): every row is summed left to right in storage order from
the stored values, so y (and y2 of op 8) must be BIT-EQUAL to the oracle's, compared as int64 so that a wrong signed zero shows.

k_csr_rows and k_csr_estream sum lane-strided partial sums and a shuffle tree (on a device copy sorted by column, where the upload sorted):
another order of the same terms.  y is held to the a-priori bound of _libs.sum_bound_ratio, |y - exact| <= (m + 1) u / (1 - (m + 1) u) sabs
(u = 2^-53, + 2^-63 |exact| for the 80-bit side), against the np.longdouble evaluation `exact` of the whole expression of the operation
(_plain_cases.longdouble_op).  With len the entries of the row, t = sum a_ij x_j and s = sum |a_ij x_j|, every product rounded once and every sum of
len terms, in any order, carrying at most len - 1 roundings per term:
  ops 0, 7, 8   y = t:                          m = len,      sabs = s.
  ops 1 .. 4    y = v0 + alpha t (v0 = b or the old y; alpha = -1, 1, -1, 0.7): the scaling and the final sum round once each:
                                                m = len + 2,  sabs = |v0| + |alpha| s.
  op 5, k_csr_rows   y = (1 - w) x_i + w (b_i - t') / d, t' and s' over the entries off the diagonal (loff of them), d the last diagonal stored;
                1 - w is rounded once and is part of the expression; b - t', w *, / d, (1 - w) * x_i and the final sum round once each:
                                                m = loff + 5, sabs = |(1 - w) x_i| + |w / d| (|b_i| + s').
  op 5, k_csr_estream   the row sum takes EVERY entry and the epilogue subtracts d x_i again (kernels3.hip.h): both products of the diagonal
                enter, and the product d x_i and its subtraction round once more each:
                                                m = len + 7,  sabs = |(1 - w) x_i| + |w / d| (|b_i| + s' + 2 |d x_i|).
                A row with |d| <= 1e-20 (no diagonal, or 0.0 stored) keeps x_i: m = 0, exact.
  op 6          y = x_i + (b_i - t) / l, l = sum |a_ij| formed on the host in double (len roundings of its own, in the divisor); b - t, / l and the
                final sum round once each:      m = 2 len + 3, sabs = |x_i| + (|b_i| + s) / l.
Rows of at most one entry have one order only: they must be bit-equal to the oracle's.  y2 of op 8 is an elementwise function of y: it must be
bit-equal to that expression evaluated on the device's own y.  The largest error / bound per kernel is printed; it is a measurement against the
bound (<= 1), not a tuned tolerance.  Measured on an MI355X: 0.597 at most (k_csr_rows<32> and <64>; the other
k_csr_rows 0.51 .. 0.55, k_csr_estream<4 .. 32> 0.35 .. 0.54).

Fused sums.  Op 7 everywhere, op 5 where the plan says fused_zr (k_csr_lstream, k_csr_wstream2, k_csr_xtile; elsewhere `red` must come back NaN):
summed over the kernel's own block layout, held to sum_bound_ratio with m = the number of rows against the np.longdouble sum of y_i b_i over the
device's y.  Every call is made twice and must repeat itself bit for bit."""
import ctypes as C

import numpy as np
import pytest

from faspsolver_amd import _types as T

import _csr_cases as cc
import _plain_cases as pc
from _libs import oracle, sum_bound_ratio

pytestmark = pytest.mark.gpu

OPNAME = {v: k for k, v in cc.OPS.items()}
_traits_seen = {}                  # device traits per case: the upload does not depend on the tune keys
_worst = {}                        # kernel -> largest error / bound seen


def _protos(L):
    P = C.POINTER
    D = P(C.c_double)
    L.fasp_hip_matrix_op.argtypes = [P(T.dCSRmat), C.c_int, D, D, D, D, C.c_double, D, P(C.c_int)]
    L.fasp_hip_matrix_traits.argtypes = [P(T.dCSRmat), P(C.c_int)]
    L.fasp_hip_csr_plan.argtypes = [P(C.c_int), C.c_int, C.c_int, C.c_int, P(C.c_int), D]


def _bits(v):
    return np.ascontiguousarray(v).view(np.int64)


def _once(L, A, nrow, op, partials, x, b, y0, scalar):
    y = y0.copy(); y2 = np.zeros(nrow); red = C.c_double(0); k = C.c_int(-1)
    st = L.fasp_hip_matrix_op(C.byref(A), op, T.dp(x), T.dp(b), T.dp(y), T.dp(y2), scalar, C.byref(red) if partials else None, C.byref(k))
    assert st == 0, st
    return y, y2, red.value, k.value


def _check(L, run, op, partials):
    c = pc.build(run)
    nrow, ncol, label = c["nrow"], c["ncol"], f"{run['id']} {OPNAME[op]}"
    A, keep = T.as_csr(c["ia"], c["ja"], c["val"], c["ncol"])
    # --- traits of the device copy, and the plan of this operation on them
    key = (run["fn"].__name__, run["args"])
    if key not in _traits_seen:
        t = (C.c_int * len(cc.TRAITS))()
        assert L.fasp_hip_matrix_traits(C.byref(A), t) == 0
        _traits_seen[key] = dict(zip(cc.TRAITS, list(t)))
    dev = _traits_seen[key]
    wrong = {k: (dev[k], c["traits"][k]) for k in cc.TRAITS if dev[k] != c["traits"][k]}
    assert not wrong, (label, "device traits != restated traits", wrong)
    t = (C.c_int * len(cc.TRAITS))(*[dev[k] for k in cc.TRAITS])
    out = (C.c_int * (len(cc.PLAN) + 1))()
    assert L.fasp_hip_csr_plan(t, 0 if op == 8 else op, 0, int(partials), out, None) == 0
    plan = dict(zip(cc.PLAN, list(out)))
    kernel = cc.KERNELS[plan["kernel"]]
    assert kernel == pc.expect(run, op, partials), (label, kernel, pc.expect(run, op, partials))
    want_plan = cc.expected_plan(c["traits"], 0 if op == 8 else op, False, partials, pc.plan_tune(run))
    assert plan == {k: want_plan[k] for k in cc.PLAN}, (label, plan, want_plan)      # tile, grid, index form (ja16 / jbase passed or dropped), fused_zr
    family0 = out[len(cc.PLAN)]
    assert family0 == cc.expected_plan(c["traits"], 0, False, False, pc.plan_tune(run))["family"]
    # --- the operation, twice
    scalar = cc.SCALAR.get(op, 0.0)
    x, b, y0 = cc.inputs(nrow, ncol, op, 7 * pc.RUNS.index(run) + op, c["inf_rows"])
    want, want2 = cc.reference(oracle(), c, op, x, b, y0, scalar)
    assert np.all(np.isfinite(want))
    y, y2, red, k1 = _once(L, A, nrow, op, partials, x, b, y0, scalar)
    ya, y2a, reda, k2 = _once(L, A, nrow, op, partials, x, b, y0, scalar)
    assert (k1, k2) == (family0, family0), (label, k1, k2, family0)
    assert np.array_equal(_bits(y), _bits(ya)), (label, "the second call differs")
    assert np.array_equal(_bits(y2), _bits(y2a)), (label, "y2: the second call differs")
    assert red == reda or (np.isnan(red) and np.isnan(reda)), (label, red, reda)
    if kernel in pc.ORDER_KERNELS:
        bad = np.flatnonzero(_bits(y) != _bits(want))
        assert len(bad) == 0, (label, kernel, len(bad), bad[:8], y[bad[:8]], want[bad[:8]])
        if op == 8:
            bad = np.flatnonzero(_bits(y2) != _bits(want2))
            assert len(bad) == 0, (label, kernel, "y2", len(bad), bad[:8], y2[bad[:8]], want2[bad[:8]])
    else:
        assert kernel.startswith("rows") or kernel.startswith("estream")
        exact, sabs, m = pc.longdouble_op(c, op, x, b, y0, scalar, diag_in_sum=kernel.startswith("estream") and op == 5)
        ratio = sum_bound_ratio(y, exact, sabs, m)
        _worst[kernel] = max(_worst.get(kernel, 0.0), ratio)
        print(f"{label} {kernel}: error / bound {ratio:.3e} (largest of {kernel} so far {_worst[kernel]:.3e})")
        assert ratio <= 1.0, (label, kernel, ratio)
        short = np.flatnonzero(np.diff(c["ia"]) <= 1)
        bad = short[_bits(y)[short] != _bits(want)[short]]
        assert len(bad) == 0, (label, kernel, "rows of at most one entry", bad[:8], y[bad[:8]], want[bad[:8]])
        if op == 8:
            with np.errstate(divide="ignore", invalid="ignore"):
                mine = np.where(np.abs(b) > 1e-20, (1 - scalar) * 0.0 + scalar * y / b, 0.0)
            bad = np.flatnonzero(_bits(y2) != _bits(mine))
            assert len(bad) == 0, (label, kernel, "y2", len(bad), bad[:8], y2[bad[:8]], mine[bad[:8]])
    # --- the fused sum
    if op == 7 or (op == 5 and partials and plan["fused_zr"]):
        ld = np.longdouble
        terms = y.astype(ld) * b.astype(ld)
        ratio = sum_bound_ratio(np.array([red]), np.array([terms.sum()]), np.array([np.abs(terms).sum()]), np.array([nrow]))
        print(f"{label} {kernel}: fused sum {red!r}, error / bound {ratio:.3e}")
        assert ratio <= 1.0, (label, kernel, red, float(terms.sum()), ratio)
    elif partials:
        assert np.isnan(red), (label, kernel, "no fused partials planned, yet a sum came back", red)


RUN_OPS = [(run, op, partials) for run in pc.RUNS for op, partials in run["ops"]]


@pytest.mark.parametrize("run,op,partials", RUN_OPS, ids=[f"{r['id']}-{OPNAME[o]}" + ("" if p == (o in (5, 7)) else "_nopartials") for r, o, p in RUN_OPS])
def test_plain_kernel_against_oracle(gpu, run, op, partials):
    L = gpu.lib()
    _protos(L)
    try:
        for key, value in run["tune"]:
            assert L.fasp_hip_tune(key.encode(), value) == 0
        _check(L, run, op, partials)
    finally:
        for key, _ in run["tune"]:
            L.fasp_hip_tune(key.encode(), pc.TUNE_RESTORE[key])

