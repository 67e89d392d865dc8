"""k_csr_sell (csrc/kernels4.hip.h): the value-indexed sliced-ELL kernel against the plain-CSR kernel it replaces (k_csr_wstream2), on
level 2 of P7(64) and on a random matrix with few distinct values, for every row operation the replaced kernel serves there.

The row sums of both kernels are the reference's left-to-right sums, so the float64 vectors must be EQUAL (np.array_equal); the fused
reductions -- (t, p) of OP_MXV_DOT, (x_new, b) of the Jacobi sweep -- are summed over another block layout and are held to 1e-13
relative, the bound of the fixed-tree reductions in tests/test_gpu_parity.py.  The coding is switched off with its own tune key
(fasp_hip_tune("sell", 0)), which leaves the other codings on (k_csr_xtile, which keeps the operators that have its lists -- level 2 at
64^3 is one -- is switched off throughout, so that the two kernels compared are k_csr_sell and k_csr_wstream2); the same again with every launch cut into three row windows
(fasp_hip_tune("split_rows", k)); and one whole solve, held to what tests/test_gpu_compress.py asks of coded against plain."""
import ctypes as C

import numpy as np
import pytest

from faspsolver_amd import _types as T

from _libs import default_params, poisson7pt

pytestmark = pytest.mark.gpu

OPS = {"mxv": 0, "resid": 1, "add": 2, "sub": 3, "axpy": 4, "jacobi": 5, "l1diag": 6, "mxv_dot": 7, "mxv_zx": 8}
SELL = 11   # kernel family code of fasp_hip_amg_kernel_info


def _protos(L):
    P = C.POINTER
    D = P(C.c_double)
    L.fasp_hip_level_op.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, D, D, D, D, C.c_double, D]
    L.fasp_hip_matrix_op.argtypes = [P(T.dCSRmat), C.c_int, D, D, D, D, C.c_double, D, P(C.c_int)]


def _params():
    itp, amgp = default_params()
    itp.tol = 1e-8; itp.itsolver_type = 1
    amgp.smoother = T.SMOOTHER_JACOBI; amgp.relaxation = 0.6667
    return itp, amgp


def _inputs(nrow, ncol, op, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(nrow if op in (5, 6) else ncol)
    b = rng.standard_normal(nrow)
    if op == 8:
        b = 1.0 + np.abs(b)           # the next level's diagonal
        b[::17] = 0.0                 # ... with entries the guard of the fused sweep catches
    # the fused sums as the solver forms them -- (A p, p) and (z, r) with z close to w r / d: sums of mostly positive terms, for which
    # the 1e-13 bound on a re-ordered sum holds (a sum of random signs loses sqrt(n) of it to cancellation)
    if op == 7:
        b = x.copy()
    if op == 5:
        x = 0.01 * x
    y0 = rng.standard_normal(nrow)
    return x, b, y0


def _run(call, nrow, ncol, op, seed, want_red):
    x, b, y0 = _inputs(nrow, ncol, op, seed)
    y = y0.copy(); y2 = np.zeros(nrow); red = C.c_double(0)
    scalar = {4: 0.7, 5: 0.6667, 6: 1.0, 8: 0.6667}.get(op, 0.0)
    st = call(op, T.dp(x), T.dp(b), T.dp(y), T.dp(y2), scalar, C.byref(red) if want_red else None)
    assert st == 0, st
    return y, y2, red.value


def _compare(L, call, nrow, ncol, name, seed):
    op = OPS[name]
    want_red = name in ("mxv_dot", "jacobi")
    out = {}
    try:
        L.fasp_hip_tune(b"xtile", 0)     # (an operator that also has k_csr_xtile's lists runs that kernel unless it is switched off)
        for sell in (1, 0):
            L.fasp_hip_tune(b"sell", sell)
            out[sell] = _run(call, nrow, ncol, op, seed, want_red)
            if sell == 1:
                again = _run(call, nrow, ncol, op, seed, want_red)
                assert np.array_equal(out[1][0], again[0]) and (not want_red or out[1][2] == again[2])   # deterministic
    finally:
        L.fasp_hip_tune(b"sell", 1); L.fasp_hip_tune(b"xtile", 1)
    assert np.all(np.isfinite(out[0][0]))
    assert np.array_equal(out[1][0], out[0][0]), name
    if name == "mxv_zx":
        assert np.array_equal(out[1][1], out[0][1]), name
    if want_red:
        r1, r0 = out[1][2], out[0][2]
        print(f"{name}: fused sum coded {r1!r} plain {r0!r} rel diff {abs(r1 - r0) / max(abs(r0), 1e-300):.3e}")
        assert np.isfinite(r1) and np.isfinite(r0)
        assert abs(r1 - r0) <= 1e-13 * abs(r0)
    return out


@pytest.fixture(scope="module")
def p7_64(gpu):
    ia, ja, a, f, ue = poisson7pt(64)
    itp, amgp = _params()
    H = gpu.AMG(ia, ja, a, amgp)
    _protos(gpu.lib())
    yield H, f, itp
    H.close()


@pytest.mark.parametrize("split", [0, 2048])
@pytest.mark.parametrize("name", list(OPS))
def test_level2_of_p7_64_every_op_equals_plain_kernel(gpu, p7_64, name, split):
    H, f, itp = p7_64
    L = gpu.lib()
    nr, nc, ia, ja, val = H.matrix(2, 0)
    try:
        L.fasp_hip_tune(b"xtile", 0)
        kind, nbytes = H.kernel_info(2, 0)
        L.fasp_hip_tune(b"sell", 0)
        kind0, nbytes0 = H.kernel_info(2, 0)
    finally:
        L.fasp_hip_tune(b"sell", 1); L.fasp_hip_tune(b"xtile", 1)
    assert kind == SELL, (kind, nr, len(ja))                   # the level the coding is for runs the new kernel ...
    assert nbytes <= 4.6 * len(ja)
    assert kind0 == 8 and nbytes0 > 12.0 * len(ja)              # ... and k_csr_wstream2 with the key off
    assert H.kernel_info(2, 0)[0] in (SELL, 10)                 # (k_csr_xtile keeps the operators it was built for)
    assert H.kernel_info(0, 0)[0] in (5, 6)                     # the key leaves the other codings alone
    call = lambda op, *rest: L.fasp_hip_level_op(H.h, 2, 0, op, *rest)
    try:
        L.fasp_hip_tune(b"split_rows", split)
        _compare(L, call, nr, nc, name, seed=OPS[name] + 100)
    finally:
        L.fasp_hip_tune(b"split_rows", 0)


def _random_matrix():
    """6 000 rows of 20-26 entries in storage order (diagonal first, the rest unsorted) with 300 distinct values; signed zeros among them;
    a row count that is no multiple of 64; an empty row and a row of one entry."""
    rng = np.random.default_rng(21)
    n = 6000 + 37
    lens = rng.integers(20, 27, n)
    lens[100] = 0; lens[200] = 1
    ia = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    table = rng.standard_normal(300)
    table[:2] = [0.0, -0.0]
    ja = np.zeros(ia[-1], np.int32)
    for r in range(n):
        if lens[r] == 0:
            continue
        lo = max(0, min(n - 3000, r - 1500))
        others = np.setdiff1d(np.arange(lo, lo + 3000), [r])
        ja[ia[r]] = r
        ja[ia[r] + 1:ia[r + 1]] = rng.choice(others, size=lens[r] - 1, replace=False)
    val = table[rng.integers(0, 300, ia[-1])]
    val[ia[:-1][lens > 0]] = 30.0 + table[rng.integers(2, 300, int((lens > 0).sum()))]    # dominant diagonals, few values
    return n, ia, ja, val


@pytest.mark.parametrize("split", [0, 1024])
@pytest.mark.parametrize("name", list(OPS))
def test_random_matrix_every_op_equals_plain_kernel(gpu, name, split):
    L = gpu.lib()
    _protos(L)
    n, ia, ja, val = _random_matrix()
    A, keep = T.as_csr(ia, ja, val)
    kinds = []

    def call(op, *rest):
        k = C.c_int(-1)
        st = L.fasp_hip_matrix_op(C.byref(A), op, *rest, C.byref(k))
        kinds.append(k.value)
        return st
    try:
        L.fasp_hip_tune(b"split_rows", split)
        out = _compare(L, call, n, n, name, seed=OPS[name] + 200)
    finally:
        L.fasp_hip_tune(b"split_rows", 0)
    assert kinds[0] == SELL and kinds[-1] != SELL, kinds
    if name == "mxv":   # ... and the reference's row loop itself
        x, b, y0 = _inputs(n, n, 0, OPS[name] + 200)
        lens = np.diff(ia)
        acc = np.zeros(n)
        for k in range(int(lens.max())):
            rows = np.nonzero(lens > k)[0]
            e = ia[rows].astype(np.int64) + k
            acc[rows] = acc[rows] + val[e] * x[ja[e]]
        assert np.array_equal(out[1][0], acc)


def test_whole_solve_with_and_without_the_coding(gpu, p7_64):
    H, f, itp = p7_64
    L = gpu.lib()
    out, pc = {}, {}
    r = np.random.default_rng(11).standard_normal(len(f))
    try:
        L.fasp_hip_tune(b"xtile", 0)
        for sell in (1, 0):
            L.fasp_hip_tune(b"sell", sell)
            pc[sell] = H.precond(r)          # one multigrid cycle: every operator and epilogue, no fused dots
            out[sell] = H.solve(f, itp)
    finally:
        L.fasp_hip_tune(b"sell", 1); L.fasp_hip_tune(b"xtile", 1)
    assert np.array_equal(pc[1], pc[0])      # bit for bit
    s1, x1, h1, _ = out[1]; s0, x0, h0, _ = out[0]
    print(f"iterations coded {s1} plain {s0}; max |dx| / max |x| = {np.abs(x1 - x0).max() / np.abs(x0).max():.3e}")
    assert s1 == s0 and s1 > 0
    assert np.allclose(h1, h0, rtol=1e-9, atol=1e-13 * h0[0])
    assert np.abs(x1 - x0).max() <= 1e-11 * np.abs(x0).max()
