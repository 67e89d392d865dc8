"""fasp_hip_blas1_op on a machine without a GPU -- declared, exported, wrapped, refusing bad arguments before any work and refusing to run
without a device (ERROR_MISC, nothing written) -- and the numpy side of tests/test_gpu_blas1_kernels.py checked on its own: the emulation
of k_finalize's order is exact where every order is, and differs from other orders on the inputs the device test folds; the plain double
sums of the references stay within the a-priori bound the device is held to."""
import os
import re

import numpy as np
import pytest

import _blas1_cases as bc
from _libs import ROOT, T, sum_bound_ratio


def test_the_entry_is_declared_exported_and_wrapped(fa):
    L = fa.lib()
    dev = open(os.path.join(ROOT, "include", "fasp_hip_dev.h")).read()
    assert hasattr(L, "fasp_hip_blas1_op") and "fasp_hip_blas1_op" in fa.EXPORTS and re.search(r"\bfasp_hip_blas1_op\s*\(", dev)
    assert callable(fa.blas1_op) and fa.BLAS1_KERNELS == bc.KERNELS
    for k, name in enumerate(bc.KERNELS):   # the header's table numbers the kernels as the wrapper does
        assert re.search(r"^ \*\s+%d k_%s\b" % (k, name), dev, flags=re.M), (k, name)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "fasp_hip_blas1_op" in design


def _bad_calls():
    n = 8
    v = [np.ones(n) for _ in range(6)]
    part = np.ones(4)
    yield "unknown kernel (below)", dict(kernel=-1, n=n, vectors=v)
    yield "unknown kernel (above)", dict(kernel=len(bc.KERNELS), n=n, vectors=v)
    yield "n = 0", dict(kernel="axpy", n=0, vectors=v[:2])
    yield "negative variant", dict(kernel="axpy", n=n, vectors=v[:2], variant=-1)
    yield "axpy has no variant", dict(kernel="axpy", n=n, vectors=v[:2], variant=1)
    yield "axpyz has three variants", dict(kernel="axpyz", n=n, vectors=v[:3], variant=3)
    yield "cg_update variant out of range", dict(kernel="cg_update", n=n, vectors=v, variant=32)
    yield "cg_update with both diagonal sources", dict(kernel="cg_update", n=n, vectors=v, variant=24)
    yield "a vector is missing", dict(kernel="dot", n=n, vectors=v[:1])
    yield "cg_update without its zdiag slot", dict(kernel="cg_update", n=n, vectors=v[:5])
    yield "folded without partials", dict(kernel="cg_update", n=n, vectors=v, variant=1)
    yield "more partials than the buffer is wide", dict(kernel="cg_update", n=n, vectors=v, variant=1, partials=np.ones(bc.MAXGRID + 1))
    yield "axpby_beta: more partials than the buffer is wide", dict(kernel="axpby_beta", n=n, vectors=v[:2], variant=1, partials=np.ones(bc.MAXGRID + 1))
    yield "mgs_step: more partials than the buffer is wide", dict(kernel="mgs_step", n=n, vectors=v[:3], variant=1, partials=np.ones(bc.MAXGRID + 1))
    yield "partials given to an unfolded variant", dict(kernel="mgs_step", n=n, vectors=v[:3], variant=2, partials=part)
    yield "partials given to a kernel that takes none", dict(kernel="dot", n=n, vectors=v[:2], partials=part)
    yield "finalize: nq = 0", dict(kernel="finalize", n=4, ipar=(0, 0), partials=part)
    yield "finalize: nq = 9", dict(kernel="finalize", n=4, ipar=(9, 0), partials=np.ones(36))
    yield "finalize: G beyond the buffer", dict(kernel="finalize", n=bc.MAXGRID + 1, ipar=(1, 0), partials=np.ones(bc.MAXGRID + 1))
    yield "finalize: npart is not nq * G", dict(kernel="finalize", n=4, ipar=(2, 0), partials=part)
    yield "finalize without partials", dict(kernel="finalize", n=4, ipar=(1, 0))
    yield "bsr_dinv_apply: nb = 0", dict(kernel="bsr_dinv_apply", n=n, vectors=v[:3], ipar=(0,))
    yield "bsr_dinv_apply: n is no multiple of nb", dict(kernel="bsr_dinv_apply", n=n, vectors=[np.ones(3 * n)] + v[:2], ipar=(3,))
    yield "pack without indices", dict(kernel="pack", n=n, vectors=v[:2], ipar=(n,))
    yield "pack: an index behind v", dict(kernel="pack", n=n, vectors=v[:2], ipar=(n,), idx=np.array([0, 1, 2, 3, 4, 5, 6, n]))
    yield "pack: a negative index", dict(kernel="pack", n=n, vectors=v[:2], ipar=(n,), idx=np.array([0, 1, 2, -1, 4, 5, 6, 7]))
    yield "pack: v of length 0", dict(kernel="pack", n=n, vectors=v[:2], ipar=(0,), idx=np.zeros(n, dtype=np.int32))


BAD = list(_bad_calls())


@pytest.mark.parametrize("why", [w for w, _ in BAD])
def test_bad_arguments_are_refused_before_any_work(fa, why):
    """ERROR_INPUT_PAR with or without a device, and nothing comes back: not a vector, not a scalar, not the grid."""
    kw = dict(BAD)[why]
    kw = dict(kw)
    kernel, n = kw.pop("kernel"), kw.pop("n")
    st, res = fa.blas1_op(kernel, n, kw.pop("vectors", ()), **kw)
    assert st == T.ERROR_INPUT_PAR, (why, st)
    assert res["grid"] == 0 and res["pub"] == 0.0 and len(res["red"]) == 0
    assert all(np.all(v == 1.0) for v in res["vec"])


def test_null_arguments_are_refused(fa):
    L = fa.lib()
    x = np.ones(4); red = np.zeros(8); part = np.zeros(8 * 2048); grid = np.zeros(2, dtype=np.int32); pub = np.zeros(1)
    sc = np.zeros(8); ip = np.zeros(4, dtype=np.int32)
    PA = T.c_double_p * 6
    vin = PA(T.dp(x), T.dp(x), None, None, None, None); vout = PA(None, None, None, None, None, None)
    good = [4, 0, 4, T.ip(ip), T.dp(sc), vin, vout, None, 0, None, T.dp(red), T.dp(part), T.ip(grid), T.dp(pub)]
    for k in (3, 4, 5, 6, 10, 11, 12, 13):
        args = list(good); args[k] = None
        assert L.fasp_hip_blas1_op(*args) == T.ERROR_INPUT_PAR, k
    assert grid[0] == 0 and np.all(red == 0.0)


def test_without_a_device_the_entry_returns_error_misc_and_writes_nothing(fa):
    if fa.available():
        pytest.skip("a GPU is present")
    for kernel, variant, _ in bc.ELEMENTWISE:
        vecs, scal, _ = bc.elementwise_case(kernel, 257, variant)
        st, res = fa.blas1_op(kernel, 257, vecs, scal=scal, variant=variant)
        assert st == T.ERROR_MISC, kernel
        assert all(bc.same_bytes(g, v) for g, v in zip(res["vec"], vecs)) and res["grid"] == 0 and res["pub"] == 0.0
    vecs = bc.vectors(6, 257, 1)
    for variant in bc.CG_VARIANTS:
        st, res = fa.blas1_op("cg_update", 257, vecs, scal=(0.83, 1.9, 0.7, -2.5), variant=variant, partials=np.ones(300) if variant & 1 else None)
        assert st == T.ERROR_MISC and all(bc.same_bytes(g, v) for g, v in zip(res["vec"], vecs)) and res["grid"] == 0
    st, res = fa.blas1_op("finalize", 257, (), ipar=(2, 2), partials=np.ones(514))
    assert st == T.ERROR_MISC and res["grid"] == 0 and len(res["red"]) == 0
    st, res = fa.blas1_op("pack", 3, [np.ones(5), np.zeros(3)], ipar=(5,), idx=np.array([4, 0, 4]))
    assert st == T.ERROR_MISC and np.all(res["vec"][1] == 0.0)


# ---------------------------------------------------------------------------
# the emulation of k_finalize's order
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("count", bc.FOLD_COUNTS + (2, 65, 512, 513))
def test_fold_sum_is_exact_where_every_order_is(count):
    p = bc.integers(count)
    assert bc.fold_sum(p) == float(sum(int(v) for v in p)) == bc.left_to_right(p)
    one = np.zeros(count); one[count // 2] = 1e-40
    assert bc.fold_sum(one) == 1e-40
    assert bc.fold_max(-np.abs(p) - 1.0) == 0.0 and bc.fold_max(np.full(count, np.nan)) == 0.0
    q = p.copy(); q[0] = np.nan
    assert bc.fold_max(q) == max(0.0, q[1:].max()) if count > 1 else bc.fold_max(q) == 0.0
    assert np.isnan(bc.fold_sum(q))


def test_fold_sum_has_the_documented_shape():
    """Thread i owns i, i + 256, ...; lanes 0 .. 63 of a wavefront fold by halves; the wavefronts are added in order.  With 1.0 in one place
    and 2^-53 elsewhere the result tells where the small terms met the large one."""
    u = 2.0 ** -53
    p = np.full(512, u); p[0] = 1.0            # thread 0: (0 + 1) + u -> 1 (ties to even); the other 510 meet first and are large enough to count
    assert bc.fold_sum(p) == 1.0 + 510 * u
    p = np.full(256, u); p[255] = 1.0          # the last lane of the last wavefront: everything else is summed before it is met
    assert bc.fold_sum(p) == 1.0 + 254 * u     # (its neighbour's u is lost to the tie, every later arrival is a multiple of 2 u)
    tree = np.zeros(256); tree[[0, 32]] = [1.0, u]; tree[[16, 48]] = [u, u]   # off = 32: 1 + u -> 1, then (u + u) arrives whole at off = 16
    assert bc.fold_sum(tree) == 1.0 + 2 * u
    waves = np.zeros(256); waves[[0, 64, 128, 192]] = [1.0, u, u, u]   # ((1 + u) + u) + u: each u is lost on its own
    assert bc.fold_sum(waves) == 1.0
    assert bc.left_to_right(waves[::-1]) == 1.0 + 4 * u   # 3 u + 1: a tie, to the even neighbour


def test_the_folded_inputs_tell_orders_apart():
    """On the mixed-magnitude partials of the device test the documented order differs from numpy's pairwise sum and from the left-to-right
    sum for at least one count: a kernel that folded in another order would be seen."""
    differs_np, differs_lr = [], []
    for count in bc.FOLD_COUNTS:
        p = bc.mixed(count)
        assert np.all(np.abs(p) >= 1e-8) and np.all(np.abs(p) <= 1e8)
        assert count < 63 or ((p > 0).any() and (p < 0).any())
        f = bc.fold_sum(p)
        if f != np.sum(p):
            differs_np.append(count)
        if f != bc.left_to_right(p):
            differs_lr.append(count)
        ex = p.astype(np.longdouble)
        assert sum_bound_ratio(np.array([f]), np.array([ex.sum()]), np.array([np.abs(ex).sum()]), np.array([max(count - 1, 0)])) <= 1.0
    print("fold_sum differs from np.sum at", differs_np, "and from the left-to-right sum at", differs_lr)
    assert differs_np and differs_lr
    assert bc.fold_sum(bc.mixed(1)) == bc.mixed(1)[0]


# ---------------------------------------------------------------------------
# the references alone, against the bound the device is held to
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", bc.SMALL + (bc.LARGE_SCALAR, bc.LARGE_PAIR))
@pytest.mark.parametrize("name,pairs", bc.REDUCERS)
def test_plain_double_sums_of_the_references_stay_within_the_bound(name, pairs, n):
    """The left-to-right double sum of the rounded products, over the whole vector and over every block of the launch, against the
    np.longdouble sum of the exact products: ratio <= 1, and above 0 wherever there is something to round -- the bound is neither
    unreachable nor vacuous."""
    a, b = bc.reducer_terms(name, n)
    ld = np.longdouble
    terms = a.astype(ld) * b.astype(ld)
    total = bc.left_to_right(a * b)
    ratio = sum_bound_ratio(np.array([total]), np.array([terms.sum()]), np.array([np.abs(terms).sum()]), np.array([n]))
    assert ratio <= 1.0, (name, n, ratio)
    G = bc.vec_grid(n)
    ex, sabs, m = bc.block_sums(terms, G, pairs)
    assert m.sum() == n and abs(ex.sum() - terms.sum()) <= 2.0 ** -60 * np.abs(terms).sum()
    rows, tail = bc._by_block(a * b, G, pairs, 0.0)
    got = np.add.accumulate(rows, axis=1)[:, -1]
    if len(tail):
        got[0] += tail[0]
    r2 = sum_bound_ratio(got, ex, sabs, m)
    assert r2 <= 1.0, (name, n, r2)
    if n >= 255 and name != "norm1_nan":
        assert ratio > 0.0 and r2 > 0.0
    print(f"{name} n = {n}: left-to-right sum at {ratio:.3e} of the bound, per block {r2:.3e}")


def test_block_layout_of_a_launch():
    """Entry i belongs to block (i / 256) % G; a pair walk deals pairs, and its odd last entry goes to block 0."""
    n, G = 2 * 3 * 256 + 5, 3
    t = np.arange(n, dtype=np.float64)
    s, _, m = bc.block_sums(t, G)
    for b in range(G):
        mine = t[(np.arange(n) // 256) % G == b]
        assert s[b] == mine.sum() and m[b] == len(mine)
    s, _, m = bc.block_sums(t, G, pairs=True)
    blk = ((np.arange(n) // 2) // 256) % G
    blk[-1] = 0
    for b in range(G):
        assert s[b] == t[blk == b].sum() and m[b] == (blk == b).sum()
    x = t.copy(); x[[0, 300, n - 1]] = np.nan
    assert np.array_equal(bc.block_nan_count(x, G), [np.isnan(x[(np.arange(n) // 256) % G == b]).sum() for b in range(G)])
    assert np.array_equal(bc.block_max(-x, G), [np.nanmax(x[(np.arange(n) // 256) % G == b]) for b in range(G)])
    assert bc.block_max(np.full(4, np.nan), 1)[0] == 0.0


def test_elementwise_references_on_the_guard_and_signed_zeros():
    d = bc.GUARD_DIAGS
    b = np.full(len(d), 0.5)
    dead = np.array([True, True, True, True, False, False, False, False, True])
    for w in bc.OMEGAS:
        z = bc.jacobi_zero_ref(w, b, d)
        assert np.all(bc.bits(z[dead]) == 0) and np.all(z[~dead] == w * 0.5 / d[~dead])
    assert np.all(bc.bits(bc.l1_zero_ref(b, d)[dead]) == 0) and bc.same_bytes(bc.diag_precond_ref(d, b)[dead], b[dead])
    # w = 1.5: (1 - w) * 0.0 is -0.0, and -0.0 + -0.0 keeps its sign; w = 0.7 gives +0.0
    assert np.signbit(bc.jacobi_zero_ref(1.5, np.array([0.0]), np.array([-3.0]))[0]) and not np.signbit(bc.jacobi_zero_ref(0.7, np.array([0.0]), np.array([-3.0]))[0])
    p, t, u, r, zx, zd = bc.vectors(6, 9, 1)
    for tp in (0.0, -0.0, 1e-40, -1e-40, np.nan):
        uo, ro, zo, upd = bc.cg_update_ref(0.83, tp, p, t, u, r, zx, zd, 0.7, 8, 0.0)
        assert not upd and bc.same_bytes(uo, u) and bc.same_bytes(ro, r) and bc.same_bytes(zo, zx)
    uo, ro, zo, upd = bc.cg_update_ref(0.83, np.nextafter(1e-40, 1.0), p, t, u, r, zx, zd, 0.7, 16, 2.0)
    assert upd and np.all(zo == 0.7 * ro / 2.0) and np.all(np.isfinite(uo))
    assert len(bc.CG_VARIANTS) == 24 and len(set(bc.CG_VARIANTS)) == 24
