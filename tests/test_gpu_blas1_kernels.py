"""The small kernels between the matrix products -- the BLAS-1 part of csrc/kernels.hip.h and k_pack of csrc/hierarchy.hip.h -- one launch at a
time through fasp_hip_blas1_op, with the grid rule and the context buffers of their production call sites, against numpy references written
here and in tests/_blas1_cases.py (no oracle library, no code of the library under test).

Elementwise outputs are BIT-EQUAL to the kernel's expression evaluated in double in the order the kernel writes it (the library is built with
-ffp-contract=off): NaN positions first, then the bits of the rest as int64, so a wrong signed zero shows.  A vector a variant must not touch
has every byte of its input.  Each per-block partial sum and each finalised sum is held to _libs.sum_bound_ratio <= 1 against the np.longdouble
sum of its terms (products of two stored doubles, formed from the device's own output vectors where the sum is over outputs), with m = the number
of terms: the one rounding of each product and the m - 1 of any order of summation are inside the bound's (m + 1) u.  Maxima and NaN counts are
exact.  A scalar a kernel sums from partials itself is bit-equal to k_finalize's sum of the same partials and to the numpy emulation of the
documented order (_blas1_cases.fold_sum).  Every call is made twice and must repeat itself bit for bit.

  kernel                      variants                                                          sizes
  k_cg_update                 {(t,p) reduced, folded} x {temp1 host, device} x {1, 5 norms}     1, 2, 3, 255, 256, 257, 511, 513, 1331: all 24;
                              x {no zx, zx / zdiag array, zx / zdiag_value}                     524 289: variant 0 and folded + device + 5 norms + zdiag
                              breakdown (+-0.0, +-1e-40, the next double), guards, NaN in u     257, 1331
  k_axpby_beta                npart = 0, > 0                                                    the small sizes; 1 048 579
  k_mgs_step                  {h_ptr, folded} x {pnext, none}; h = 0, h = 1 with pj = pi        the small sizes; 524 289
  fold = finalize             the three above, 1, 63, 64, 255, 256, 257, 1000, 2048 partials    513
  k_finalize                  nq 1, 5, 8 (and 2, 3, 4, 6, 7 at G = 257) x masks 0, 8, 0xaa      G = 1, 255, 256, 257, 2048
  k_dot, k_norms, k_norm1_nan plain, NaN at 0, n / 2, n - 1; k_norms with an Inf               the small sizes; 1 048 579 (k_dot), 524 289
  k_axpy, k_axpby             --                                                                the small sizes; 1 048 579
  k_axpyz                     z apart, z = x, z = y                                             the small sizes; 524 289
  k_axpy_self, k_scale, k_set, k_poly_scale, k_poly_start, k_poly_step                          the small sizes; 524 289
  k_jacobi_zero, k_l1_zero, k_diag_precond   w = 1, 0.7, 1.5; diagonals around the 1e-20 guard  the small sizes; 524 289; 300 (guards)
  k_bsr_dinv_apply            nb = 1, 2, 3, 4, 5, 7, 8                                          1, 64 / nb + 1, 300 block rows
  k_pack                      repeated, descending indices with 0 and the last entry            nsend = 1, 257, 1331

The largest error / bound per reducing kernel is printed by every test that measures one; it is a measurement against the a-priori bound
(<= 1), not a tuned tolerance.  Measured on an MI355X, the largest over all cases of the file: k_cg_update 0.447, k_mgs_step 0.382, k_norms 0.377,
k_dot 0.299, k_norm1_nan 0.241, k_finalize 0.0042 (its mixed-magnitude inputs: the bound follows the largest partial)."""
import numpy as np
import pytest

import _blas1_cases as bc
from _libs import sum_bound_ratio

pytestmark = pytest.mark.gpu

_worst = {}   # kernel -> largest error / bound so far (printed, never asserted beyond <= 1)


def run(gpu, kernel, n, vectors=(), **kw):
    """The call, twice: both must succeed and agree in every bit they return."""
    st, a = gpu.blas1_op(kernel, n, vectors, **kw)
    st2, b = gpu.blas1_op(kernel, n, vectors, **kw)
    assert st == 0 and st2 == 0, (kernel, n, kw.get("variant", 0), st, st2)
    assert a["grid"] == b["grid"] and len(a["vec"]) == len(b["vec"])
    for k, (va, vb) in enumerate(zip(a["vec"], b["vec"])):
        assert bc.same_bytes(va, vb), (kernel, n, "slot", k, "differs between two calls")
    assert bc.same_bytes(a["red"], b["red"]) and bc.same_bytes(a["partials"], b["partials"]) and bc.same_bytes([a["pub"]], [b["pub"]]), (kernel, n)
    return a


def assert_bits(label, got, want):
    bad = bc.bit_mismatches(got, want)
    assert len(bad) == 0, (label, len(bad), bad[:8], np.asarray(got)[bad[:8]], np.asarray(want)[bad[:8]])


def note(kernel, ratio):
    _worst[kernel] = max(_worst.get(kernel, 0.0), ratio)
    print(f"{kernel}: error / bound {ratio:.3e} (largest of {kernel} so far {_worst[kernel]:.3e})")


def check_sum(label, kernel, a, b, G, pairs, partials, red):
    """The per-block partials and the finalised sum of the terms a_i * b_i: NaN where the exact sum is NaN, equal where it is infinite,
    within the a-priori bound elsewhere; the finalised value is also k_finalize's order over the partials the kernel left."""
    ld = np.longdouble
    with np.errstate(all="ignore"):
        terms = np.asarray(a).astype(ld) * np.asarray(b).astype(ld)
        ex, sabs, m = bc.block_sums(terms, G, pairs)
        tot, tabs = terms.sum(), np.abs(terms).sum()
    assert partials.shape == (G,), (label, partials.shape, G)
    assert np.array_equal(np.isnan(partials), np.isnan(ex)), (label, "NaN blocks", np.flatnonzero(np.isnan(partials) != np.isnan(ex))[:8])
    inf = np.isinf(ex)
    assert np.array_equal(partials[inf].astype(ld), ex[inf]), (label, "infinite blocks")
    fin = np.isfinite(ex)
    ratio = sum_bound_ratio(partials[fin], ex[fin], sabs[fin], m[fin]) if fin.any() else 0.0
    assert ratio <= 1.0, (label, "partials", ratio)
    if np.isnan(tot):
        assert np.isnan(red), (label, red)
    elif np.isinf(tot):
        assert red == float(tot), (label, red)
    else:
        r2 = sum_bound_ratio(np.array([red]), np.array([tot]), np.array([tabs]), np.array([len(terms)]))
        assert r2 <= 1.0, (label, "finalised", red, float(tot), r2)
        ratio = max(ratio, r2)
    assert_bits((label, "k_finalize's order over the partials"), [red], [bc.fold_sum(partials)])
    note(kernel, ratio)


def check_max(label, x, G, partials, red):
    want = bc.block_max(x, G)
    assert_bits((label, "max partials"), partials, want)
    assert_bits((label, "max"), [red], [bc.fold_max(np.abs(x))])


def check_nan_count(label, x, G, partials, red):
    assert_bits((label, "NaN partials"), partials, bc.block_nan_count(x, G))
    assert red == float(np.isnan(x).sum()), (label, red)


# ---------------------------------------------------------------------------
# k_cg_update
# ---------------------------------------------------------------------------
TEMP1, ZOMEGA, ZVALUE = 0.83, 0.7, -2.5


def cg_case(gpu, n, variant, tp=None, tp_partials=None, vecs=None, zomega=ZOMEGA, zvalue=ZVALUE, temp1=TEMP1):
    """One k_cg_update launch checked in full -> (result, updated).  Folded variants take tp_partials, the others tp."""
    folded, full, zmode = variant & 1, variant & 4, variant & 24
    p, t, u, r, zx, zd = vecs if vecs is not None else bc.vectors(6, n, 1)
    if folded:
        tp = bc.fold_sum(tp_partials)
    res = run(gpu, "cg_update", n, [p, t, u, r, zx, zd], scal=(temp1, 0.0 if folded else tp, zomega, zvalue), variant=variant,
              partials=tp_partials if folded else None)
    label = ("cg_update", n, variant, tp)
    G = bc.vec_grid(n)
    assert res["grid"] == G
    assert_bits((label, "published (t,p)"), [res["pub"]], [tp])
    uo, ro, zo, updated = bc.cg_update_ref(temp1, tp, p, t, u, r, zx, zd, zomega, zmode, zvalue)
    gp, gt, gu, gr, gz, gd = res["vec"]
    assert bc.same_bytes(gp, p) and bc.same_bytes(gt, t) and bc.same_bytes(gd, zd), (label, "an input changed")
    if not updated:
        assert bc.same_bytes(gu, u) and bc.same_bytes(gr, r) and bc.same_bytes(gz, zx), (label, "breakdown: a vector changed")
        assert res["partials"].shape == (5 if full else 1, G) and np.all(bc.bits(res["partials"]) == 0) and np.all(bc.bits(res["red"]) == 0), label
        return res, updated
    assert_bits((label, "u"), gu, uo)
    assert_bits((label, "r"), gr, ro)
    if zmode:
        assert_bits((label, "zx"), gz, zo)
    else:
        assert bc.same_bytes(gz, zx), (label, "zx written without being asked for")
    assert res["partials"].shape == (5 if full else 1, G)
    check_sum((label, "r.r"), "k_cg_update", gr, gr, G, False, res["partials"][0], res["red"][0])
    if full:
        check_sum((label, "u.u"), "k_cg_update", gu, gu, G, False, res["partials"][1], res["red"][1])
        check_sum((label, "p.p"), "k_cg_update", p, p, G, False, res["partials"][2], res["red"][2])
        check_max((label, "max|u|"), gu, G, res["partials"][3], res["red"][3])
        check_nan_count((label, "#NaN(u)"), gu, G, res["partials"][4], res["red"][4])
    return res, updated


def cg_partials(n, variant):
    return bc.rand(bc.rng(n, variant, 2), 300) if variant & 1 else None


@pytest.mark.parametrize("variant", bc.CG_VARIANTS)
@pytest.mark.parametrize("n", bc.SMALL)
def test_cg_update_every_variant(gpu, n, variant):
    _, updated = cg_case(gpu, n, variant, tp=1.9, tp_partials=cg_partials(n, variant))
    assert updated


@pytest.mark.parametrize("variant", (0, 1 | 2 | 4 | 8))
def test_cg_update_second_grid_stride_trip(gpu, variant):
    n = bc.LARGE_SCALAR
    _, updated = cg_case(gpu, n, variant, tp=-0.77, tp_partials=bc.mixed(bc.MAXGRID, 5) if variant & 1 else None)
    assert updated


def test_cg_update_folded_equals_reduced_in_every_vector(gpu):
    """The same inputs through the folded and the unfolded variant: the same bits in u, r, zx and every partial."""
    n = 1331
    vecs = bc.vectors(6, n, 1)
    for count in bc.FOLD_COUNTS:
        part = bc.mixed(count)
        a, _ = cg_case(gpu, n, 1 | 4 | 8, tp_partials=part, vecs=vecs)
        b, _ = cg_case(gpu, n, 4 | 8, tp=bc.fold_sum(part), vecs=vecs)
        for k in (2, 3, 4):
            assert bc.same_bytes(a["vec"][k], b["vec"][k]), (count, k)
        assert bc.same_bytes(a["partials"], b["partials"]) and bc.same_bytes(a["red"], b["red"]), count


BREAKDOWN = (0.0, -0.0, 1e-40, -1e-40)


@pytest.mark.parametrize("variant", (0, 1, 4 | 8, 1 | 2 | 4 | 8, 16, 1 | 4 | 16))
@pytest.mark.parametrize("n", (257, 1331))
def test_cg_update_breakdown_leaves_everything(gpu, n, variant):
    """|(t,p)| <= 1e-40: u, r and zx keep every byte, all partials are 0.0, the host sees (t,p) itself; the next double above 1e-40 updates.
    Folded: the partial array holds that single nonzero entry, so its sum is exact in any order."""
    for tp in BREAKDOWN + (np.nextafter(1e-40, 1.0), -np.nextafter(1e-40, 1.0)):
        part = None
        if variant & 1:
            part = np.zeros(257); part[100] = tp
        res, updated = cg_case(gpu, n, variant, tp=tp, tp_partials=part)
        assert updated == (abs(tp) > 1e-40), (tp, updated)
        assert res["pub"] == tp, (tp, res["pub"])   # (a folded -0.0 is summed onto 0.0: numerically the value, the bits of the emulation)


@pytest.mark.parametrize("variant", (8, 1 | 2 | 4 | 8))
@pytest.mark.parametrize("omega", bc.OMEGAS)
def test_cg_update_zx_diagonal_guard(gpu, omega, variant):
    """zx next to diagonal entries on both sides of |d| > 1e-20, zero, negative, huge and NaN."""
    n = 300
    vecs = bc.vectors(6, n, 4)
    vecs[5][:len(bc.GUARD_DIAGS)] = bc.GUARD_DIAGS
    vecs[5][-len(bc.GUARD_DIAGS):] = bc.GUARD_DIAGS[::-1]
    res, updated = cg_case(gpu, n, variant, tp=1.9, tp_partials=cg_partials(n, variant), vecs=vecs, zomega=omega)
    assert updated
    dead = ~(np.abs(vecs[5]) > 1e-20)
    assert dead.sum() == 10 and np.all(bc.bits(res["vec"][4][dead]) == 0)


@pytest.mark.parametrize("variant", (16, 1 | 2 | 4 | 16))
@pytest.mark.parametrize("zvalue", (1e-20, np.nextafter(1e-20, 1.0), -1e-20, -np.nextafter(1e-20, 1.0)))
def test_cg_update_uniform_diagonal_on_each_side_of_the_guard(gpu, zvalue, variant):
    n = 513
    vecs = bc.vectors(6, n, 5)   # (the zdiag array is passed but must not be read: its values differ from zvalue)
    res, updated = cg_case(gpu, n, variant, tp=1.9, tp_partials=cg_partials(n, variant), vecs=vecs, zvalue=zvalue, zomega=1.5)
    assert updated
    if abs(zvalue) > 1e-20:
        assert np.all(res["vec"][4] == 1.5 * res["vec"][3] / zvalue)
    else:
        assert np.all(bc.bits(res["vec"][4]) == 0)


@pytest.mark.parametrize("n", bc.SMALL)
def test_cg_update_nan_in_u(gpu, n):
    """NaN in u at 0, n / 2, n - 1: the count is exact, the maximum skips them, u.u is NaN, r.r is not."""
    vecs = bc.vectors(6, n, 6)
    vecs[2][[0, n // 2, n - 1]] = np.nan
    res, _ = cg_case(gpu, n, 4, tp=1.9, vecs=vecs)
    assert res["red"][4] == len({0, n // 2, n - 1}) and np.isnan(res["red"][1]) and np.isfinite(res["red"][0])
    rest = np.delete(res["vec"][2], [0, n // 2, n - 1])
    assert res["red"][3] == (np.abs(rest).max() if len(rest) else 0.0)


# ---------------------------------------------------------------------------
# k_axpby_beta, k_mgs_step
# ---------------------------------------------------------------------------
def axpby_beta_case(gpu, n, partials=None, num=0.61, den=-1.7, vecs=None):
    x, y = vecs if vecs is not None else bc.vectors(2, n, 2)
    if partials is not None:
        num = bc.fold_sum(partials)
    res = run(gpu, "axpby_beta", n, [x, y], scal=(0.0 if partials is not None else num, den), variant=int(partials is not None), partials=partials)
    label = ("axpby_beta", n, None if partials is None else len(partials))
    assert res["grid"] == bc.vec_grid(n // 2 + 1) and res["partials"].size == 0
    assert_bits((label, "published numerator"), [res["pub"]], [num])
    assert bc.same_bytes(res["vec"][0], x)
    assert_bits((label, "y"), res["vec"][1], bc.axpby_beta_ref(num, den, x, y))
    return res


@pytest.mark.parametrize("folded", (0, 1))
@pytest.mark.parametrize("n", bc.SMALL + (bc.LARGE_PAIR,))
def test_axpby_beta(gpu, n, folded):
    axpby_beta_case(gpu, n, bc.rand(bc.rng(n, 8), bc.vec_grid(n)) if folded else None)


def mgs_case(gpu, n, variant, partials=None, h=0.61, vecs=None):
    pj, pi, pnext = vecs if vecs is not None else bc.vectors(3, n, 3)
    if variant & 1:
        h = bc.fold_sum(partials)
    res = run(gpu, "mgs_step", n, [pj, pi, pnext], scal=(0.0 if variant & 1 else h,), variant=variant, partials=partials if variant & 1 else None)
    label = ("mgs_step", n, variant, h)
    G = bc.vec_grid(n)
    assert res["grid"] == G and res["partials"].shape == (1, G)
    assert_bits((label, "published h"), [res["pub"]], [h])
    assert bc.same_bytes(res["vec"][0], pj) and bc.same_bytes(res["vec"][2], pnext)
    assert_bits((label, "pi"), res["vec"][1], bc.mgs_step_ref(h, pj, pi))
    v = res["vec"][1]
    check_sum(label, "k_mgs_step", pnext if variant & 2 else v, v, G, False, res["partials"][0], res["red"][0])
    return res


@pytest.mark.parametrize("variant", (0, 1, 2, 3))
@pytest.mark.parametrize("n", bc.SMALL)
def test_mgs_step_every_variant(gpu, n, variant):
    mgs_case(gpu, n, variant, bc.rand(bc.rng(n, 9), bc.vec_grid(n)))


@pytest.mark.parametrize("variant", (2, 1))
def test_mgs_step_second_grid_stride_trip(gpu, variant):
    mgs_case(gpu, bc.LARGE_SCALAR, variant, bc.mixed(bc.MAXGRID, 6))


@pytest.mark.parametrize("variant", (0, 1, 2, 3))
def test_mgs_step_with_h_zero_and_with_equal_vectors(gpu, variant):
    """h = 0.0: p_i keeps its value (numpy's p_i + (-0.0) * p_j, signed zeros as they fall); h = 1 on p_j = p_i: exact zeros, and a zero sum."""
    n = 513
    pj, pi, pnext = bc.vectors(3, n, 3)
    pi[:4] = [0.0, -0.0, 0.0, -0.0]; pj[:4] = [1.0, 1.0, -1.0, -1.0]
    zero = np.zeros(3); one = np.zeros(3); one[1] = 1.0
    res = mgs_case(gpu, n, variant, zero, h=0.0, vecs=[pj, pi, pnext])
    assert np.array_equal(res["vec"][1], pi)
    res = mgs_case(gpu, n, variant, one, h=1.0, vecs=[pi.copy(), pi, pnext])
    assert np.all(res["vec"][1] == 0.0) and res["red"][0] == 0.0 and np.all(res["partials"] == 0.0)


# ---------------------------------------------------------------------------
# a kernel's own sum of partials is k_finalize's
# ---------------------------------------------------------------------------
def finalize(gpu, partials, nq=1, maxmask=0):
    partials = np.asarray(partials, dtype=np.float64).reshape(nq, -1)
    res = run(gpu, "finalize", partials.shape[1], (), ipar=(nq, maxmask), partials=partials)
    assert res["grid"] == partials.shape[1] and bc.same_bytes(res["partials"], partials)
    return res["red"]


@pytest.mark.parametrize("count", bc.FOLD_COUNTS)
@pytest.mark.parametrize("kernel", ("cg_update", "axpby_beta", "mgs_step"))
def test_fold_equals_finalize(gpu, kernel, count):
    """The scalar the kernel sums for itself has the bits of k_finalize over the same partials and of the emulated order, and the vectors are
    those of the unfolded variant fed with k_finalize's value.  The partials' sum depends on the order (test_blas1_host.py shows it does)."""
    n = 513
    part = bc.mixed(count)
    fin = finalize(gpu, part)[0]
    assert_bits((kernel, count, "k_finalize against its documented order"), [fin], [bc.fold_sum(part)])
    if kernel == "cg_update":
        a, _ = cg_case(gpu, n, 1 | 8, tp_partials=part)
        b, _ = cg_case(gpu, n, 8, tp=fin)
        slots = (2, 3, 4)
    elif kernel == "axpby_beta":
        a = axpby_beta_case(gpu, n, part)
        b = axpby_beta_case(gpu, n, None, num=fin)
        slots = (1,)
    else:
        a = mgs_case(gpu, n, 1 | 2, part)
        b = mgs_case(gpu, n, 2, h=fin)
        slots = (1,)
    assert_bits((kernel, count, "published scalar against k_finalize"), [a["pub"]], [fin])
    for k in slots:
        assert bc.same_bytes(a["vec"][k], b["vec"][k]), (kernel, count, "slot", k)
    assert bc.same_bytes(a["partials"], b["partials"]) and bc.same_bytes(a["red"], b["red"]), (kernel, count)


# ---------------------------------------------------------------------------
# k_finalize
# ---------------------------------------------------------------------------
FINALIZE_CASES = [(G, nq) for G in (1, 255, 256, 257, 2048) for nq in (1, 5, 8)] + [(257, nq) for nq in (2, 3, 4, 6, 7)]


@pytest.mark.parametrize("maxmask", (0, 0b01000, 0b10101010))
@pytest.mark.parametrize("G,nq", FINALIZE_CASES)
def test_finalize(gpu, G, nq, maxmask):
    """Sums in the documented order (and within the bound); maxima skip NaN and start from 0.0: a quantity of negative and NaN partials gives 0.0."""
    part = np.stack([bc.mixed(G, 10 + q) for q in range(nq)])
    for q in range(nq):
        if (maxmask >> q) & 1:
            part[q, 0] = np.nan; part[q, G // 2] = np.nan; part[q, G - 1] = -abs(part[q, G - 1])
            if q == 1:
                part[q] = -np.abs(part[q])   # NaN stay NaN: nothing here is above 0.0
    red = finalize(gpu, part, nq, maxmask)
    assert len(red) == nq
    worst = 0.0
    for q in range(nq):
        if (maxmask >> q) & 1:
            assert_bits(("finalize", G, nq, maxmask, q, "max"), [red[q]], [bc.fold_max(part[q])])
            if q == 1 or G <= 2:
                assert bc.bits([red[q]])[0] == 0
        else:
            assert_bits(("finalize", G, nq, maxmask, q, "sum"), [red[q]], [bc.fold_sum(part[q])])
            ex = part[q].astype(np.longdouble)
            worst = max(worst, sum_bound_ratio(np.array([red[q]]), np.array([ex.sum()]), np.array([np.abs(ex).sum()]), np.array([G - 1])))
    assert worst <= 1.0
    note("k_finalize", worst)


# ---------------------------------------------------------------------------
# k_dot, k_norms, k_norm1_nan
# ---------------------------------------------------------------------------
def poison(x, mode):
    n = len(x)
    if mode == "nan":
        x[[0, n // 2, n - 1]] = np.nan
    elif mode == "inf":
        x[n // 2] = -np.inf
    return x


@pytest.mark.parametrize("mode", ("plain", "nan"))
@pytest.mark.parametrize("n", bc.SMALL + (bc.LARGE_PAIR,))
def test_dot(gpu, n, mode):
    x, y = bc.vectors(2, n, 21)
    poison(x, mode)
    res = run(gpu, "dot", n, [x, y])
    G = bc.vec_grid(n)
    assert res["grid"] == G and bc.same_bytes(res["vec"][0], x) and bc.same_bytes(res["vec"][1], y)
    check_sum(("dot", n, mode), "k_dot", x, y, G, True, res["partials"][0], res["red"][0])
    assert np.isnan(res["red"][0]) == (mode == "nan")


@pytest.mark.parametrize("mode", ("plain", "nan", "inf"))
@pytest.mark.parametrize("n", bc.SMALL + (bc.LARGE_SCALAR,))
def test_norms(gpu, n, mode):
    x, = bc.vectors(1, n, 22)
    poison(x, mode)
    res = run(gpu, "norms", n, [x])
    G = bc.vec_grid(n)
    assert res["grid"] == G and res["partials"].shape == (2, G)
    check_sum(("norms", n, mode), "k_norms", x, x, G, False, res["partials"][0], res["red"][0])
    check_max(("norms", n, mode), x, G, res["partials"][1], res["red"][1])
    if mode == "inf":
        assert res["red"][0] == np.inf and res["red"][1] == np.inf
    if mode == "nan":
        rest = np.delete(x, [0, n // 2, n - 1])
        assert np.isnan(res["red"][0]) and res["red"][1] == (np.abs(rest).max() if len(rest) else 0.0)


@pytest.mark.parametrize("mode", ("plain", "nan"))
@pytest.mark.parametrize("n", bc.SMALL + (bc.LARGE_SCALAR,))
def test_norm1_nan(gpu, n, mode):
    x, = bc.vectors(1, n, 23)
    poison(x, mode)
    res = run(gpu, "norm1_nan", n, [x])
    G = bc.vec_grid(n)
    assert res["grid"] == G and res["partials"].shape == (2, G)
    check_sum(("norm1_nan", n, mode), "k_norm1_nan", np.abs(x), np.ones(n), G, False, res["partials"][0], res["red"][0])
    check_nan_count(("norm1_nan", n, mode), x, G, res["partials"][1], res["red"][1])
    assert res["red"][1] == (len({0, n // 2, n - 1}) if mode == "nan" else 0)


# ---------------------------------------------------------------------------
# the plain elementwise kernels
# ---------------------------------------------------------------------------
ELEMENTWISE_CASES = [(k, v, n) for k, v, pairs in bc.ELEMENTWISE for n in bc.SMALL + ((bc.LARGE_PAIR if pairs else bc.LARGE_SCALAR),)]


@pytest.mark.parametrize("kernel,variant,n", ELEMENTWISE_CASES)
def test_elementwise(gpu, kernel, variant, n):
    vecs, scal, want = bc.elementwise_case(kernel, n, variant)
    res = run(gpu, kernel, n, vecs, scal=scal, variant=variant)
    pairs = dict((k, p) for k, _, p in bc.ELEMENTWISE)[kernel]
    assert res["grid"] == bc.vec_grid(n // 2 + 1 if pairs else n) and res["partials"].size == 0
    for k, (g, w, v) in enumerate(zip(res["vec"], want, vecs)):
        if w is v:
            assert bc.same_bytes(g, v), (kernel, variant, n, "slot", k, "changed")
        else:
            assert_bits((kernel, variant, n, "slot", k), g, w)


def guarded(kernel, w, b, d):
    if kernel == "jacobi_zero":
        return [b, d, np.full(len(b), 9.0)], (w,), bc.jacobi_zero_ref(w, b, d)
    if kernel == "l1_zero":
        return [b, d, np.full(len(b), 9.0)], (), bc.l1_zero_ref(b, d)
    return [d, b, np.full(len(b), 9.0)], (), bc.diag_precond_ref(d, b)


@pytest.mark.parametrize("n", bc.SMALL + (bc.LARGE_SCALAR,))
@pytest.mark.parametrize("kernel", ("jacobi_zero", "l1_zero", "diag_precond"))
def test_zero_start_sweeps_and_diagonal_preconditioner(gpu, kernel, n):
    b, d = bc.vectors(2, n, 16)
    vecs, scal, want = guarded(kernel, 0.7, b, d)
    res = run(gpu, kernel, n, vecs, scal=scal)
    assert res["grid"] == bc.vec_grid(n) and bc.same_bytes(res["vec"][0], vecs[0]) and bc.same_bytes(res["vec"][1], vecs[1])
    assert_bits((kernel, n), res["vec"][2], want)


@pytest.mark.parametrize("w", bc.OMEGAS)
@pytest.mark.parametrize("kernel", ("jacobi_zero", "l1_zero", "diag_precond"))
def test_diagonal_guard(gpu, kernel, w):
    """Diagonal entries 0.0, -0.0, +-1e-20 (not divided by), the next doubles beyond (divided by), 1e300, -3.0 and NaN, first against
    right-hand sides of both signs and zeros, then at both ends of a vector of several blocks."""
    nd = len(bc.GUARD_DIAGS)
    rhs = np.array([0.6, -0.6, 0.0, -0.0])
    d = np.concatenate([np.repeat(bc.GUARD_DIAGS, len(rhs)), bc.rand(bc.rng(17), 300 - nd * len(rhs) - nd), bc.GUARD_DIAGS[::-1]])
    b = bc.rand(bc.rng(18), 300)
    b[:nd * len(rhs)] = np.tile(rhs, nd)
    vecs, scal, want = guarded(kernel, w, b, d)
    res = run(gpu, kernel, 300, vecs, scal=scal)
    assert_bits((kernel, w), res["vec"][2], want)
    dead = ~(np.abs(d) > 1e-20)
    assert dead.sum() == 5 * len(rhs) + 5
    if kernel == "diag_precond":
        assert bc.same_bytes(res["vec"][2][dead], b[dead])
    else:
        assert np.all(bc.bits(res["vec"][2][dead]) == 0)


# ---------------------------------------------------------------------------
# k_bsr_dinv_apply, k_pack
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nb", (1, 2, 3, 4, 5, 7, 8))
def test_bsr_dinv_apply(gpu, nb):
    for rows in (1, 64 // nb + 1, 300):
        n = rows * nb
        g = bc.rng(19, nb, rows)
        dinv, b = bc.rand(g, n * nb), bc.rand(g, n)
        res = run(gpu, "bsr_dinv_apply", n, [dinv, b, np.full(n, 9.0)], ipar=(nb,))
        assert res["grid"] == bc.vec_grid(n) and bc.same_bytes(res["vec"][0], dinv) and bc.same_bytes(res["vec"][1], b)
        assert_bits(("bsr_dinv_apply", nb, rows), res["vec"][2], bc.bsr_dinv_apply_ref(nb, dinv, b))


@pytest.mark.parametrize("nsend", (1, 257, 1331))
def test_pack(gpu, nsend):
    nv = 1000
    v = bc.rand(bc.rng(20), nv)
    v[[0, nv - 1]] = [-0.0, np.nan]
    idx = np.sort(bc.rng(20, nsend).integers(0, nv, nsend))[::-1].copy()   # descending, with repeats once nsend > nv
    idx[0] = nv - 1; idx[-1] = 0
    if nsend > 2:
        idx[1] = nv - 1; idx[-2] = 0
        assert len(np.unique(idx)) < nsend and np.all(np.diff(idx) <= 0)
    res = run(gpu, "pack", nsend, [v, np.full(nsend, 9.0)], ipar=(nv,), idx=idx)
    assert res["grid"] == bc.vec_grid(nsend) and bc.same_bytes(res["vec"][0], v)
    assert bc.same_bytes(res["vec"][1], v[idx])
