"""Inputs, references and the reduction-order emulation for the tests of the small kernels between the matrix products (the BLAS-1 part of
csrc/kernels.hip.h and k_pack of csrc/hierarchy.hip.h, reached through fasp_hip_blas1_op): tests/test_gpu_blas1_kernels.py on the device,
tests/test_blas1_host.py without one.  Everything here is numpy: no oracle library, no code of the library under test.

Elementwise references evaluate the kernel's own expression in double, operation by operation in the order the kernel writes it (the library
is built with -ffp-contract=off, numpy contracts nothing), so the device must return the same bits.  Sums are described by their TERMS
(two double arrays whose products are summed) and laid out over the blocks of the launch by block_sums, in np.longdouble."""
import numpy as np

BLOCK = 256                  # threads of a workgroup (csrc/kernels.hip.h)
MAXGRID = 2048               # the largest grid of a vector kernel, and the width of a partial buffer per quantity
SMALL = (1, 2, 3, 255, 256, 257, 511, 513, 1331)
LARGE_SCALAR = MAXGRID * BLOCK + 1          # a second grid-stride trip of the kernels that walk single entries
LARGE_PAIR = 2 * MAXGRID * BLOCK + 3        # ... of the kernels that walk double2 pairs (and an odd tail)
FOLD_COUNTS = (1, 63, 64, 255, 256, 257, 1000, 2048)
GUARD = 1e-20                # |d| > GUARD: the diagonal entry divides
TINY = 1e-40                 # |(t,p)| > TINY: CG goes on
GUARD_DIAGS = np.array([0.0, -0.0, 1e-20, -1e-20, np.nextafter(1e-20, 1.0), -np.nextafter(1e-20, 1.0), 1e300, -3.0, np.nan])
OMEGAS = (1.0, 0.7, 1.5)

KERNELS = ("cg_update", "axpby_beta", "mgs_step", "finalize", "dot", "norms", "norm1_nan", "axpy", "axpby", "axpyz", "axpy_self",
           "scale", "set", "poly_scale", "poly_start", "poly_step", "jacobi_zero", "l1_zero", "diag_precond", "bsr_dinv_apply", "pack")
# k_cg_update's variants: bit 0 folded (t,p), bit 1 temp1 on the device, bit 2 full norms, bit 3 zx with a diagonal array, bit 4 zx with one value
CG_VARIANTS = tuple(f | t | q | z for f in (0, 1) for t in (0, 2) for q in (0, 4) for z in (0, 8, 16))


def vec_grid(n):
    return max(1, min(MAXGRID, (n + BLOCK - 1) // BLOCK))


def rng(*key):
    return np.random.default_rng([20240917, *[int(k) for k in key]])


def rand(g, n):
    """n doubles in [-1, 1)."""
    return g.random(n) * 2.0 - 1.0


def vectors(count, n, *key):
    g = rng(n, *key)
    return [rand(g, n) for _ in range(count)]


def mixed(count, seed=0):
    """Partials whose sum depends on the order: magnitudes 1e-8 .. 1e8, both signs."""
    g = rng(4711, count, seed)
    return np.where(g.random(count) < 0.5, -1.0, 1.0) * 10.0 ** (g.random(count) * 16.0 - 8.0)


def integers(count, seed=0):
    """Integer-valued partials (|v| < 2^20): every order of summation is exact."""
    return rng(815, count, seed).integers(-(1 << 20), 1 << 20, count).astype(np.float64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def bit_mismatches(got, want):
    """Indices where got and want differ: first in where their NaN sit, then in the bits of the rest (a wrong signed zero shows)."""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    if np.any(gn != wn):
        return np.flatnonzero(gn != wn)
    return np.flatnonzero(~gn & (bits(got) != bits(want)))


def same_bytes(got, want):
    """Untouched: every byte as it was, NaN payloads included."""
    return np.array_equal(bits(got), bits(want))


# ---------------------------------------------------------------------------
# the documented order of k_finalize and of the kernels that sum partials themselves
# ---------------------------------------------------------------------------
def fold_sum(p):
    """k_finalize's sum of the partials p, in double: thread i adds p[i], p[i + 256], ... left to right to 0.0; each wavefront of 64 lanes
    folds v[:off] += v[off:2 * off] for off = 32 .. 1; thread 0 adds the four wavefronts as ((w0 + w1) + w2) + w3."""
    p = np.asarray(p, dtype=np.float64)
    v = np.zeros(BLOCK)
    with np.errstate(all="ignore"):
        for k in range(0, len(p), BLOCK):
            c = p[k:k + BLOCK]
            v[:len(c)] = v[:len(c)] + c
        w = v.reshape(4, 64).copy()
        off = 32
        while off:
            w[:, :off] = w[:, :off] + w[:, off:2 * off]
            off >>= 1
        return np.float64(((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])


def fold_max(p):
    """k_finalize's maximum: fmax from 0.0, so NaN entries are skipped and nothing below 0.0 shows."""
    p = np.asarray(p, dtype=np.float64)
    p = p[~np.isnan(p)]
    return np.float64(max(0.0, p.max())) if len(p) else np.float64(0.0)


def left_to_right(p):
    """The plain double sum p[0] + p[1] + ... in index order."""
    return np.add.accumulate(np.asarray(p, dtype=np.float64))[-1]


# ---------------------------------------------------------------------------
# the block layout of a reducing launch
# ---------------------------------------------------------------------------
def _by_block(a, G, pairs, fill):
    """a (one value per vector entry) as an array (G, entries of that block), padded with `fill`; the odd tail of a pair walk apart."""
    n = len(a)
    width = 2 if pairs else 1
    items = n // width
    body, tail = a[:items * width], a[items * width:]
    stride = G * BLOCK
    trips = max(1, -(-items // stride))
    padded = np.full(trips * stride * width, fill, dtype=a.dtype)
    padded[:len(body)] = body
    return padded.reshape(trips, G, BLOCK * width).transpose(1, 0, 2).reshape(G, -1), tail


def block_sums(terms, G, pairs=False):
    """The np.longdouble sum, the sum of magnitudes and the number of terms each of the G blocks of a grid-stride walk takes: entry i goes
    to block (i / 256) % G -- with pairs, pair i (entries 2 i, 2 i + 1) does, and block 0 takes the odd last entry."""
    terms = np.asarray(terms, dtype=np.longdouble)
    with np.errstate(all="ignore"):
        t, tail = _by_block(terms, G, pairs, 0.0)
        c, _ = _by_block(np.ones(len(terms), dtype=np.int64), G, pairs, 0)
        s, a, m = t.sum(axis=1), np.abs(t).sum(axis=1), c.sum(axis=1)
        if len(tail):
            s[0] += tail[0]; a[0] += abs(tail[0]); m[0] += 1
    return s, a, m


def block_max(a, G):
    """max |a_i| per block of a single-entry walk, as fmax from 0.0 gives it (NaN skipped)."""
    t, _ = _by_block(np.abs(np.asarray(a, dtype=np.float64)), G, False, 0.0)
    return np.fmax(np.fmax.reduce(t, axis=1), 0.0)


def block_nan_count(a, G):
    t, _ = _by_block(np.isnan(a).astype(np.float64), G, False, 0.0)
    return t.sum(axis=1)


# ---------------------------------------------------------------------------
# elementwise references: the kernel's expression, operation by operation
# ---------------------------------------------------------------------------
def jacobi_zero_ref(w, b, d):
    """(1 - w) * 0.0 + w * b / d where |d| > 1e-20, else 0.0 (k_jacobi_zero, and zx of k_cg_update)."""
    with np.errstate(all="ignore"):
        val = (np.float64(1) - np.float64(w)) * np.float64(0.0) + np.float64(w) * b / d
        return np.where(np.abs(d) > GUARD, val, 0.0)


def l1_zero_ref(b, d):
    with np.errstate(all="ignore"):
        return np.where(np.abs(d) > GUARD, np.float64(0.0) + b / d, 0.0)


def diag_precond_ref(d, r):
    with np.errstate(all="ignore"):
        return np.where(np.abs(d) > GUARD, r / d, r)


def cg_update_ref(temp1, tp, p, t, u, r, zx, zdiag, zomega, zmode, zvalue):
    """-> (u, r, zx, updated): alpha = temp1 / (t,p); u + alpha * p; r + (-alpha) * t; zx from the NEW r (zmode 8: zdiag, 16: zvalue in every
    row, 0: untouched).  |(t,p)| <= 1e-40 (or NaN): nothing is updated."""
    if not abs(tp) > TINY:
        return u.copy(), r.copy(), zx.copy(), False
    with np.errstate(all="ignore"):
        alpha = np.float64(temp1) / np.float64(tp)
        uo = u + alpha * p
        ro = r + (-alpha) * t
    zo = zx.copy()
    if zmode:
        zo = jacobi_zero_ref(zomega, ro, zdiag if zmode == 8 else np.full(len(r), zvalue))
    return uo, ro, zo, True


def axpby_beta_ref(num, den, x, y):
    with np.errstate(all="ignore"):
        b = np.float64(num) / np.float64(den)
        return np.float64(1.0) * x + b * y


def mgs_step_ref(h, pj, pi):
    with np.errstate(all="ignore"):
        return pi + (-np.float64(h)) * pj


def bsr_dinv_apply_ref(nb, dinv, b):
    """Row r of block row br: D[0] * b[0] + D[1] * b[1] + ... left to right."""
    D = dinv.reshape(-1, nb, nb)
    B = b.reshape(-1, nb)
    s = D[:, :, 0] * B[:, 0:1]
    for c in range(1, nb):
        s = s + D[:, :, c] * B[:, c:c + 1]
    return s.reshape(-1)


def elementwise_case(kernel, n, variant=0):
    """Inputs of one of the plain elementwise kernels and what it must leave in every slot -> (vectors, scal, expected vectors)."""
    a, b = 0.37, -1.29
    if kernel == "axpy":
        x, y = vectors(2, n, 7)
        return [x, y], (a,), [x, y + a * x]
    if kernel == "axpby":
        x, y = vectors(2, n, 8)
        return [x, y], (a, b), [x, a * x + b * y]
    if kernel == "axpyz":
        x, y, z = vectors(3, n, 9)
        out = a * x + y
        return [x, y, z], (a,), [out if variant == 1 else x, out if variant == 2 else y, z if variant else out]
    if kernel == "axpy_self":
        y, = vectors(1, n, 10)
        return [y], (a,), [y + a * y]
    if kernel == "scale":
        x, = vectors(1, n, 11)
        return [x], (b,), [x * b]
    if kernel == "set":
        x, = vectors(1, n, 12)
        return [x], (-0.0,), [np.full(n, -0.0)]
    if kernel == "poly_scale":
        dinv, r, rbar = vectors(3, n, 13)
        return [dinv, r, rbar], (), [dinv, r, dinv * r]
    if kernel == "poly_start":
        dinv, rbar, v0, v1 = vectors(4, n, 14)
        k1, k2, k3 = 0.91, -1.7, 0.43
        w = dinv * v1
        return [dinv, rbar, v0, v1], (k1, k2, k3), [dinv, rbar, k1 * rbar, k2 * rbar - k3 * w]
    if kernel == "poly_step":
        dinv, r, rbar, v0, v1, vnew = vectors(6, n, 15)
        k4, k5 = 0.77, -0.31
        rb = (r - rbar) * dinv
        nw = v1 + k5 * (v1 - v0) + k4 * rb
        return [dinv, r, rbar, v0, v1, vnew], (k4, k5), [dinv, r, rb, v1, nw, nw]
    raise KeyError(kernel)


ELEMENTWISE = (("axpy", 0, True), ("axpby", 0, True), ("axpyz", 0, False), ("axpyz", 1, False), ("axpyz", 2, False), ("axpy_self", 0, False),
               ("scale", 0, False), ("set", 0, False), ("poly_scale", 0, False), ("poly_start", 0, False), ("poly_step", 0, False))   # (kernel, variant, walks pairs)


# ---------------------------------------------------------------------------
# the sums: (name, pairs) -> the two factors of every term on random inputs (the host test sums them left to right)
# ---------------------------------------------------------------------------
def reducer_terms(name, n):
    if name == "dot":
        x, y = vectors(2, n, 21)
        return x, y
    if name == "norms":
        x, = vectors(1, n, 22)
        return x, x
    if name == "norm1_nan":
        x, = vectors(1, n, 23)
        return np.abs(x), np.ones(n)
    if name == "mgs_step":
        pj, pi, pnext = vectors(3, n, 3)
        return pnext, mgs_step_ref(0.61, pj, pi)
    if name == "cg_update":
        p, t, u, r, zx, zd = vectors(6, n, 1)
        ro = cg_update_ref(0.83, 1.9, p, t, u, r, zx, zd, 0.0, 0, 0.0)[1]
        return ro, ro
    raise KeyError(name)


REDUCERS = (("dot", True), ("norms", False), ("norm1_nan", False), ("mgs_step", False), ("cg_update", False))
