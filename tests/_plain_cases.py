"""Irregular CSR matrices for the plain CSR kernels -- k_csr_lstream, k_csr_wstream2, k_csr_xtile (csrc/kernels2.hip.h), the four
k_csr_wstream<OP, RW, CAPW> and the six k_csr_rows<L, OP> (csrc/kernels.hip.h), the four k_csr_estream<L, OP> (csrc/kernels3.hip.h) -- built so
that each reaches the edges of its kernel, with the upload rules they depend on restated in numpy and ASSERTED: pick_kernel, the refusal of
every coding, the row sort, upload_ja16, build_xtile, build_estream (csrc/device_csr.hip.h) and upload_diag (csrc/hierarchy.hip.h).  restate()
gives the 28 traits of fasp_hip_csr_plan the device copy must have; RUNS names, per run and operation, the kernel instantiation the matrix is
built for (tests/_csr_cases.py, KERNELS).

All values are standard normal, so no coding applies (asserted).  Unless an edge is about them, the columns of a row are unsorted and distinct
and the diagonal sits at a random position.  Cases are built once per process and their arrays are read-only."""
import functools
import itertools

import numpy as np

import _csr_cases as cc
from _csr_cases import BLOCK, KERNELS, OPS_RECT, OPS_SQUARE, TRAIT_DEFAULTS, block_tiles, persistent_grid

MAXGRID = 2048               # csrc/kernels.hip.h
SMALL_XFER_ROWS = 256 * 1024   # pick_kernel: rectangular operators with fewer rows keep the row kernel
XT_XCAP = 1024               # k_csr_xtile: distinct columns of a listed tile
ES_CAP, ES_PER_WAVE, ES_WMAX = 512, 3072, 5120
SELL_MAXV = 9216
LS_CAP = 512                 # k_csr_lstream<OP, 512>: entries of a wave's slab
WS2_STEP = 508               # k_csr_wstream2: entries of a chunk
WIN_ALIGN = 1024


# ------------------------------------------------------------------------------------------------------------------------------
# the upload rules, restated
# ------------------------------------------------------------------------------------------------------------------------------
def pick_kernel(nrow, ncol, nnz):
    """pick_kernel -> (kind, lanes)"""
    avg = nnz / nrow if nrow > 0 else 1.0
    kind = 2 if avg <= 48.0 else 0
    lanes = 16 if avg < 300.0 else 32 if avg < 1000.0 else 64
    while lanes < 64 and nrow * lanes < 0.75 * MAXGRID * BLOCK:
        lanes *= 2
    if avg < 48.0:
        lanes = 2 if avg < 3.0 else 4 if avg < 6.0 else 8 if avg < 24.0 else 16
    if kind == 2 and nrow != ncol and nrow < SMALL_XFER_ROWS:
        kind = 0
    return kind, lanes


def assert_uncoded(ia, ja, val, nrow, ncol):
    """upload_csr tries the row patterns and the byte dictionary where nnz >= 4096 and nnz <= 48 row; both must refuse.  Two rows of one
    pattern have the same first value, so there are at least as many patterns as distinct first values: more than row / 8 (cc.coding: "patterns
    * 8 <= row"); and more than 256 distinct values are more than 256 (offset, value) pairs."""
    nnz = len(ja)
    if not (nnz >= 4096 and nnz <= 48.0 * nrow):
        return
    lens = np.diff(ia)
    first = val[ia[:-1][lens > 0]]
    assert len(np.unique(first)) * 8 > nrow and len(np.unique(val)) > 256


def assert_no_sell(ia, val, nrow, ncol):
    """build_sell refuses: sizes outside its range, a row beyond 255 entries, padding over 125 %, or more than SELL_MAXV distinct values."""
    nnz, lens = len(val), np.diff(ia).astype(np.int64)
    if nrow <= 0 or nnz < 4096 or nnz > 48.0 * nrow or nnz <= 7.6 * nrow or ncol >= 1 << 28 or lens.max() > 255:
        return
    pad = np.zeros((nrow + 63) // 64 * 64, dtype=np.int64)
    pad[:nrow] = lens
    slots = 64 * int(pad.reshape(-1, 64).max(axis=1).sum())
    assert slots * 100 > 125 * nnz or len(np.unique(val)) > SELL_MAXV


def xtile_lists(ia, ja, nrow, ncol):
    """build_xtile -> (lists built, ntcols, distinct columns per 64-row tile)"""
    nnz = len(ja)
    ntile = (nrow + 63) // 64
    lens = np.diff(ia).astype(np.int64)
    tile = np.repeat(np.arange(nrow, dtype=np.int64), lens) // 64
    key = np.unique(tile * ncol + ja)
    cnt = np.bincount(key // ncol, minlength=ntile)
    if nrow < 4096 or nnz < 16 * nrow:
        return False, 0, cnt
    ent = np.bincount(tile, minlength=ntile)
    samp = np.arange(0, ntile, 61)
    if (cnt[samp] > XT_XCAP).sum() * 20 > len(samp) or cnt[samp].sum() * 2.5 > 1.1 * ent[samp].sum():
        return False, 0, cnt
    if (cnt > XT_XCAP).sum() * 20 > ntile:
        return False, 0, cnt
    total = int(cnt[cnt <= XT_XCAP].sum())
    if total * 2.5 > nnz:
        return False, 0, cnt
    return True, total, cnt


def estream_tables(ia, nrow, nnz):
    """build_estream_host -> (W, chunks)"""
    W = min(ES_WMAX, (nnz + ES_PER_WAVE - 1) // ES_PER_WAVE)
    W = max(32, (W + 31) // 32 * 32)
    ebeg = (nnz * np.arange(W + 1, dtype=np.int64) // W) & ~7
    ebeg[W] = nnz
    nc = 0
    for w in range(W):
        n = int(ebeg[w + 1] - ebeg[w])
        if n <= 0:
            continue
        nch = (n + ES_CAP - 1) // ES_CAP
        size = ((n + nch - 1) // nch + 7) & ~7
        nc += sum(1 for j in range(nch) if j * size < n)
    return W, nc


def restate(nrow, ncol, ia, ja, val):
    """-> (traits of the device copy upload_csr (+ upload_diag, square) makes, in the layout of fasp_hip_csr_plan; device copy sorted by column)"""
    nnz = len(ja)
    lens = np.diff(ia).astype(np.int64)
    rows = np.repeat(np.arange(nrow, dtype=np.int64), lens)
    kind, lanes = pick_kernel(nrow, ncol, nnz)
    assert_uncoded(ia, ja, val, nrow, ncol)
    t = dict(TRAIT_DEFAULTS, row=nrow, col=ncol, nnz=nnz, kind=kind, lanes=lanes)
    is_sorted = nnz > 0 and kind == 0                       # do_sort (the device sort or, beyond 16384 entries in a row, the host's)
    if kind == 2:
        built, ntcols, _ = xtile_lists(ia, ja, nrow, ncol)
        t.update(lja16=int(built), ntcols=ntcols)
        assert_no_sell(ia, val, nrow, ncol)
    if kind == 0 and nnz >= 4096:                           # upload_ja16 / the same rule in upload_sorted_on_device
        relative = ncol > 65536
        ok = True
        if relative and nnz:
            hi = np.full(nrow, -1, dtype=np.int64); lo = np.full(nrow, 1 << 40, dtype=np.int64)
            np.maximum.at(hi, rows, ja); np.minimum.at(lo, rows, ja)
            ok = bool(np.all((hi - lo)[lens > 0] < 65536))
        if ok:
            t.update(ja16=1, jbase=int(relative))
            if nnz >= 65536 and nrow >= 1 and nnz >= 48.0 * nrow:     # build_estream
                assert not relative, "chunk-relative columns are not restated: keep k_csr_estream cases within 65536 columns"
                W, nc = estream_tables(ia, nrow, nnz)
                t.update(es_tab=1, es_W=W, es_nc=nc)
    if nrow == ncol:                                        # upload_diag
        ndiag = np.bincount(rows[ja == rows], minlength=nrow)
        t.update(dup_diag=int((ndiag > 1).any()), dpos=int(not is_sorted))
    return t, is_sorted


# ------------------------------------------------------------------------------------------------------------------------------
# a matrix from row lengths
# ------------------------------------------------------------------------------------------------------------------------------
def _prime_at_most(n):
    for p in range(n, 1, -1):
        if all(p % d for d in range(2, int(p ** 0.5) + 1)):
            return p
    return 1


def assemble(nrow, ncol, lens, rng, has_diag=None, dpos=None, qcap=2003, lo_min=0, free=(), sort_cols=False):
    """CSR matrix with the row lengths lens, standard-normal values.  Row r draws its off-centre columns WITHOUT repetition from a window of Q + 1
    columns around its centre (r; rectangular: r ncol / nrow), Q the largest prime <= min(ncol - 1, qcap): the q-th one is candidate (a_r + q g_r)
    mod Q, g_r random, so they come unsorted.  has_diag[r]: the centre column is stored, at position dpos[r] (default: square matrices store it in every
    non-empty row, at a random position).  lo_min: no column below it.  free: rows whose columns are drawn WITH repetition from all columns but r
    (rows longer than the matrix is wide), the diagonal first.  sort_cols: every row ascending.  -> (ia, ja, val, has_diag, dpos)"""
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.shape == (nrow,)
    square = nrow == ncol
    nnz = int(lens.sum())
    ia = np.zeros(nrow + 1, dtype=np.int32)
    ia[1:] = np.cumsum(lens)
    rows = np.repeat(np.arange(nrow, dtype=np.int64), lens)
    pos = np.arange(nnz, dtype=np.int64) - np.repeat(ia[:-1].astype(np.int64), lens)
    Q = _prime_at_most(min(ncol - 1, qcap)) if ncol >= 3 else max(ncol - 1, 0)
    centre = np.arange(nrow, dtype=np.int64) if square else np.arange(nrow, dtype=np.int64) * ncol // max(nrow, 1)
    assert ncol - Q - 1 >= lo_min or Q == 0
    lo = np.clip(centre - Q // 2, lo_min, max(ncol - Q - 1, lo_min))
    has_diag = (np.full(nrow, square) if has_diag is None else np.asarray(has_diag, dtype=bool)) & (lens > 0)
    dp = rng.integers(0, np.maximum(lens, 1)) if dpos is None else np.asarray(dpos, dtype=np.int64)
    dp = np.where(has_diag, np.minimum(dp, np.maximum(lens - 1, 0)), -1)
    isd = has_diag[rows] & (pos == dp[rows])
    q = pos - (has_diag[rows] & (pos > dp[rows]))
    noff = lens - has_diag
    fr = np.zeros(nrow, dtype=bool)
    fr[list(free)] = True
    assert noff[~fr].max(initial=0) <= Q
    a = rng.integers(0, max(Q, 1), size=nrow)
    g = rng.integers(1, max(Q, 2), size=nrow)
    idx = (a[rows] + q * g[rows]) % max(Q, 1)
    col = lo[rows] + idx + (idx >= (centre - lo)[rows])
    col = np.where(isd, centre[rows], col)
    for r in free:
        k0, k1 = int(ia[r]), int(ia[r + 1])
        c = rng.integers(0, ncol - 1, size=k1 - k0)
        c += c >= centre[r]
        if has_diag[r]:
            c[dp[r]] = centre[r]
        col[k0:k1] = c
    if sort_cols:
        col = col[np.lexsort((col, rows))]
    assert nnz == 0 or (col.min() >= lo_min and col.max() < ncol)
    return ia, col.astype(np.int32), rng.standard_normal(nnz), has_diag, dp


def _fill(total, nrows, rng):
    """`total` entries over nrows rows, as evenly as it goes, in random order"""
    v = np.full(nrows, total // nrows, dtype=np.int64)
    v[:total % nrows] += 1
    return rng.permutation(v)


def _align(lens, tile, a):
    """Lengthens the last row in front of wave tile `tile` so that the tile's first entry k0 has k0 & 3 == a."""
    lens[64 * tile - 1] += (a - int(lens[:64 * tile].sum())) % 4


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _finish(name, nrow, ncol, ia, ja, val, ops, inf_rows=None, **extra):
    nnz = len(ja)
    assert ia[0] == 0 and ia[-1] == nnz and len(ia) == nrow + 1 and len(val) == nnz
    assert nnz == 0 or (ja.min() >= 0 and ja.max() < ncol)
    traits, is_sorted = restate(nrow, ncol, ia, ja, val)
    c = dict(name=name, nrow=nrow, ncol=ncol, ia=ia, ja=ja, val=val, ops=tuple(ops), inf_rows=inf_rows, traits=traits, sorted=is_sorted)
    c.update(extra)
    return _freeze(c)


def _row_info(c):
    n, ia, ja = c["nrow"], c["ia"], c["ja"]
    lens = np.diff(ia).astype(np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    pos = np.arange(len(ja), dtype=np.int64) - np.repeat(ia[:-1].astype(np.int64), lens)
    return lens, rows, pos


def diagonal_set(n, ia, ja, val, has_diag, dp, rng, dup, skip=(), maxlen=1 << 30):
    """The edges of the diagonal's handling, on rows drawn at random outside `skip`: the stored diagonal equal to 0.0 (the |d| <= 1e-20 guard), an
    off-diagonal column stored twice and -- dup -- the diagonal stored twice (an off-diagonal entry of the row moved onto it; the last one stored is
    the reference's d).  Rows WITHOUT a diagonal and its position in the row are has_diag / dpos of assemble().  -> the rows of each kind"""
    lens = np.diff(ia)
    ok = np.ones(n, dtype=bool)
    ok[list(skip)] = False
    cand = np.flatnonzero(ok & has_diag & (lens >= 4) & (lens <= maxlen))
    pick = rng.permutation(cand)[:3 * max(8, n // 50)]
    zero, twice, offdup = np.array_split(pick, 3)
    for r in zero:
        val[ia[r] + dp[r]] = 0.0
    for r in offdup:
        p = [k for k in range(ia[r], ia[r + 1]) if k != ia[r] + dp[r]]
        ja[p[-1]] = ja[p[0]]
    if dup:
        for r in twice:
            p = [k for k in range(ia[r], ia[r + 1]) if k != ia[r] + dp[r]]
            ja[p[int(rng.integers(0, len(p)))]] = r
    return zero, (twice if dup else twice[:0]), offdup


def _diag_policy(n, lens, rng, no_diag_rows=()):
    """has_diag / dpos: a tenth of the rows store no diagonal; of the others a fifth store it first, a fifth last, a fifth as their 9th entry
    (rows of 9 and more: the second round of 8), the rest anywhere."""
    has = rng.random(n) >= 0.1
    has[list(no_diag_rows)] = False
    u = rng.random(n)
    dp = rng.integers(0, np.maximum(lens, 1))
    dp = np.where(u < 0.2, 0, np.where(u < 0.4, lens - 1, np.where((u < 0.6) & (lens >= 9), 8, dp)))
    return has, np.maximum(dp, 0)


def _assert_diag_edges(c, has, dp, zero, twice, offdup, dup):
    n, ia, ja, val = c["nrow"], c["ia"], c["ja"], c["val"]
    lens, rows, pos = _row_info(c)
    ndiag = np.bincount(rows[ja == rows], minlength=n)
    assert ((ndiag == 0) & (lens > 0)).sum() >= 8                                  # rows without a diagonal
    assert all(val[ia[r] + dp[r]] == 0.0 and ja[ia[r] + dp[r]] == r for r in zero) and len(zero) >= 8
    assert (ndiag > 1).any() == bool(dup) and (not dup or all(ndiag[r] == 2 for r in twice))
    assert all(len(np.unique(ja[ia[r]:ia[r + 1]])) < lens[r] for r in offdup) and len(offdup) >= 8
    h = has & (lens > 0)
    assert (h & (dp == 0) & (lens > 1)).sum() >= 8 and (h & (dp == lens - 1) & (lens > 1)).sum() >= 8 and (h & (dp == 8) & (lens > 9)).sum() >= 8
    assert c["traits"]["dup_diag"] == int(bool(dup))


# ------------------------------------------------------------------------------------------------------------------------------
# ls_*: k_csr_lstream<OP, 512>
# ------------------------------------------------------------------------------------------------------------------------------
TAILS = (0, 1, 63, 64, 65, 255)
LS_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17)
LS_P = (.10, .12, .12, .12, .12, .12, .08, .08, .06, .04, .04)
LS_SPANS = tuple(itertools.product((0, 1, 3), (511, 512, 513)))      # (k0 & 3, k1 - s0)


@functools.lru_cache(maxsize=None)
def ls_main(t=65, empty_ends=False, inf=False):
    """Square, n = 8192 + t, mean row about 6: k_csr_lstream.  Wave tile = 64 rows; its slab holds the 512 entries from s0 = k0 & ~3 on, a tile
    fits iff k1 - s0 <= 512.  Wave tiles 4, 8, ..., 36: k1 - s0 = 511, 512, 513 with k0 & 3 = 0, 1, 3 (rows of 7 and 8 entries); tile 40 holds a row
    of 600 entries, tile 44 one of 1500 (the oversized path, rows read from global memory); tile 48: every row exactly 8 entries (one full round, no
    second); tile 52 is EMPTY between the full tiles 51 and 53.  empty_ends: the first and the last wave tile are empty.  Every other row draws its
    length from 0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17.  The diagonal set: _diag_policy and diagonal_set (the diagonal twice: k_csr_lstream tests c != r
    itself and stays selected for the Jacobi sweep).  inf: no row references column 0 (row 0 stores no diagonal), and the tests set x[0] = +inf: the
    padding lanes gather x[0], a product that leaks into a sum makes it non-finite."""
    n = 8192 + t
    rng = np.random.default_rng(9100 + t + 1000 * empty_ends + 2000 * inf)
    ntile = (n + 63) // 64
    lens = rng.choice(LS_LENS, size=n, p=LS_P).astype(np.int64)
    special = {}
    for i, (a, span) in enumerate(LS_SPANS):
        T = 4 + 4 * i
        lens[64 * T:64 * T + 64] = _fill(span - a, 64, rng)
        special[T] = (a, span)
    for T, L in ((40, 600), (44, 1500)):
        lens[64 * T:64 * T + 64] = rng.integers(0, 4, size=64)
        lens[64 * T + 20] = L
    lens[64 * 48:64 * 49] = 8
    lens[64 * 51:64 * 54] = 8
    lens[64 * 52:64 * 53] = 0
    lens[-1] = max(lens[-1], 3)
    if empty_ends:
        lens[:64] = 0
        lens[64 * (ntile - 1):] = 0
    for T, (a, span) in special.items():
        _align(lens, T, a)
    has, dp = _diag_policy(n, lens, rng, no_diag_rows=(0,) if inf else ())
    ia, ja, val, has, dp = assemble(n, n, lens, rng, has_diag=has, dpos=dp, lo_min=1 if inf else 0)
    zero, twice, offdup = diagonal_set(n, ia, ja, val, has, dp, rng, dup=True, skip=(0,), maxlen=40)
    inf_rows = None
    if inf:
        inf_rows = np.zeros(n, dtype=bool)
        inf_rows[0] = True
        assert ja.min() >= 1
    name = f"ls_n{n}" + ("_empty_ends" if empty_ends else "") + ("_inf" if inf else "")
    c = _finish(name, n, n, ia, ja, val, OPS_RECT if inf else OPS_SQUARE, inf_rows)
    tr = c["traits"]
    assert tr["kind"] == 2 and len(ja) <= 7.6 * n and tr["dpos"] == 1 and not c["sorted"] and tr["lja16"] == 0
    k0, k1 = ia[0:64 * ntile:64].astype(np.int64), ia[np.minimum(np.arange(1, ntile + 1) * 64, n)].astype(np.int64)
    span = k1 - (k0 & ~3)
    for T, (a, sp) in special.items():
        assert k0[T] & 3 == a and span[T] == sp, (T, a, sp, k0[T], span[T])
    assert span[40] > LS_CAP and span[44] > LS_CAP and lens[64 * 40 + 20] == 600 and lens[64 * 44 + 20] == 1500
    assert span[52] == (k0[52] & 3) and k1[52] == k0[52] and span[51] >= 512 and span[53] >= 512
    assert set(LS_LENS) <= set(lens.tolist())
    if empty_ends:
        assert k1[0] == 0 and k0[ntile - 1] == len(ja) and lens[-1] == 0
    else:
        assert lens[64 * (ntile - 1):].sum() > 0
    assert n - 64 * (ntile - 1) == (t % 64 or 64)
    _assert_diag_edges(c, has, dp, zero, twice, offdup, True)
    # a persistent grid of 8 workgroups (maxgrid 1 | 2): some workgroup walks three tiles and more -- the A / B / C look-ahead is all in use
    nt256 = (n + BLOCK - 1) // BLOCK
    assert all(persistent_grid(g, nt256) == 8 for g in (1, 2)) and max(len(block_tiles(nt256, 8, b)) for b in range(8)) >= 3
    assert n >= 4 * WIN_ALIGN                                # split_rows splits
    return c


LS_TINY = (1, 2, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def ls_tiny(n):
    """Square, n rows, k_csr_lstream: one wave tile, shorter than, exactly and just beyond 64 rows."""
    rng = np.random.default_rng(9300 + n)
    lens = np.minimum(rng.choice(LS_LENS, size=n, p=LS_P), 1 if n < 3 else 17).astype(np.int64)
    lens[0] = max(lens[0], 1)
    ia, ja, val, _, _ = assemble(n, n, lens, rng)
    c = _finish(f"ls_tiny{n}", n, n, ia, ja, val, OPS_SQUARE)
    assert c["traits"]["kind"] == 2 and 0 < len(ja) <= 7.6 * n
    return c


@functools.lru_cache(maxsize=None)
def ls_empty():
    """Square, 300 rows, no entry at all."""
    n = 300
    ia, ja, val, _, _ = assemble(n, n, np.zeros(n, dtype=np.int64), np.random.default_rng(1))
    c = _finish("ls_nnz0", n, n, ia, ja, val, OPS_SQUARE)
    assert len(ja) == 0 and c["traits"]["kind"] == 2 and not c["sorted"] and c["traits"]["dpos"] == 1
    return c


# ------------------------------------------------------------------------------------------------------------------------------
# ws2_*: k_csr_wstream2, and the k_csr_wstream forms under gen2 = 0
# ------------------------------------------------------------------------------------------------------------------------------
WS2_LENS = (0, 1, 2, 3, 5, 7, 8, 9, 12, 16, 20, 24, 31, 40)
WS2_SPANS = tuple(itertools.product((0, 1, 2, 3), (507, 508, 509, 1016, 1017)))     # (k0 & 3, k1 - k0)
WS_SPANS = (511, 512, 513, 1023, 1024, 1025)      # k_csr_wstream: outer chunk CAPW = 512 | 1024, inner step 512


@functools.lru_cache(maxsize=None)
def ws2_main(t=65, dup=False):
    """Square, n = 8192 + t, mean row about 14: k_csr_wstream2 (7.6 < mean <= 48; tiles share too few columns for k_csr_xtile's lists).  A wave tile's
    entries [k0, k1) are worked through in chunks of 508, staged from lo & ~3.  Wave tiles 4, 7, ..., 61: k1 - k0 = 507, 508, 509, 1016, 1017 at every
    k0 & 3; tiles 64, 67, ..., 79: k1 - k0 = 511, 512, 513, 1023, 1024, 1025 with all entries in the first 32 rows (the rows 32 .. 63 are empty: the same
    span for the 32-row tiles of k_csr_wstream<., 32, .>); tile 82: a row of 600 entries alone in its tile, its diagonal the FIRST slot of the second
    chunk; tile 85: one of 600 among neighbours, its diagonal the LAST slot of the first chunk; tile 88: one of 1300 alone, its diagonal deep in the third
    chunk; tile 91: one of 1300 among neighbours; tile 94 empty and 95 full (a zero-length stage in front of a full one).  Every other row draws its
    length from WS2_LENS.  The diagonal set as in ls_main; dup: with the diagonal stored twice in some rows -- then the Jacobi sweep keeps k_csr_rows."""
    n = 8192 + t
    rng = np.random.default_rng(9500 + t + 1000 * dup)
    ntile = (n + 63) // 64
    lens = rng.choice(WS2_LENS, size=n).astype(np.int64)
    special = {}
    for i, (a, span) in enumerate(WS2_SPANS):
        T = 4 + 3 * i
        lens[64 * T:64 * T + 64] = _fill(span, 64, rng)
        special[T] = (a, span)
    for i, span in enumerate(WS_SPANS):
        T = 64 + 3 * i
        lens[64 * T:64 * T + 32] = _fill(span, 32, rng)
        lens[64 * T + 32:64 * T + 64] = 0
        special[T] = (None, span)
    for T, L, alone in ((82, 600, True), (85, 600, False), (88, 1300, True), (91, 1300, False)):
        if alone:
            lens[64 * T:64 * T + 64] = 0
        lens[64 * T + 10] = L
    lens[64 * 94:64 * 95] = 0
    lens[64 * 95:64 * 96] = 8
    for T, (a, span) in special.items():
        if a is not None:
            _align(lens, T, a)
    has, dp = _diag_policy(n, lens, rng)
    long_rows = [64 * T + 10 for T in (82, 85, 88, 91)]
    has[long_rows] = True
    front85 = int(lens[64 * 85:64 * 85 + 10].sum())
    assert front85 <= 507
    dp[long_rows] = (WS2_STEP, WS2_STEP - 1 - front85, 2 * WS2_STEP + 200, 700)
    ia, ja, val, has, dp = assemble(n, n, lens, rng, has_diag=has, dpos=dp)
    zero, twice, offdup = diagonal_set(n, ia, ja, val, has, dp, rng, dup=dup, skip=long_rows, maxlen=40)
    c = _finish(f"ws2_n{n}" + ("_dup" if dup else ""), n, n, ia, ja, val, OPS_SQUARE)
    tr = c["traits"]
    nnz = len(ja)
    assert tr["kind"] == 2 and 7.6 * n < nnz <= 48.0 * n and tr["dpos"] == 1 and tr["lja16"] == 0 and tr["sell_code"] == 0 and not c["sorted"]
    k0, k1 = ia[0:64 * ntile:64].astype(np.int64), ia[np.minimum(np.arange(1, ntile + 1) * 64, n)].astype(np.int64)
    for T, (a, sp) in special.items():
        assert k1[T] - k0[T] == sp and (a is None or k0[T] & 3 == a), (T, a, sp)
        if a is None:
            assert ia[64 * T + 32] == k1[T]
    # rows straddling a chunk boundary, in the tiles of 1016 and 1017 entries too
    straddled = set()
    for T in special:
        r = np.arange(64 * T, 64 * T + 64)
        for cut in range(int(k0[T]) + WS2_STEP, int(k1[T]), WS2_STEP):
            if ((ia[r] < cut) & (ia[r + 1] > cut)).any():
                straddled.add(special[T][1])
    assert {1016, 1017} & straddled and len(straddled) >= 3, straddled
    # the diagonals of the long rows, by storage index, against the chunk boundaries of their tile
    d82, d85, d88 = (int(ia[64 * T + 10] + dp[64 * T + 10]) for T in (82, 85, 88))
    assert ja[d82] == 64 * 82 + 10 and d82 == k0[82] + WS2_STEP and k1[82] - k0[82] == 600
    assert ja[d85] == 64 * 85 + 10 and d85 == k0[85] + WS2_STEP - 1 and k1[85] - k0[85] > 600
    assert ja[d88] == 64 * 88 + 10 and 2 * WS2_STEP < d88 - k0[88] < k1[88] - k0[88] and k1[88] - k0[88] == 1300
    assert k1[91] - k0[91] > 1300 and k1[94] == k0[94] and k1[95] - k0[95] == 512
    assert {7, 8, 9} <= set(lens.tolist())
    _assert_diag_edges(c, has, dp, zero, twice, offdup, dup)
    nt256 = (n + BLOCK - 1) // BLOCK
    assert all(persistent_grid(g, nt256) == 8 for g in (1, 2)) and max(len(block_tiles(nt256, 8, b)) for b in range(8)) >= 3
    return c


# ------------------------------------------------------------------------------------------------------------------------------
# xt_*: k_csr_xtile
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def xt_main(t=65):
    """Square, n = 4160 + t, banded: every row stores its diagonal and 19 of the 31 columns around it -- 64 rows share about 95 columns, 13 entries per
    distinct column: build_xtile lists every tile.  Wave tile 10: exactly 1024 distinct columns (16 of its own per row, 3 of them twice, and the diagonal) -- the largest list;
    tile 20: 1025 -- no list, the operands come from global memory; tile 30: every entry hits column 1900; tile 40 is empty; tile 50 holds a row of 600
    entries.  (The sample takes the tiles 0 and 61: ordinary ones.)"""
    n = 4160 + t
    rng = np.random.default_rng(9700 + t)
    lens = np.full(n, 20, dtype=np.int64)
    lens[64 * 40:64 * 41] = 0
    lens[64 * 50 + 10] = 1                  # (placeholder: the 600 entries are put in below)
    ia, ja, _, _, _ = assemble(n, n, lens, rng, qcap=31)
    lens[64 * 50 + 10] = 600
    ia2 = np.zeros(n + 1, dtype=np.int32)
    ia2[1:] = np.cumsum(lens)
    ja2 = np.empty(ia2[-1], dtype=np.int32)
    for r in range(n):
        if r != 64 * 50 + 10:
            ja2[ia2[r]:ia2[r + 1]] = ja[ia[r]:ia[r + 1]]
    ja2[ia2[64 * 50 + 10]:ia2[64 * 50 + 11]] = 3300 + rng.permutation(700)[:600]
    ia, ja = ia2, ja2
    for T, extra in ((10, 0), (20, 1)):
        B = 64 * T - 480                    # the tile's own rows lie among its 1024 columns: every row stores its diagonal, once
        for i in range(64):
            r = 64 * T + i
            cols = B + 16 * i + rng.permutation(16)
            other = cols[cols != r]
            row = np.concatenate([cols, other[:3], [other[3] if r in cols else r]])
            if extra and i == 0:
                row[-2] = B + 1024
            ja[ia[r]:ia[r + 1]] = rng.permutation(row)
    ja[ia[64 * 30]:ia[64 * 31]] = 1900
    val = rng.standard_normal(len(ja))
    c = _finish(f"xt_n{n}", n, n, ia, ja, val, OPS_SQUARE)
    tr = c["traits"]
    built, ntcols, cnt = xtile_lists(ia, ja, n, n)
    assert tr["kind"] == 2 and tr["lja16"] == 1 and built and tr["dup_diag"] == 0 and tr["dpos"] == 1 and len(ja) >= 16 * n and len(ja) > 7.6 * n
    assert cnt[10] == XT_XCAP and cnt[20] == XT_XCAP + 1 and cnt[30] == 1 and cnt[40] == 0 and 600 < cnt[50] <= XT_XCAP
    assert (cnt > XT_XCAP).sum() == 1 and cnt[0] <= 128 and cnt[61] <= 128 and ntcols == cnt.sum() - cnt[20]
    _, rows, _ = _row_info(c)
    ndiag = np.bincount(rows[ja == rows], minlength=n)
    assert (ndiag[:64 * 30] == 1).all() and ndiag.max() == 1            # (the fat tile's rows too: their Jacobi sweep depends on their sums)
    return c


# ------------------------------------------------------------------------------------------------------------------------------
# rows_*: k_csr_rows<L, OP>
# ------------------------------------------------------------------------------------------------------------------------------
ROWS_L = (2, 4, 8, 16, 32, 64)
ROWS_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 1100)
ROWS_FORMS = ("a", "b", "c", "d", "e", "f")


@functools.lru_cache(maxsize=None)
def rows_case(form):
    """The index forms k_csr_rows reads.  Every matrix holds each length of ROWS_LENS (a: those up to 300) at least once: L - 1, L, L + 1, 3 L, 3 L + 1,
    4 L, 4 L + 1 for every L -- the 4-stride main loop with nothing, one, two and three strides left for the clamped tail.
    a  rectangular 1001 x 777, nnz < 4096: 32-bit columns;            b  rectangular 1001 x 3000, nnz >= 4096: absolute 16-bit columns;
    c  1001 x 70000, every row inside a band of 2004 columns: 16-bit columns relative to the row's smallest (jbase);
    d  as c, but row 500 spans 68900 columns: 32-bit columns;          e  square 1301, mean row > 48: a device copy sorted by column, no diagonal
    positions, the diagonal set with the diagonal twice;              f  square 1301, mean row about 13: a stream-kernel matrix (unsorted, diagonal
    positions, no 16-bit copy) sent to k_csr_rows by fasp_hip_tune("kind", 0)."""
    rng = np.random.default_rng(9800 + ROWS_FORMS.index(form))
    square = form in "ef"
    nrow = 1301 if square else 1001
    ncol = {"a": 777, "b": 3000, "c": 70000, "d": 70000, "e": nrow, "f": nrow}[form]
    want = [L for L in ROWS_LENS if L <= (300 if form == "a" else 1100)]
    fill = {"a": (0, 4), "b": (0, 41), "c": (0, 41), "d": (0, 41), "e": (44, 51), "f": (0, 21)}[form]
    lens = rng.integers(*fill, size=nrow).astype(np.int64)
    where = rng.permutation(np.delete(np.arange(nrow), 500))[:len(want)]
    lens[where] = want
    lens[500] = 12
    has = dp = None
    if square:
        has, dp = _diag_policy(nrow, lens, rng)
    ia, ja, val, has, dp = assemble(nrow, ncol, lens, rng, has_diag=has, dpos=dp, qcap=2003)
    if form == "d":
        ja[ia[500]], ja[ia[500] + 1] = 100, 69000
    zero = twice = offdup = None
    if square:
        zero, twice, offdup = diagonal_set(nrow, ia, ja, val, has, dp, rng, dup=form == "e")
    c = _finish(f"rows_{form}", nrow, ncol, ia, ja, val, OPS_SQUARE if square else OPS_RECT)
    tr, nnz = c["traits"], len(ja)
    assert set(want) <= set(np.diff(ia).tolist()) and all(nrow % (BLOCK // L) for L in ROWS_L)
    assert tr["es_tab"] == 0 and tr["lja16"] == 0
    if form == "a": assert nnz < 4096 and tr["kind"] == 0 and c["sorted"] and (tr["ja16"], tr["jbase"]) == (0, 0)
    if form == "b": assert nnz >= 4096 and tr["kind"] == 0 and c["sorted"] and (tr["ja16"], tr["jbase"]) == (1, 0)
    if form == "c": assert nnz >= 4096 and tr["kind"] == 0 and c["sorted"] and (tr["ja16"], tr["jbase"]) == (1, 1)
    if form == "d": assert nnz >= 4096 and tr["kind"] == 0 and c["sorted"] and (tr["ja16"], tr["jbase"]) == (0, 0) and lens[500] >= 2
    if form == "e":
        assert nnz > 48.0 * nrow and nnz < 65536 and tr["kind"] == 0 and c["sorted"] and tr["dpos"] == 0 and tr["ja16"] == 1 and tr["dup_diag"] == 1
    if form == "f":
        assert 7.6 * nrow < nnz <= 48.0 * nrow and tr["kind"] == 2 and not c["sorted"] and tr["dpos"] == 1 and tr["ja16"] == 0 and tr["dup_diag"] == 0
    if square:
        _assert_diag_edges(c, has, dp, zero, twice, offdup, form == "e")
    return c


@functools.lru_cache(maxsize=None)
def rect_stream(which):
    """A rectangular matrix (a transfer operator: k_csr_rows by pick_kernel, its device copy SORTED by column) sent to the stream kernels by
    fasp_hip_tune("kind", 2).  The stream kernels follow the storage order of the DEVICE copy, so -- the edge here being the sorted copy -- the
    rows are generated with ascending columns: the oracle on the host matrix then sums in the same order.  ls: 2085 x 70000, mean row about 5 -- k_csr_lstream;
    the row-relative 16-bit copy the upload made (jbase) must not be passed.  ws2: 2085 x 3000, mean row about 14 -- k_csr_wstream2."""
    rng = np.random.default_rng(9900 + (which == "ws2"))
    nrow = 2085
    if which == "ls":
        ncol, lens = 70000, rng.choice(LS_LENS, size=nrow, p=LS_P).astype(np.int64)
    else:
        ncol, lens = 3000, rng.choice(WS2_LENS, size=nrow).astype(np.int64)
        lens[700] = 600
    ia, ja, val, _, _ = assemble(nrow, ncol, lens, rng, sort_cols=True)
    c = _finish(f"rect_stream_{which}", nrow, ncol, ia, ja, val, OPS_RECT)
    tr, nnz = c["traits"], len(ja)
    r = np.repeat(np.arange(nrow), np.diff(ia))
    assert np.all((np.diff(ja.astype(np.int64)) > 0) | (np.diff(r) > 0))               # ascending, no column twice
    assert tr["kind"] == 0 and c["sorted"] and nnz >= 4096 and tr["ja16"] == 1 and tr["jbase"] == int(which == "ls") and tr["dpos"] == 0
    assert (nnz <= 7.6 * nrow) == (which == "ls") and nnz <= 48.0 * nrow
    return c


@functools.lru_cache(maxsize=None)
def ws2_nodpos():
    """Square, 1301 rows, mean row just above 48: pick_kernel gives it to k_csr_rows, so its device copy is SORTED by column and carries NO
    diagonal positions -- and fasp_hip_tune("kind", 2) sends it to k_csr_wstream2, whose Jacobi sweep takes the diagonal out by its position.  The
    plan must keep the Jacobi sweep on k_csr_rows (with and without the fused partials) and leave every other operation on k_csr_wstream2.  As in
    rect_stream the rows are generated with ascending, distinct columns: the sorted copy's storage order is the host's, and the oracle's sums
    are bit for bit the stream kernel's.  No diagonal is stored twice; a tenth of the rows store none, some store 0.0; rows of 0, 1, 7, 8, 9
    and 1100 entries; every wave tile holds about 3000 entries, six chunks.  nnz < 65536: no k_csr_estream tables."""
    n = 1301
    rng = np.random.default_rng(9870)
    lens = rng.integers(45, 52, size=n).astype(np.int64)
    where = rng.permutation(n)[:12]
    lens[where] = (0, 0, 1, 1, 7, 8, 9, 15, 16, 17, 300, 1100)
    has = rng.random(n) >= 0.1
    ia, ja, val, has, _ = assemble(n, n, lens, rng, has_diag=has, sort_cols=True)
    rows = np.repeat(np.arange(n), np.diff(ia))
    ond = np.flatnonzero(ja == rows)
    zero = ond[rng.permutation(len(ond))[:20]]
    val[zero] = 0.0
    c = _finish("ws2_nodpos", n, n, ia, ja, val, OPS_SQUARE)
    tr, nnz = c["traits"], len(ja)
    assert np.all((np.diff(ja.astype(np.int64)) > 0) | (np.diff(rows) > 0))            # ascending, no column twice
    assert tr["kind"] == 0 and c["sorted"] and tr["dpos"] == 0 and tr["dup_diag"] == 0 and nnz > 48.0 * n and nnz < 65536 and tr["es_tab"] == 0
    assert tr["ja16"] == 1 and tr["jbase"] == 0 and tr["lja16"] == 0
    ndiag = np.bincount(rows[ond], minlength=n)
    assert ndiag.max() == 1 and ((ndiag == 0) & (lens > 0)).sum() >= 8 and (val[zero] == 0.0).all() and (ja[zero] == rows[zero]).all()
    k0, k1 = ia[0:n:64].astype(np.int64), ia[np.minimum(np.arange(64, n + 64, 64), n)].astype(np.int64)
    assert (k1 - k0)[:-1].min() > 5 * WS2_STEP and {0, 1, 7, 8, 9, 1100} <= set(lens.tolist())
    return c


# ------------------------------------------------------------------------------------------------------------------------------
# es_*: k_csr_estream<L, OP>
# ------------------------------------------------------------------------------------------------------------------------------
ES_LANES = {4: (1201, 110, 131), 8: (601, 150, 191), 16: (601, 280, 321), 32: (601, 570, 600)}     # L -> (rows, row lengths from .. to)


@functools.lru_cache(maxsize=None)
def es_case(L):
    """Square, mean row about 100, 180, 310, 580: k_csr_estream<4 | 8 | 16 | 32> (lanes by the mean: 128, 256, 512).  Built where the upload made
    16-bit columns (kind 0, at most 65536 columns), nnz >= 65536 and nnz >= 48 row.  Ten rows are empty, five hold one entry, row 300 holds 8000 entries
    -- several wave ranges of about 2400 .. 2800 (its columns repeat: it is longer than the matrix is wide; its diagonal is stored once).  L = 4: the rows
    500 .. 1099 hold 1 .. 3 entries, so that chunks touch more rows than the 127 whose pointers are staged (the second copy of the rows pass).  No row stores
    its diagonal twice (k_csr_estream takes the diagonal's product out of a full row sum)."""
    n, lo, hi = ES_LANES[L]
    rng = np.random.default_rng(9950 + L)
    lens = rng.integers(lo, hi, size=n).astype(np.int64)
    if L == 4:
        lens[500:1100] = rng.integers(1, 4, size=600)
    lens[[3, 77, 78, 150, 299, 301, 350, 351, 352, n - 1]] = 0
    lens[[5, 79, 200, 353, n - 2]] = 1
    lens[300] = 8000
    has, dp = _diag_policy(n, lens, rng)
    has[300] = True
    ia, ja, val, has, dp = assemble(n, n, lens, rng, has_diag=has, dpos=dp, free=(300,))
    zero, twice, offdup = diagonal_set(n, ia, ja, val, has, dp, rng, dup=False, skip=(300,))
    c = _finish(f"es_L{L}", n, n, ia, ja, val, OPS_SQUARE)
    tr, nnz = c["traits"], len(ja)
    avg = nnz / n
    assert tr["kind"] == 0 and c["sorted"] and tr["ja16"] == 1 and tr["jbase"] == 0 and tr["es_tab"] == 1 and tr["dup_diag"] == 0 and tr["dpos"] == 0
    assert nnz >= 65536 and nnz >= 48.0 * n and (4 if avg < 128 else 8 if avg < 256 else 16 if avg < 512 else 32) == L, avg
    assert 8000 >= 2.5 * nnz / tr["es_W"] and (np.diff(ia) == 0).sum() == 10 and (np.diff(ia) == 1).sum() >= 5
    if L == 4:
        assert ia[1100] - ia[500] > 2 * ES_CAP and (ia[500 + 128:1101] - ia[500:1101 - 128]).max() < 400     # chunks hold about 496 entries: more than any 128 rows there
    return c


# ------------------------------------------------------------------------------------------------------------------------------
# the runs: id, case builder and arguments, tune keys of the run, the kernel per (op, partials)
# ------------------------------------------------------------------------------------------------------------------------------
TUNE_RESTORE = dict(cc.TUNE_DEFAULTS, maxgrid=-1)
ORDER_KERNELS = ("lstream", "wstream2", "xtile") + KERNELS[6:10]      # sum every row left to right: bit-equal to the oracle


def _wname(wrows, wcap):
    return f"wstream_{wrows}_{wcap}"


def _runs():
    R = []
    SQUARE = tuple((op, op in (5, 7)) for op in OPS_SQUARE)       # the Jacobi sweep with the fused partials asked for
    BOTH = SQUARE + ((5, False),)                                 # ... and once more without: the kernels' paths with a.partials == nullptr
    RECT = tuple((op, op == 7) for op in OPS_RECT)

    def add(rid, fn, args, tune, kernel, other=None, ops=SQUARE):
        """kernel: the instantiation every operation must run on; other: {(op, partials): instantiation} where the plan says otherwise ("rows*":
        k_csr_rows with the lanes pick_kernel gave the matrix).  ops: (op, partials) pairs -- partials: the call asks for the fused sum."""
        R.append(dict(id=rid, fn=fn, args=tuple(args), tune=tuple(tune), kernel=kernel, other=dict(other or {}), ops=ops))

    geometry = [("default", ())] + [(f"maxgrid{g}", (("maxgrid", g),)) for g in (1, 2)] + [(f"split{k}", (("split_rows", k),)) for k in (1024, 3000)]
    # ls_*
    for t in TAILS:
        add(f"ls_t{t}", ls_main, (t,), (), "lstream", None, BOTH if t == 65 else SQUARE)
    for gname, tune in geometry[1:]:
        add(f"ls_{gname}", ls_main, (), tune, "lstream")
    add("ls_empty_ends", ls_main, (65, True), (), "lstream")
    add("ls_inf", ls_main, (65, False, True), (), "lstream", None, RECT)
    for n in LS_TINY:
        add(f"ls_tiny{n}", ls_tiny, (n,), (), "lstream")
    add("ls_nnz0", ls_empty, (), (), "lstream")
    # ws2_*
    for t in TAILS:
        add(f"ws2_t{t}", ws2_main, (t,), (), "wstream2", None, BOTH if t == 65 else SQUARE)
    for gname, tune in geometry[1:] + [("bpc1", (("ws2_bpc", 1),))]:
        add(f"ws2_{gname}", ws2_main, (), tune, "wstream2")
    jac8 = {(5, True): "rows*"}
    for gname, tune in (geometry[0], geometry[1], geometry[3]):
        add(f"ws2_dup_{gname}", ws2_main, (65, True), tune, "wstream2", jac8)
    # no diagonal positions on the device copy: the Jacobi sweep keeps k_csr_rows, everything else runs on k_csr_wstream2
    add("ws2_nodpos", ws2_nodpos, (), (("kind", 2),), "wstream2", {(5, True): "rows*", (5, False): "rows*"}, BOTH)
    # ws_*: gen2 = 0 (the diagonal twice in ls_main: its Jacobi sweep keeps k_csr_rows, lanes by its mean row)
    for wrows, wcap in ((64, 512), (64, 1024), (32, 512), (32, 1024)):
        tune = (("gen2", 0), ("wrows", wrows), ("wcap", wcap))
        add(f"ws_{wrows}_{wcap}_ls_main", ls_main, (), tune, _wname(wrows, wcap), jac8)
        add(f"ws_{wrows}_{wcap}_ws2_main", ws2_main, (), tune, _wname(wrows, wcap))
    add("ws_gen2_1_ws2_main", ws2_main, (), (("gen2", 1),), "wstream_64_512")
    add("ws_gen2_1_ls_main", ls_main, (), (("gen2", 1),), "lstream")
    # xt_*
    for t in TAILS:
        add(f"xt_t{t}", xt_main, (t,), (), "xtile", None, BOTH if t == 65 else SQUARE)
    add("xt_maxgrid1", xt_main, (), (("maxgrid", 1),), "xtile")
    add("xt_lists_off", xt_main, (), (("xtile", 0),), "wstream2")
    # rows_*
    for form in ROWS_FORMS:
        for L in ROWS_L:
            add(f"rows_{form}_L{L}", rows_case, (form,), (("lanes", L),) + ((("kind", 0),) if form == "f" else ()), f"rows{L}", None, SQUARE if form in "ef" else RECT)
    add("rows_b_ja16_off", rows_case, ("b",), (("ja16", 0),), "rows*", None, RECT)      # (the lanes of pick_kernel)
    add("rows_c_ja16_off", rows_case, ("c",), (("ja16", 0),), "rows*", None, RECT)
    # rect_stream
    add("rect_stream_ls", rect_stream, ("ls",), (("kind", 2),), "lstream", None, RECT)
    add("rect_stream_ws2", rect_stream, ("ws2",), (("kind", 2),), "wstream2", None, RECT)
    # es_*: estream = 2 (wherever the tables exist); op 7 and the Jacobi sweep with partials keep k_csr_rows (lanes by pick_kernel)
    es_ops = tuple((op, op == 7) for op in OPS_SQUARE) + ((5, True),)
    keep = {(7, True): "rows*", (5, True): "rows*"}
    for L in ES_LANES:
        add(f"es_L{L}", es_case, (L,), (("estream", 2),), f"estream{L}", keep, es_ops)
    # split_rows in force: every launch is PLANNED as a row window and keeps k_csr_rows (the 1201 rows are fewer than launch_csr splits: one launch)
    add("es_L4_planned_windowed", es_case, (4,), (("estream", 2), ("split_rows", 1024)), "rows*", None, es_ops)
    add("es_L8_rule_default", es_case, (8,), (), "estream8", keep, es_ops)     # estream = 1: nnz < 256 row
    return R


RUNS = _runs()


def build(run):
    return run["fn"](*run["args"])


def expect(run, op, partials):
    name = run["other"].get((op, partials), run["kernel"])
    return f"rows{build(run)['traits']['lanes']}" if name == "rows*" else name


def plan_tune(run):
    """The tune keys of a run that the plan reads (maxgrid is launch_persistent's)."""
    return {k: v for k, v in run["tune"] if k in cc.TUNE_DEFAULTS}


def all_cases():
    seen, out = set(), []
    for run in RUNS:
        key = (run["fn"].__name__, run["args"])
        if key not in seen:
            seen.add(key)
            out.append((build(run)["name"], run))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# np.longdouble evaluation of a row operation, with the terms and the rounded operations behind it
# ------------------------------------------------------------------------------------------------------------------------------
def longdouble_op(c, op, x, b, y0, scalar, diag_in_sum=False):
    """(exact, sabs, m) of row operation `op` in np.longdouble: the value, the absolute sum of every term that enters, the rounded operations
    behind an entry.  diag_in_sum: the Jacobi sweep of k_csr_estream, whose row sum takes EVERY entry and whose epilogue subtracts d x_i again:
    both products enter, two more operations.  (The derivation is in tests/test_gpu_plain_kernels.py.)"""
    from _libs import csr_mxv_longdouble
    ld = np.longdouble
    ia, ja, val, n = c["ia"], c["ja"], c["val"], c["nrow"]
    lens = np.diff(ia)
    if op == 5:
        rows = np.repeat(np.arange(n), lens)
        ond = ja == rows
        d = np.zeros(n)
        d[rows[ond]] = val[ond]                 # (the last one stored, as in the reference's loop)
        t, s, m = csr_mxv_longdouble(ia, ja, np.where(ond, 0.0, val), x)
        moff = m - np.bincount(rows[ond], minlength=n)
        live = np.abs(d) > 1e-20
        dd = np.where(live, d, 1.0).astype(ld)
        w, one_w = ld(scalar), ld(1 - scalar)   # (1 - w is rounded once in double: part of the expression)
        xl = x.astype(ld)
        exact = np.where(live, one_w * xl + w * (b.astype(ld) - t) / dd, xl)
        inner = np.abs(b).astype(ld) + s
        mm = moff + 5
        if diag_in_sum:
            inner = inner + 2 * np.abs(dd * xl)
            mm = m + 7
        return exact, np.abs(one_w * xl) + np.abs(w / dd) * inner, np.where(live, mm, 0)
    t, s, m = csr_mxv_longdouble(ia, ja, val, x)
    if op in (0, 7, 8):
        return t, s, m
    if op in (1, 2, 3, 4):
        alpha = {1: -1.0, 2: 1.0, 3: -1.0, 4: scalar}[op]
        v0 = (b if op == 1 else y0).astype(ld)
        return v0 + ld(alpha) * t, np.abs(v0) + abs(ld(alpha)) * s, np.where(m > 0, m + 2, 0)
    d = np.add.reduceat(np.abs(np.r_[val, 0.0]).astype(ld), np.minimum(ia[:-1], len(val)))
    d = np.where(lens > 0, d, 0.0)
    live = np.abs(d.astype(np.float64)) > 1e-20
    dd = np.where(live, d, 1.0)
    exact = np.where(live, x.astype(ld) + (b.astype(ld) - t) / dd, x.astype(ld))
    return exact, np.abs(x).astype(ld) + (np.abs(b).astype(ld) + s) / dd, np.where(live, 2 * m + 3, 0)
