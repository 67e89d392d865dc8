"""Irregular CSR matrices for the lossless coded kernels -- k_csr_rowpat4, k_csr_rowpat5 (csrc/kernels2.hip.h), k_csr_rowpat and
k_csr_dict8 (csrc/kernels.hip.h) -- built so that each reaches the paths a 7-point stencil never does, with the upload rules they
depend on restated in numpy and ASSERTED: a later edit of a generator (or of the rules) cannot quietly send a matrix to another kernel
or lose an edge.  The rules restated: upload_csr, build_rowpat, build_dict8, grid_plane_of (csrc/device_csr.hip.h), the tile schedule
tile_vmax / tile_of (csrc/kernels.hip.h) and the grid of launch_persistent.

Everything is vectorised over the entries; the only Python loops run over a palette's patterns or a handful of special rows.
Cases are built once per process (functools.lru_cache) and their arrays are read-only."""
import ctypes as C
import functools

import numpy as np

from faspsolver_amd import _types as T

BLOCK = 256            # threads of a workgroup; rows of a tile of k_csr_rowpat<., ., 1> and k_csr_dict8
PAIR_TILE = 2 * BLOCK  # rows of a tile of the pair sweeps (k_csr_rowpat4 / 5): four wave tiles of 128 rows
WAVE_ROWS = 128        # rows of a wave tile of the pair sweeps: lane i owns rows 2 i, 2 i + 1; its middle lane 32 owns row 64
RP_QCAP = 192          # per-wave queue of the pair sweeps (kernels2.hip.h)
DICT_CAP = 2048        # code bytes k_csr_dict8 stages per wave and step
KIND = {"dict8": 4, "rowpat": 5, "rowpat4": 6, "rowpat5": 9}
OPS = {"mxv": 0, "resid": 1, "add": 2, "sub": 3, "axpy": 4, "jacobi": 5, "l1diag": 6, "mxv_dot": 7, "mxv_zx": 8}
OPS_SQUARE = tuple(range(9))
OPS_RECT = (0, 1, 2, 3, 4, 7, 8)    # no smoother runs on a rectangular operator
SCALAR = {4: 0.7, 5: 0.6667, 6: 1.0, 8: 0.6667}


# ------------------------------------------------------------------------------------------------------------------------------
# a matrix from a palette of row patterns
# ------------------------------------------------------------------------------------------------------------------------------
def palette_csr(nrow, ncol, palette, assign, base=None):
    """CSR matrix whose row r carries pattern palette[assign[r]] = (offsets, values), in that storage order, at the columns
    base[r] + offset -- base = the row index (base None: the square form of build_rowpat / build_dict8) or the given per-row
    column, which must then be the row's first stored column (the rectangular form).  Entries whose column falls outside
    [0, ncol) are dropped: such a row gets a clipped pattern.  -> (ia, ja, val)"""
    lens = np.array([len(o) for o, _ in palette], dtype=np.int64)
    lmax = max(int(lens.max()), 1)
    OFF = np.zeros((len(palette), lmax), dtype=np.int64)
    VAL = np.zeros((len(palette), lmax))
    for p, (o, v) in enumerate(palette):
        assert len(o) == len(v)
        OFF[p, :len(o)] = o
        VAL[p, :len(o)] = v
    assign = np.asarray(assign, dtype=np.int64)
    assert assign.shape == (nrow,) and assign.min() >= 0 and assign.max() < len(palette)
    b = np.arange(nrow, dtype=np.int64) if base is None else np.asarray(base, dtype=np.int64)
    cols = b[:, None] + OFF[assign]
    keep = (np.arange(lmax)[None, :] < lens[assign][:, None]) & (cols >= 0) & (cols < ncol)
    if base is not None:   # the base of a rectangular row IS its first stored column: it must survive, with offset 0
        first = lens[assign] > 0
        assert np.all(keep[first, 0]) and np.all(OFF[assign][first, 0] == 0)
    ia = np.zeros(nrow + 1, dtype=np.int32)
    ia[1:] = np.cumsum(keep.sum(axis=1))
    return ia, cols[keep].astype(np.int32), VAL[assign][keep]


# ------------------------------------------------------------------------------------------------------------------------------
# the upload rules, restated
# ------------------------------------------------------------------------------------------------------------------------------
def _bases(ia, ja, nrow, ncol):
    lens = np.diff(ia).astype(np.int64)
    if nrow == ncol:
        return lens, np.arange(nrow, dtype=np.int64)
    first = ja[np.minimum(ia[:-1], max(len(ja) - 1, 0))].astype(np.int64) if len(ja) else np.zeros(nrow, dtype=np.int64)
    return lens, np.where(lens > 0, first, 0)


def coding(ia, ja, val, ncol):
    """What upload_csr makes of a matrix -> dict(kind = 5 row patterns / 4 byte dictionary / 0 plain, why = the rule that refused
    the row patterns (None: coded), pat = pattern id per row numbered by first occurrence, plen = true length per pattern, npat,
    npent = padded table entries, npairs = distinct (offset, value) pairs or None when not counted)."""
    nrow, nnz = len(ia) - 1, len(ja)
    out = dict(kind=0, why=None, pat=None, plen=None, npat=0, npent=0, npairs=None)
    if not (nnz >= 4096 and nnz <= 48 * nrow):
        out["why"] = "nnz >= 4096 and nnz <= 48 * row"
        return out
    lens, base = _bases(ia, ja, nrow, ncol)
    rows = np.repeat(np.arange(nrow), lens)
    pos = np.arange(nnz) - np.repeat(ia[:-1].astype(np.int64), lens)
    off = ja.astype(np.int64) - base[rows]
    bits = np.ascontiguousarray(val).view(np.int64)
    lmax = int(lens.max())
    key = np.full((nrow, 1 + 2 * lmax), np.iinfo(np.int64).min, dtype=np.int64)
    key[:, 0] = lens
    key[rows, 1 + pos] = off
    key[rows, 1 + lmax + pos] = bits
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")            # ids by first occurrence, as build_rowpat numbers them
    rank = np.empty(len(first), dtype=np.int64)
    rank[order] = np.arange(len(first))
    pat = rank[np.asarray(inv).reshape(-1)]
    plen = lens[first[order]]
    npat, tot = len(first), int(((plen + 7) // 8 * 8).sum())
    why = None
    if ncol >= 1 << 28: why = "col < 2^28"
    elif npat > min(65535, nrow // 8) or npat * 8 > nrow: why = "patterns * 8 <= row"
    elif tot > 1 << 20: why = "padded table entries <= 2^20"
    elif tot * 4 > nnz: why = "padded table entries * 4 <= nnz"
    if why is None:
        out.update(kind=5, pat=pat, plen=plen, npat=npat, npent=tot)
        return out
    out["why"] = why
    pairs = np.unique(np.stack([off, bits], axis=1), axis=0)
    out["npairs"] = len(pairs)
    if len(pairs) <= 256:
        out["kind"] = 4
    return out


def off_pattern(pat, nrow, square):
    """The rule of upload_csr, "k_csr_rowpat4 / k_csr_rowpat5: the sweep computes the row pairs ...": the pairs (2 i, 2 i + 1) whose
    rows carry the pattern (square) or the pair of patterns (rectangular) of the middle pair of their 128-row wave tile -- the pair
    of row 128 w + 64, clamped to the last pair -- are swept; every other row is off-pattern.  -> (nx, swept: bool per pair)"""
    npair = (nrow + 1) // 2
    w0 = np.arange(0, nrow, WAVE_ROWS)
    pm = np.minimum((w0 + 64) // 2, npair - 1)
    domA = pat[2 * pm]
    domB = domA if square else np.where(2 * pm + 1 < nrow, pat[np.minimum(2 * pm + 1, nrow - 1)], 0xffff)
    r = np.arange(0, nrow, 2)
    vb = r + 1 < nrow
    t = r // WAVE_ROWS
    swept = vb & (pat[r] == domA[t]) & (pat[np.minimum(r + 1, nrow - 1)] == domB[t])
    return int(np.where(swept, 0, np.where(vb, 2, 1)).sum()), swept


def family(cd, nrow, ncol, nnz):
    """Kernel family code of a freshly uploaded matrix under the default tune keys (kernel_family, csrc/device_csr.hip.h)."""
    if cd["kind"] != 5:
        return cd["kind"]
    nx, _ = off_pattern(cd["pat"], nrow, nrow == ncol)
    if nx * 4 > nrow:
        return 5
    if nrow == ncol:
        return 6
    return 9 if nnz <= 4.5 * nrow else 5


# ------------------------------------------------------------------------------------------------------------------------------
# the kernel plan of a launch, restated
# ------------------------------------------------------------------------------------------------------------------------------
# the traits of fasp_hip_csr_plan (include/fasp_hip_dev.h), in its order: sizes, then 0 / 1 per pointer
TRAITS = ("row", "col", "nnz", "kind", "lanes", "wrows", "wcap", "nxrows", "plane", "npat", "npent", "sell_nv", "sell_nslice", "sell_slots",
          "ntcols", "es_W", "es_nc", "code", "pat", "rowbase", "dpos", "dup_diag", "ja16", "jbase", "lja16", "sell_code", "es_tab", "es_ja16")
TRAIT_DEFAULTS = dict(dict.fromkeys(TRAITS, 0), lanes=8, wrows=64, wcap=512, nxrows=-1)     # a DevCSR as constructed
# CsrKernel (csrc/device_csr.hip.h), in its order
KERNELS = ("rows2", "rows4", "rows8", "rows16", "rows32", "rows64", "wstream_64_512", "wstream_64_1024", "wstream_32_512", "wstream_32_1024",
           "rowpat_0_1", "rowpat_0_2", "rowpat_1_1", "rowpat_1_2", "rowpat_2_1", "rowpat_2_2", "dict8_8", "dict8_16", "dict8_24",
           "estream4", "estream8", "estream16", "estream32", "rowpat4", "rowpat5", "lstream", "xtile", "sell", "wstream2")
PLAN = ("kernel", "family", "tile_rows", "bpc", "xcd_map", "tpp", "nt", "ja16", "jbase", "fused_zr")     # the ints fasp_hip_csr_plan writes
# the tune keys the plan reads, with their defaults (struct Tuning)
TUNE_DEFAULTS = dict(gen2=2, ws2_bpc=3, xcd=16, nt=1, kind=-1, lanes=-1, wrows=-1, wcap=-1, compress=1, rpl=-1, lds_tab=1, xcd_pat=64, ja16=1,
                     split_rows=0, xtile=1, rp5_max=45, rp_bpc=5, rp_xcd=-1, rp_strip=2, rp_stream=-1, estream=1, sell=1)
OP_JACOBI, OP_L1DIAG, OP_MXV_DOT = 5, 6, 7
SELL_BLOCK = 1024


def expected_plan(t, op, windowed, want_partials, tune=None):
    """The launch that launch_csr<op> of the commit BEFORE plan_csr existed (b70c478) made of an operator with the traits t, walked the
    way that function walked: one `if` after the other, in its order, with its line of csrc/device_csr.hip.h beside each.  windowed: a
    row window of all rows (win.hi >= 0).  -> dict of PLAN + bytes (the count its kernel_family gave the family, :1158-1173)."""
    g = dict(TUNE_DEFAULTS, **(tune or {}))
    M = dict(t)
    row, nnz = M["row"], M["nnz"]
    a = {}

    def tiles(rpb):                                                                       # :1281 set_tiles
        a["tile_rows"], a["ntiles"] = rpb, (row + rpb - 1) // rpb

    def strips(rpb):                                                                      # :1294
        if not g["rp_strip"] or M["plane"] < 8 * rpb or M["plane"] % (8 * rpb) != 0 or a["ntiles"] < 4 * (M["plane"] // rpb):
            return
        a["xcd_map"], a["tpp"] = -2, M["plane"] // rpb

    def done(kernel, fam, bpc=0, fused=False):
        base = 4.0 * row if M["rowbase"] else 0.0
        if fam in (5, 6, 9): nbytes = 2.0 * row + base + 12.0 * M["npent"]                # :1161
        elif fam == 4: nbytes = 1.0 * nnz + 4.0 * (row + 1.0) + base                      # :1160
        elif fam == 10: nbytes = 10.0 * nnz + 4.0 * (row + 1.0) + 4.0 * M["ntcols"] + 4.0 * ((row + 63) // 64 + 1.0)      # :1169
        elif fam == 11: nbytes = 4.0 * M["sell_slots"] + 1.0 * row + 4.0 * (2.0 * M["sell_nslice"] + 1.0) + 8.0 * M["sell_nv"]   # :1173
        elif fam == 0 and a["ja16"]: nbytes = 10.0 * nnz + 4.0 * (row + 1.0) + (4.0 * row if a["jbase"] else 0.0)   # :1159
        else: nbytes = 12.0 * nnz + 4.0 * (row + 1.0)                                     # :1158
        return dict(kernel=KERNELS.index(kernel), family=fam, tile_rows=a["tile_rows"], bpc=bpc, xcd_map=a["xcd_map"], tpp=a.get("tpp", 0),
                    nt=a["nt"], ja16=int(a["ja16"]), jbase=int(a["jbase"]), fused_zr=int(fused), bytes=nbytes)

    windowed = windowed or g["split_rows"] > 0                                            # :1409 (win.hi < 0 && g_tune.split_rows <= 0)
    if M["code"] and g["compress"]: M["kind"] = 4                                         # :1299
    if M["pat"] and g["compress"]: M["kind"] = 5                                          # :1300
    if g["kind"] >= 0 and not (g["kind"] == 4 and not M["code"]) and not (g["kind"] == 5 and not M["pat"]): M["kind"] = g["kind"]   # :1301
    if g["lanes"] > 0: M["lanes"] = g["lanes"]                                            # :1302
    if g["wrows"] > 0: M["wrows"] = g["wrows"]                                            # :1303
    if g["wcap"] > 0: M["wcap"] = g["wcap"]                                               # :1304
    w64 = M["wrows"] == 64 and M["wcap"] == 512
    lstream_ok = bool(g["gen2"]) and M["kind"] == 2 and w64 and nnz <= 7.6 * row           # :1305
    if op == OP_JACOBI and M["kind"] != 0 and M["kind"] < 4 and (M["dup_diag"] or not M["dpos"]) and not lstream_ok: M["kind"] = 0   # :1306
    a["xcd_map"] = g["xcd"]                                                               # :1307
    a["nt"] = g["nt"]                                                                     # :1308
    if g["rp_stream"] > 0 or (g["rp_stream"] < 0 and row * 8 > 96 << 20): a["nt"] |= 4    # :1311
    a["ja16"] = bool(g["ja16"] and M["ja16"])                                             # :1313
    a["jbase"] = bool(g["ja16"] and M["jbase"])                                           # :1314
    if M["jbase"] and M["kind"] != 0: a["ja16"] = a["jbase"] = False                      # :1315
    if M["kind"] in (1, 3): M["kind"] = 0                                                 # :1316
    tiles(BLOCK if M["kind"] >= 4 else 4 * M["wrows"] if M["kind"] == 2 else BLOCK // M["lanes"])     # :1317
    jac_fused = op == OP_JACOBI and want_partials
    diag_ok = op != OP_JACOBI or (M["dpos"] and not M["dup_diag"])
    if M["kind"] == 5 and g["gen2"] and M["nxrows"] >= 0 and not M["rowbase"] and g["rpl"] <= 0:      # :1319
        tiles(2 * BLOCK)                                                                  # :1323
        a["xcd_map"] = g["rp_xcd"] if a["ntiles"] >= 8 * 64 else 16                       # :1324
        if a["xcd_map"] == -1: strips(2 * BLOCK)                                          # :1326
        return done("rowpat4", 6, 3 if a["xcd_map"] == -2 and g["rp_bpc"] == 5 else g["rp_bpc"], jac_fused)      # :1327, :1330
    if (M["kind"] == 5 and g["gen2"] >= 2 and M["nxrows"] >= 0 and M["rowbase"] and g["rpl"] <= 0 and op not in (OP_JACOBI, OP_L1DIAG)
            and nnz <= 0.1 * g["rp5_max"] * row):                                         # :1334
        tiles(2 * BLOCK)                                                                  # :1339
        a["xcd_map"] = -1 if a["ntiles"] >= 8 * 64 else 16                                # :1340
        if g["rp_strip"] >= 2: strips(2 * BLOCK)                                          # :1341
        return done("rowpat5", 9, 5)                                                      # :1342, :1214
    if M["kind"] == 5:                                                                    # :1344
        lds = M["npat"] <= 512 and M["npent"] <= 2048 and g["lds_tab"] != 0               # :1348
        rpl = g["rpl"] if g["rpl"] > 0 else 1                                             # :1349
        if g["xcd_pat"] != 0: a["xcd_map"] = g["xcd_pat"]                                 # :1351
        tiles(BLOCK * rpl)                                                                # :1352
        if g["xcd_pat"] == 64 and g["rp_strip"] >= 2: strips(BLOCK * rpl)                 # :1353
        R = 1 if rpl == 1 else 2
        if lds and M["npat"] <= 64 and M["npent"] <= 512 and g["lds_tab"] != 3: return done(f"rowpat_2_{R}", 5)     # :1355
        if lds: return done(f"rowpat_1_{R}", 5)                                           # :1359
        return done(f"rowpat_0_{R}", 5)                                                   # :1363
    if M["kind"] == 4:                                                                    # :1366
        avg = nnz / row if row > 0 else 1.0
        return done("dict8_8" if avg <= 8.5 else "dict8_16" if avg <= 20.0 else "dict8_24", 4)     # :1369
    if M["kind"] == 2 and g["gen2"] and w64 and nnz <= 7.6 * row:                         # :1373
        return done("lstream", 7, 4, jac_fused)
    if M["kind"] == 2 and g["gen2"] >= 2 and g["xtile"] and M["lja16"] and w64 and diag_ok:       # :1378
        return done("xtile", 10, 3, jac_fused)
    sell_active = M["sell_code"] and g["compress"] and g["sell"] and g["gen2"] >= 2 and not (g["xtile"] and M["lja16"])   # :1150
    if M["kind"] == 2 and sell_active and w64 and diag_ok:                                # :1385
        tiles(SELL_BLOCK)                                                                 # :1388
        return done("sell", 11, 0, jac_fused)
    if M["kind"] == 2 and g["gen2"] >= 2 and w64 and diag_ok:                             # :1392
        return done("wstream2", 8, g["ws2_bpc"], jac_fused)
    if M["kind"] == 2:                                                                    # :1397
        return done("wstream_64_512" if w64 else "wstream_64_1024" if M["wrows"] == 64 else
                    "wstream_32_512" if M["wrows"] == 32 and M["wcap"] == 512 else "wstream_32_1024", 2)
    es_rule = g["estream"] >= 2 or (g["estream"] == 1 and nnz < 256.0 * row)              # :1408
    if (M["es_tab"] and es_rule and a["ja16"] and not windowed and op != OP_MXV_DOT
            and not (op == OP_JACOBI and (want_partials or M["dup_diag"]))):              # :1409
        avg = nnz / row if row > 0 else 1.0
        return done("estream32" if avg >= 512.0 else "estream16" if avg >= 256.0 else "estream8" if avg >= 128.0 else "estream4", 0)   # :1416
    return done(f"rows{M['lanes']}" if M["lanes"] in (2, 4, 8, 16, 32) else "rows64", 0)  # :1441


def fresh_traits(cd, nrow, ncol, nnz):
    """The traits the plan reads of a freshly uploaded matrix with the coding cd (upload_csr; the 16-bit copies and the k_csr_estream,
    k_csr_xtile and k_csr_sell forms belong to uncoded operators)."""
    t = dict(TRAIT_DEFAULTS, row=nrow, col=ncol, nnz=nnz, kind=2 if nnz <= 48.0 * nrow else 0, rowbase=int(nrow != ncol), dpos=int(nrow == ncol))
    if cd["kind"] == 5:
        nx, _ = off_pattern(cd["pat"], nrow, nrow == ncol)
        t.update(pat=1, npat=cd["npat"], npent=cd["npent"], nxrows=nx if nx * 4 <= nrow else -1)
    elif cd["kind"] == 4:
        t.update(code=1)
    return t


def grid_plane(poff, nrow):
    """grid_plane_of: the row distance the XCD strips of a square pattern-coded operator are cut along (0: none)."""
    unit = 8 * PAIR_TILE
    poff = np.asarray(poff, dtype=np.int64)
    cand = []
    for o in poff:
        c = (abs(int(o)) + unit // 2) // unit * unit
        if unit <= c <= nrow // 4 and c not in cand and len(cand) < 64:
            cand.append(c)
    best, best_cost = 0, 0.2
    for P in cand:
        r = np.fmod(poff, P)                      # C's %: the sign of the dividend
        r = np.where(r > P // 2, r - P, r)
        r = np.where(r < -(P // 2), r + P, r)
        cost = float(np.mean(np.minimum(np.abs(r), P // 8) / (P // 8)))
        if cost < best_cost or (cost == best_cost and P > best):
            best, best_cost = P, cost
    return best


def persistent_grid(maxgrid, ntiles):
    """launch_persistent with fasp_hip_tune("maxgrid", g > 0): min(g, tiles), rounded up to a multiple of 8, at least 8."""
    g = min(min(maxgrid, 2048), ntiles)
    return max(8, (g + 7) // 8 * 8)


def block_tiles(ntiles, grid, block, xcd_map=16):
    """tile_vmax / tile_of for xcd_map = G > 0: the tiles workgroup `block` of `grid` takes, in its order."""
    G = xcd_map
    span = 8 * G
    vmax = (ntiles + span - 1) // span * span
    v = np.arange(block, vmax, grid)
    q = v >> 3
    t = ((q // G) * 8 + (v & 7)) * G + q % G
    return t[t < ntiles]


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _finish(name, nrow, ncol, ia, ja, val, kind, ops, **extra):
    """Checks the kernel family a case is built for against the restated rules and packs it."""
    nnz = len(ja)
    assert ia[0] == 0 and ia[-1] == nnz and len(ia) == nrow + 1 and len(val) == nnz
    assert nnz == 0 or (ja.min() >= 0 and ja.max() < ncol)
    cd = coding(ia, ja, val, ncol)
    fam = family(cd, nrow, ncol, nnz)
    assert fam == kind, (name, fam, kind, cd["why"], cd["npat"], cd["npairs"])
    c = dict(name=name, nrow=nrow, ncol=ncol, ia=ia, ja=ja, val=val, kind=kind, ops=tuple(ops), coding=cd, inf_rows=None)
    c.update(extra)
    return _freeze(c)


P4_INTERIOR = ([0, -64, -1, 1, 64], [6.0, -1.0, -1.25, -0.75, -1.5])
P4_OTHER = ([0, 5, -3], [3.0, 0.5, -0.25])


def _p4_assign(n, period=37):
    a = np.zeros(n, dtype=np.int64)
    a[::period] = 1
    return a


def _swept_share(c):
    nx, swept = off_pattern(c["coding"]["pat"], c["nrow"], c["nrow"] == c["ncol"])
    return nx, swept


@functools.lru_cache(maxsize=None)
def p4_main(n=8193):
    """Square, k_csr_rowpat4.  Interior offsets {0, -64, -1, 1, 64}; every 37th row carries a 3-entry pattern, so pairs split both
    ways (row A in the wave's pattern and row B not, and the reverse); wave tile 18 has its MIDDLE row (2368 = 37 * 64) off the
    interior pattern, so the 3-entry pattern is that wave's and all its 64 pairs are queued; the rows within 64 of either end
    carry clipped patterns.  n = 8192 + t: an odd last row and a last wave tile shorter than 65 rows (the clamp of the middle pair)."""
    ia, ja, val = palette_csr(n, n, [P4_INTERIOR, P4_OTHER], _p4_assign(n))
    c = _finish(f"p4_n{n}", n, n, ia, ja, val, KIND["rowpat4"], OPS_SQUARE)
    pat = c["coding"]["pat"]
    nx, swept = _swept_share(c)
    assert nx * 4 <= n
    r = np.arange(0, n - 1, 2)
    dom = pat[200]                                          # the interior pattern
    assert pat[201] == dom and pat[37 * 6] != dom
    assert np.any((pat[r] == dom) & (pat[r + 1] != dom)) and np.any((pat[r] != dom) & (pat[r + 1] == dom))
    if n > 18 * WAVE_ROWS + 64 + 64:
        assert (18 * WAVE_ROWS + 64) % 37 == 0 and pat[18 * WAVE_ROWS + 64] == pat[37 * 6]
        assert not swept[18 * 64:19 * 64].any()             # the whole wave tile goes through the queue: 128 rows, two drains
    return c


P4_TAILS = (0, 1, 2, 63, 64, 65, 127)


def p4_tail(t):
    c = p4_main(8192 + t)
    n = c["nrow"]
    assert (n % 2 == 1) == (t % 2 == 1)
    assert n - (n - 1) // WAVE_ROWS * WAVE_ROWS == (t or WAVE_ROWS)     # rows of the last wave tile: 1, 2, 63, 64 are shorter than 65
    return c


P4_LENGTHS = (0, 1, 7, 8, 9, 16, 17)


@functools.lru_cache(maxsize=None)
def p4_length(L):
    """Square, k_csr_rowpat4, the wave's pattern has L entries: every remainder of the `switch (min(dlen - k, 8))` but 7 that a
    stencil never has (1; 8 = no remainder; 9 and 17 = a remainder of 1 behind full chunks; 16) and 7 itself.  L = 0: the swept
    rows are EMPTY (the `dlen == 0` flush); a quarter of the rows, in whole pairs away from the wave tiles' middle pairs, carry
    the 3-entry pattern."""
    if L == 0:
        n = 8192
        a = np.zeros(n, dtype=np.int64)
        r = np.arange(n)
        a[(r % 8) >= 6] = 1                                  # pairs (8 j + 6, 8 j + 7): never a middle pair (64 = 8 * 8)
        ia, ja, val = palette_csr(n, n, [([], []), ([0, 2, -2], [3.0, 0.5, -0.25])], a)
        c = _finish("p4_len0", n, n, ia, ja, val, KIND["rowpat4"], OPS_SQUARE)
        nx, swept = _swept_share(c)
        assert nx * 4 <= n and nx >= n // 4 - 8 and c["coding"]["plen"][c["coding"]["pat"][64]] == 0
        return c
    n = 8193
    offs = [0] + [s * k for k in range(1, 9) for s in (-1, 1)]          # 0, -1, 1, -2, 2, ...
    vals = [9.0] + [-(0.5 + 0.03125 * k) for k in range(16)]
    ia, ja, val = palette_csr(n, n, [(offs[:L], vals[:L]), ([0, 12, -11], [3.0, 0.5, -0.25])], _p4_assign(n))
    c = _finish(f"p4_len{L}", n, n, ia, ja, val, KIND["rowpat4"], OPS_SQUARE)
    nx, _ = _swept_share(c)
    assert nx * 4 <= n and c["coding"]["plen"][c["coding"]["pat"][64]] == L
    return c


@functools.lru_cache(maxsize=None)
def p4_queue():
    """Square, k_csr_rowpat4, the per-wave queue at its capacity.  Run with fasp_hip_tune("maxgrid", 1 | 2): launch_persistent rounds
    either up to 8 workgroups, of which workgroup 0 takes the tiles 0 .. 15 in order (xcd_map 16), so wave 1 of workgroup 0 sweeps the
    rows 128 .. 255 and then 640 .. 767.  The first of these wave tiles has exactly 31 off-pattern pairs (62 rows stay queued: fewer than
    a drain takes), the second alternates two patterns, so none of its 64 pairs is the wave's: 62 left over + 128 pushed = 190 of the
    192 slots, then two drains."""
    n = 16384
    a = np.zeros(n, dtype=np.int64)
    a[128:128 + 62:2] = 1                                    # 31 pairs (off, interior); the middle pair (192, 193) stays interior
    a[640:768:2] = 1                                         # (off, interior) x 64: the middle row 704 carries the other pattern
    ia, ja, val = palette_csr(n, n, [P4_INTERIOR, P4_OTHER], a)
    c = _finish("p4_queue", n, n, ia, ja, val, KIND["rowpat4"], OPS_SQUARE)
    nx, swept = _swept_share(c)
    ntiles = (n + PAIR_TILE - 1) // PAIR_TILE
    for g in (1, 2):
        grid = persistent_grid(g, ntiles)
        assert grid == 8 and ntiles < 8 * 64                 # (fewer than 512 tiles: xcd_map 16, no slabs or strips)
        assert list(block_tiles(ntiles, grid, 0)[:2]) == [0, 1]
    w0, w1 = 128 // 2, 640 // 2                              # first pairs of the two wave tiles
    assert (~swept[w0:w0 + 64]).sum() == 31 and (~swept[w1:w1 + 64]).sum() == 64
    assert swept[:64].sum() < 64                             # (wave 0 starts with the clipped rows: why wave 1 is the one)
    assert 2 * 31 < 64 and 2 * 31 + 128 <= RP_QCAP
    return c


def _diag_palette():
    return {
        "diag_not_first": ([-1, 0, 1, 64, -64], [-1.0, 6.0, -0.75, -1.5, -1.25]),
        "diag_absent":    ([-1, 1, 64], [-1.0, -0.75, -1.5]),
        "diag_zero":      ([0, -1, 1], [0.0, -1.0, -0.75]),
        "diag_tiny":      ([0, -1, 1, 2], [1e-21, -1.0, -0.75, 0.5]),
        "diag_twice":     ([0, 1, 0, -1], [2.0, -0.75, 3.0, -1.0]),
        "minus_zero":     ([0, 1, -1, 3, -64], [4.0, -0.0, -0.0, 0.25, -0.0]),
        "empty":          ([], []),
    }


P4_DIAGONALS = ("diag_not_first", "diag_absent", "diag_zero", "diag_tiny", "diag_twice", "minus_zero")


@functools.lru_cache(maxsize=None)
def p4_diagonal(which):
    """Square, k_csr_rowpat4, one odd pattern as the waves' pattern (the sweep's own diagonal handling) and the others -- with an
    EMPTY row, which can only ever be off-pattern here -- on every 41st row (the queued rows' handling): the diagonal not stored first,
    absent, stored as 0.0, stored as 1e-21 (below the 1e-20 guard), stored twice (the last one counts), values that are -0.0."""
    n = 8193
    pal = _diag_palette()
    names = [which] + [k for k in pal if k != which]
    a = np.zeros(n, dtype=np.int64)
    sp = np.arange(41, n, 41)
    a[sp] = 1 + np.arange(len(sp)) % (len(names) - 1)
    ia, ja, val = palette_csr(n, n, [pal[k] for k in names], a)
    c = _finish(f"p4_{which}", n, n, ia, ja, val, KIND["rowpat4"], OPS_SQUARE)
    nx, _ = _swept_share(c)
    assert nx * 4 <= n
    lens = np.diff(ia)
    rows = np.repeat(np.arange(n), lens)
    ond = ja == rows
    ndiag = np.bincount(rows[ond], minlength=n)
    r = 4096                                                  # an interior row of the waves' pattern
    assert a[r] == 0 and a[r + 1] == 0
    if which == "diag_not_first": assert ja[ia[r]] != r and ndiag[r] == 1
    if which == "diag_absent": assert ndiag[r] == 0
    if which == "diag_zero": assert val[ia[r]] == 0.0 and ja[ia[r]] == r
    if which == "diag_tiny": assert 0.0 < val[ia[r]] < 1e-20 and ja[ia[r]] == r
    if which == "diag_twice": assert ndiag[r] == 2
    if which == "minus_zero": assert np.signbit(val[ia[r]:ia[r + 1]]).sum() == 3 and (val[ia[r]:ia[r + 1]] == 0.0).sum() == 3
    assert (lens == 0).sum() >= 10 and (ndiag == 2).any() and (ndiag == 0).any()     # the sprinkled ones are there
    return c


@functools.lru_cache(maxsize=None)
def p4_padding():
    """Square, k_csr_rowpat4 (and, under fasp_hip_tune("rpl", 1), k_csr_rowpat).  The rows S whose pattern has no offset-0 entry and a
    length that is no multiple of 8 -- their padding entries (offset 0, value 0) gather x[r] -- get x[r] = inf, and no row references a
    column of S: a padding entry that enters a sum makes it NaN.  S = two whole wave tiles (5 and 20: the pattern is the wave's, the
    sweep's padding behind a remainder of 3 and of 7) whose entries lie 4096 .. 4700 rows ahead, and the rows = 7 (mod 16) below 4000 outside them (queued rows);
    every other row references rows of its own residue mod 16 only, and the rows within 32 of the two tiles just themselves."""
    n = 8192
    r = np.arange(n)
    pal = [([0, -16, 16, -32, 32], [6.0, -1.0, -1.25, -0.75, -1.5]),     # 0 interior
           ([0], [2.5]),                                                  # 1 beside the S tiles
           ([1, -2, 3], [0.5, -0.25, 0.125]),                             # 2 S, sprinkled: residues 8, 5, 10
           ([4200, 4300, 4096], [0.5, -0.25, 0.125]),                     # 3 S, whole tiles: into the upper half
           ([-3, 0, 16, 1, -2], [0.5, 4.0, -1.0, 0.25, 0.125]),           # 4 five entries WITH the diagonal, residue 3: padding of a row that is not in S
           ([4200, 4300, 4096, 4400, 4500, 4600, 4700], [0.5, -0.25, 0.125, 1.5, -0.75, 0.375, 2.0])]   # 5 S, whole tile, SEVEN entries: the remainder a stencil has
    a = np.zeros(n, dtype=np.int64)
    a[(r % 16 == 7) & (r < 4000)] = 2
    a[(r % 16 == 7) & (r >= 4000) & (r < 4064)] = 1            # (the next rows of that residue would read them)
    a[(r % 16 == 3) & (r >= 4200)] = 4
    for t in (5, 20):
        lo, hi = t * WAVE_ROWS, (t + 1) * WAVE_ROWS
        a[max(lo - 32, 0):hi + 32] = 1
        a[lo:hi] = 3 if t == 5 else 5
    ia, ja, val = palette_csr(n, n, pal, a)
    c = _finish("p4_padding", n, n, ia, ja, val, KIND["rowpat4"], OPS_RECT)
    lens = np.diff(ia)
    rows = np.repeat(r, lens)
    has0 = np.bincount(rows[ja == rows], minlength=n) > 0
    S = ~has0 & (lens % 8 != 0)
    assert S.sum() > 256 + 200 and not S[ja].any()            # nobody reads an inf
    nx, swept = _swept_share(c)
    assert nx * 4 <= n
    for t in (5, 20):
        assert swept[t * 64:(t + 1) * 64].all() and S[t * WAVE_ROWS:(t + 1) * WAVE_ROWS].all()     # S swept as a wave's pattern ...
    assert lens[5 * WAVE_ROWS] == 3 and lens[20 * WAVE_ROWS] == 7
    assert ((S[::2] | S[1::2])[~swept]).any()                                                    # ... and S among the queued rows
    c = dict(c)
    c["inf_rows"] = S
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def p4_strips():
    """Square, k_csr_rowpat4 with its XCD strip map: 66 planes of 4096 rows + 1537 rows, offsets {0, +-1, +-64, +-4096} -- at least
    512 tiles, so the slab / strip maps engage (launch_csr: ntiles >= 8 * 64), grid plane 4096, a partial last plane, odd n."""
    n = 66 * 4096 + 1537
    ia, ja, val = palette_csr(n, n, [([0, -1, 1, -64, 64, -4096, 4096], [6.0, -1.0, -0.75, -1.25, -1.5, -0.5, -0.625])], np.zeros(n, dtype=np.int64))
    c = _finish("p4_strips", n, n, ia, ja, val, KIND["rowpat4"], (0, 1, 5))
    ntiles = (n + PAIR_TILE - 1) // PAIR_TILE
    lens, base = _bases(ia, ja, n, n)
    # the table of build_rowpat: every pattern's offsets (padding offsets are 0 and cost nothing)
    cd = c["coding"]
    firsts = np.unique(cd["pat"], return_index=True)[1]
    poff = np.concatenate([ja[ia[f]:ia[f + 1]].astype(np.int64) - f for f in firsts] + [np.zeros(int(cd["npent"] - cd["plen"].sum()), dtype=np.int64)])
    plane = grid_plane(poff, n)
    assert ntiles >= 512 and plane == 4096 and plane % (8 * PAIR_TILE) == 0 and ntiles >= 4 * (plane // PAIR_TILE)
    assert n % 2 == 1 and n % 4096 != 0
    nx, _ = _swept_share(c)
    assert nx * 4 <= n
    return c


P5_TAILS = (0, 1, 65)


@functools.lru_cache(maxsize=None)
def p5(t, long_rows=False):
    """Rectangular (ncol = 3 nrow + 8), k_csr_rowpat5: rows alternate a 1-entry pattern and a 4-entry pattern whose first stored column
    is not its smallest (negative offsets from the row base); the wave tiles 3, 7 and 40 have the alternation flipped (their middle pair
    says so: they are swept like the others); a few rows are empty (their pairs are queued; the row base of an empty row is 0).
    nrow = 8192 + t: t = 1 an odd last row alone in its wave tile, t = 65 a last wave tile whose middle pair is the last row and the
    0xffff pad -- no pair of that tile is swept.  long_rows: the second pattern has 11 entries, the mean row 6: beyond what
    k_csr_rowpat5 takes (nnz <= 4.5 row), so k_csr_rowpat with its per-row bases runs."""
    nrow = 8192 + t
    ncol = 3 * nrow + 8
    r = np.arange(nrow)
    if long_rows:
        second = ([0, -2, 1, -1, 3, 2, 5, -3, 4, 6, -4], [0.5, 0.25, -0.125, 0.375, 1.5, -1.0, 0.75, -0.625, 0.0625, 2.0, -0.3125])
    else:
        second = ([0, -2, 1, -1], [0.5, 0.25, -0.125, 0.375])
    pal = [([0], [1.0]), second, ([], [])]
    flipped = np.isin(r // WAVE_ROWS, (3, 7, 40))
    a = ((r % 2) ^ flipped).astype(np.int64)
    empty = np.array([10, 11, 700, 3001, 5555, 8000])
    a[empty] = 2
    base = 3 * r + 4
    ia, ja, val = palette_csr(nrow, ncol, pal, a, base=base)
    kind = KIND["rowpat"] if long_rows else KIND["rowpat5"]
    c = _finish(f"p5_t{t}" + ("_long" if long_rows else ""), nrow, ncol, ia, ja, val, kind, OPS_RECT)
    lens = np.diff(ia)
    nnz = len(ja)
    assert (nnz <= 4.5 * nrow) == (not long_rows) and (not long_rows or 5.5 <= nnz / nrow <= 6.5)
    k = ia[1]                                                  # row 1 (or 0 in a flipped tile: tile 0 is not) carries the long pattern
    assert lens[1] == len(second[0]) and ja[k] > ja[k:ia[2]].min()
    nx, swept = off_pattern(c["coding"]["pat"], nrow, False)
    assert nx * 4 <= nrow
    assert swept[3 * 64:4 * 64].all() and swept[64:128].all() and not swept[5].any() and (lens == 0).sum() == len(empty)
    if t == 65:
        assert not swept[8192 // 2:].any() and len(swept) - 8192 // 2 == 33
    if t == 1:
        assert not swept[-1]
    return c


RP_PALETTES = {"pal8": 2, "pal200": 1, "pal40x16": 1, "pal600": 0}     # palette -> table form of k_csr_rowpat<OP, LDS_TAB, RPL>


@functools.lru_cache(maxsize=None)
def rp(which):
    """Square, k_csr_rowpat: the rows draw their pattern at random from a palette, so no wave has a pattern (nx * 4 > row).
    n = 8192 + 77: a last tile of 77 rows, a last step of the two-rows-per-lane form with its second row beyond the matrix.
    pal8: 8 patterns (LDS table, small form 2) -- among them an empty one, one without the diagonal, one with it twice;
    pal200: 200 patterns (LDS table, form 1); pal40x16: 40 patterns of 16 entries, more than 512 table entries (form 1);
    pal600: 600 patterns, more than 512 (table in global memory, form 0).  Offsets within +-8: few clipped patterns on top."""
    n = 8192 + 77
    seed = list(RP_PALETTES).index(which)
    rng = np.random.default_rng(500 + seed)
    npal = {"pal8": 8, "pal200": 200, "pal40x16": 40, "pal600": 600}[which]
    cand = np.arange(-8, 9)
    cand = cand[cand != 0]
    pal = []
    for p in range(npal):
        L = 16 if which == "pal40x16" else int(rng.integers(2, 9))
        o = [0] + list(rng.choice(cand, size=L - 1, replace=False))
        v = [4.0 + p / 64.0] + list(rng.integers(-8, 9, size=L - 1) / 8.0)
        perm = rng.permutation(L)                               # the diagonal anywhere in the row
        pal.append(([o[i] for i in perm], [v[i] for i in perm]))
    if which == "pal8":
        pal[5] = ([], [])
        pal[6] = ([-1, 2, 7], [0.5, -0.25, 0.125])
        pal[7] = ([0, 3, 0, -5, 1], [2.0, 0.5, 3.0, -1.0, 0.25])
    a = rng.integers(0, npal, size=n)
    ia, ja, val = palette_csr(n, n, pal, a)
    c = _finish(f"rp_{which}", n, n, ia, ja, val, KIND["rowpat"], OPS_SQUARE)
    cd = c["coding"]
    nx, _ = _swept_share(c)
    assert nx * 4 > n
    form = 2 if (cd["npat"] <= 64 and cd["npent"] <= 512) else 1 if (cd["npat"] <= 512 and cd["npent"] <= 2048) else 0
    assert form == RP_PALETTES[which], (which, cd["npat"], cd["npent"])
    if which == "pal40x16": assert cd["npat"] <= 64 and cd["npent"] > 512
    if which == "pal600": assert cd["npat"] > 512
    assert n % BLOCK != 0 and n % (2 * BLOCK) < BLOCK           # RPL 2: the last tile's second rows are all beyond the matrix
    c = dict(c)
    c["form"] = form
    return _freeze(c)


D8_MEANS = {5: 8, 14: 16, 30: 24}      # mean row -> U of k_csr_dict8<OP, U>


@functools.lru_cache(maxsize=None)
def d8(mean, rect=False):
    """k_csr_dict8<., U>: a band matrix (+-100) over a dictionary of 240 (offset, value) pairs in which no row repeats -- every row is
    the anchor pair (offset 0: the diagonal, or a rectangular row's first stored column) and a random draw of the others in random
    order (the first and last 100 rows: the anchor alone) -- so the row patterns are refused and the byte dictionary codes it.  n = 6000 + 37.  Rows 100 and 101 empty, row 200 one
    entry, row 300 all 200 offsets; the 64-row group at 1024 holds 40-entry rows (a code span of 2560 bytes: the oversized path, read
    from global memory); the groups at 2048 and 3072 start at a multiple of 16 entries and span exactly 2048 bytes (the largest staged
    span) and 2049 (the smallest oversized one).  rect: 500 more columns and per-row bases (rowbase)."""
    n = 6000 + 37
    U = D8_MEANS[mean]
    rng = np.random.default_rng(800 + mean + (1 if rect else 0))
    offs = np.arange(-100, 100)
    offs = offs[offs != 0]                                       # 199 offsets + the anchor
    p_off = np.concatenate([[0], offs, offs[:40]])               # 240 pairs: 40 offsets carry a second value
    p_val = np.concatenate([[8.0], rng.choice([1.0, -2.0, 0.5], size=199), np.full(40, -0.25)])
    npair = len(p_off)
    lo, hi = {5: (2, 6), 14: (9, 17), 30: (24, 34)}[mean]
    lens = rng.integers(lo, hi + 1, size=n)
    lens[:100] = 1                                               # (the band stays inside the matrix: nothing is clipped)
    lens[n - 100:] = 1
    lens[[100, 101]] = 0
    lens[200] = 1
    lens[300] = 200
    lens[1024:1088] = 40
    lens[2048:2112] = 32
    lens[3072:3136] = 32
    lens[3135] = 33
    for g in (2048, 3072):                                       # the row in front of a group takes up the slack to a multiple of 16
        lens[g - 1] += (-int(lens[:g].sum())) % 16
    # per row: the anchor, then the lens - 1 pairs with the smallest random keys, in key order
    keys = rng.random((n, npair))
    keys[:, 0] = -1.0
    keys[300, 200:] = 2.0                                        # row 300: the 200 distinct offsets
    order = np.argsort(keys, axis=1)
    take = np.arange(npair)[None, :] < lens[:, None]
    pick = order[take]                                           # row-major: rows in order, each in key order
    rows = np.repeat(np.arange(n), lens)
    center = rows + (250 if rect else 0)
    ncol = n + 500 if rect else n
    col = center + p_off[pick]
    val = p_val[pick]
    assert col.min() >= 0 and col.max() < ncol
    ia = np.zeros(n + 1, dtype=np.int32)
    ia[1:] = np.cumsum(lens)
    ja = col.astype(np.int32)
    c = _finish(f"d8_mean{mean}" + ("_rect" if rect else ""), n, ncol, ia, ja, val, KIND["dict8"], OPS_RECT if rect else OPS_SQUARE)
    cd = c["coding"]
    avg = len(ja) / n
    assert cd["why"] == "patterns * 8 <= row" and cd["npairs"] <= 256
    assert (U == 8 and avg <= 8.5) or (U == 16 and 8.5 < avg <= 20.0) or (U == 24 and avg > 20.0), avg
    assert abs(avg - mean) <= 0.15 * mean + 1.2, avg
    span = lambda g: int(ia[g + 64] - (ia[g] & ~15))
    assert lens[100] == 0 and lens[101] == 0 and lens[200] == 1 and lens[300] == 200
    assert span(1024) > DICT_CAP and ia[2048] % 16 == 0 and ia[3072] % 16 == 0
    assert span(2048) == DICT_CAP and span(3072) == DICT_CAP + 1
    assert n % 64 != 0
    return c


# ------------------------------------------------------------------------------------------------------------------------------
# the runs: (id, case builder, its arguments, tune keys set for the run, ops)
# ------------------------------------------------------------------------------------------------------------------------------
def _runs():
    R = []
    add = lambda rid, fn, args=(), tune=(), kind=None, ops=None: R.append(dict(id=rid, fn=fn, args=args, tune=tuple(tune), kind=kind, ops=ops))
    add("p4_main", p4_main)
    for t in P4_TAILS:
        add(f"p4_tail{t}", p4_tail, (t,))
    for L in P4_LENGTHS:
        add(f"p4_len{L}", p4_length, (L,))
    for g in (1, 2):
        add(f"p4_queue_maxgrid{g}", p4_queue, (), [("maxgrid", g, -1)])
    for w in P4_DIAGONALS:
        add(f"p4_{w}", p4_diagonal, (w,))
    add("p4_padding", p4_padding)
    add("p4_strips", p4_strips)
    for t in P5_TAILS:
        add(f"p5_t{t}", p5, (t,))
    for t in P5_TAILS:
        add(f"p5_t{t}_mean6", p5, (t, True))
    for w in RP_PALETTES:
        for rpl in (1, 2):
            add(f"rp_{w}_rpl{rpl}", rp, (w,), [("rpl", rpl, -1)])
    add("rp_pal8_global_table", rp, ("pal8",), [("lds_tab", 0, 1)])
    add("rp_p4_main_gen2_off", p4_main, (), [("gen2", 0, 2)], kind=KIND["rowpat"])
    add("rp_p4_padding_rpl1", p4_padding, (), [("rpl", 1, -1)], kind=KIND["rowpat"])     # the padding of k_csr_rowpat (a select on the accumulate)
    for m in D8_MEANS:
        add(f"d8_mean{m}", d8, (m,))
    add("d8_mean5_rect", d8, (5, True))
    for g in (1, 2):
        add(f"d8_mean14_maxgrid{g}", d8, (14,), [("maxgrid", g, -1)])
    for k in (1024, 3000):                                       # row windows: split_rows alone, no other geometry key
        add(f"p4_main_split{k}", p4_main, (), [("split_rows", k, 0)])
        add(f"rp_pal200_split{k}", rp, ("pal200",), [("split_rows", k, 0)])
        add(f"d8_mean14_split{k}", d8, (14,), [("split_rows", k, 0)])
    return R


RUNS = _runs()      # tune: (key, value for the run, value restored afterwards)


def build(run):
    """The case of a run and the kernel family code the run must report."""
    c = run["fn"](*run["args"])
    return c, (run["kind"] if run["kind"] is not None else c["kind"])


def all_cases():
    """Every distinct case of RUNS, once."""
    seen, out = set(), []
    for run in RUNS:
        key = (run["fn"].__name__, run["args"])
        if key not in seen:
            seen.add(key)
            out.append((run["id"], run))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# inputs and references
# ------------------------------------------------------------------------------------------------------------------------------
def inputs(nrow, ncol, op, seed, inf_rows=None):
    """The vectors of tests/test_gpu_sell.py::_inputs (zeros in the op-8 diagonal included); a rectangular operator's dotted vector
    is x cut, or repeated, to nrow entries.  inf_rows: x = inf there (ops whose x is the gathered vector only), the dotted vector stays finite."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(nrow if op in (5, 6) else ncol)
    b = rng.standard_normal(nrow)
    if op == 8:
        b = 1.0 + np.abs(b)
        b[::17] = 0.0
    if op == 7:
        b = np.resize(x, nrow)                                   # (x itself; cut or repeated to nrow entries where the operator is rectangular)
    if op == 5:
        x = 0.01 * x
    y0 = rng.standard_normal(nrow)
    if inf_rows is not None:
        assert op not in (5, 6)
        x[:nrow][inf_rows] = np.inf
    return x, b, y0


def reference(orc, c, op, x, b, y0, scalar):
    """(y, y2) of row operation `op` by the oracle's restatement of the reference (left-to-right row sums): ops 0, 7, 8 orc_mxv;
    1 = w = b, w -= A x (orc_aAxpy with -1); 2, 3, 4 orc_aAxpy; 5 orc_smoother_jacobi; 6 orc_smoother_l1diag; y2 of op 8 restated."""
    A, keep = T.as_csr(c["ia"], c["ja"], c["val"], c["ncol"])
    n = c["nrow"]
    x = np.ascontiguousarray(x)
    y2 = None
    if op in (0, 7, 8):
        y = np.zeros(n)
        orc.orc_mxv(C.byref(A), T.dp(x), T.dp(y))
        if op == 8:
            with np.errstate(divide="ignore", invalid="ignore"):
                y2 = np.where(np.abs(b) > 1e-20, (1 - scalar) * 0.0 + scalar * y / b, 0.0)
    elif op in (1, 2, 3, 4):
        y = (b if op == 1 else y0).copy()
        orc.orc_aAxpy({1: -1.0, 2: 1.0, 3: -1.0, 4: scalar}[op], C.byref(A), T.dp(x), T.dp(y))
    elif op == 5:
        y = x.copy()
        orc.orc_smoother_jacobi(T.dp(y), 0, n - 1, 1, C.byref(A), T.dp(np.ascontiguousarray(b)), 1, scalar)
    else:
        y = x.copy()
        orc.orc_smoother_l1diag(T.dp(y), 0, n - 1, 1, C.byref(A), T.dp(np.ascontiguousarray(b)), 1)
    return y, y2
