"""Deterministic cases for the sequential sweep kernels (csrc/seq_split.hip.h, csrc/seq_chain.hip.h, k_seq_level of csrc/kernels.hip.h): one
run per instantiation or path of the dispatch in smoothers.hip.h (seq_sweep_launch), each through fasp_hip_csr_sweep.

A run is a dict: id, mat = (generator, args), seq = (kind, args), form, w, zero_start, u0 ('random' or 'zeros'), tune = ((key, value), ..),
path (the code of fasp_hip_csr_sweep's info[0]), want = the shape the run was built for -- L, rounds, spine, virtual ('>0' or 0), strips, LR,
n1b, t1, t2, launches where they are stated --, group = runs whose results must agree (None: none), same = how: 'bits', or 'values' (equal
numbers, the sign of a zero apart).  Every tune key a run sets is in
TUNE_RESTORE.  tests/test_sweep_cases.py checks, without a GPU, that the host self-tests report that shape for the run's parameters and that the
runs cover every path and instantiation; tests/test_gpu_sweep_kernels.py runs them."""
import ctypes as C
import functools

import numpy as np

import faspsolver_amd as fa
from faspsolver_amd import _types as T

from test_seq_schedule import _banded as banded      # (n, bw, fill, seed): the generator of the host-side schedule tests

TUNE_RESTORE = dict(gs_multicolor=0, seq_flow=1, seq_strip_kb=0, seq_spine=1, seq_grid=0, seq_chain=1, seq_chain_n1=0, seq_chain_grid=0,
                    seq_chain_ref=0, seq_rest_lanes=0, seq_lanes=0, seq_zero_skip=1)
SMALLREAL = 1e-20
PATHS = {0: "nothing", 1: "k_split_direct", 2: "rest+scatter_final", 3: "rest+k_tri_flow", 4: "rest+k_tri_level", 5: "rest+k_tri_chain",
         6: "rest+k_tri_chain_ref", 7: "k_seq_level/levels", 8: "k_seq_level/colours"}


# ---------------------------------------------------------------------------------------------------------------- matrices
def _csr(M):
    M = M.tocsr()
    M.sort_indices()
    return M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64).copy()


def banded_zero_diag(n, bw, fill, seed, row):
    """banded with the diagonal of one row stored as 0.0: the reference leaves the row alone, the chain form does not apply."""
    ia, ja, a = banded(n, bw, fill, seed)
    a = a.copy()
    k = np.flatnonzero(ja[ia[row]:ia[row + 1]] == row) + ia[row]
    assert len(k) == 1
    a[k] = 0.0
    return ia, ja, a


def grid5(nx, ny, diag=4.5, far=0, gap=0):
    """Five-point grid in natural order (x fastest) plus `far` symmetric couplings `gap` rows apart."""
    import scipy.sparse as sp
    n = nx * ny
    I = sp.identity(nx, format="csr"); J = sp.identity(ny, format="csr")
    Tx = sp.diags([-1.0, -1.0], [-1, 1], shape=(nx, nx)); Ty = sp.diags([-1.0, -1.0], [-1, 1], shape=(ny, ny))
    M = (sp.kron(J, Tx) + sp.kron(Ty, I) + diag * sp.identity(n)).tolil()
    if far:
        rng = np.random.default_rng(9)
        for i in rng.choice(np.arange(gap, n), size=far, replace=False):
            M[i, i - gap] = -0.25; M[i - gap, i] = -0.25
    return _csr(M)


def ragged700():
    """What a stencil never shows (test_precond_objects.py::test_standalone_sweeps_on_a_ragged_matrix): an unsymmetric pattern
    (anti-dependencies), three full rows (more lower entries than 8 x 64 slots), empty rows, a stored zero diagonal (row 20), no diagonal at
    all (row 21), a diagonal stored twice (row 100: the last one counts, nothing is subtracted for either)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    n = 700
    M = sp.random(n, n, density=0.03, random_state=7, format="lil")
    for i in (3, 250, 699):                       # very long rows: more lower entries than 8 x 64 slots
        M[i, :] = rng.standard_normal(n)
    for i in range(n): M[i, i] = 30.0 + rng.random()
    for i in (10, 11, 400): M[i, :] = 0.0         # empty rows
    M[20, 20] = 0.0                               # stored zero diagonal
    M = M.tocsr(); M.sort_indices()
    M[21, 21] = 0.0; M.eliminate_zeros()          # no diagonal at all in row 21 (row 20 lost its zero too: put it back below)
    ia = M.indptr.astype(np.int32).tolist(); ja = M.indices.astype(np.int32).tolist(); a = M.data.tolist()
    def insert(row, col, v):                      # append an entry to a row (unsorted storage is allowed)
        k = ia[row + 1]
        ja.insert(k, col); a.insert(k, v)
        for r in range(row + 1, n + 1): ia[r] += 1
    insert(20, 20, 0.0)                           # zero diagonal, stored
    insert(100, 100, 55.0)                        # diagonal stored twice: the last one counts
    return np.array(ia, dtype=np.int32), np.array(ja, dtype=np.int32), np.array(a)


def diagonal(n):
    import scipy.sparse as sp
    return _csr(sp.diags([2.0 + 0.01 * np.arange(n)], [0], shape=(n, n)))


def upper(n, density, seed):
    """Diagonal plus a random strictly upper triangle: an ascending sweep reads old values only, yet its rows couple."""
    import scipy.sparse as sp
    M = sp.triu(sp.random(n, n, density=density, random_state=seed, format="csr"), k=1) + sp.diags([3.0 + 0.01 * np.arange(n)], [0], shape=(n, n))
    return _csr(M)


def arrow(n):
    """4 I plus a last row of -1e-4 across all columns: one row reads more earlier rows than a strip's LDS holds."""
    import scipy.sparse as sp
    M = (sp.identity(n, format="lil") * 4.0).tolil()
    M[n - 1, : n - 1] = -1e-4
    return _csr(M)


def tridiag(n):
    import scipy.sparse as sp
    return _csr(sp.diags([-1.0, 2.5, -1.0], [-1, 0, 1], shape=(n, n)) if n > 1 else sp.csr_matrix(np.array([[2.5]])))


@functools.lru_cache(maxsize=None)
def matrix(fn, args):
    ia, ja, a = fn(*args)
    for v in (ia, ja, a): v.setflags(write=False)
    return ia, ja, a


def sequence(run):
    """The rows of the run's sweep, in sweep order."""
    n = len(matrix(*run["mat"])[0]) - 1
    kind, args = run["seq"][0], run["seq"][1:]
    i = np.arange(n)
    if kind == "asc": s = i
    elif kind == "desc": s = i[::-1]
    elif kind == "sgs": s = i[: max(n - 1, 0)][::-1]          # descending from row n - 2 (the back sweep of SGS)
    elif kind == "mod3": s = i[i % 3 != 1]
    elif kind == "red": s = i[((i % args[0]) + i // args[0]) % 2 == 0]      # red rows of a grid with args[0] points per line
    elif kind == "half": s = i[(i * 7) % 10 < 5]
    elif kind == "scramble": s = np.random.default_rng(args[0]).permutation(n)[: args[1]]
    elif kind == "rows": s = np.array(args, dtype=np.int64)
    else: raise ValueError(kind)
    return np.ascontiguousarray(s, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- runs
def _run(rid, mat, seq, form, path, tune=(), w=1.0, zero_start=0, u0="random", group=None, same="bits", **want):
    assert form in (0, 1, 2) and same in ("bits", "values") and all(k in TUNE_RESTORE for k, _ in tune), rid
    return dict(id=rid, mat=mat, seq=seq if isinstance(seq, tuple) else (seq,), form=form, w=1.1 if form == 2 and w == 1.0 else w,
                zero_start=zero_start, u0=u0, tune=tuple(tune), path=path, want=want, group=group, same=same)


def _flow_level(rid, mat, seq, form, tune, **kw):
    """The dataflow form and its plain partner (one launch per dependency class): same slots, same arithmetic, same bits."""
    group = kw.pop("group", rid)
    return [_run(f"{rid}_flow", mat, seq, form, 3, tune + (("seq_flow", 1),), group=group, **kw),
            _run(f"{rid}_level", mat, seq, form, 4, tune + (("seq_flow", 0),), group=group, **kw)]


def _split_runs():
    """k_tri_flow / k_tri_level <L, 4 | 8>: banded matrices, lanes forced, bandwidth 3 L (four rounds), 6 L (eight), 10 L (eight, virtual rows)."""
    out = []
    for li, L in enumerate((1, 2, 4, 8, 16, 32, 64)):
        # (a spine comes with eight rounds: the four-round kernels are reached without one)
        for bi, (mult, combos) in enumerate(((3, (("asc", 0), ("desc", 0))), (6, (("asc", 2), ("desc", 0))), (10, (("asc", 0), ("desc", 2))))):
            bw = mult * L
            n = max(200, int(2.5 * bw))
            for ci, (direction, spine) in enumerate(combos):
                form = (li + bi + ci) % 3
                kt = 2 if (spine == 2 and L >= 2) else 0
                rounds = 8 if (mult > 4 or kt) else 4
                out += _flow_level(f"L{L}_bw{bw}_{direction}_spine{spine}", (banded, (n, bw, 1.0, 0)), direction, form,
                                   (("seq_chain", 0), ("seq_lanes", L), ("seq_spine", spine)), L=L, rounds=rounds, spine=kt,
                                   virtual=">0" if mult == 10 else 0)
    return out


GRID = (grid5, (60, 50, 4.5, 10, 2400))


def _grid_runs():
    out = []
    kb16 = (("seq_chain", 0), ("seq_strip_kb", 16))
    for si, (seq, strips) in enumerate(((("asc",), 12), (("desc",), 12), (("sgs",), 12), (("mod3",), 8), (("red", 60), 4))):
        sid = seq[0]
        form = si % 3
        out += _flow_level(f"grid_{sid}_kb16", GRID, seq, form, kb16, L=1, rounds=4, spine=0, virtual=0, strips=strips, group=f"grid_{sid}")
        for g in (1, 2):    # fewer workgroups than strips: the ticket counter hands every strip out in order
            out.append(_run(f"grid_{sid}_kb16_grid{g}", GRID, seq, form, 3, kb16 + (("seq_flow", 1), ("seq_grid", g)), group=f"grid_{sid}",
                            L=1, rounds=4, spine=0, virtual=0, strips=strips))
        # one strip (512 KB hold the whole sweep): same lanes, same rounds -- same bits
        out.append(_run(f"grid_{sid}_kb512", GRID, seq, form, 3, (("seq_chain", 0), ("seq_strip_kb", 512), ("seq_flow", 1)), group=f"grid_{sid}",
                        L=1, rounds=4, spine=0, virtual=0, strips=1))
    return out


RAGGED = (ragged700, ())


def _ragged_runs():
    out = []
    for seq in (("asc",), ("desc",), ("mod3",), ("half",)):
        for form in (0, 2):
            if seq[0] in ("mod3", "half") and form != (0 if seq[0] == "mod3" else 2):
                continue
            rid = f"ragged_{seq[0]}_f{form}"
            out += _flow_level(rid, RAGGED, seq, form, (("seq_chain", 0),), virtual=">0" if seq[0] in ("asc", "desc") else None)
    # default tune keys: the chain form is tried first (the sweep is chain-bound) and refuses rows that are left alone
    out.append(_run("ragged_asc_f0_default_keys", RAGGED, "asc", 0, 3, (("seq_flow", 1),), group="ragged_asc_f0"))
    # the zero-start pass: flagged zero with and without the skip, and the same sweep from a vector of stored zeros
    for seq in (("asc",), ("mod3",)):
        for form in (0, 2):
            g = f"ragged_{seq[0]}_f{form}_zero"
            t = (("seq_chain", 0), ("seq_flow", 1))
            out.append(_run(f"{g}_skip", RAGGED, seq, form, 3, t + (("seq_zero_skip", 1),), zero_start=1, group=g, same="values"))
            out.append(_run(f"{g}_noskip", RAGGED, seq, form, 3, t + (("seq_zero_skip", 0),), zero_start=1, group=g, same="values"))
            out.append(_run(f"{g}_stored", RAGGED, seq, form, 3, t, u0="zeros", group=g, same="values"))
    out.append(_run("ragged_desc_f2_zero_level", RAGGED, "desc", 2, 4, (("seq_chain", 0), ("seq_flow", 0)), zero_start=1))
    return out


def _nolower_runs():
    out = []
    DIAG, PLAIN, UP = (diagonal, (300,)), (grid5, (30, 20, 4.0, 0, 0)), (upper, (500, 0.05, 3))
    out.append(_run("diag_asc", DIAG, "asc", 0, 1, LR=1))
    out.append(_run("diag_desc_sor", DIAG, "desc", 2, 1, LR=1))
    out.append(_run("redrows", PLAIN, ("red", 30), 1, 1, LR=1))
    out.append(_run("redrows_zero", PLAIN, ("red", 30), 2, 1, zero_start=1, LR=1))
    out.append(_run("upper_asc", UP, "asc", 0, 2, launches=1))
    out.append(_run("upper_asc_zero", UP, "asc", 2, 2, zero_start=1, launches=1))
    for k, lr in enumerate((1, 2, 4, 8, 16, 32, 64)):
        out.append(_run(f"redrows_LR{lr}", PLAIN, ("red", 30), k % 3, 1, (("seq_rest_lanes", lr),), LR=lr))
        out.append(_run(f"upper_asc_LR{lr}", UP, "asc", (k + 1) % 3, 2, (("seq_rest_lanes", lr),), LR=lr, launches=1))
    out.append(_run("upper_asc_LR48", UP, "asc", 1, 2, (("seq_rest_lanes", 48),), LR=64, launches=1))   # rounded up to a power of two
    return out


# (n, bw, fill, seed): the shapes of test_chain_schedule_reproduces_the_sequential_sweep, which seeds every matrix with its n; the tier counts
# the runs state are asserted on the host self-test (tests/test_sweep_cases.py)
CHAIN = ((333, 200, 0.5, 333), (300, 30, 1.0, 300), (65, 64, 1.0, 65), (40, 5, 1.0, 40))


def _chain_runs():
    out = []
    def pair(rid, mat, seq, form, tune, **kw):
        ns = len(sequence(dict(mat=mat, seq=seq)))
        t = tune + (("seq_flow", 1),) + ((("seq_chain", 2),) if ns < 256 else ())
        return [_run(f"{rid}_chain", mat, seq, form, 5, t, group=rid, **kw),
                _run(f"{rid}_ref", mat, seq, form, 6, t + (("seq_chain_ref", 1),), group=rid, **kw)]
    for mi, args in enumerate(CHAIN):
        mat = (banded, args)
        n = args[0]
        for si, seq in enumerate((("asc",), ("desc",), ("mod3",))):
            form = (mi + si) % 3
            kw = {}
            if n == 333 and seq[0] == "asc":
                kw = dict(n1b=2, t1=272, t2=16)
            out += pair(f"chain{n}_{seq[0]}_f{form}", mat, seq, form, (), **kw)
    big = (banded, CHAIN[0])
    out += pair("chain333_asc_n1_1_f2", big, ("asc",), 2, (("seq_chain_n1", 1),), n1b=1, t1=184, t2=128)
    out += pair("chain333_desc_n1_1_f0", big, ("desc",), 0, (("seq_chain_n1", 1),), n1b=1)
    out += pair("chain333_asc_n1_1_f1", big, ("asc",), 1, (("seq_chain_n1", 1),), n1b=1, t1=184, t2=128)
    # three tier-2 workgroups instead of 95: the same sums by other hands
    out.append(_run("chain333_asc_n1_1_f2_grid3", big, ("asc",), 2, 5, (("seq_chain_n1", 1), ("seq_flow", 1), ("seq_chain_grid", 3)), group="chain333_asc_n1_1_f2",
                    n1b=1, t1=184, t2=128))
    out.append(_run("chain333_asc_f0_grid3", big, ("asc",), 0, 5, (("seq_flow", 1), ("seq_chain_grid", 3)), group="chain333_asc_f0", n1b=2, t1=272, t2=16))
    out.append(_run("chain333_asc_zero_f2", big, ("asc",), 2, 5, (("seq_flow", 1),), zero_start=1))
    # one diagonal zeroed: a row that is left alone -- the chain form refuses, the dataflow form takes the sweep
    out += _flow_level("chain333_zero_diag", (banded_zero_diag, CHAIN[0] + (150,)), ("asc",), 1, ())
    return out


ARROW = (arrow, (19600,))


def _rowlevel_runs():
    out = [_run(f"arrow_L{L}", ARROW, "asc", k % 3, 7, (("seq_lanes", L),), L=L, launches=2) for k, L in enumerate((2, 4, 8, 16, 32, 64))]
    out.append(_run("arrow_L1_selects_64", ARROW, "asc", 1, 7, (("seq_lanes", 1),), L=64, launches=2))
    out.append(_run("arrow_desc_no_lower", ARROW, "desc", 0, 2, launches=1))      # the long row first: nobody reads a new value
    return out


def _multicolour_runs():
    out = []
    mc = (("gs_multicolor", 1),)
    for k, (mat, name, L) in enumerate(((RAGGED, "ragged", 8), (GRID, "grid", 2))):
        for d, seq in enumerate(("asc", "desc")):
            out.append(_run(f"mc_{name}_{seq}", mat, seq, (k + 2 * d) % 3, 8, mc + (("seq_lanes", L),), L=L))
    out.append(_run("mc_ragged_mod3_zero", RAGGED, "mod3", 2, 8, mc + (("seq_lanes", 16),), zero_start=1, L=16))
    out.append(_run("mc_grid_asc_default_lanes", GRID, "asc", 1, 8, mc, L=4))        # (4.9 entries per row: the operator's kernel takes 4 lanes)
    return out


def _edge_runs():
    out = []
    c0 = (("seq_chain", 0),)
    out.append(_run("n1", (tridiag, (1,)), "asc", 0, 1))
    out += _flow_level("n2_asc", (tridiag, (2,)), "asc", 1, c0, L=1, rounds=4, strips=1)
    out += _flow_level("n2_desc", (tridiag, (2,)), "desc", 2, c0, L=1, rounds=4, strips=1)
    out.append(_run("ns0", (tridiag, (65,)), ("rows",), 0, 0))
    out.append(_run("ns0_multicolour", (tridiag, (65,)), ("rows",), 0, 0, (("gs_multicolor", 1),)))
    out.append(_run("ns1", (tridiag, (65,)), ("rows", 40), 2, 1))
    for n in (63, 64, 65):
        out += _flow_level(f"tri{n}_asc", (tridiag, (n,)), "asc", n % 3, c0, L=1, rounds=4, strips=1)
        out += _flow_level(f"tri{n}_desc_L4", (tridiag, (n,)), "desc", (n + 1) % 3, c0 + (("seq_lanes", 4),), L=4, rounds=4)
        out.append(_run(f"tri{n}_chain", (tridiag, (n,)), "asc", (n + 2) % 3, 5, (("seq_chain", 2), ("seq_flow", 1)), group=f"tri{n}_chain"))
        out.append(_run(f"tri{n}_chain_ref", (tridiag, (n,)), "asc", (n + 2) % 3, 6, (("seq_chain", 2), ("seq_flow", 1), ("seq_chain_ref", 1)), group=f"tri{n}_chain"))
    out += _flow_level("grid_scrambled", GRID, ("scramble", 11, 2000), 1, c0 + (("seq_strip_kb", 16),))
    out += _flow_level("ragged_scrambled", RAGGED, ("scramble", 12, 700), 2, c0)
    return out


RUNS = _split_runs() + _grid_runs() + _ragged_runs() + _nolower_runs() + _chain_runs() + _rowlevel_runs() + _multicolour_runs() + _edge_runs()
assert len({r["id"] for r in RUNS}) == len(RUNS)
BY_ID = {r["id"]: r for r in RUNS}
GROUPS = {}
for _r in RUNS:
    if _r["group"] is not None:
        GROUPS.setdefault(_r["group"], []).append(_r["id"])
GROUPS = {g: ids for g, ids in GROUPS.items() if len(ids) > 1}
GROUP_SAME = {g: BY_ID[ids[0]]["same"] for g, ids in GROUPS.items()}
assert all(BY_ID[i]["same"] == GROUP_SAME[g] for g, ids in GROUPS.items() for i in ids)


def tune_of(run):
    t = dict(TUNE_RESTORE)
    t.update(dict(run["tune"]))
    return t


# ---------------------------------------------------------------------------------------------------------------- host side
def _seq_p(seq):
    return seq.ctypes.data_as(C.POINTER(C.c_int))


def schedule_selftest(run):
    """fasp_hip_seq_schedule_selftest under the run's strip size, lanes and spine -> (result, info dict)."""
    L = fa.lib()
    L.fasp_hip_seq_schedule_selftest.restype = C.c_double
    L.fasp_hip_seq_schedule_selftest.argtypes = [C.POINTER(T.dCSRmat), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    ia, ja, a = matrix(*run["mat"])
    A, keep = T.as_csr(ia, ja, a)
    seq = sequence(run)
    t = tune_of(run)
    buf = (C.c_int * 8)()
    r = L.fasp_hip_seq_schedule_selftest(C.byref(A), _seq_p(seq), len(seq), t["seq_strip_kb"], t["seq_lanes"], t["seq_spine"], buf)
    return r, dict(lanes=buf[0], rounds=buf[1], spine=buf[2], virtual=buf[3], strips=buf[4], chunks=buf[5])


def chain_selftest(run):
    """fasp_hip_seq_chain_selftest under the run's tier-1 blocks, form and weight -> (result, info dict)."""
    L = fa.lib()
    L.fasp_hip_seq_chain_selftest.restype = C.c_double
    L.fasp_hip_seq_chain_selftest.argtypes = [C.POINTER(T.dCSRmat), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    ia, ja, a = matrix(*run["mat"])
    A, keep = T.as_csr(ia, ja, a)
    seq = sequence(run)
    buf = (C.c_int * 10)()
    r = L.fasp_hip_seq_chain_selftest(C.byref(A), _seq_p(seq), len(seq), tune_of(run)["seq_chain_n1"], run["form"], run["w"], buf, None)
    return r, dict(blocks=buf[0], n1b=buf[1], rx=buf[2], rg=buf[3], t1_steps=buf[4], t2_steps=buf[5], band=buf[6], t1=buf[7], t2=buf[8], classes=buf[9])


def structure(run):
    return _structure(run["mat"], run["seq"])


@functools.lru_cache(maxsize=None)
def _structure(mat, seqspec):
    """What the dispatch reads of the sweep, restated: entries that read a row swept earlier (lower), a row swept later (upper), the mean
    number of entries the rest pass reads per row, dependency classes of the true dependencies."""
    ia, ja, a = matrix(*mat)
    n = len(ia) - 1
    seq = sequence(dict(mat=mat, seq=seqspec))
    pos = np.full(n, -1, dtype=np.int64)
    pos[seq] = np.arange(len(seq))
    row = np.repeat(np.arange(n), np.diff(ia))
    off = ja != row
    swept = pos[row] >= 0
    lower = off & swept & (pos[ja] >= 0) & (pos[ja] < pos[row])
    upper = off & swept & (pos[ja] > pos[row])
    rest = off & swept & ~lower
    lev = np.zeros(n, dtype=np.int64)
    nlev = 0
    for i in seq:
        k = np.arange(ia[i], ia[i + 1])[lower[ia[i]:ia[i + 1]]]
        lev[i] = 1 + (lev[ja[k]].max() if len(k) else 0)
        nlev = max(nlev, int(lev[i]))
    return dict(ns=len(seq), lower=int(lower.sum()), upper=int(upper.sum()), rest=int(rest.sum()), classes=nlev)


def rest_lanes(run, st=None):
    """Lanes per row of k_split_rest / k_split_direct: forced (rounded up to a power of two), or from the mean row of the rest pass."""
    t = tune_of(run)
    if t["seq_rest_lanes"] > 0:
        lr = 1
        while lr < 64 and lr < t["seq_rest_lanes"]: lr *= 2
        return lr
    st = st or structure(run)
    avg = st["rest"] / st["ns"] if st["ns"] else 0.0
    lr = 1
    while lr < 64 and 4 * lr < avg: lr *= 2
    return lr


def level_lanes(run):
    """k_seq_level's lanes per row (smoothers.hip.h): seq_lanes where it is set, else 64 for rows of 96 entries and more, else the lanes of the
    level's operator kernel -- for rows of fewer than 48 entries (device_csr.hip.h, pick_kernel) 2, 4, 8 or 16 by the mean row -- and the
    instantiation that serves that number."""
    t = tune_of(run)
    ia = matrix(*run["mat"])[0]
    avg = float(ia[-1]) / (len(ia) - 1)
    if t["seq_lanes"] > 0: L = t["seq_lanes"]
    elif avg >= 96.0: L = 64
    else:
        assert avg < 48.0, (run["id"], "lanes of longer rows depend on the grid size: force seq_lanes")
        L = 2 if avg < 3.0 else 4 if avg < 6.0 else 8 if avg < 24.0 else 16
    return L if L in (2, 4, 8, 16, 32) else 64


def derive(run):
    """Path and shape of the run from the host self-tests and the dispatch rules of smoothers.hip.h / seq_sched.cpp, restated:
    -> dict(path, L, rounds, LR, spine, virtual, strips, chunks, n1b, t1, t2) (0 where the path has no such number)."""
    t = tune_of(run)
    st = structure(run)
    d = dict(path=0, L=0, rounds=0, LR=0, spine=0, virtual=0, strips=0, chunks=0, n1b=0, t1=0, t2=0)
    if st["ns"] == 0:
        return d
    if t["gs_multicolor"]:
        d.update(path=8, L=level_lanes(run))
        return d
    d["LR"] = rest_lanes(run, st)
    if st["lower"] == 0:
        d["path"] = 1 if st["upper"] == 0 else 2
        return d
    if t["seq_chain"] == 2 or (t["seq_chain"] == 1 and st["ns"] >= 256 and st["ns"] < 16 * st["classes"]):
        r, ci = chain_selftest(run)
        assert r >= 0.0 or r == -2.0, (run["id"], r)
        if r >= 0.0:
            assert r <= 1e-12, (run["id"], r)
            d.update(path=6 if (t["seq_chain_ref"] or not t["seq_flow"]) else 5, L=64, n1b=ci["n1b"], t1=ci["t1_steps"], t2=ci["t2_steps"], chain=ci)
            return d
    r, si = schedule_selftest(run)
    if r == -2.0:
        d.update(path=7, LR=0, L=level_lanes(run))
        return d
    assert 0.0 <= r <= 1e-12, (run["id"], r)
    d.update(path=3 if t["seq_flow"] else 4, L=si["lanes"], rounds=si["rounds"], spine=si["spine"], virtual=si["virtual"], strips=si["strips"], chunks=si["chunks"])
    return d


# ---------------------------------------------------------------------------------------------------------------- references
def colour_order(run):
    """The multicolour mode's order of the run's rows, restated: greedy colouring in ascending row order (the smallest colour no coupled row
    of A or A^T has), classes in ascending colour order -- descending for a descending sweep -> (rows in sweep order, colours)."""
    ia, ja, a = matrix(*run["mat"])
    n = len(ia) - 1
    seq = sequence(run)
    import scipy.sparse as sp
    P = sp.csr_matrix((np.ones(len(ja)), ja, ia), shape=(n, n))
    P = (P + P.T).tocsr()
    colour = np.full(n, -1, dtype=np.int64)
    for i in np.sort(seq):
        nb = P.indices[P.indptr[i]:P.indptr[i + 1]]
        used = set(colour[nb[nb != i]].tolist())
        c = 0
        while c in used: c += 1
        colour[i] = c
    rows = np.sort(seq)
    ncol = int(colour[rows].max()) + 1 if len(rows) else 0
    descending = len(seq) > 1 and seq[0] > seq[-1]
    key = -colour[rows] if descending else colour[rows]
    return rows[np.argsort(key, kind="stable")].astype(np.int32), ncol


def effective_sequence(run):
    """The order in which the device relaxes the run's rows: the sequence itself, or colour by colour."""
    return colour_order(run)[0] if tune_of(run)["gs_multicolor"] else sequence(run)


def inputs(run):
    ia, ja, a = matrix(*run["mat"])
    n = len(ia) - 1
    rng = np.random.default_rng(1000 + sum(map(ord, run["mat"][0].__name__)) + 7 * len(sequence(run)) + run["form"])
    b = rng.standard_normal(n)
    u0 = rng.standard_normal(n)
    if run["u0"] == "zeros":
        u0 = np.zeros(n)
    return b, u0


def diagonals(ia, ja, a):
    """Per row: the LAST diagonal entry stored (0.0: none), and whether the reference leaves the row alone."""
    n = len(ia) - 1
    row = np.repeat(np.arange(n), np.diff(ia))
    d = np.zeros(n)
    k = np.flatnonzero(ja == row)
    d[row[k]] = a[k]              # (later hits overwrite earlier ones: storage order)
    return d, ~(np.abs(d) > SMALLREAL)


def reference_sweep(run):
    """The plain sequential sweep of ItrSmootherCSR.c over the run's rows (in the order the device relaxes them) on the run's inputs:
    t = b_i minus the off-diagonal products one after the other in storage order, then the update of the run's form."""
    ia, ja, a = matrix(*run["mat"])
    b, u0 = inputs(run)
    u = np.zeros_like(u0) if run["zero_start"] else u0.copy()
    d, alone = diagonals(ia, ja, a)
    form, w = run["form"], run["w"]
    for i in effective_sequence(run):
        if alone[i]:
            continue
        c = ja[ia[i]:ia[i + 1]]; v = a[ia[i]:ia[i + 1]]
        m = c != i
        t = np.subtract.accumulate(np.concatenate(([b[i]], v[m] * u[c[m]])))[-1]      # (strictly left to right)
        u[i] = t * (1.0 / d[i]) if form == 0 else t / d[i] if form == 1 else w * (t / d[i]) + (1 - w) * u[i]
    return u


# roundings on top of the products and their sum, per path group and form (derivation: tests/test_gpu_sweep_kernels.py)
EXTRA = {"split": {0: 3, 1: 5, 2: 7}, "rows": {0: 3, 1: 2, 2: 4}}


def row_equation(run, u_out):
    """Every swept row's own equation in np.longdouble on the device's output: s = sum_{j != i} a_ij v_j with v_j = u_out[j] where j is swept
    before i, else the input (0 under zero_start) -> (rows, exact, sabs, m) for _libs.sum_bound_ratio; rows that are left alone: m = 0 and
    exact = the input."""
    ld = np.longdouble
    ia, ja, a = matrix(*run["mat"])
    n = len(ia) - 1
    b, u0 = inputs(run)
    uin = np.zeros(n) if run["zero_start"] else u0
    seq = effective_sequence(run)
    pos = np.full(n, -1, dtype=np.int64)
    pos[seq] = np.arange(len(seq))
    d, alone = diagonals(ia, ja, a)
    row = np.repeat(np.arange(n), np.diff(ia))
    keep = (ja != row) & (pos[row] >= 0)
    r, c, v = row[keep], ja[keep], a[keep]
    before = (pos[c] >= 0) & (pos[c] < pos[r])
    x = np.where(before, u_out[c], uin[c]).astype(ld)
    prod = v.astype(ld) * x
    s = np.zeros(n, dtype=ld); sa = np.zeros(n, dtype=ld)
    cnt = np.bincount(r, minlength=n)
    nz = np.flatnonzero(cnt)
    if len(nz):
        start = np.concatenate(([0], np.cumsum(cnt[nz])[:-1]))
        s[nz] = np.add.reduceat(prod, start)
        sa[nz] = np.add.reduceat(np.abs(prod), start)
    rows = np.sort(seq)
    dl = d[rows].astype(ld)
    form, w = run["form"], ld(run["w"])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (b[rows].astype(ld) - s[rows]) / dl
        qa = (np.abs(b[rows]).astype(ld) + sa[rows]) / np.abs(dl)
    if form == 2:
        keepold = (1 - w) * uin[rows].astype(ld)
        exact, sabs = w * q + keepold, np.abs(w) * qa + np.abs(keepold)
    else:
        exact, sabs = q, qa
    group = "rows" if run["path"] in (7, 8) else "split"
    m = cnt[rows] + EXTRA[group][form]
    al = alone[rows]
    exact = np.where(al, uin[rows].astype(ld), exact)
    sabs = np.where(al, ld(0), sabs)
    m = np.where(al, 0, m)
    return rows, exact, sabs, m
