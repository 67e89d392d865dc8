"""Cases of the block (BSR) smoother entries (fasp_smoother_dbsr_*, ItrSmootherBSR.c) shared by tools/gen_golden_bsr_smoothers.py (which
records the reference's results in tests/golden/bsr_smoothers.npz), tests/test_bsr_smoother_host.py and tests/test_gpu_bsr_smoother.py:
the matrices, the visiting sequences, the inputs, a numpy restatement of the sweeps in the reference's order of operations, a restatement
of the plan rule of csrc/bsr_sweep_plan.h, and the ctypes call of an entry (the reference and the library share the signatures).

Fixture layout:  <matrix>/b, <matrix>/u0   the inputs of every case on that matrix and on its scaled form (u0: the random start; a zero
                                           start is not stored)
                 <case id>/out             u after the reference's entry"""
import ctypes as C
import functools
import os

import numpy as np

import _libs
from _libs import T

GOLDEN = os.path.join(_libs.ROOT, "tests", "golden", "bsr_smoothers.npz")
ASCEND, DESCEND = 12, 21
GS, SOR, IDENT, JACOBI = 0, 1, 2, 3   # 0 .. 2: `kind` of fasp_hip_bsr_smoother_apply

# entry -> (kind, arguments after (A, b, u), fixed sequence or None)
ENTRIES = {
    "jacobi": (JACOBI, (), "asc"),
    "gs": (GS, ("order", "mark"), None), "gs1": (GS, ("order", "mark", "dinv"), None),
    "gs_ascend": (GS, ("dinv",), "asc"), "gs_ascend1": (IDENT, (), "asc"),
    "gs_descend": (GS, ("dinv",), "desc"), "gs_descend1": (IDENT, (), "desc"),
    "gs_order1": (GS, ("dinv", "mark"), None), "gs_order2": (IDENT, ("mark", "work"), None),
    "sor": (SOR, ("order", "mark", "w"), None), "sor1": (SOR, ("order", "mark", "dinv", "w"), None),
    "sor_ascend": (SOR, ("dinv", "w"), "asc"), "sor_descend": (SOR, ("dinv", "w"), "desc"),
    "sor_order": (SOR, ("dinv", "mark", "w"), None),
}
SELF_INVERTING = ("jacobi", "gs", "sor")   # invert the diagonal blocks themselves
MARK_ORDERS = ("perm", "rb", "ident", "rev")


# ---------------------------------------------------------------------------------------------------------------------------
# matrices -> (ia, ja, val, nb), read-only
# ---------------------------------------------------------------------------------------------------------------------------
def block(nb):
    """B_nb: _libs.B3 for nb = 3, else a nonsymmetric diagonally dominant block"""
    if nb == 3:
        return _libs.B3
    return (nb + 2.0) * np.eye(nb) + 0.5 * np.triu(np.ones((nb, nb)), 1) + 0.25 * np.tril(np.ones((nb, nb)), -1)


def chain(ROW, nb=2, seed=11):
    """Block tridiagonal: one dependency level per row in either direction; ROW = 63, 64, 65, 129 cross the chunk edges"""
    rng = np.random.default_rng(seed + ROW)
    ia = [0]; ja = []
    for i in range(ROW):
        ja += [j for j in (i - 1, i, i + 1) if 0 <= j < ROW]
        ia.append(len(ja))
    ia = np.array(ia, dtype=np.int32); ja = np.array(ja, dtype=np.int32)
    val = rng.standard_normal((len(ja), nb, nb))
    rows = np.repeat(np.arange(ROW), np.diff(ia))
    val[ja == rows] += 4.0 * nb * np.eye(nb)
    return ia, ja, val.reshape(-1), nb


def odd(nb, seed=5):
    """70 block rows that the generators of _libs do not have: empty rows (9, 64), diagonal-only rows (10, 65), row 20 with TWO stored
    diagonal blocks (the last one counts for the inversion, both are skipped by the sweeps), columns unsorted, and a pattern that is not
    symmetric in both position orders: row 3 reads 40 but 40 does not read 3, row 50 reads 7 but 7 does not read 50."""
    ROW = 70
    rng = np.random.default_rng(seed + nb)
    cols = []
    for i in range(ROW):
        if i in (9, 64):
            cols.append([])
        elif i in (10, 65):
            cols.append([i])
        else:
            c = [int(j) for j in rng.choice(ROW, size=int(rng.integers(2, 7)), replace=False) if j != i and j not in (3, 50)]
            c.append(i)
            rng.shuffle(c)
            cols.append(c)
    cols[3] = [40, 3, 1] if 40 not in cols[3] else cols[3]
    cols[40] = [j for j in cols[40] if j != 3]
    cols[50] = [7, 60, 50] if 7 not in cols[50] else cols[50]
    cols[7] = [j for j in cols[7] if j != 50]
    cols[20] = [20, 33, 20, 2]
    assert 40 in cols[3] and 3 not in cols[40] and 7 in cols[50] and 50 not in cols[7]
    ia = np.zeros(ROW + 1, dtype=np.int32)
    ia[1:] = np.cumsum([len(c) for c in cols])
    ja = np.array([j for c in cols for j in c], dtype=np.int32)
    assert any(np.any(np.diff(c) < 0) for c in cols if len(c) > 1)
    val = rng.standard_normal((len(ja), nb, nb))
    rows = np.repeat(np.arange(ROW), np.diff(ia))
    val[ja == rows] += 3.0 * nb * np.eye(nb)
    return ia, ja, val.reshape(-1), nb


def scaled(M):
    """Dinv A: identity diagonal blocks up to rounding, for the entries that assume them.  Elementwise products summed in a fixed order, so
    the matrix is the same on every machine."""
    ia, ja, val, nb = M
    d = diaginv(M).reshape(-1, nb, nb)
    blocks = val.reshape(-1, nb, nb)
    rows = np.repeat(np.arange(len(ia) - 1), np.diff(ia))
    out = np.zeros_like(blocks)
    for k in range(nb):
        out = out + d[rows][:, :, k:k + 1] * blocks[:, k:k + 1, :]
    return ia, ja, out.reshape(-1), nb


@functools.lru_cache(maxsize=None)
def matrix(name):
    kind, *args = name.split(":")
    if kind == "chain":
        M = chain(int(args[0]))
    elif kind == "p7":      # p7:<n>:<nb>
        M = _libs.poisson7pt_bsr(int(args[0]), block(int(args[1])))
    elif kind == "ragged":
        c = _libs.ragged_case(int(args[0]), "square")
        M = (c["ia"], c["ja"], c["val"], c["nb"])
    elif kind == "odd":
        M = odd(int(args[0]))
    elif kind == "scaled":  # scaled:<any other name>
        M = scaled(matrix(":".join(args)))
    else:
        raise KeyError(name)
    ia, ja, val, nb = M
    out = (np.ascontiguousarray(ia, dtype=np.int32), np.ascontiguousarray(ja, dtype=np.int32), np.ascontiguousarray(val, dtype=np.float64), nb)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def grid_of(name):
    parts = name.split(":")
    while parts[0] == "scaled":
        parts = parts[1:]
    return int(parts[1]) if parts[0] == "p7" else None


@functools.lru_cache(maxsize=None)
def _diaginv_cached(name):
    return _diaginv(matrix(name))


def _diaginv(M):
    """The inverse diagonal blocks as the library's host code computes them (fasp_smat_inv's operations; tests/test_gpu_bsr_kernels.py and
    the generator compare it with the reference's).  Rows without a diagonal block get the identity."""
    import faspsolver_amd as fa
    ia, ja, val, nb = M
    A, keep = T.as_bsr(ia, ja, val, nb)
    d = np.zeros((len(ia) - 1) * nb * nb)
    fa.lib().fasp_smoother_dbsr_jacobi_setup(C.byref(A), T.dp(d))
    d = d.reshape(-1, nb, nb)
    rows = np.repeat(np.arange(len(ia) - 1), np.diff(ia))
    has = np.zeros(len(ia) - 1, dtype=bool)
    has[rows[ja == rows]] = True
    d[~has] = np.eye(nb)
    return d.reshape(-1)


def diaginv(M_or_name):
    return _diaginv_cached(M_or_name) if isinstance(M_or_name, str) else _diaginv(M_or_name)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(b, u0) of every case on the matrix; a scaled matrix shares them with the matrix it is made of"""
    if name.startswith("scaled:"):
        return inputs(name[len("scaled:"):])
    ia, ja, val, nb = matrix(name)
    rng = np.random.default_rng(abs(hash_name(name)) % (2 ** 31))
    n = (len(ia) - 1) * nb
    b, u0 = rng.standard_normal(n), rng.standard_normal(n)
    b.setflags(write=False); u0.setflags(write=False)
    return b, u0


def hash_name(name):
    h = 7
    for ch in name:
        h = (h * 131 + ord(ch)) % 1000003
    return h


def mark_of(name, order):
    """The user sequence of an order: a seeded permutation (deep schedule), red-black of the grid (two levels), identity, reversed"""
    ROW = len(matrix(name)[0]) - 1
    if order == "perm":
        return np.random.default_rng(1000 + hash_name(name)).permutation(ROW).astype(np.int32)
    if order == "ident":
        return np.arange(ROW, dtype=np.int32)
    if order == "rev":
        return np.arange(ROW - 1, -1, -1, dtype=np.int32)
    if order == "rb":
        n = grid_of(name)
        i = np.arange(ROW)
        colour = (i % n + (i // n) % n + i // (n * n)) % 2
        return np.concatenate([i[colour == 0], i[colour == 1]]).astype(np.int32)
    return None


def sequence(case):
    """The rows in visiting order (None: the entry does nothing)"""
    ROW = len(matrix(case["mat"])[0]) - 1
    fixed = ENTRIES[case["entry"]][2]
    order = fixed or case["order"]
    if order in MARK_ORDERS:
        return mark_of(case["mat"], order)
    if order == "asc":
        return np.arange(ROW, dtype=np.int32)
    if order == "desc":
        return np.arange(ROW - 1, -1, -1, dtype=np.int32)
    return None   # "none": mark NULL and an order that is neither ASCEND nor DESCEND


def order_args(case):
    """(order, mark) as the entry takes them"""
    o = case["order"]
    if o in MARK_ORDERS:
        return 0, mark_of(case["mat"], o)
    return {"asc": ASCEND, "desc": DESCEND, "none": 5}[o], None


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
def _case(mat, entry, order="asc", w=1.0, u0="rand"):
    kind = ENTRIES[entry][0]
    if kind == IDENT and not mat.startswith("scaled:"):
        mat = "scaled:" + mat
    cid = f"{mat}|{entry}|{order}|{w}|{u0}"
    return dict(id=cid, mat=mat, entry=entry, order=order, w=w, u0=u0)


def _cases():
    out = []
    for ROW in (1, 63, 64, 65, 129):
        m = f"chain:{ROW}"
        out += [_case(m, "gs", "asc"), _case(m, "gs1", "desc"), _case(m, "sor_order", "perm", 1.3)]
    m = "p7:6:1"   # every entry on the scalar path (nb = 1), in every order
    out += [_case(m, "jacobi"), _case(m, "gs", "asc"), _case(m, "gs", "desc", u0="zero"), _case(m, "gs", "perm"), _case(m, "gs", "none"),
            _case(m, "gs1", "asc"), _case(m, "gs1", "rb"), _case(m, "gs1", "ident"), _case(m, "gs1", "rev"), _case(m, "gs1", "desc"),
            _case(m, "gs_ascend"), _case(m, "gs_ascend1"), _case(m, "gs_descend"), _case(m, "gs_descend1"),
            _case(m, "gs_order1", "perm"), _case(m, "gs_order1", "rb", u0="zero"), _case(m, "gs_order2", "perm"), _case(m, "gs_order2", "rb"),
            _case(m, "sor", "asc", 1.3), _case(m, "sor", "perm", 1.0), _case(m, "sor1", "desc", 1.3), _case(m, "sor1", "rb", 1.0),
            _case(m, "sor1", "none", 1.3), _case(m, "sor_ascend", w=1.0), _case(m, "sor_ascend", w=1.3), _case(m, "sor_descend", w=1.3),
            _case(m, "sor_descend", w=1.0, u0="zero"), _case(m, "sor_order", "perm", 1.3), _case(m, "sor_order", "rb", 1.0)]
    m = "p7:6:3"   # ... and every entry once on a block path
    out += [_case(m, "jacobi"), _case(m, "gs", "perm"), _case(m, "gs", "none"), _case(m, "gs1", "asc"), _case(m, "gs1", "ident"), _case(m, "gs1", "rb"),
            _case(m, "gs_ascend", u0="zero"), _case(m, "gs_ascend1"), _case(m, "gs_descend"), _case(m, "gs_descend1"),
            _case(m, "gs_order1", "perm"), _case(m, "gs_order2", "rb"), _case(m, "sor", "asc", 1.3), _case(m, "sor1", "desc", 1.3),
            _case(m, "sor_ascend", w=1.0), _case(m, "sor_descend", w=1.3, u0="zero"), _case(m, "sor_order", "perm", 1.3)]
    for nb in (2, 4, 5, 6, 7):
        m = f"p7:6:{nb}"
        out += [_case(m, "gs_ascend"), _case(m, "sor_descend", w=1.3), _case(m, "gs_order1", "perm"), _case(m, "gs_ascend1")]
    m = "p7:10:3"   # 28 levels
    out += [_case(m, "gs", "asc"), _case(m, "sor_order", "perm", 1.3), _case(m, "gs_order1", "rb", u0="zero")]
    m = "ragged:3"
    out += [_case(m, "gs1", "asc"), _case(m, "sor1", "desc", 1.3), _case(m, "gs_order1", "perm"), _case(m, "gs", "desc")]
    for nb in (1, 3):
        m = f"odd:{nb}"
        out += [_case(m, "gs1", "asc"), _case(m, "gs1", "desc"), _case(m, "gs1", "ident"), _case(m, "gs1", "rev"), _case(m, "gs_order1", "perm"),
                _case(m, "sor1", "perm", 1.3), _case(m, "sor_descend", w=1.0, u0="zero"), _case(m, "gs_order2", "perm"), _case(m, "gs_descend1")]
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids)
    return out


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
MATRICES = sorted({c["mat"] for c in CASES})


def start_of(case):
    b, u0 = inputs(case["mat"])
    return b, (u0.copy() if case["u0"] == "rand" else np.zeros_like(u0))


# ---------------------------------------------------------------------------------------------------------------------------
# one entry through ctypes: the library and the compiled reference share names and signatures
# ---------------------------------------------------------------------------------------------------------------------------
def protos(L):
    M, V, D, I = C.POINTER(T.dBSRmat), C.POINTER(T.dvector), T.c_double_p, T.c_int_p
    sig = {"order": C.c_int, "mark": I, "dinv": D, "w": C.c_double, "work": D}
    for name, (_, args, _) in ENTRIES.items():
        f = getattr(L, "fasp_smoother_dbsr_" + name)
        f.argtypes, f.restype = [M, V, V] + [sig[a] for a in args], None
    L.fasp_smoother_dbsr_jacobi_setup.argtypes, L.fasp_smoother_dbsr_jacobi_setup.restype = [M, D], None
    return L


def given_diaginv(case):
    """the diaginv argument of the entries that take one"""
    return diaginv(case["mat"]).copy()


def call_entry(L, case):
    """u after fasp_smoother_dbsr_<entry> of L (prototypes set by protos)"""
    ia, ja, val, nb = matrix(case["mat"])
    A, keep = T.as_bsr(ia.copy(), ja.copy(), val.copy(), nb)
    b, u = start_of(case)
    bv, bk = T.as_vec(b.copy())
    uv = T.dvector(len(u), T.dp(u))
    order, mark = order_args(case)
    d = given_diaginv(case)
    work = np.zeros(max(nb, 1))
    vals = {"order": order, "mark": None if mark is None else mark.ctypes.data_as(T.c_int_p), "dinv": T.dp(d), "w": float(case["w"]),
            "work": T.dp(work)}
    getattr(L, "fasp_smoother_dbsr_" + case["entry"])(C.byref(A), C.byref(bv), C.byref(uv), *[vals[a] for a in ENTRIES[case["entry"]][1]])
    return u


# ---------------------------------------------------------------------------------------------------------------------------
# numpy restatement: a plain loop in the reference's order (ItrSmootherBSR.c; BlaSmallMat.c: fasp_blas_smat_ymAx, _mxv, _aAxpby)
# ---------------------------------------------------------------------------------------------------------------------------
def _mxv(Dm, x, nb):
    if nb == 6:   # the default branch of fasp_blas_smat_mxv: temp = 0.0; temp += ...
        t = np.zeros(nb)
        for j in range(nb):
            t = t + Dm[:, j] * x[j]
        return t
    t = Dm[:, 0] * x[0]
    for j in range(1, nb):
        t = t + Dm[:, j] * x[j]
    return t


def restated(case):
    ia, ja, val, nb = matrix(case["mat"])
    kind = ENTRIES[case["entry"]][0]
    b, u = start_of(case)
    w = float(case["w"])
    d = diaginv(case["mat"]).reshape(-1, nb, nb)   # (the self-inverting entries: rows of their cases all hold a diagonal block)
    blocks = val.reshape(-1, nb, nb)
    seq = sequence(case)
    if seq is None:
        return u
    src = u.copy() if kind == JACOBI else u   # Jacobi reads the old iterate throughout
    for i in seq:
        i = int(i)
        bt = b[i * nb:(i + 1) * nb].copy()
        for k in range(ia[i], ia[i + 1]):
            j = int(ja[k])
            if j == i:
                continue
            x = src[j * nb:(j + 1) * nb]
            m = blocks[k][:, 0] * x[0]
            for c in range(1, nb):
                m = m + blocks[k][:, c] * x[c]
            bt -= m
        if kind == IDENT:
            new = bt
        elif kind in (GS, JACOBI):
            new = bt * d[i][0, 0] if nb == 1 else _mxv(d[i], bt, nb)
        elif nb == 1:
            new = (1.0 - w) * u[i:i + 1] + w * (bt * d[i][0, 0])
        else:   # fasp_blas_smat_aAxpby(w, Dinv, bt, 1 - w, u_i)
            y = u[i * nb:(i + 1) * nb].copy()
            if w == 0:
                y *= 1.0 - w
            else:
                tmp = (1.0 - w) / w
                if tmp != 1.0:
                    y *= tmp
                for c in range(nb):
                    y = y + d[i][:, c] * bt[c]
                if w != 1.0:
                    y *= w
            new = y
        u[i * nb:(i + 1) * nb] = new
    return u


# ---------------------------------------------------------------------------------------------------------------------------
# restatement of the plan rule (csrc/bsr_sweep_plan.h)
# ---------------------------------------------------------------------------------------------------------------------------
def plan_rule(ia, ja, seq):
    """-> (level of every row, {row: [(column, reads new) of its off-diagonal entries in storage order]})"""
    ROW = len(ia) - 1
    pos = np.empty(ROW, dtype=np.int64)
    pos[np.asarray(seq)] = np.arange(ROW)
    level = np.zeros(ROW, dtype=np.int64)
    entries = {}
    for i in seq:
        i = int(i)
        e = [(int(j), bool(pos[j] < pos[i])) for j in ja[ia[i]:ia[i + 1]] if j != i]
        entries[i] = e
        level[i] = 1 + max((level[j] for j, new in e if new), default=-1)
    return level, entries
