"""Structured ILU(0) / ILU(1) on the host (csrc/str_ilu_setup.cpp; no GPU): fasp_ilu_dstr_setup0 / _setup1 give the reference's factor byte
for byte, fasp_precond_dstr_ilu0 / _ilu1 its z bit for bit.

Against the recorded reference (tests/golden/str_ilu.npz, written by tools/gen_golden_str_ilu.py: SHA-256 of every factor, the factor
itself up to 2000 doubles) and, where oracle/_ref is built, against the live reference.  Cases (tests/_str_ilu_cases.py): nc 1 .. 7 on
the 3-D grids 5 x 4 x 3 and 7 x 6 x 5 and the 2-D grids 9 x 7 x 1 and 1 x 8 x 6 (nband 4; the second has nline = ny); for setup0 also a
storage order with +1 before -1, where the reference stays inside its bands.

The applications: the reference's texts for nc = 3, 5 and 7 subtract each product with fasp_blas_darray_axpy_nc3 / _nc5 / _nc7, which run
over nc * nc entries where nc are meant -- they read past the product and write past the row, in the last rows past the vector -- so those
are never called: nc = 3, 5, 7 are held to the numpy restatement of the general block text (_str_ilu_cases.model_apply), which the
generator proves against the reference at nc = 1, 2, 4, 6."""
import ctypes as C

import numpy as np
import pytest

import _libs
import _str_ilu_cases as I
from _libs import T


@pytest.fixture(scope="module")
def L(fa):
    return I.protos(fa.lib())


@pytest.fixture(scope="module")
def G():
    return np.load(I.GOLDEN)


@pytest.fixture(scope="module")
def R():
    lib = _libs.ref()
    return I.protos(lib) if lib is not None else None


HOST = [(key, c, lfil) for key, c, lfils in I.host_cases() for lfil in lfils]


@pytest.mark.parametrize("key,case,lfil", HOST, ids=[f"{k}-ilu{l}" for k, _, l in HOST])
def test_factor_is_the_reference_factor(L, G, R, key, case, lfil):
    snap = I.factor(L, case, lfil)
    assert snap is not None
    nband = len(case["offsets"])
    nline, nplane = I.lines(case["nx"], case["ny"], case["nz"])
    want_offsets = (I.canonical_offsets(case["nx"], case["ny"], case["nz"], nband) if lfil == 0 else
                    [-1, 1, 1 - nline, nline - 1, -nline, nline, nline - nplane, nplane - nline, 1 - nplane, nplane - 1, -nplane, nplane])
    assert snap["offsets"] == want_offsets          # canonical whatever A's storage order is
    assert (snap["nx"], snap["ny"], snap["nz"], snap["nc"], snap["ngrid"]) == (case["nx"], case["ny"], case["nz"], case["nc"], case["diag"].size // case["nc"] ** 2)
    raw = I.factor_bytes(snap)
    k = list(G["fact_keys"]).index(f"{key}/{lfil}")
    whole = f"fact_{key}_{lfil}"
    if whole in G.files:
        got, want = np.frombuffer(raw, dtype=np.uint64), G[whole].view(np.uint64)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, bad[:8]
    assert np.array_equal(I.digest(raw), G["fact_sha"][k])
    if R is not None:
        ref = I.factor(R, case, lfil)
        assert raw == I.factor_bytes(ref)


def test_scalar_setup0_takes_the_plane_band_of_L_from_the_minus_one_band():
    """BlaILUSetupSTR.c:144, kept because bytes are the contract; pinned by a matrix whose -1 and -nplane bands differ."""
    import faspsolver_amd as fa
    lib = I.protos(fa.lib())
    case = I.grid_case((5, 4, 3), 1)
    assert not np.array_equal(case["bands"][0][:40], case["bands"][4][:40])
    snap = I.factor(lib, case, 0)
    d, bands = I.model_setup0_nc1(case, quirk=True)
    assert snap["diag"].tobytes() == d.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(snap["bands"], bands))
    d2, bands2 = I.model_setup0_nc1(case, quirk=False)
    assert not np.array_equal(snap["bands"][4], bands2[4]) and not np.array_equal(snap["diag"], d2)


def _refused(L, case, lfil):
    A, keep = I.as_str(case)
    LU = T.dSTRmat()
    C.memset(C.byref(LU), 0x55, C.sizeof(LU))
    getattr(L, f"fasp_ilu_dstr_setup{lfil}")(C.byref(A), C.byref(LU))
    return bytes(C.string_at(C.byref(LU), C.sizeof(LU))) == bytes(C.sizeof(LU))


def _printed(capfd):
    C.CDLL(None).fflush(None)   # the library prints through C's stdout
    return capfd.readouterr().out


@pytest.mark.parametrize("lfil", [0, 1])
def test_refusals_leave_LU_zeroed(L, lfil, capfd):
    base = I.grid_case((5, 4, 3), 2)
    ngrid, nc2 = 60, 4

    def with_offsets(offsets):
        return dict(base, offsets=list(offsets), bands=[np.zeros(max(ngrid - abs(o), 0) * nc2) for o in offsets])

    assert _refused(L, with_offsets([-1, 1, -5, 5, -20]), lfil)                    # nband 5
    assert _refused(L, with_offsets([-1, 1]), lfil)                                # nband 2
    assert "number of bands for structured ILU is illegal" in _printed(capfd)
    assert _refused(L, with_offsets([-1, 1, -5, 5, -20, 21]), lfil)                # an offset that is none of the six
    assert _refused(L, with_offsets([-1, 1, -5, 5, -20, -20]), lfil)               # one of them twice
    assert _refused(L, with_offsets([-1, 1, -5, 5]), lfil)                         # a 2-D stencil on a 3-D grid: the plane bands are missing
    assert "Illegal offset for ILU" in _printed(capfd)
    line = dict(name="line", nx=1, ny=1, nz=6, nc=1, offsets=[-1, 1, -1, 1], diag=np.ones(6), bands=[np.zeros(5)] * 4)
    assert _refused(L, line, lfil)                                                 # nline = ny = 1
    one = dict(name="one_line", nx=6, ny=1, nz=1, nc=1, offsets=[-1, 1, -6, 6], diag=np.ones(6), bands=[np.zeros(5), np.zeros(5), np.zeros(0), np.zeros(0)])
    assert _refused(L, one, lfil)                                                  # a grid of one line
    big = dict(base, nc=8, diag=np.ones(ngrid * 64), bands=[np.zeros((ngrid - abs(o)) * 64) for o in base["offsets"]])
    assert _refused(L, big, lfil)                                                  # nc outside 1 .. 7
    if lfil == 1:
        swapped = I.grid_case((5, 4, 3), 2, order=I.SWAPPED, tag="_swap")
        assert _refused(L, swapped, 1)                                             # setup1 reads A's bands by position: canonical order only
        assert "Illegal offset for ILU" in _printed(capfd)
    assert I.factor(L, base, lfil) is not None                                     # the matrix itself is fine


APPLY = [(key, c, lfil) for key, c, lfils in I.host_cases() for lfil in lfils
         if (c["nx"], c["ny"], c["nz"]) in I.APPLY_GRIDS and not key.endswith("_swap")]


@pytest.mark.parametrize("key,case,lfil", APPLY, ids=[f"{k}-ilu{l}" for k, _, l in APPLY])
def test_host_preconditioner_bit_for_bit(L, G, R, key, case, lfil):
    snap = I.factor(L, case, lfil)
    r = I.rhs(case)
    z = I.host_apply(L, snap, lfil, r)
    want = G[f"apply_{key}_{lfil}"]
    bad = np.flatnonzero(z.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, (bad[:8], z[bad[:8]], want[bad[:8]])
    if R is not None and case["nc"] in I.REF_APPLY_OK:
        zr = I.host_apply(R, snap, lfil, r)
        assert np.array_equal(z.view(np.uint64), zr.view(np.uint64))


def test_host_preconditioner_on_a_zeroed_factor_touches_nothing(L):
    LU = T.dSTRmat()
    z = np.full(4, 7.0)
    for f in (L.fasp_precond_dstr_ilu0, L.fasp_precond_dstr_ilu1):
        f(T.dp(np.ones(4)), T.dp(z), C.cast(C.pointer(LU), C.c_void_p))
    assert np.all(z == 7.0)
