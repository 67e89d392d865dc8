"""plan_coarse_spcg (csrc/coarse_cg.hip.h) and plan_coarse_bsr (csrc/bsr.hip.h) -- the ONE place each that decides which kernel solves the
coarsest level and how it is launched -- checked on the CPU through fasp_hip_coarse_plan / fasp_hip_bsr_coarse_plan against the selection
restated in tests/_coarse_cases.py (expected_kernel, persist_ne, expected_block_kernel): the control flow coarse_spcg() and mgcycle_bsr()
were before the plans existed.  tests/test_gpu_coarse_direct.py holds the kernels that RAN to the same table on the device.

The plans read sizes, the row pointer and the tune keys, never a value: the cases here are row pointers.  Every plan is also held to what
any device demands (LDS <= 160 KiB, threads <= 1024, blocks >= 1), to MaxIt = max(250, min(m^2, 1000)), and to the launch geometry the
kernels are written for (read off small_solvers.hip.h: threads per block of each family, the LDS each form lays out)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import faspsolver_amd as fa
import _libs
import _coarse_cases as cc

PLAN = ("family", "p1", "p2", "threads", "blocks", "lds", "LD", "MaxIt", "lazy", "dev_start", "batch")   # fasp_hip_coarse_plan's layout
BSR_PLAN = ("family", "LV", "cache2", "lds", "threads", "blocks")                                        # fasp_hip_bsr_coarse_plan's
NUM_CU = 256
TUNE0 = dict(cc.DEFAULTS, spcg_grid=0)
SPCG_REG_NT = 256


def _lib():
    L = fa.lib()
    L.fasp_hip_coarse_plan.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.fasp_hip_bsr_coarse_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    return L


def set_tune(**kw):
    for key, v in kw.items():
        assert fa.lib().fasp_hip_tune(key.encode(), int(v)) >= 0, key


@pytest.fixture(autouse=True)
def _defaults_back():
    yield
    set_tune(**TUNE0)


def plan_of(ia, plain_csr=1, num_cu=NUM_CU, with_ia=True):
    ia = np.ascontiguousarray(ia, dtype=np.int32)
    out = (C.c_int * len(PLAN))()
    ptr = ia.ctypes.data_as(C.POINTER(C.c_int)) if with_ia else None
    assert _lib().fasp_hip_coarse_plan(len(ia) - 1, int(ia[-1]), ptr, int(plain_csr), int(num_cu), out) == 0
    return dict(zip(PLAN, list(out)))


def rows(m, nnz):
    """Row pointer of m rows that hold nnz entries, as evenly as they go (nnz >= m: no empty row)."""
    ia = np.zeros(m + 1, dtype=np.int64)
    ia[1:] = np.cumsum(nnz // m + (np.arange(m) < nnz % m))
    assert ia[-1] == nnz
    return ia.astype(np.int32)


def from_lengths(lengths):
    ia = np.zeros(len(lengths) + 1, dtype=np.int64)
    ia[1:] = np.cumsum(lengths)
    return ia.astype(np.int32)


def check(ia, tune, plain_csr=1, num_cu=NUM_CU, small_coarse=True, with_ia=True, tag=""):
    """The plan under the keys `tune` (already set) against the restated table, the device's limits and the kernels' geometry."""
    m, nnz = len(ia) - 1, int(ia[-1])
    p = plan_of(ia, plain_csr, num_cu, with_ia)
    tag = f"{tag} m {m} nnz {nnz} plain {plain_csr} cu {num_cu} {tune} -> {p}"
    want = cc.expected_kernel(ia if with_ia else from_lengths(np.zeros(m, dtype=np.int64)), tune, num_cu, not plain_csr, small_coarse)
    assert (p["family"], p["p1"], p["p2"]) == want, (tag, cc.kernel_name(want))
    # what must hold on any device
    assert 0 <= p["lds"] <= 160 * 1024 and 1 <= p["threads"] <= 1024 and p["blocks"] >= 1, tag
    assert p["MaxIt"] == max(250, min(m * m, 1000)) == cc.max_it(m), tag
    # who reads the verdict lazily, who starts on the device
    f, p1, p2 = want
    assert p["lazy"] == (1 if f <= 4 else 0) and p["dev_start"] == (1 if f in (5, 6) else 0), tag
    # the geometry the kernels are written for
    if f <= 3:
        assert p["LD"] >= m and p["LD"] % 32 == 1 and p["LD"] - m < 32, tag
    else:
        assert p["LD"] == 0, tag
    if f == 1:      # 16 lanes per (column block, copy), a wavefront more when the direction is sent ahead; no dynamic LDS
        assert (p["threads"], p["blocks"], p["lds"]) == (16 * p1 * (4 if p1 == 4 else 2) + 64 * p2, 1, 0), tag
    elif f == 2:    # two doubles per column pair + 4
        assert (p["threads"], p["blocks"], p["lds"]) == (SPCG_REG_NT, 1, 8 * (2 * p1 + 4)), tag
    elif f == 3:    # 128 dense rows of LD doubles + 128
        assert (p["threads"], p["blocks"], p["lds"]) == (64, 1, 8 * (128 * p["LD"] + 128)), tag
    elif f == 4:
        lds = {2: 40 * m + 12 * nnz + 4 * (m + 1), 1: 40 * m, 0: 0}[p1]
        assert (p["threads"], p["blocks"], p["lds"]) == (cc.SMALL_BLOCK, 1, lds) and lds <= 148 * 1024, tag
    elif f == 5:    # p in LDS; block 0 + one wave of blocks of 8 rows, two per CU resident at most
        cap = tune.get("spcg_grid", 0) if tune.get("spcg_grid", 0) > 0 else 2 * num_cu - 1
        assert (p["threads"], p["blocks"], p["lds"]) == (512, 1 + max(1, min((m + 7) // 8, cap)), 8 * m), tag
    elif f == 6:    # one block per CU; p, r, t (and u) in LDS
        assert (p["threads"], p["blocks"], p["lds"]) == (512, num_cu, 8 * m * (4 if p2 else 3)), tag
    else:
        assert (p["threads"], p["blocks"], p["lds"]) == (512 if p1 else cc.SMALL_BLOCK, 1, 0), tag
    if f >= 5:
        b = tune.get("spcg_batch", 16)
        assert p["batch"] == max(1, min(b if b > 0 else 8, 64)), tag
    return p


# ---------------------------------------------------------------------------------------------------------------------
# scalar path, small forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("onewave", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("small_lds", [0, 1])
def test_small_forms(onewave, small_lds):
    tune = dict(TUNE0, small_onewave=onewave, small_lds=small_lds)
    set_tune(**tune)
    seen = set()
    for m in (1, 64, 65, 96, 97, 128, 129, 4096, 4097):
        for nnz in (m, 5 * m):
            seen.add(check(rows(m, nnz), tune)["family"])
    for m in (600, 4096):                               # the stored-values edge of the one-launch solvers
        assert check(rows(m, 131072), tune)["family"] == 4
        assert check(rows(m, 131073), tune)["family"] in (5, 6)
    # the two 148 KiB edges of k_spcg_small: 5 m doubles + 12 nnz + 4 (m + 1) bytes with the matrix, 5 m doubles without
    m = 1000
    nnz = (148 * 1024 - 40 * m - 4 * (m + 1)) // 12
    assert check(rows(m, nnz), tune)["p1"] == (2 if small_lds else 0)
    assert check(rows(m, nnz + 1), tune)["p1"] == (1 if small_lds else 0)
    m = 148 * 1024 // 40
    assert check(rows(m, m), tune)["p1"] == (1 if small_lds else 0)
    assert check(rows(m + 1, m + 1), tune)["p1"] == 0
    assert seen == {4, 6} | ({1} if onewave >= 3 else {2} if onewave == 2 else {3} if onewave == 1 else set())


# ---------------------------------------------------------------------------------------------------------------------
# scalar path, batched forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused,persist", [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("plain_csr", [0, 1])
def test_batched_forms(fused, persist, plain_csr):
    tune = dict(TUNE0, spcg_fused=fused, spcg_persist=persist)
    set_tune(**tune)
    for m in (2048, 2049, 5120, 5121, 8000, 8001):
        p = check(rows(m, max(7 * m, 131073)), tune, plain_csr)
        if not (fused and plain_csr) or m > 8000:
            assert p["family"] == 7
        elif persist and m <= 6144:
            assert p["family"] == 6
        else:
            assert p["family"] == 5
        E = 4 if m <= 2048 else 10 if m <= 5120 else None    # elements per thread of the 512-thread vector passes
        assert p["p1"] == {5: E or 16, 6: 32, 7: E or 0}[p["family"]]


def test_batch_and_grid_keys():
    ia = rows(5000, 35000)
    for batch, grid in ((16, 0), (1, 0), (8, 7), (0, 1), (-3, 100000), (64, 510), (65, 511), (1000, 512)):
        tune = dict(TUNE0, spcg_batch=batch, spcg_grid=grid, spcg_persist=0)
        set_tune(**tune)
        p = check(ia, tune)
        assert p["family"] == 5 and p["blocks"] == 1 + (min(625, grid) if grid > 0 else 511)
        tune["spcg_fused"] = 0
        set_tune(**tune)
        assert check(ia, tune)["family"] == 7


# ---------------------------------------------------------------------------------------------------------------------
# scalar path, persistent form
# ---------------------------------------------------------------------------------------------------------------------
def test_persistent_size_edges():
    set_tune(**TUNE0)
    for m, want in ((5088, (6, 32, 1)), (5089, (6, 32, 0)),      # u in LDS too: 32 m + 1024 <= 160 KiB
                    (6144, (6, 32, 0)), (6145, (5, 16, 0)),      # 16-bit byte offsets into p's LDS image
                    (6400, (5, 16, 0)), (6401, (5, 16, 0))):     # m * 24 <= 150 KiB, behind the bound above
        p = check(rows(m, 7 * m), TUNE0)
        assert (p["family"], p["p1"], p["p2"]) == want, (m, p)
    # without the row pointer the persistent form counts as refused
    assert check(rows(5000, 35000), TUNE0, with_ia=False)["family"] == 5


@pytest.mark.parametrize("m,lengths", cc.ARROW)
def test_persistent_register_budget(m, lengths):
    """The arrowhead cases of the device test: dense leading rows of 30, 46, 54, 61 and 66 slots of 64 entries."""
    set_tune(**TUNE0)
    ia = cc.arrowhead(m, lengths, np.random.default_rng(m + sum(lengths)))[0]
    longest = int(np.diff(ia).max())
    want_ne = {30: 32, 46: 48, 54: 56, 61: 64, 66: 0}[(longest + 63) // 64]
    assert cc.persist_ne(ia, NUM_CU) == want_ne
    p = check(ia, TUNE0)
    assert (p["family"], p["p1"], p["p2"]) == ((6, want_ne, 1 if m <= 5088 else 0) if want_ne else (5, 10 if m <= 5120 else 16, 0))


def test_persistent_refusals():
    set_tune(**TUNE0)
    m = 5000
    ok = np.full(m, 7)
    assert check(from_lengths(ok), TUNE0)["family"] == 6
    empty = ok.copy(); empty[m // 3] = 0                      # an empty row
    assert check(from_lengths(empty), TUNE0)["family"] == 5
    for slots, fam in ((64, 6), (65, 5)):                     # a load above 64 slots
        one = ok.copy(); one[17] = 64 * slots
        assert check(from_lengths(one), TUNE0)["family"] == fam
    # a ninth row on a wave: 2039 of the 2040 waves take one row of 9 slots each, the last wave takes the short rows until it is as loaded
    nw = (NUM_CU - 1) * 8
    for short, fam in ((8, 6), (9, 5)):
        p = check(from_lengths(np.concatenate([np.full(nw - 1, 9 * 64 - 5), np.full(short, 3)])), TUNE0)
        assert p["family"] == fam and (fam != 6 or p["p1"] == 32)
    # the chip: 256 CUs deal; on 2 (8 waves) and 1 (none) a level of the batched path never fits
    big = from_lengths(ok)
    assert check(big, TUNE0, num_cu=256)["family"] == 6
    for cu in (2, 1):
        p = check(big, TUNE0, num_cu=cu)
        assert p["family"] == 5 and p["blocks"] == 1 + (2 * cu - 1)


def test_each_switch_off_and_on():
    ia_small, ia_mid, ia_big = rows(100, 500), rows(1000, 7000), rows(5000, 35000)
    for key, ia, off, on in (("small_onewave", ia_small, 4, 3), ("small_lds", ia_mid, 4, 4), ("spcg_fused", ia_big, 7, 6),
                             ("spcg_persist", ia_big, 5, 6)):
        for v, fam in ((0, off), (1, on), (0, off)):
            tune = dict(TUNE0, **{key: v})
            set_tune(**tune)
            assert check(ia, tune, tag=key)["family"] == fam, (key, v)
    for v, lvl in ((0, 0), (1, 2)):
        set_tune(small_lds=v)
        assert check(ia_mid, dict(TUNE0, small_lds=v))["p1"] == lvl


def test_bad_arguments_are_refused():
    L = _lib()
    out = (C.c_int * len(PLAN))()
    assert L.fasp_hip_coarse_plan(0, 0, None, 1, NUM_CU, out) < 0 and L.fasp_hip_coarse_plan(5, 5, None, 1, NUM_CU, None) < 0
    assert L.fasp_hip_bsr_coarse_plan(0, 5, 5, out) < 0 and L.fasp_hip_bsr_coarse_plan(3, 0, 5, out) < 0
    assert L.fasp_hip_bsr_coarse_plan(3, 5, 5, None) < 0


# ---------------------------------------------------------------------------------------------------------------------
# block path
# ---------------------------------------------------------------------------------------------------------------------
def bsr_plan(nb, ROW, NNZ):
    out = (C.c_int * len(BSR_PLAN))()
    assert _lib().fasp_hip_bsr_coarse_plan(nb, ROW, NNZ, out) == 0
    return dict(zip(BSR_PLAN, list(out)))


def _block_cases():
    G = []
    for nb in range(1, 8):
        top = 4096 // nb
        G += [(nb, r, 5 * r) for r in (1, 2, top, top + 1) if 5 * r * nb * nb <= 131072 or r > top]
        G += [(nb, r, r) for r in (top, top + 1)]                                     # the n = 4096 edge
        nz = 131072 // (nb * nb)
        G += [(nb, min(top, nz), nz), (nb, min(top, nz), nz + 1)]                      # the NNZ nb^2 = 131072 edge
        lv = 140 * 1024 // (8 * (cc.GM_RESTART + 2) * nb)
        G += [(nb, lv, 5 * lv), (nb, lv + 1, 5 * (lv + 1))]                            # the basis in LDS: 216 n <= 140 KiB
    G += [(3, r, 5 * r) for r in (170, 171, 341, 342, 188, 189, 221, 222)]             # nb = 3: registers to 512 rows, cache2 to 1024 rows and to 140 KiB
    return G


@pytest.mark.parametrize("small_lds", [1, 0])
def test_block_plan(small_lds):
    set_tune(small_lds=small_lds)
    seen = set()
    for nb, ROW, NNZ in _block_cases():
        p = bsr_plan(nb, ROW, NNZ)
        want = cc.expected_block_kernel(nb, ROW, NNZ, small_lds)
        tag = (nb, ROW, NNZ, small_lds, p)
        assert (p["family"], p["LV"], p["cache2"]) == want, (tag, want)
        assert 0 <= p["lds"] <= 160 * 1024 and p["threads"] <= 1024 and p["blocks"] >= 1, tag
        n = ROW * nb
        if p["family"] == 8:
            lds = 8 * (cc.GM_RESTART + 2) * n + (max(n - cc.SMALL_BLOCK, 0) * cc.GM_CB * 28 if p["cache2"] else 0)
            assert (p["threads"], p["blocks"], p["lds"]) == (cc.SMALL_BLOCK, 1, lds if p["LV"] else 0), tag
            assert p["lds"] <= 140 * 1024, tag
        else:
            assert n > 4096 or NNZ * nb * nb > 131072, tag
        seen.add(want)
    # (cache2 = 1 means basis + blocks fit 140 KiB: without the basis in LDS only when small_lds is off)
    assert seen == ({(8, 1, 0), (8, 1, 1), (8, 0, 0), (9, 0, 0)} if small_lds else {(8, 0, 0), (8, 0, 1), (9, 0, 0)})
    # the cache2 rule by hand: nb = 3 only, n <= 1024, basis + blocks <= 140 KiB (n <= 565 with the basis in LDS)
    assert bsr_plan(3, 188, 940)["cache2"] == 1 and bsr_plan(3, 189, 945)["cache2"] == 0
    assert bsr_plan(3, 170, 850)["cache2"] == 1 and bsr_plan(2, 282, 1410)["cache2"] == 0 and bsr_plan(4, 141, 705)["cache2"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# FASP_HIP_SMALL_COARSE=0 is read once per process: a fresh child
# ---------------------------------------------------------------------------------------------------------------------
_CHILD = """
import sys, numpy as np
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import test_coarse_plan as t
for m in (1, 64, 65, 128, 129, 1000, 4096, 4097):
    for fused, persist in ((1, 1), (1, 0), (0, 0)):
        tune = dict(t.TUNE0, spcg_fused=fused, spcg_persist=persist)
        t.set_tune(**tune)
        p = t.check(t.rows(m, 5 * m), tune, small_coarse=False)
        assert p["family"] == (7 if not fused else 6 if persist else 5), (m, tune, p)
t.set_tune(**t.TUNE0)
# 2 CUs = 8 waves still deal: 64 rows of one slot, eight per wave; a 65th row is the ninth of some wave; 1 CU has no wave to deal to
assert t.check(t.rows(64, 320), t.TUNE0, num_cu=2, small_coarse=False)["family"] == 6
assert t.check(t.rows(65, 325), t.TUNE0, num_cu=2, small_coarse=False)["family"] == 5
assert t.check(t.rows(64, 320), t.TUNE0, num_cu=1, small_coarse=False)["family"] == 5
for nb, ROW in ((1, 10), (3, 100), (7, 585)):
    assert t.bsr_plan(nb, ROW, 5 * ROW)["family"] == 9
print("CHILD OK")
"""


def test_small_coarse_switch_in_a_child_process():
    root = _libs.ROOT
    env = dict(os.environ, FASP_HIP_SMALL_COARSE="0")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(tests=os.path.join(root, "tests"), root=root)], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:]); print(r.stderr[-3000:])
    assert r.returncode == 0 and "CHILD OK" in r.stdout
