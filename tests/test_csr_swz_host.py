"""The host side of the CSR overlapping Schwarz method (csrc/csr_swz_setup.cpp; no GPU needed): struct layouts, the symmetrised pattern, the
independent set, the blocks and their matrices bit-equal to what the reference leaves (tests/golden/csr_swz.npz, recorded by
tools/gen_golden_csr_swz.py), the dependency levels, the refusals, the defaults, free-after-setup."""
import ctypes as C

import numpy as np
import pytest

import _csr_swz_cases as W
from _libs import T

PARAM_FIELDS = ("print_level", "SWZ_type", "SWZ_maxlvl", "SWZ_mmsize", "SWZ_blksolver")
DATA_FIELDS = ("A", "nblk", "iblock", "jblock", "rhsloc", "rhsloc1", "xloc1", "au", "al", "SWZ_type", "blk_solver", "memt", "mask", "maxbs",
               "maxa", "blk_data", "mumps", "swzparam")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_struct_layouts_are_the_references():
    g = W.golden()
    for struct, fields, rec in ((T.SWZ_param, PARAM_FIELDS, g["layout_param"]), (T.SWZ_data, DATA_FIELDS, g["layout_data"])):
        assert [f for f, _ in struct._fields_] == list(fields)
        assert C.sizeof(struct) == rec[0]
        assert [getattr(struct, f).offset for f in fields] == list(rec[1:])


def test_header_declares_the_same_layouts(tmp_path):
    """sizeof / offsetof of include/fasp_hip.h, compiled as C, against the recorded values."""
    import os
    import subprocess
    from _libs import ROOT
    g = W.golden()
    text = '#include <stdio.h>\n#include <stddef.h>\n#include "fasp_hip.h"\nint main(void) {\n'
    for struct, fields in (("SWZ_param", PARAM_FIELDS), ("SWZ_data", DATA_FIELDS)):
        text += f'    printf("%d", (int)sizeof({struct}));\n' + "".join(f'    printf(" %d", (int)offsetof({struct}, {f}));\n' for f in fields)
        text += '    printf("\\n");\n'
    text += "    return 0;\n}\n"
    src, exe = tmp_path / "l.c", tmp_path / "l"
    src.write_text(text)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert [int(v) for v in lines[0].split()] == list(g["layout_param"])
    assert [int(v) for v in lines[1].split()] == list(g["layout_data"])


def test_param_defaults(fa):
    p = T.SWZ_param(7, 7, 7, 7, 7)
    fa.lib().fasp_param_swz_init(C.byref(p))
    assert (p.print_level, p.SWZ_type, p.SWZ_maxlvl, p.SWZ_mmsize, p.SWZ_blksolver) == (0, 3, 2, 200, 0)


@pytest.mark.parametrize("key", list(W.SWEEP_CASES))
def test_setup_equals_the_reference(fa, key):
    g, c = W.golden(), W.sweep_case(key)
    S = W.LibSwz(fa, c["ia"], c["ja"], c["val"], c["maxlvl"], typ=2)
    assert S.st == 0
    a = S.arrays()
    for k in ("sia", "sja", "mis", "iblock", "jblock", "maxbs", "maxa", "bia", "bja"):
        assert np.array_equal(a[k], g[f"{key}/{k}"]), k
    for k in ("sval", "bval"):
        assert np.array_equal(bits(a[k]), bits(g[f"{key}/{k}"])), k
    D = S.D
    assert D.nblk == len(a["iblock"]) - 1 and not a["mask"].any()
    assert D.rhsloc1.row == D.maxbs and D.xloc1.row == D.maxbs and D.rhsloc1.val and D.xloc1.val
    assert D.SWZ_type == 2 and C.addressof(D.swzparam.contents) == C.addressof(S.prm)
    assert not D.mumps and not D.au and not D.al and not D.rhsloc and D.memt == 0 and D.blk_solver == 0
    for v in range(D.nblk):
        B = D.blk_data[v]
        m = a["iblock"][v + 1] - a["iblock"][v]
        assert (B.row, B.col) == (m, m) and B.nnz == np.ctypeslib.as_array(B.IA, (m + 1,))[m]
    # the restatement is the same partition (what the GPU tests lean on)
    R = c["R"]
    assert np.array_equal(a["iblock"], R.iblock) and np.array_equal(a["jblock"], R.jblock) and np.array_equal(a["mis"], R.mis)
    S.free()
    assert D.nblk == 0 and not D.iblock and not D.jblock and not D.mask and not D.maxa and not D.A.IA and not D.rhsloc1.val and not D.xloc1.val


@pytest.mark.parametrize("key", list(W.SWEEP_CASES))
def test_levels(fa, key):
    c = W.sweep_case(key)
    R = c["R"]
    S = W.LibSwz(fa, c["ia"], c["ja"], c["val"], c["maxlvl"])
    for backward in (False, True):
        nlev, lev = S.levels(backward)
        want = R.levels(backward)
        assert np.array_equal(lev, want) and nlev == want.max() + 1
        R.factors
        order = list(range(R.nblk - 1, -1, -1) if backward else range(R.nblk))
        # no two blocks of one level share a written point, or have one writing what the other reads
        for l in range(nlev):
            grp = [v for v in order if lev[v] == l]
            wr = [set(R.members(v).tolist()) for v in grp]
            rd = [set(np.concatenate([cc for cc, _ in R._out[v]]).tolist()) if len(R._out[v]) else set() for v in grp]
            seen_w, seen_r = set(), set()
            for w_, r_ in zip(wr, rd):
                assert not (w_ & seen_w) and not (w_ & seen_r) and not (r_ & seen_w)
                seen_w |= w_; seen_r |= r_
        # sequential equivalence: a block's level is above that of every earlier block it conflicts with
        lw, mr = {}, {}
        for v in order:
            w_ = R.members(v).tolist()
            r_ = np.concatenate([cc for cc, _ in R._out[v]]).tolist() if len(w_) else []
            need = max([max(lw.get(p, -1), mr.get(p, -1)) for p in w_] + [lw.get(p, -1) for p in r_]) + 1
            assert lev[v] == need
            for p in w_:
                lw[p] = lev[v]
            for p in r_:
                mr[p] = max(mr.get(p, -1), lev[v])
    S.free()


def test_refusals_come_before_any_device_work(fa, capfd):
    L = fa.lib()
    ia, ja, val = W.REFUSED_HUB[0]()
    S = W.LibSwz(fa, ia, ja, val, W.REFUSED_HUB[1])
    assert S.st == T.ERROR_INPUT_PAR and S.D.nblk == 0 and not S.D.iblock and not S.D.blk_data
    assert "257 rows" in capfd.readouterr().out and int(W.golden()["refused/maxbs"]) == 257
    S.free()
    # ... and through the solver: x untouched
    A, keep = T.as_csr(ia, ja, val)
    n = len(ia) - 1
    b = np.ones(n); x = np.full(n, 0.25)
    bv, _ = T.as_vec(b); xv = T.dvector(n, T.dp(x))
    it = fa.param_solver_init()
    prm = T.SWZ_param(); L.fasp_param_swz_init(C.byref(prm)); prm.SWZ_maxlvl = 1
    assert L.fasp_solver_dcsr_krylov_swz(C.byref(A), C.byref(bv), C.byref(xv), C.byref(it), C.byref(prm)) == T.ERROR_INPUT_PAR
    assert np.all(x == 0.25)
    c = W.sweep_case("p5_9x7_l1")
    A, keep = T.as_csr(c["ia"], c["ja"], c["val"])
    n = len(c["ia"]) - 1
    x = np.full(n, 0.25); bv, _ = T.as_vec(np.ones(n)); xv = T.dvector(n, T.dp(x))
    prm.SWZ_maxlvl = -1
    assert L.fasp_solver_dcsr_krylov_swz(C.byref(A), C.byref(bv), C.byref(xv), C.byref(it), C.byref(prm)) == T.ERROR_INPUT_PAR
    S = W.LibSwz(fa, c["ia"], c["ja"], c["val"], -1)
    assert S.st == T.ERROR_INPUT_PAR
    S.free()
    Arect, keep = T.as_csr(c["ia"], c["ja"], c["val"], ncol=n + 1)
    prm.SWZ_maxlvl = 2
    assert L.fasp_solver_dcsr_krylov_swz(C.byref(Arect), C.byref(bv), C.byref(xv), C.byref(it), C.byref(prm)) == T.ERROR_INPUT_PAR
    D = T.SWZ_data(); D.A = Arect
    assert L.fasp_swz_dcsr_setup(C.byref(D), C.byref(prm)) == T.ERROR_INPUT_PAR
    assert np.all(x == 0.25)
    capfd.readouterr()


def test_no_device_no_result(fa):
    """Without a device the solve refuses with ERROR_MISC after the host setup; with one it is the GPU tests' business."""
    if fa.available():
        pytest.skip("a GPU is present")
    c = W.sweep_case("p5_9x7_l2")
    A, keep = T.as_csr(c["ia"], c["ja"], c["val"])
    n = len(c["ia"]) - 1
    x = np.zeros(n); bv, _ = T.as_vec(np.ones(n)); xv = T.dvector(n, T.dp(x))
    it = fa.param_solver_init()
    prm = T.SWZ_param(); fa.lib().fasp_param_swz_init(C.byref(prm))
    assert fa.lib().fasp_solver_dcsr_krylov_swz(C.byref(A), C.byref(bv), C.byref(xv), C.byref(it), C.byref(prm)) == T.ERROR_MISC
    assert np.all(x == 0.0)
    S = W.LibSwz(fa, c["ia"], c["ja"], c["val"], 2)
    st, xs, info, _, _ = S.sweeps(1, c["b"], c["x0"])
    assert st == T.ERROR_MISC and np.array_equal(xs, c["x0"])
    assert fa.lib().fasp_hip_csr_swz_resident_count() == 0
    S.free()
