"""plan_csr (csrc/device_csr.hip.h) -- the ONE place that decides which CSR kernel a launch runs, with which tile size, blocks per CU, XCD
map and index form -- checked on the CPU through fasp_hip_csr_plan against expected_plan (tests/_csr_cases.py): the if-chain launch_csr was
before the plan existed, restated line by line.  All CSR kernels agree bit for bit, so a wrong selection fails no numerical test: it shows
only as time.  Here it fails.

The grid of operator traits sits on both sides of every threshold of the chain and reaches every kernel instantiation; it runs for the
eight row operations, whole operators and row windows, with and without a partials array, under the default tune keys and under every key
that switches a kernel family off or asks for another form."""
import ctypes as C

import numpy as np
import pytest

import faspsolver_amd as fa
import _csr_cases as cc

OPS = range(8)
# (key, value) lists; the defaults are restored after each
TUNE_STATES = [(), (("compress", 0),), (("gen2", 0),), (("gen2", 1),), (("xtile", 0),), (("sell", 0),), (("estream", 0),), (("estream", 2),),
               (("ja16", 0),), (("rpl", 1),), (("rpl", 2),), (("lds_tab", 0),), (("lds_tab", 3),), (("kind", 0),), (("kind", 2),),
               (("split_rows", 64),)]


def _lib():
    L = fa.lib()
    L.fasp_hip_csr_plan.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    return L


def _plan(L, t, op, windowed, want_partials):
    """-> (dict of cc.PLAN + bytes, the family code kernel_family reports for the operator)"""
    traits = (C.c_int * len(cc.TRAITS))(*[int(t[k]) for k in cc.TRAITS])
    out = (C.c_int * (len(cc.PLAN) + 1))()
    nbytes = C.c_double(-1.0)
    assert L.fasp_hip_csr_plan(traits, op, int(windowed), int(want_partials), out, C.byref(nbytes)) == 0
    p = dict(zip(cc.PLAN, list(out)))
    p["bytes"] = nbytes.value
    return p, out[len(cc.PLAN)]


def _t(**kw):
    return dict(cc.TRAIT_DEFAULTS, **kw)


def _grid():
    """Operator traits: (name, traits).  Neighbouring entries named a / b sit on the two sides of one threshold."""
    G = []
    add = lambda name, **kw: G.append((name, _t(**kw)))
    R = 3000
    # --- plain, long rows (kind 0): k_csr_rows<L>, k_csr_estream<L>; 16-bit columns absolute / relative / absent
    for lanes in (2, 4, 8, 16, 32, 64, 3):
        add(f"rows_L{lanes}", row=R, col=R, nnz=100 * R, kind=0, lanes=lanes, dpos=1)
    es = dict(row=R, col=R, kind=0, lanes=16, ja16=1, es_tab=1, es_W=64, es_nc=700, dpos=1)
    for name, nnz in (("avg100", 100 * R), ("avg128a", 128 * R - 1), ("avg128b", 128 * R), ("avg256a", 256 * R - 1), ("avg256b", 256 * R),
                      ("avg512a", 512 * R - 1), ("avg512b", 512 * R)):      # lanes of k_csr_estream at 128, 256, 512; its rule at 256
        add(f"es_{name}", nnz=nnz, **es)
    add("es_relative", nnz=100 * R, **dict(es, col=200000, jbase=1, es_ja16=1))
    add("es_no_tables", nnz=100 * R, **dict(es, es_tab=0))
    add("es_no_ja16", nnz=100 * R, **dict(es, ja16=0))
    add("es_dup_diag", nnz=100 * R, **dict(es, dup_diag=1))
    for kind in (1, 3):                                                       # retired kinds; their row bases are dropped BEFORE they retire
        add(f"retired{kind}", row=R, col=200000, nnz=100 * R, kind=kind, lanes=32, ja16=1, jbase=1)
        add(f"retired{kind}_abs", row=R, col=R, nnz=100 * R, kind=kind, lanes=32, ja16=1)
    # --- plain, short and mid rows (kind 2): k_csr_lstream at nnz <= 7.6 row, then k_csr_xtile / k_csr_sell / k_csr_wstream2, k_csr_wstream
    S = 4005                                                                  # 7.6 * 4005 = 30438
    k2 = dict(row=S, col=S, kind=2)
    for dpos, dup in ((1, 0), (0, 0), (1, 1)):                                # a Jacobi sweep without usable diagonal positions
        d = dict(k2, dpos=dpos, dup_diag=dup)
        add(f"short_a_d{dpos}{dup}", nnz=int(7.6 * S), **d)
        add(f"short_b_d{dpos}{dup}", nnz=int(7.6 * S) + 1, **d)
        add(f"mid_xtile_d{dpos}{dup}", nnz=30 * S, lja16=1, ntcols=9000, **d)
        add(f"mid_xtile_sell_d{dpos}{dup}", nnz=30 * S, lja16=1, ntcols=9000, sell_code=1, sell_nv=500, sell_nslice=63, sell_slots=140000, **d)
        add(f"mid_sell_d{dpos}{dup}", nnz=30 * S, sell_code=1, sell_nv=500, sell_nslice=63, sell_slots=140000, **d)
        add(f"mid_ws2_d{dpos}{dup}", nnz=30 * S, ja16=1, **d)
    for wrows, wcap in ((64, 1024), (32, 512), (32, 1024)):
        add(f"wstream_{wrows}_{wcap}", nnz=30 * S, wrows=wrows, wcap=wcap, dpos=1, **k2)
        add(f"wstream_{wrows}_{wcap}_short", nnz=5 * S, wrows=wrows, wcap=wcap, dpos=1, **k2)
    add("mid_relative", row=S, col=300000, kind=2, nnz=30 * S, ja16=1, jbase=1)      # row bases on an operator the row kernel does not serve
    # --- byte dictionary (kind 4): U at mean row 8.5 and 20.0
    D = 2000
    for name, nnz in (("8a", 17000), ("8b", 17001), ("16a", 40000), ("16b", 40001)):
        add(f"dict_{name}", row=D, col=D, nnz=nnz, kind=2, code=1, dpos=1)
    add("dict_rect", row=D, col=900, nnz=12000, kind=2, code=1, rowbase=1)
    # --- row patterns (kind 5): the pair sweeps, k_csr_rowpat's three table forms
    P = 1000
    sq = dict(row=P, col=P, nnz=7 * P, kind=2, pat=1, dpos=1, npat=27, npent=216)
    add("p4", nxrows=40, **sq)
    add("p4_no_pairs", **sq)                                                  # nxrows -1: k_csr_rowpat
    for npat, npent in ((64, 512), (65, 512), (64, 513), (512, 2048), (513, 2048), (512, 2049)):
        add(f"rowpat_{npat}_{npent}", **dict(sq, npat=npat, npent=npent))
    rect = dict(row=P, col=400, kind=2, pat=1, rowbase=1, npat=30, npent=300, nxrows=10)
    add("p5_a", nnz=4500, **rect)                                             # 0.1 * rp5_max * row
    add("p5_b", nnz=4501, **rect)
    add("p5_no_pairs", nnz=4000, **dict(rect, nxrows=-1))
    # tiles of 512 rows: slabs / strips from 8 * 64 tiles on; strips need a plane of 8 k tiles that fits the launch four times
    for name, rows in (("511", 511 * 512), ("512", 512 * 512)):
        for plane in (0, 4096, 2048, 4096 + 512, 69632):                      # none; 8 tiles; too short; no multiple of 8 tiles; 136 tiles: 4 * 136 > 512
            add(f"p4_tiles{name}_plane{plane}", **dict(sq, row=rows, col=rows, nnz=7 * rows, nxrows=0, plane=plane))
            add(f"p5_tiles{name}_plane{plane}", **dict(rect, row=rows, col=rows // 2, nnz=3 * rows, plane=plane))
            add(f"rowpat_tiles{name}_plane{plane}", **dict(sq, row=rows, col=rows, nnz=7 * rows, plane=plane))
    for name, rows in (("543", 543 * 512), ("544", 544 * 512)):               # 4 * (69632 / 512) = 544 tiles
        add(f"p4_tiles{name}_plane69632", **dict(sq, row=rows, col=rows, nnz=7 * rows, nxrows=0, plane=69632))
    for name, rows in (("31", 31 * 512), ("32", 32 * 512)):                   # k_csr_rowpat5 takes strips below 8 * 64 tiles too
        add(f"p5_tiles{name}_plane4096", **dict(rect, row=rows, col=rows // 2, nnz=3 * rows, plane=4096))
    for name, rows in (("a", (96 << 20) // 8), ("b", (96 << 20) // 8 + 1)):   # the streaming hint: a vector of more than 96 MiB
        add(f"p4_nt_{name}", **dict(sq, row=rows, col=rows, nnz=7 * rows, nxrows=0))
    return G


GRID = _grid()


@pytest.fixture(scope="module")
def plans():
    """Every plan of the grid under every tune state, computed once: {state: [(name, op, windowed, want_partials, got, family code, want)]}"""
    L = _lib()
    out = {}
    for state in TUNE_STATES:
        rows = []
        try:
            for key, value in state:
                assert L.fasp_hip_tune(key.encode(), value) == 0
            for name, t in GRID:
                for op in OPS:
                    for windowed in (False, True):
                        for want in (False, True):
                            got, fam = _plan(L, t, op, windowed, want)
                            rows.append((name, op, windowed, want, got, fam, cc.expected_plan(t, op, windowed, want, dict(state))))
        finally:
            for key, _ in state:
                L.fasp_hip_tune(key.encode(), cc.TUNE_DEFAULTS[key])
        out[state] = rows
    return out


@pytest.mark.parametrize("state", TUNE_STATES, ids=lambda s: "-".join(f"{k}{v}" for k, v in s) or "defaults")
def test_plan_is_the_launch_chain(plans, state):
    for name, op, windowed, want, got, _fam, exp in plans[state]:
        assert got == exp, (name, op, windowed, want)


def test_reports_read_the_plan(plans):
    """fasp_hip_amg_kernel_info and fasp_hip_matrix_op report the family of the plan of y = M x on the whole operator -- whatever the
    operation asked about -- under every tune state."""
    for state, rows in plans.items():
        mxv = {name: got["family"] for name, op, windowed, want, got, _f, _e in rows if op == 0 and not windowed and not want}
        for name, _op, _w, _p, _got, fam, _e in rows:
            assert fam == mxv[name], (state, name)


def test_grid_reaches_every_kernel_and_both_sides_of_every_threshold(plans):
    seen = {got["kernel"] for rows in plans.values() for *_x, got, _f, _e in rows}
    assert seen == set(range(len(cc.KERNELS))), sorted(cc.KERNELS[k] for k in set(range(len(cc.KERNELS))) - seen)
    d = {(name, op, windowed, want): got for name, op, windowed, want, got, _f, _e in plans[()]}
    e2 = {(name, op, windowed, want): got for name, op, windowed, want, got, _f, _e in plans[(("estream", 2),)]}
    kernel = lambda name, op=0, table=d: cc.KERNELS[table[(name, op, False, False)]["kernel"]]
    get = lambda name, field, op=0: d[(name, op, False, False)][field]
    assert (kernel("short_a_d10"), kernel("short_b_d10")) == ("lstream", "wstream2")
    assert (kernel("p5_a"), kernel("p5_b")) == ("rowpat5", "rowpat_2_1")
    assert [kernel(f"dict_{n}") for n in ("8a", "8b", "16a", "16b")] == ["dict8_8", "dict8_16", "dict8_16", "dict8_24"]
    assert [kernel(f"es_{n}") for n in ("avg128a", "avg128b", "avg256a", "avg256b")] == ["estream4", "estream8", "estream8", "rows16"]
    assert [kernel(f"es_{n}", table=e2) for n in ("avg256a", "avg256b", "avg512a", "avg512b")] == ["estream8", "estream16", "estream16", "estream32"]
    assert [kernel(f"rowpat_{n}") for n in ("64_512", "65_512", "64_513", "512_2048", "513_2048", "512_2049")] == \
        ["rowpat_2_1", "rowpat_1_1", "rowpat_1_1", "rowpat_1_1", "rowpat_0_1", "rowpat_0_1"]
    assert (get("p4_nt_a", "nt"), get("p4_nt_b", "nt")) == (1, 5)
    assert (get("p4_tiles511_plane0", "xcd_map"), get("p4_tiles512_plane0", "xcd_map")) == (16, -1)
    assert (get("p5_tiles511_plane0", "xcd_map"), get("p5_tiles512_plane0", "xcd_map")) == (16, -1)
    assert [get(f"p4_tiles512_plane{p}", "tpp") for p in (0, 4096, 2048, 4608, 69632)] == [0, 8, 0, 0, 0]
    assert (get("p4_tiles512_plane4096", "xcd_map"), get("p4_tiles512_plane4096", "bpc"), get("p4_tiles512_plane0", "bpc")) == (-2, 3, 5)
    assert (get("p4_tiles543_plane69632", "tpp"), get("p4_tiles544_plane69632", "tpp")) == (0, 136)
    assert (get("p5_tiles31_plane4096", "tpp"), get("p5_tiles32_plane4096", "tpp")) == (0, 8)
    assert get("rowpat_tiles512_plane4096", "tpp") == 16                     # tiles of 256 rows
    # the operation is part of the decision: a Jacobi sweep without usable diagonal positions, a smoother on a transfer operator's form
    assert (kernel("mid_ws2_d00"), kernel("mid_ws2_d00", 5), kernel("short_a_d00", 5)) == ("wstream2", "rows8", "lstream")
    assert (kernel("p5_a", cc.OP_L1DIAG), get("mid_sell_d10", "fused_zr", 5)) == ("rowpat_2_1", 0)
    assert d[("mid_sell_d10", 5, False, True)]["fused_zr"] == 1 and d[("rows_L8", 5, False, True)]["fused_zr"] == 0
    # row windows keep the row kernel; the row bases go when the row kernel does
    assert cc.KERNELS[d[("es_avg100", 0, True, False)]["kernel"]] == "rows16" and kernel("es_avg100", cc.OP_MXV_DOT) == "rows16"
    assert (get("es_relative", "jbase"), get("mid_relative", "ja16"), get("retired1", "ja16"), get("retired1_abs", "ja16")) == (1, 0, 0, 1)


def test_family_of_the_case_generators_agrees():
    """family() -- what the irregular matrices of this folder are built for -- is the plan's family of a freshly uploaded operator."""
    L = _lib()
    for rid, run in cc.all_cases():
        c = run["fn"](*run["args"])
        t = cc.fresh_traits(c["coding"], c["nrow"], c["ncol"], len(c["ja"]))
        fam = cc.family(c["coding"], c["nrow"], c["ncol"], len(c["ja"]))
        assert cc.expected_plan(t, 0, False, False)["family"] == fam == _plan(L, t, 0, False, False)[0]["family"], rid


def test_bad_arguments_are_refused():
    L = _lib()
    out = (C.c_int * (len(cc.PLAN) + 1))()
    traits = (C.c_int * len(cc.TRAITS))()
    assert L.fasp_hip_csr_plan(None, 0, 0, 0, out, None) < 0 and L.fasp_hip_csr_plan(traits, 0, 0, 0, None, None) < 0
    assert L.fasp_hip_csr_plan(traits, 8, 0, 0, out, None) < 0 and L.fasp_hip_csr_plan(traits, -1, 0, 0, out, None) < 0
