"""Block Gauss-Seidel sweeps of a dBSRmat on the device (csrc/bsr_sweep.hip.h): the slab plan with one launch per level and with the single
launch beside the per-level k_bsr_seq_level launches the block AMG cycle takes by default, on P7(n) (x) B_nb; a red-black `mark` sweep with
its bytes and TB/s; levels, microseconds per level and plan creation time.  Ends with the GS-smoothed block solve (config 3 of the tests,
tests/test_bsr_amg.py: UA-AMG, VGMRES(30), tol 1e-8) at P7(64) (x) B3 with fasp_hip_tune("bsr_cycle_sweep", 0 / 1), the two settings
alternating over the rounds of one run.  Times are HIP events around `reps` back-to-back sweeps after one warm-up (fasp_hip_bsr_sweep_time);
the solve is a host clock around a call that ends in a device synchronise.

    python tools/perf_bsr_sweep.py [--cases 64:1,64:3,64:5,128:1,128:3,128:5] [--reps 10] [--rounds 4] [--out profiles/bsr_sweep.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import faspsolver_amd as fa  # noqa: E402
from faspsolver_amd import _types as T  # noqa: E402
import _libs  # noqa: E402
import _bsr_smoother_cases as S  # noqa: E402

FORMS = ((0, "k_bsr_seq_level per level"), (1, "slab, launch per level"), (2, "slab, single launch"))


def sweep_time(L, A, order, mark, form, reps):
    info = np.zeros(8)
    mp = None if mark is None else mark.ctypes.data_as(T.c_int_p)
    us = L.fasp_hip_bsr_sweep_time(C.byref(A), order, mp, S.GS, 1.0, form, reps, T.dp(info))
    assert us > 0, (form, us)
    return us, info


def sweeps(args, L, out):
    out(f"{'matrix':16s} {'sweep':10s} {'form':28s} {'levels':>6s} {'us/sweep':>10s} {'us/level':>9s} {'MB moved':>9s} {'TB/s':>6s} {'plan ms':>8s} {'pad %':>6s}")
    table = []
    for spec in args.cases.split(","):
        n, nb = (int(t) for t in spec.split(":"))
        ia, ja, val, _ = _libs.poisson7pt_bsr(n, S.block(nb))
        A, keep = T.as_bsr(ia, ja, val, nb)
        ROW = len(ia) - 1
        i = np.arange(ROW)
        colour = (i % n + (i // n) % n + i // (n * n)) % 2
        rb = np.concatenate([i[colour == 0], i[colour == 1]]).astype(np.int32)
        name = f"P7({n}) (x) B{nb}"
        row = {}
        for form, fname in FORMS:
            us, info = sweep_time(L, A, S.ASCEND, None, form, args.reps)
            row[form] = us
            pad = 100.0 * (info[2] - info[3]) / max(info[2], 1.0)
            out(f"{name:16s} {'ascending':10s} {fname:28s} {int(info[0]):6d} {us:10.1f} {us / info[0]:9.2f} {info[5] / 1e6:9.1f} {info[5] / us / 1e6:6.3f} {info[6]:8.1f} {pad:6.1f}")
        for form, fname in FORMS[1:]:
            us, info = sweep_time(L, A, 0, rb, form, args.reps)
            row["rb%d" % form] = us
            out(f"{name:16s} {'red-black':10s} {fname:28s} {int(info[0]):6d} {us:10.1f} {us / info[0]:9.2f} {info[5] / 1e6:9.1f} {info[5] / us / 1e6:6.3f} {info[6]:8.1f} {0.0:6.1f}")
        table.append((name, int(info[0]), row))
    out("")
    out("ascending sweep, slab forms against the per-level k_bsr_seq_level launches (> 1: the slab form is faster):")
    for name, _, row in table:
        out(f"  {name:16s} launch per level {row[0] / row[1]:5.2f} x   single launch {row[0] / row[2]:5.2f} x   single / per level {row[1] / row[2]:5.2f} x"
            f"   red-black: per level {row['rb1']:8.1f} us, single launch {row['rb2']:8.1f} us")


def narrow(args, L, out):
    """where the single launch can pay: deep schedules of narrow levels -- the rule of the auto form is read off this table"""
    out("")
    out("narrow schedules, ascending Gauss-Seidel sweep (chunks/level: chunks of 64 block rows per dependency level, on average):")
    out(f"{'matrix':18s} {'levels':>6s} {'chunks':>7s} {'chunks/level':>12s} {'per level us':>13s} {'single us':>10s} {'per level / single':>19s} {'auto takes':>11s}")
    cases = [("chain:4096", nb) for nb in (1, 3, 5)] + [(f"p7:{n}", 3) for n in (8, 12, 16, 24, 32, 48)] + [("p7:16", 1), ("p7:16", 5), ("p7:32", 1), ("p7:32", 5)]
    for mat, nb in cases:
        kind, n = mat.split(":")
        ia, ja, val, _ = S.chain(int(n), nb) if kind == "chain" else _libs.poisson7pt_bsr(int(n), S.block(nb))
        A, keep = T.as_bsr(ia, ja, val, nb)
        t = {}
        for form in (1, 2, -1):
            t[form], info = sweep_time(L, A, S.ASCEND, None, form, args.reps)
        name = (f"chain({n})" if kind == "chain" else f"P7({n})") + f" (x) B{nb}"
        out(f"{name:18s} {int(info[0]):6d} {int(info[1]):7d} {info[1] / info[0]:12.2f} {t[1]:13.1f} {t[2]:10.1f} {t[1] / t[2]:19.2f} "
            f"{'single' if info[4] == 2 else 'per level':>11s}")


def solve_ab(args, L, out):
    n, nb = 64, 3
    ia, ja, val, _ = _libs.poisson7pt_bsr(n)
    f = np.sin(0.37 * np.arange((len(ia) - 1) * nb)) + 0.1
    t = {0: [], 1: []}
    its = {}
    x = {}
    try:
        for rnd in range(args.rounds + 1):   # round 0 warms both settings up and is not counted
            for key in (0, 1):
                L.fasp_hip_tune(b"bsr_cycle_sweep", key)
                itp, amgp = _libs.bsr_params(5, 1, 2)
                amgp.smoother, amgp.relaxation = T.SMOOTHER_GS, 1.0
                G = fa.BSRAMG(ia, ja, val, nb, amgp)
                G.solve(f, itp)                 # the hierarchy's schedules / plans are built at their first sweep
                t0 = time.perf_counter()
                st, xs, hist, stats = G.solve(f, itp)
                dt = time.perf_counter() - t0
                G.free()
                its[key], x[key] = st, xs
                if rnd:
                    t[key].append(dt)
    finally:
        L.fasp_hip_tune(b"bsr_cycle_sweep", 0)
    out("")
    out(f"GS-smoothed block solve, P7({n}) (x) B{nb} (UA-AMG VMB, V-cycle, VGMRES(30), tol 1e-8), second solve on a resident hierarchy, {args.rounds} rounds alternating:")
    for key in (0, 1):
        v = 1e3 * np.array(t[key])
        out(f"  bsr_cycle_sweep {key}: {its[key]:3d} iterations, median {np.median(v):8.2f} ms, min {v.min():8.2f}, max {v.max():8.2f}")
    out(f"  solutions equal bit for bit: {np.array_equal(x[0].view(np.uint64), x[1].view(np.uint64))}; "
        f"bsr_cycle_sweep 1 / 0 = {np.median(t[1]) / np.median(t[0]):.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="64:1,64:3,64:5,128:1,128:3,128:5", help="n:nb of P7(n) (x) B_nb")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--no-sweeps", action="store_true", help="skip the large P7(n) table")
    args = ap.parse_args()
    if not fa.available():
        sys.exit("needs a HIP device: nothing here is measured without one")
    L = fa.lib()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out("# tools/perf_bsr_sweep.py: one block Gauss-Seidel sweep, HIP events over %d sweeps after one warm-up; MB moved = the least a sweep moves "
        "(slab or BSR arrays, gathered operands, vectors, the sentinel fill of the single launch)" % args.reps)
    if not args.no_sweeps:
        sweeps(args, L, out)
    narrow(args, L, out)
    if not args.no_solve:
        solve_ab(args, L, out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
