"""The structured block Gauss-Seidel (Schwarz) smoother on the device (csrc/str_swz.hip.h): milliseconds of the factorisation of every patch
(k_str_swz_factor) and per sweep (k_str_swz_level, one launch per level) on P7(n) (x) B_nc with the six geometric neighbours, in the natural
order and in the 12-colour order, beside the project's Gauss-Seidel sweep of the same matrix (fasp_hip_time_str_sweep: ASCEND in the plan's
form, and the natural order as a sequence in the ordered form, whose launch per level is the comparison for the per-level cost).  One
process, alternating rounds, medians reported.  Bytes moved: per visit its factor (8 m^2), its pivots (4 m), the matrix rows of its members
(8 m (nband + 1) nc), b and u of its members read and u written (24 m) and the neighbour list.  Then the time to solution of
fasp_solver_dstr_krylov_blockgs against _krylov_diag and _krylov_ilu on the same matrix (BiCGstab, tol 1e-8, wall clock, setup included).

    python tools/perf_str_swz.py [--cases 128:1,64:3] [--rounds 3] [--reps 3] [--out profiles/str_swz.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import faspsolver_amd as fa  # noqa: E402
from faspsolver_amd import _types as T  # noqa: E402
from perf_str_ilu import p7_str  # noqa: E402

P = C.POINTER
GS = 1


def geometric(n):
    i = np.arange(n ** 3)
    x, y, z = i % n, (i // n) % n, i // (n * n)
    cols = [np.where(x > 0, i - 1, -1), np.where(x < n - 1, i + 1, -1), np.where(y > 0, i - n, -1), np.where(y < n - 1, i + n, -1),
            np.where(z > 0, i - n * n, -1), np.where(z < n - 1, i + n * n, -1)]
    return np.ascontiguousarray(np.stack(cols, axis=1), dtype=np.int32)


def colour12(n):
    i = np.arange(n ** 3)
    return np.argsort((i % n + 3 * ((i // n) % n) + 7 * (i // (n * n))) % 12, kind="stable").astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="128:1,64:3", help="n:nc on P7(n) (x) B_nc, comma separated")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = fa.lib()
    if not fa.available():
        raise SystemExit("perf_str_swz: no HIP device")
    lines = [f"# tools/perf_str_swz.py on {L.fasp_hip_version().decode()}, {args.rounds} alternating rounds of {args.reps} factorisations / sweeps, medians"]

    def out(s):
        print(s, flush=True)
        lines.append(s)

    ip = lambda a: a.ctypes.data_as(T.c_int_p)   # noqa: E731
    for case in args.cases.split(","):
        n, nc = (int(v) for v in case.split(":"))
        A, keep = p7_str(n, nc)
        ngrid = A.ngrid
        geo = geometric(n)
        members = 1 + (geo >= 0).sum(axis=1)
        m = members * nc
        nbytes = float(np.sum(8.0 * m * m + 4.0 * m + 8.0 * m * (7 * nc + 3) + 4.0 * 7))
        orders = {"natural order": None, "12-colour order": colour12(n)}
        natural = np.arange(ngrid, dtype=np.int32)
        tf, ts, info_of = {k: [] for k in orders}, {k: [] for k in orders}, {}
        tg = {"GS ASCEND (the plan's form)": [], "GS, ordered form (natural sequence)": []}
        for rnd in range(args.rounds + 1):   # round 0 warms every path up and is dropped
            for key, order in orders.items():
                f, s, info = C.c_double(0), C.c_double(0), (C.c_int * 8)()
                st = L.fasp_hip_time_str_swz(C.byref(A), ip(geo), 6, None if order is None else ip(order), args.reps, C.byref(f), C.byref(s), info)
                assert st == 0, (key, st)
                info_of[key] = list(info)
                if rnd:
                    tf[key].append(f.value); ts[key].append(s.value)
            for key, (order, mark, form) in {"GS ASCEND (the plan's form)": (T.ASCEND, None, -1), "GS, ordered form (natural sequence)": (T.USERDEFINED, natural, 2)}.items():
                L.fasp_hip_tune(b"str_sweep_form", form)
                ms = L.fasp_hip_time_str_sweep(C.byref(A), GS, order, None if mark is None else ip(mark), 1.0, args.reps)
                L.fasp_hip_tune(b"str_sweep_form", -1)
                assert ms > 0, key
                if rnd:
                    tg[key].append(ms)
        out(f"\nP7({n}) (x) B{nc}: {ngrid} grid points, nc {nc}, six geometric neighbours, m = {m.min()} .. {m.max()}, factor store "
            f"{8.0 * ((ngrid + 63) // 64 * 64) * m.max() ** 2 / 1e6:.1f} MB, bytes moved per sweep {nbytes / 1e6:.1f} MB")
        for key in orders:
            info = info_of[key]
            f, s = statistics.median(tf[key]), statistics.median(ts[key])
            out(f"  {key:18s}: factor {f:9.3f} ms (min {min(tf[key]):.3f}, max {max(tf[key]):.3f}), sweep {s:9.3f} ms (min {min(ts[key]):.3f}, max {max(ts[key]):.3f})  "
                f"{nbytes / (s * 1e6):7.1f} GB/s  {info[0]:5d} levels (widest {info[3]}), {s * 1e3 / info[0]:8.2f} us per level; interchanges {info[5]}, stopped {info[6]}")
        for key, v in tg.items():
            mth = statistics.median(v)
            steps = 3 * (n - 1) + 1
            out(f"  {key:40s}: {mth:9.3f} ms per sweep (min {min(v):.3f}, max {max(v):.3f}), {steps} levels" + (f", {mth * 1e3 / steps:8.2f} us per level" if "ordered" in key else ""))
        # time to solution, BiCGstab, tol 1e-8, zero guess, wall clock
        b = np.random.default_rng(n * 10 + nc).standard_normal(ngrid * nc)
        itp = fa.param_solver_init(); itp.itsolver_type = T.SOLVER_BiCGstab; itp.tol = 1e-8; itp.maxit = 2000; itp.print_level = 0; itp.stop_type = T.STOP_REL_RES
        ilup = T.ILU_param(); ilup.print_level = 0; ilup.ILU_type = 1; ilup.ILU_lfil = 0
        L.fasp_solver_dstr_krylov_ilu.argtypes = [P(T.dSTRmat), P(T.dvector), P(T.dvector), P(T.ITS_param), P(T.ILU_param)]
        nv = T.ivector(geo.size, ip(geo))
        solves = [("fasp_solver_dstr_krylov_diag", lambda bv, xv: L.fasp_solver_dstr_krylov_diag(C.byref(A), C.byref(bv), C.byref(xv), C.byref(itp))),
                  ("fasp_solver_dstr_krylov_ilu, ILU(0)", lambda bv, xv: L.fasp_solver_dstr_krylov_ilu(C.byref(A), C.byref(bv), C.byref(xv), C.byref(itp), C.byref(ilup)))]
        for key, order in orders.items():
            ov = None if order is None else T.ivector(order.size, ip(order))
            solves.append((f"fasp_solver_dstr_krylov_blockgs, {key}",
                           lambda bv, xv, ov=ov: L.fasp_solver_dstr_krylov_blockgs(C.byref(A), C.byref(bv), C.byref(xv), C.byref(itp), C.byref(nv), None if ov is None else C.byref(ov))))
        for name, fn in solves:
            walls, its = [], None
            for rnd in range(2):
                x = np.zeros_like(b)
                bv, kb = T.as_vec(b)
                xv = T.dvector(x.size, T.dp(x))
                t0 = time.perf_counter()
                its = fn(bv, xv)
                walls.append(time.perf_counter() - t0)
            out(f"  BiCGstab to 1e-8, {name:52s}: {its:5d} iterations, {min(walls) * 1e3:10.1f} ms wall (second of two runs: {walls[1] * 1e3:.1f})")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
