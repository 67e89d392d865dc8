"""Structured ILU triangular solves on the device (csrc/str_ilu.hip.h): milliseconds per application z = U^-1 L^-1 r of the level form
and of the plane-pipelined form of k_str_tri, beside the project's generic path on the same problem -- fasp_ilu_dcsr_setup ILUk(0) on
fasp_format_dstr_dcsr(A), applied by k_ilu_flow / k_ilu_level (csrc/ilu.hip.h) -- in one process, in alternating rounds, medians reported.
Achieved bytes per second are on the algorithmic bytes: per row (nL + nU + 1) nc^2 matrix values plus four vector passes of nc doubles.
One end-to-end line: BiCGstab + ILU(0) through fasp_solver_dstr_krylov_ilu against fasp_solver_dstr_krylov_diag on the same system.

    python tools/perf_str_ilu.py [--cases 128:1:0,256:1:0,128:3:0] [--rounds 5] [--reps 5] [--solve 256] [--out profiles/str_ilu_apply.txt]
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

P = C.POINTER
B3 = np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 2.0]])


def p7_str(n, nc):
    """P7(n) (x) B as a dSTRmat in canonical band order (B = 1 for nc = 1, B3 for nc = 3, else I + a shifted ramp)."""
    ngrid = n ** 3
    B = np.ones((1, 1)) if nc == 1 else B3 if nc == 3 else np.eye(nc) + 0.1 * np.arange(nc * nc).reshape(nc, nc) / (nc * nc)
    i = np.arange(ngrid)
    inside = {1: i % n < n - 1, n: (i // n) % n < n - 1, n * n: i // (n * n) < n - 1}
    diag = np.ascontiguousarray(np.broadcast_to(6.0 * B, (ngrid, nc, nc))).reshape(-1)
    offsets, bands = [], []
    for d in (1, n, n * n):
        k = np.where(inside[d], -1.0, 0.0)[:ngrid - d]
        blk = (k[:, None, None] * B[None]).reshape(-1)
        offsets += [-d, d]
        bands += [blk, blk.copy()]
    return T.as_str(n, n, n, nc, offsets, diag, bands)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="128:1:0,256:1:0,128:3:0", help="n:nc:lfil on P7(n) (x) B_nc, comma separated")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solve", type=int, default=256, help="n of the end-to-end BiCGstab solve (0: none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = fa.lib()
    if not fa.available():
        raise SystemExit("perf_str_ilu: no HIP device")
    lines = [f"# tools/perf_str_ilu.py on {L.fasp_hip_version().decode()}, {args.rounds} alternating rounds of {args.reps} applications, medians"]

    def out(s):
        print(s, flush=True)
        lines.append(s)

    for case in args.cases.split(","):
        n, nc, lfil = (int(v) for v in case.split(":"))
        A, keep = p7_str(n, nc)
        LU = T.dSTRmat()
        t0 = time.perf_counter()
        getattr(L, f"fasp_ilu_dstr_setup{lfil}")(C.byref(A), C.byref(LU))
        t_setup = time.perf_counter() - t0
        assert LU.ngrid == A.ngrid
        nterm = 3 if lfil == 0 else 6
        nbytes = 8.0 * ((2 * nterm + 1) * nc * nc + 4 * nc) * A.ngrid
        # the generic path: scalar ILUk(0) of the converted matrix
        Acsr = T.dCSRmat()
        assert L.fasp_format_dstr_dcsr(C.byref(A), C.byref(Acsr)) == 0
        prm = T.ILU_param(); L.fasp_param_ilu_init(C.byref(prm))
        prm.ILU_type, prm.ILU_lfil = T.ILUk, 0
        d = T.ILU_data()
        assert L.fasp_ilu_dcsr_setup(C.byref(Acsr), C.byref(d), C.byref(prm)) == 0
        info = (C.c_double * 6)()
        t = {"level": [], "pipe": [], "generic": []}
        forms = {}
        for rnd in range(args.rounds + 1):   # round 0 warms every path up (uploads, schedules) and is dropped
            for name, form in (("level", 0), ("pipe", 1)):
                L.fasp_hip_tune(b"str_ilu_form", form)
                forms[name] = L.fasp_hip_str_ilu_form(C.byref(LU), lfil)
                ms = L.fasp_hip_time_str_ilu(C.byref(LU), lfil, args.reps)
                assert ms > 0
                if rnd:
                    t[name].append(ms)
            us = L.fasp_hip_ilu_time(C.byref(d), 1, args.reps, info) + L.fasp_hip_ilu_time(C.byref(d), 2, args.reps, info)
            if rnd:
                t["generic"].append(us / 1e3)
        L.fasp_hip_tune(b"str_ilu_form", -1)
        out(f"\nILU({lfil}) of P7({n}) (x) B{nc}: {A.ngrid} grid points, nc {nc}, host setup {t_setup:.2f} s, algorithmic bytes {nbytes / 1e6:.1f} MB per application")
        for name in ("level", "pipe", "generic"):
            m = statistics.median(t[name])
            what = {"level": f"k_str_tri level form (form {forms['level']})", "pipe": f"k_str_tri pipelined form (form {forms['pipe']})",
                    "generic": "generic ILUk(0) of the converted CSR matrix (k_ilu_flow)"}[name]
            out(f"  {what:62s}: {m:9.3f} ms  (min {min(t[name]):.3f}, max {max(t[name]):.3f})  {nbytes / (m * 1e6):7.1f} GB/s")
        L.fasp_ilu_data_free(C.byref(d))
        L.fasp_dcsr_free(C.byref(Acsr))
        L.fasp_dstr_free(C.byref(LU))

    if args.solve > 0:
        n = args.solve
        A, keep = p7_str(n, 1)
        b = np.sin(0.37 * np.arange(A.ngrid)) + 0.1
        for entry in ("krylov_ilu", "krylov_diag"):
            x = np.zeros_like(b)
            bv, kb = T.as_vec(b)
            xv = T.dvector(x.size, T.dp(x))
            p = T.ITS_param()
            p.print_level = 0; p.itsolver_type = T.SOLVER_BiCGstab; p.stop_type = T.STOP_REL_RES; p.restart = 25; p.maxit = 2000; p.tol = 1e-8; p.abstol = 1e-18
            ip = T.ILU_param(); L.fasp_param_ilu_init(C.byref(ip)); ip.ILU_lfil = 0
            t0 = time.perf_counter()
            if entry == "krylov_ilu":
                it = L.fasp_solver_dstr_krylov_ilu(C.byref(A), C.byref(bv), C.byref(xv), C.byref(p), C.byref(ip))
            else:
                it = L.fasp_solver_dstr_krylov_diag(C.byref(A), C.byref(bv), C.byref(xv), C.byref(p))
            ms = (time.perf_counter() - t0) * 1e3
            out(f"BiCGstab on P7({n}), tol 1e-8, fasp_solver_dstr_{entry}: {it} iterations, {ms:.1f} ms wall (host setup and uploads included)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
