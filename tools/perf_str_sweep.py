"""Structured smoothers on the device (csrc/str_sweep.hip.h): milliseconds per sweep of Gauss-Seidel ASCEND and SOR(1.1) ASCEND in the level
form, the plane-pipelined form and the ordered form (the natural order handed in as a sequence), of the red-black CPFIRST sweep and of
Jacobi, on P7(n) (x) B_nc -- beside the project's generic path on the same problem for nc = 1: the ascending Gauss-Seidel sweep of the
cycle on fasp_format_dstr_dcsr(A) (the schedule builders and launch half that fasp_hip_csr_sweep runs, here on a resident one-level handle
so that it can be timed with events: fasp_hip_time_kernel kind 10).  One process, alternating rounds, medians reported.  The bytes floor is
on the algorithmic bytes of a sweep: per grid point (nband + 1) nc^2 matrix values (diagonal or its inverse included) and three vector
passes of nc doubles (b, u read, u written); the per-step latency is the time over the launches (level, ordered) or over the pipeline
steps (planes + in-plane levels - 1).

    python tools/perf_str_sweep.py [--cases 128:1,256:1,128:3] [--rounds 5] [--reps 5] [--out profiles/str_sweep.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import faspsolver_amd as fa  # noqa: E402
from faspsolver_amd import _types as T  # noqa: E402
from perf_str_ilu import p7_str  # noqa: E402

P = C.POINTER
GS, SOR, JACOBI = 1, 2, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="128:1,256:1,128:3", help="n:nc on P7(n) (x) B_nc, comma separated")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = fa.lib()
    if not fa.available():
        raise SystemExit("perf_str_sweep: no HIP device")
    L.fasp_hip_amg_create.argtypes = [P(C.c_void_p), P(T.dCSRmat), P(T.AMG_param)]
    L.fasp_hip_time_kernel.restype = C.c_double
    lines = [f"# tools/perf_str_sweep.py on {L.fasp_hip_version().decode()}, {args.rounds} alternating rounds of {args.reps} sweeps, medians"]

    def out(s):
        print(s, flush=True)
        lines.append(s)

    for case in args.cases.split(","):
        n, nc = (int(v) for v in case.split(":"))
        A, keep = p7_str(n, nc)
        ngrid = A.ngrid
        nbytes = 8.0 * ((6 + 1) * nc * nc + 3 * nc) * ngrid
        natural = np.arange(ngrid, dtype=np.int32)
        i = np.arange(ngrid)
        rb = np.where((i % n + (i // n) % n + i // (n * n)) % 2 == 0, 1, -1).astype(np.int32)
        ip = lambda a: a.ctypes.data_as(T.c_int_p)   # noqa: E731
        nlev = 3 * (n - 1) + 1
        # (name, kind, order, mark, weight, forced form, steps)
        runs = [("GS ASCEND, level form", GS, T.ASCEND, None, 1.0, 0, nlev),
                ("GS ASCEND, pipelined form", GS, T.ASCEND, None, 1.0, 1, n + 2 * (n - 1)),
                ("GS ASCEND, ordered form (natural sequence)", GS, T.USERDEFINED, natural, 1.0, 2, nlev),
                ("SOR(1.1) ASCEND, level form", SOR, T.ASCEND, None, 1.1, 0, nlev),
                ("SOR(1.1) ASCEND, pipelined form", SOR, T.ASCEND, None, 1.1, 1, n + 2 * (n - 1)),
                ("SOR(1.1) ASCEND, ordered form (natural sequence)", SOR, T.USERDEFINED, natural, 1.1, 2, nlev),
                ("GS CPFIRST red-black, ordered form", GS, T.CPFIRST, rb, 1.0, -1, 2),
                ("SOR(1.1) CPFIRST red-black, ordered form", SOR, T.CPFIRST, rb, 1.1, -1, 2),
                ("Jacobi", JACOBI, 0, None, 1.0, -1, 1)]
        h = C.c_void_p()
        Acsr = T.dCSRmat()
        if nc == 1:   # the generic path: the cycle's ascending Gauss-Seidel sweep of the converted matrix, resident
            assert L.fasp_format_dstr_dcsr(C.byref(A), C.byref(Acsr)) == 0
            p = fa.param_amg_init(); p.max_levels = 1; p.smoother = T.SMOOTHER_GS; p.print_level = 0
            assert L.fasp_hip_amg_create(C.byref(h), C.byref(Acsr), C.byref(p)) >= 0
        t = {r[0]: [] for r in runs}
        t["generic"] = []
        forms = {}
        for rnd in range(args.rounds + 1):   # round 0 warms every path up (uploads, schedules) and is dropped
            for name, kind, order, mark, w, form, steps in runs:
                L.fasp_hip_tune(b"str_sweep_form", form)
                forms[name] = L.fasp_hip_str_sweep_form(C.byref(A), order, None if mark is None else ip(mark)) if kind != JACOBI else 3
                ms = L.fasp_hip_time_str_sweep(C.byref(A), kind, order, None if mark is None else ip(mark), w, args.reps)
                assert ms > 0, name
                if rnd:
                    t[name].append(ms)
            if nc == 1:
                ms = L.fasp_hip_time_kernel(h, 10, 0, args.reps)
                if rnd:
                    t["generic"].append(ms)
        L.fasp_hip_tune(b"str_sweep_form", -1)
        out(f"\nP7({n}) (x) B{nc}: {ngrid} grid points, nc {nc}, algorithmic bytes {nbytes / 1e6:.1f} MB per sweep")
        for name, kind, order, mark, w, form, steps in runs:
            m = statistics.median(t[name])
            out(f"  {name + ' (form ' + str(forms[name]) + ')':58s}: {m:9.3f} ms  (min {min(t[name]):.3f}, max {max(t[name]):.3f})  "
                f"{nbytes / (m * 1e6):7.1f} GB/s  {steps:4d} steps, {m * 1e3 / steps:8.2f} us per step")
        if nc == 1:
            m = statistics.median(t["generic"])
            out(f"  {'generic GS sweep of the converted CSR matrix (seq_sweep)':58s}: {m:9.3f} ms  (min {min(t['generic']):.3f}, max {max(t['generic']):.3f})  "
                f"{nbytes / (m * 1e6):7.1f} GB/s on the same bytes")
            L.fasp_hip_amg_destroy(h)
            L.fasp_dcsr_free(C.byref(Acsr))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
