"""ILU triangular solves on the device (csrc/ilu.hip.h): levels of L and U, the form that ran, microseconds and bytes per
solve, beside the compiled reference's single-thread fasp_precond_ilu on the same factor and, in the same process, one
ascending plus one descending sequential sweep of A (the smoother's sweep on a resident one-level handle, timed after
the first call so its schedule build is excluded; for ILU(0) of the 7-point operator the sweep pair has the same
dependency graph as the two triangular solves).

    python tools/perf_ilu.py [--cases 128:0,256:0,128:2] [--reps 20] [--out profiles/ilu_apply.txt]
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

P = C.POINTER


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="128:0,256:0,128:2", help="n:lfil of ILUk on P7(n), comma separated")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-ref", action="store_true", help="skip the reference's CPU application")
    args = ap.parse_args()
    L = fa.lib()
    if not fa.available():
        raise SystemExit("perf_ilu: no HIP device")
    ref = None if args.no_ref else _libs.ref()
    if ref is not None:
        ref.fasp_precond_ilu.argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
        ref.fasp_precond_ilu.restype = None
    L.fasp_hip_amg_create.argtypes = [P(C.c_void_p), P(T.dCSRmat), P(T.AMG_param)]
    L.fasp_hip_time_kernel.restype = C.c_double
    lines = [f"# tools/perf_ilu.py on {L.fasp_hip_version().decode()}, reps {args.reps}"]

    def out(s):
        print(s, flush=True)
        lines.append(s)

    for case in args.cases.split(","):
        n, lfil = (int(v) for v in case.split(":"))
        A = T.dCSRmat(); b = T.dvector(); u = T.dvector()
        assert L.fasp_hip_poisson7pt(n, n, n, C.byref(A), C.byref(b), C.byref(u)) == 0
        prm = T.ILU_param(); L.fasp_param_ilu_init(C.byref(prm))
        prm.ILU_type, prm.ILU_lfil = T.ILUk, lfil
        d = T.ILU_data()
        t0 = time.perf_counter()
        assert L.fasp_ilu_dcsr_setup(C.byref(A), C.byref(d), C.byref(prm)) == 0
        t_setup = time.perf_counter() - t0
        out(f"\nILUk({lfil}) of P7({n}): {A.row} rows, factor {d.nzlu - A.row - 1} off-diagonal entries, host setup {t_setup:.2f} s")
        tot = 0.0
        for which, name in ((1, "L"), (2, "U")):
            info = (C.c_double * 6)()
            us = L.fasp_hip_ilu_time(C.byref(d), which, args.reps, info)
            tot += us
            out(f"  {name}: {int(info[0])} levels, {'single launch' if info[1] else 'level launches'}: {us:9.1f} us per solve, "
                f"{info[2] / 1e6:8.1f} MB moved ({info[2] / (us * 1e3):6.0f} GB/s), slab {int(info[3])} entries for {int(info[4])}, "
                f"longest row {int(info[5])}")
        out(f"  L + U: {tot:9.1f} us")
        if ref is not None:
            r = np.sin(0.37 * np.arange(A.row)) + 0.1
            z = np.zeros(A.row)
            t0 = time.perf_counter()
            ref.fasp_precond_ilu(r.ctypes.data_as(T.c_double_p), z.ctypes.data_as(T.c_double_p), C.cast(C.byref(d), C.c_void_p))
            t_ref = time.perf_counter() - t0
            out(f"  reference fasp_precond_ilu (one CPU thread): {t_ref * 1e6:11.1f} us  ({t_ref * 1e6 / tot:.0f}x the device)")
        # the sweep pair on a resident one-level handle (ascending + descending Gauss-Seidel = SOR's graph)
        p = fa.param_amg_init(); p.max_levels = 1; p.smoother = T.SMOOTHER_SOR; p.print_level = 0
        h = C.c_void_p()
        if L.fasp_hip_amg_create(C.byref(h), C.byref(A), C.byref(p)) >= 0:
            L.fasp_hip_time_kernel(h, 10, 0, 1); L.fasp_hip_time_kernel(h, 11, 0, 1)   # schedules built here
            fw = L.fasp_hip_time_kernel(h, 10, 0, args.reps) * 1e3
            bw = L.fasp_hip_time_kernel(h, 11, 0, args.reps) * 1e3
            out(f"  sweep pair of A (resident schedule): ascending {fw:9.1f} us + descending {bw:9.1f} us = {fw + bw:9.1f} us; "
                f"ILU / sweep pair = {tot / (fw + bw):.2f}")
            L.fasp_hip_amg_destroy(h)
        L.fasp_ilu_data_free(C.byref(d))
        L.fasp_hip_free_system(C.byref(A), C.byref(b), C.byref(u))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
