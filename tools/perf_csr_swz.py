"""The CSR overlapping Schwarz method on the device (csrc/csr_swz.hip.h): the host setup (sympart, shift, fasp_swz_dcsr_setup: wall clock),
milliseconds of the factorisation of every block (k_csr_swz_factor) and of one forward and one backward sweep (k_csr_swz_level, one launch
per dependency level) with the size of the factor store and the bytes a sweep moves at least (per block its factor, per member its index,
b read, x written and the two offsets, per outside entry its column, its value and the x it reads), then CG with SWZ_type 3 to 1e-8 beside
fasp_solver_dcsr_krylov_diag and fasp_solver_dcsr_krylov_ilu (ILUk(0)) on the same system (wall clock, setup included).

    python tools/perf_csr_swz.py [--cases p7:64,var:64,p7:128] [--levels 2,3] [--reps 3] [--out profiles/csr_swz.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import faspsolver_amd as fa  # noqa: E402
from faspsolver_amd import _types as T  # noqa: E402


def system(kind, n):
    p7 = fa.poisson7pt(n)
    if kind == "p7":
        return p7[0], p7[1], p7[2], f"P7({n})"
    ia, ja, a, _ = fa.poisson7pt_var(n, p7)
    return ia, ja, a, f"variable-coefficient P7({n}) (contrast 9)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="p7:64,var:64,p7:128")
    ap.add_argument("--levels", default="2,3", help="SWZ_maxlvl values")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = fa.lib()
    if not fa.available():
        raise SystemExit("perf_csr_swz: no HIP device")
    sink = open(args.out, "w") if args.out else None

    def out(s):
        print(s, flush=True)
        if sink:
            sink.write(s + "\n"); sink.flush()

    out(f"# tools/perf_csr_swz.py on {L.fasp_hip_version().decode()}, {args.reps} factorisations / sweeps per figure (HIP events), solves: wall clock")
    for case in args.cases.split(","):
        kind, n = case.split(":")
        ia, ja, a, name = system(kind, int(n))
        m = len(ia) - 1
        A, keep = T.as_csr(ia, ja, a)
        b = np.random.default_rng(int(n)).standard_normal(m)
        out(f"\n{name}: {m} rows, {len(ja)} entries")
        for lvl in (int(v) for v in args.levels.split(",")):
            prm = T.SWZ_param(); L.fasp_param_swz_init(C.byref(prm)); prm.SWZ_maxlvl = lvl; prm.SWZ_type = 3
            t0 = time.perf_counter()
            D = T.SWZ_data()
            D.A = L.fasp_dcsr_sympart(C.byref(A))
            L.fasp_dcsr_shift(C.byref(D.A), 1)
            st = L.fasp_swz_dcsr_setup(C.byref(D), C.byref(prm))
            t_host = time.perf_counter() - t0
            assert st == 0, st
            sizes = np.diff(np.ctypeslib.as_array(D.iblock, (D.nblk + 1,)))
            ms, nbytes, info = (C.c_double * 3)(), (C.c_double * 2)(), (C.c_int * 8)()
            t0 = time.perf_counter()
            st = L.fasp_hip_time_csr_swz(C.byref(D), args.reps, ms, nbytes, info)
            t_first = time.perf_counter() - t0
            assert st == 0, st
            out(f"  SWZ_maxlvl {lvl}: {D.nblk} blocks of {sizes.min()} .. {sizes.max()} rows (mean {sizes.mean():.1f}); host setup {t_host:.2f} s; "
                f"upload + schedule + first factorisation + timing {t_first:.2f} s")
            out(f"    factor {ms[0]:10.3f} ms, store {nbytes[0] / 1e6:9.1f} MB ({nbytes[0] / (ms[0] * 1e6):7.1f} GB/s written once); "
                f"interchanging blocks {info[5]}, stopped {info[6]}")
            for tag, t, lv in (("forward ", ms[1], info[0]), ("backward", ms[2], info[1])):
                out(f"    {tag} sweep {t:10.3f} ms, {lv:6d} levels, {t * 1e3 / lv:7.2f} us per level, {nbytes[1] / 1e6:9.1f} MB moved at least, {nbytes[1] / (t * 1e6):7.1f} GB/s")
            L.fasp_swz_data_free(C.byref(D))
            itp = fa.param_solver_init(); itp.itsolver_type = T.SOLVER_CG; itp.tol = 1e-8; itp.maxit = 5000; itp.print_level = 0
            x = np.zeros(m); bv, kb = T.as_vec(b); xv = T.dvector(m, T.dp(x))
            sys.stdout.flush()
            t0 = time.perf_counter()
            its = L.fasp_solver_dcsr_krylov_swz(C.byref(A), C.byref(bv), C.byref(xv), C.byref(itp), C.byref(prm))
            out(f"    CG to 1e-8, fasp_solver_dcsr_krylov_swz (SWZ_type 3): {its:5d} iterations, {(time.perf_counter() - t0) * 1e3:10.1f} ms wall, setup included")
        itp = fa.param_solver_init(); itp.itsolver_type = T.SOLVER_CG; itp.tol = 1e-8; itp.maxit = 5000; itp.print_level = 0
        ilup = T.ILU_param(); L.fasp_param_ilu_init(C.byref(ilup)); ilup.ILU_type = T.ILUk; ilup.ILU_lfil = 0; ilup.print_level = 0
        L.fasp_solver_dcsr_krylov_diag.argtypes = [C.POINTER(T.dCSRmat), C.POINTER(T.dvector), C.POINTER(T.dvector), C.POINTER(T.ITS_param)]
        for label, fn in (("fasp_solver_dcsr_krylov_diag", lambda bv, xv: L.fasp_solver_dcsr_krylov_diag(C.byref(A), C.byref(bv), C.byref(xv), C.byref(itp))),
                          ("fasp_solver_dcsr_krylov_ilu, ILUk(0)", lambda bv, xv: L.fasp_solver_dcsr_krylov_ilu(C.byref(A), C.byref(bv), C.byref(xv), C.byref(itp), C.byref(ilup)))):
            x = np.zeros(m); bv, kb = T.as_vec(b); xv = T.dvector(m, T.dp(x))
            t0 = time.perf_counter()
            its = fn(bv, xv)
            out(f"  CG to 1e-8, {label:40s}: {its:5d} iterations, {(time.perf_counter() - t0) * 1e3:10.1f} ms wall, setup included")
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
