"""Block ILU triangular solves on the device (csrc/ilu.hip.h, NB-templated): levels of L and U, the form that ran,
microseconds, bytes and GB/s per solve, beside the compiled reference's single-thread fasp_precond_dbsr_ilu on the same
factor, one BSR SpMV of A (fasp_hip_time_bsr_mxv) and the scalar ILU(0) of P7(128) (profiles/ilu_apply.txt: 4338 us
for L + U).  Ends with one end-to-end fasp_solver_dbsr_krylov_ilu (BiCGstab, ILU(0)) at P7(128) (x) B3.

    python tools/perf_bilu.py [--cases 128:3:0,64:2:0,64:5:0,64:7:0,64:3:1] [--reps 20] [--out profiles/bilu_apply.txt]

--smoother times the ILU smoothing step of the block AMG cycle instead (AMG_param.ILU_levels = 1, level 0 of P7(64) (x) B3,
ILU(0)): the step whose U solve writes x = x + z itself against the three passes it replaces (residual, both solves, axpy),
the two forms alternating in one run on one resident hierarchy.

    python tools/perf_bilu.py --smoother [--n 64] [--reps 20] [--rounds 5] [--out profiles/bilu_smoother.txt]
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

SCALAR_ILU0_P7_128_US = 4337.9   # profiles/ilu_apply.txt


def block_of(nb):
    """B3 of the config-3 operator for nb = 3, else a fixed SPD tridiagonal block"""
    if nb == 3:
        return _libs.B3
    return np.diag(np.full(nb, 4.0)) + np.diag(np.ones(nb - 1), 1) + np.diag(np.ones(nb - 1), -1)


def smoother_leg(args, L, out):
    n, nb = args.n, 3
    ia, ja, val, _ = _libs.poisson7pt_bsr(n)
    amgp = fa.param_amg_init()
    amgp.AMG_type, amgp.aggregation_type, amgp.smoother = T.UA_AMG, 2, T.SMOOTHER_JACOBI
    amgp.ILU_levels, amgp.ILU_lfil = 1, 0
    G = fa.BSRAMG(ia, ja, val, nb, amgp)
    info = G.ilu_info(0)
    out(f"\nILU smoothing step of the block cycle, level 0 of P7({n}) (x) B{nb}, ILU(0): {n ** 3} block rows, {G.num_levels} levels, "
        f"L / U {info[0]} / {info[1]} dependency levels, {'single launch' if info[3] else 'level launches'}")
    t = {1: [], 0: []}
    try:
        for rnd in range(args.rounds):   # the forms alternate: drifts of the machine hit both alike
            for fused in (1, 0):
                L.fasp_hip_tune(b"ilu_smooth_fused", fused)
                us = G.ilu_smooth_time(0, args.reps)
                assert us > 0
                t[fused].append(us)
    finally:
        L.fasp_hip_tune(b"ilu_smooth_fused", 1)
        G.free()
    for fused, name in ((1, "fused (U solve writes x = x + z)"), (0, "three calls (residual, both solves, axpy)")):
        v = np.array(t[fused])
        out(f"  {name:44s}: median {np.median(v):9.1f} us per step, min {v.min():9.1f}, max {v.max():9.1f}  ({args.rounds} rounds x {args.reps} steps)")
    m1, m0 = np.median(t[1]), np.median(t[0])
    out(f"  fused / three calls = {m1 / m0:.4f} ({m0 - m1:+.1f} us saved per step; one vector pass over {n ** 3 * nb} doubles read twice and "
        f"written once = {24.0 * n ** 3 * nb / 1e6:.1f} MB)")
    out("  the cycle uses the " + ("fused form" if m1 <= m0 else "THREE-CALL form would be faster here: see fasp_hip_tune(\"ilu_smooth_fused\", 0)"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="128:3:0,64:2:0,64:5:0,64:7:0,64:3:1", help="n:nb:lfil of ILUk on P7(n) (x) B_nb")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-ref", action="store_true", help="skip the reference's CPU application")
    ap.add_argument("--no-solve", action="store_true", help="skip the end-to-end solve")
    ap.add_argument("--smoother", action="store_true", help="time the ILU smoothing step of the block AMG cycle instead")
    ap.add_argument("--n", type=int, default=64, help="--smoother: P7(n) (x) B3")
    ap.add_argument("--rounds", type=int, default=5, help="--smoother: alternations of the two forms")
    args = ap.parse_args()
    L = fa.lib()
    if not fa.available():
        raise SystemExit("perf_bilu: no HIP device")
    ref = None if args.no_ref else _libs.ref()
    if ref is not None:
        ref.fasp_precond_dbsr_ilu.argtypes = [T.c_double_p, T.c_double_p, C.c_void_p]
        ref.fasp_precond_dbsr_ilu.restype = None
    L.fasp_hip_time_bsr_mxv.argtypes = [C.POINTER(T.dBSRmat), C.c_int]
    L.fasp_hip_time_bsr_mxv.restype = C.c_double
    lines = [f"# tools/perf_bilu.py on {L.fasp_hip_version().decode()}, reps {args.reps}"]

    def out(s):
        print(s, flush=True)
        lines.append(s)

    if args.smoother:
        smoother_leg(args, L, out)
        args.cases, args.no_solve = "", True
    for case in filter(None, args.cases.split(",")):
        n, nb, lfil = (int(v) for v in case.split(":"))
        ia, ja, val, _ = _libs.poisson7pt_bsr(n, block_of(nb))
        A, keep = T.as_bsr(ia, ja, val, nb)
        prm = T.ILU_param(); L.fasp_param_ilu_init(C.byref(prm))
        prm.ILU_type, prm.ILU_lfil = T.ILUk, lfil
        d = T.ILU_data()
        t0 = time.perf_counter()
        assert L.fasp_ilu_dbsr_setup(C.byref(A), C.byref(d), C.byref(prm)) == 0
        t_setup = time.perf_counter() - t0
        out(f"\nILUk({lfil}) of P7({n}) (x) B{nb}: {A.ROW} block rows, factor {d.nzlu - A.ROW - 1} off-diagonal blocks, "
            f"host setup {t_setup:.2f} s")
        tot = 0.0
        for which, name in ((1, "L"), (2, "U")):
            info = (C.c_double * 6)()
            us = L.fasp_hip_ilu_time(C.byref(d), which, args.reps, info)
            tot += us
            out(f"  {name}: {int(info[0])} levels, {'single launch' if info[1] else 'level launches'}: {us:9.1f} us per solve, "
                f"{info[2] / 1e6:8.1f} MB moved ({info[2] / (us * 1e3):6.0f} GB/s), slab {int(info[3])} entries for {int(info[4])}, "
                f"longest row {int(info[5])}")
        mxv_us = L.fasp_hip_time_bsr_mxv(C.byref(A), args.reps) * 1e3
        out(f"  L + U: {tot:9.1f} us = {tot / mxv_us:.1f} BSR SpMVs of A ({mxv_us:.1f} us); "
            f"{tot / SCALAR_ILU0_P7_128_US:.2f}x the scalar ILU(0) of P7(128)")
        if ref is not None:
            r = np.sin(0.37 * np.arange(A.ROW * nb)) + 0.1
            z = np.zeros(A.ROW * nb)
            t0 = time.perf_counter()
            ref.fasp_precond_dbsr_ilu(r.ctypes.data_as(T.c_double_p), z.ctypes.data_as(T.c_double_p), C.cast(C.byref(d), C.c_void_p))
            t_ref = time.perf_counter() - t0
            out(f"  reference fasp_precond_dbsr_ilu (one CPU thread): {t_ref * 1e6:11.1f} us  ({t_ref * 1e6 / tot:.0f}x the device)")
        L.fasp_ilu_data_free(C.byref(d))
    if not args.no_solve:
        ia, ja, val, nb = _libs.poisson7pt_bsr(128)
        b = np.random.default_rng(128).uniform(-1.0, 1.0, (len(ia) - 1) * nb)
        t0 = time.perf_counter()
        st, x = fa.solve_bsr_ilu(ia, ja, val, nb, b, solver=T.SOLVER_BiCGstab, tol=1e-8, maxit=500, lfil=0)
        t = time.perf_counter() - t0
        out(f"\nfasp_solver_dbsr_krylov_ilu, BiCGstab + ILU(0), P7(128) (x) B3, tol 1e-8: {st} iterations, {t * 1e3:.0f} ms "
            f"end to end (host setup + upload included), {t * 1e3 / max(st, 1):.1f} ms per iteration "
            f"(config 3's AMG solve: 166-174 ms)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
