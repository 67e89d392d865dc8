#!/usr/bin/env python3
"""Time per iteration of the safe-net Krylov solvers (csrc/safe_krylov.hip.h) beside their non-safe twins, in one process, warm.

    python tools/perf_safe_krylov.py [--sizes 128,256] [--iters 60] [--rounds 5] [--out profiles/safe_krylov.txt]

Per size P7(n) and preconditioner (none, the diagonal one -- fasp_precond_diag, which stays on the device): fasp_solver_dcsr_spcg /
_spbcgs / _spminres with fasp_hip_tune("safe_fused", 1) (the fused update kernels and the swapping iterate buffers) and 0 (the reference's
pass-by-pass sequence over the existing BLAS-1 launches with a real copy to u_best), and the unchanged fasp_solver_dcsr_pcg / _pbcgs /
_pminres of the same build.  Every solve runs `iters` iterations from a zero guess on a seeded standard-normal right-hand side (tol 1e-30:
it ends at MaxIt); the time is what fasp_hip_plugin_solve_seconds reports (the driver alone: the upload of the operator is outside), divided by the iterations.  The three
forms of a method alternate inside a round, after one warm-up solve each; the table shows the median over the rounds and the spread.
The vector traffic of the model: one vector of P7(n) is 8 n^3 bytes (134 MB at n = 256)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import faspsolver_amd as fa  # noqa: E402
from faspsolver_amd import _types as T  # noqa: E402

PAIRS = (("spcg", "pcg"), ("spbcgs", "pbcgs"), ("spminres", "pminres"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "safe_krylov.txt"))
    args = ap.parse_args()
    if not fa.available():
        raise SystemExit("perf_safe_krylov: no HIP device (timings are taken on the GPU only)")
    L = fa.lib()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"safe-net Krylov solvers, milliseconds per iteration ({args.iters} iterations per solve, median of {args.rounds} rounds, [min .. max]);")
    out("fused: safe_fused 1 (default), unfused: safe_fused 0, twin: the non-safe entry of the same build; ratio = fused / twin, fused / unfused")
    for n in (int(v) for v in args.sizes.split(",")):
        ia, ja, a, f, _ = fa.poisson7pt(n)
        A, keep = T.as_csr(ia, ja, a)
        N = A.row
        f = np.random.default_rng(n).standard_normal(N)   # (the generator's own f is an eigenvector of P7: BiCGstab breaks down on it)
        bv, _b = T.as_vec(f)
        diag = np.full(N, 6.0)
        dv = T.dvector(N, T.dp(diag))
        pcd = T.precond(C.cast(C.pointer(dv), C.c_void_p), C.cast(L.fasp_precond_diag, T.PRECOND_FCT))
        x = np.zeros(N)
        xv = T.dvector(N, T.dp(x))

        def solve(name, pc, fused):
            x[:] = 0.0
            L.fasp_hip_tune(b"safe_fused", fused)
            fn = getattr(L, "fasp_solver_dcsr_" + name)
            extra = () if name.startswith("sp") else (0.0,)   # the non-safe prototypes have abstol
            st = fn(C.byref(A), C.byref(bv), C.byref(xv), C.byref(pc) if pc is not None else None, 1e-30, *extra, args.iters, T.STOP_REL_RES, 0)
            L.fasp_hip_tune(b"safe_fused", 1)
            # (the non-safe BiCGstab returns the iteration of its smallest residual, MaxIt or just below it, where the others return ERROR_SOLVER_MAXIT)
            if st != T.ERROR_SOLVER_MAXIT and not (name == "pbcgs" and st >= args.iters - 2):
                out(f"    (note: {name} ended with {st} instead of running {args.iters} iterations)")
            return 1e3 * L.fasp_hip_plugin_solve_seconds() / args.iters

        out(f"\nP7({n}): {N} rows, {A.nnz} entries, one vector = {8.0 * N / 1e6:.1f} MB")
        out(f"  {'pc':5s} {'method':9s} {'fused':>24s} {'unfused':>24s} {'twin':>24s}  f/twin  f/unf")
        for pcname, pc in (("none", None), ("diag", pcd)):
            for safe, twin in PAIRS:
                forms = ((safe, 1), (safe, 0), (twin, 1))
                for name, fused in forms:
                    solve(name, pc, fused)   # warm-up
                t = {k: [] for k in forms}
                for _ in range(args.rounds):
                    for k in forms:
                        t[k].append(solve(k[0], pc, k[1]))
                med = [float(np.median(t[k])) for k in forms]
                cells = [f"{m:8.3f} [{min(t[k]):.3f} .. {max(t[k]):.3f}]" for m, k in zip(med, forms)]
                out(f"  {pcname:5s} {safe:9s} {cells[0]:>24s} {cells[1]:>24s} {cells[2]:>24s}  {med[0] / med[2]:6.3f} {med[0] / med[1]:6.3f}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
