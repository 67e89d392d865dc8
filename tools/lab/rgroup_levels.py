"""Long-row levels of the P7(n) hierarchy, COLD (one launch behind a 512 MB read, as a V-cycle meets them): the kernel the plan picks
without the row-group form (k_csr_rows / k_csr_estream; three repeats: their spread is the yardstick) against k_csr_rgroup with 16 and 8
rows per group and 4 and 8 waves per group -- y = A x / y -= A x / Jacobi, us per launch; the plain 16-byte read of the level's values
beside them.  FASP_HIP_SETUP_TIMING=1 prints what the coding made of every level.   python tools/lab/rgroup_levels.py [n] [reps]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import faspsolver_amd as fa
from faspsolver_amd import _types as T
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
L = fa.lib()
ia, ja, a, f, ue = fa.poisson7pt(n)
amgp = fa.param_amg_init(); amgp.smoother = T.SMOOTHER_JACOBI; amgp.relaxation = 0.6667
fmt = lambda v: " / ".join(f"{x:6.1f}" for x in v)
for R in (16, 8):
    L.fasp_hip_tune(b"rgroup", 2); L.fasp_hip_tune(b"rgroup_rows", R)
    H = fa.AMG(ia, ja, a, amgp)
    L.fasp_hip_tune(b"time_cold", 1)
    levels = [l for l in range(H.num_levels - 1) if H.kernel_info(l, 0)[0] == 0]
    print(f"P7({n}), {R} rows per group: long-row levels {levels}; us per launch cold: y = A x / y -= A x / Jacobi", flush=True)
    for l in levels:
        r, c, lia, *_ = H.matrix(l, 0)
        L.fasp_hip_tune(b"rgroup", 2); L.fasp_hip_tune(b"rgroup_waves", 4)
        kind, mb = H.kernel_info(l, 0)
        print(f"level {l}: {r:8d} rows {lia[r] / r:7.1f} per row, {mb / 1e6:7.1f} MB as planned under rgroup 2", flush=True)
        L.fasp_hip_tune(b"rgroup", 0)
        for k in range(3):
            print(f"    plan without ({k}) " + fmt([H.time_kernel(q, l, reps) * 1e3 for q in (0, 1, 2)]), flush=True)
        L.fasp_hip_tune(b"rgroup", 2)
        for W in (2, 4, 8):
            L.fasp_hip_tune(b"rgroup_waves", W)
            for k in range(2):
                print(f"    rgroup R {R:2d} W {W} ({k}) " + fmt([H.time_kernel(q, l, reps) * 1e3 for q in (0, 1, 2)]), flush=True)
        print(f"    plain read of the values {H.time_kernel(8, l, reps) * 1e3:6.1f}", flush=True)
    L.fasp_hip_tune(b"time_cold", 0); L.fasp_hip_tune(b"rgroup_waves", 0)
    H.close()
L.fasp_hip_tune(b"rgroup", 1); L.fasp_hip_tune(b"rgroup_rows", 0)
