"""The Galerkin product on the device (csrc/rap.hip.h) beside the host product of the setups, level by level of the host
hierarchies of P7(n) with the headline parameters: rows, entries of the result, the form the automatic choice takes, seconds of
the host product (fasp_hip_rap_time, where = 0), of the device product end to end (1: upload of the three operands, kernels,
download of the result) and of its kernels alone (2) in both forms; the totals over the levels; then setup_seconds of
fasp_hip_amg_create with fasp_hip_tune("device_rap") 0 and 1, three runs each in this process.

    python tools/perf_rap.py [--sizes 128,256] [--reps 2] [--arena-kb 262144] [--out profiles/rap_device.txt]
"""
import argparse
import ctypes as C
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import faspsolver_amd as fa  # noqa: E402
from faspsolver_amd import _types as T  # noqa: E402

P = C.POINTER


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return platform.processor() or "?"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--arena-kb", default="262144", help="rap_arena_kb values to time form 0's kernels at, comma separated (the first one serves the rest of the table)")
    ap.add_argument("--no-setup", action="store_true", help="skip the fasp_hip_amg_create runs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = fa.lib()
    if not fa.available():
        raise SystemExit("perf_rap: no HIP device")
    ident = C.create_string_buffer(64)
    L.fasp_hip_device_identity(ident, 64)
    arenas = [int(v) for v in args.arena_kb.split(",")]
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"# tools/perf_rap.py on {L.fasp_hip_version().decode()}, reps {args.reps}")
    out(f"# box: {cpu_model()}, {os.cpu_count()} hardware threads, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', '-')}; device {ident.value.decode()}")

    def tune(key, v):
        assert L.fasp_hip_tune(key.encode(), v) == 0, key

    for n in (int(v) for v in args.sizes.split(",")):
        A = T.dCSRmat(); b = T.dvector(); u = T.dvector()
        assert L.fasp_hip_poisson7pt(n, n, n, C.byref(A), C.byref(b), C.byref(u)) == 0
        amgp = fa.param_amg_init(); amgp.smoother = T.SMOOTHER_JACOBI; amgp.relaxation = 0.6667; amgp.print_level = 0
        h = C.c_void_p()
        t0 = time.perf_counter()
        assert L.fasp_hip_amg_create_host(C.byref(h), C.byref(A), C.byref(amgp)) == 0
        nl = L.fasp_hip_amg_num_levels(h)
        out(f"\nP7({n}): {A.row} rows, {nl} levels, host setup {time.perf_counter() - t0:.2f} s")
        out("  level      rows        nf   nnz(RAP)  auto   host s   dev e2e s  kernels f0 s  kernels f1 s" +
            "".join(f"  f0 @{kb} KiB" for kb in arenas[1:]))
        tot = [0.0] * 5
        for l in range(nl - 1):
            Al, Pl, Rl, Ac = T.dCSRmat(), T.dCSRmat(), T.dCSRmat(), T.dCSRmat()
            L.fasp_hip_amg_get_matrix(h, l, 0, C.byref(Al)); L.fasp_hip_amg_get_matrix(h, l, 1, C.byref(Pl))
            L.fasp_hip_amg_get_matrix(h, l, 2, C.byref(Rl)); L.fasp_hip_amg_get_matrix(h, l + 1, 0, C.byref(Ac))
            ops = (C.byref(Rl), C.byref(Al), C.byref(Pl))
            tune("rap_arena_kb", arenas[0])
            tune("rap_form", -1)
            t_host = L.fasp_hip_rap_time(*ops, 0, args.reps)
            t_e2e = L.fasp_hip_rap_time(*ops, 1, args.reps)
            info = fa.rap_info()
            tk = []
            for form in (0, 1):
                tune("rap_form", form)
                tk.append(L.fasp_hip_rap_time(*ops, 2, args.reps))
            extra = []
            tune("rap_form", 0)
            for kb in arenas[1:]:
                tune("rap_arena_kb", kb)
                extra.append(L.fasp_hip_rap_time(*ops, 2, args.reps))
            tune("rap_form", -1); tune("rap_arena_kb", arenas[0])
            out(f"  {l:5d} {Rl.row:9d} {Al.row:9d} {Ac.nnz:10d}  f{info['form']} ({info['batches']:3d} b{', LDS' if info['lds'] else ''}) "
                f"{t_host:8.4f} {t_e2e:10.4f} {tk[0]:12.4f} {tk[1]:12.4f}" + "".join(f" {t:12.4f}" for t in extra))
            for i, t in enumerate((t_host, t_e2e, tk[0], tk[1], min(tk))):
                tot[i] += t
        out(f"  total over the levels: host {tot[0]:.4f} s, device end to end {tot[1]:.4f} s, kernels form 0 {tot[2]:.4f} s, form 1 {tot[3]:.4f} s, "
            f"the faster form per level {tot[4]:.4f} s")
        L.fasp_hip_amg_destroy(h)
        if not args.no_setup:
            for dev in (0, 1):
                tune("device_rap", dev)
                ts = []
                for _ in range(3):
                    h = C.c_void_p()
                    t0 = time.perf_counter()
                    assert L.fasp_hip_amg_create(C.byref(h), C.byref(A), C.byref(amgp)) == 0
                    ts.append(time.perf_counter() - t0)
                    L.fasp_hip_amg_destroy(h)
                out(f"  fasp_hip_amg_create, device_rap {dev}: setup_seconds " + ", ".join(f"{t:.3f}" for t in ts))
            tune("device_rap", 0)
        L.fasp_hip_free_system(C.byref(A), C.byref(b), C.byref(u))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
