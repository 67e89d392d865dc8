#!/usr/bin/env python3
"""Band SpMV of a structured matrix (k_str_band, fasp_hip_time_str_mxv) beside the products of the same matrix converted to the formats
the library already serves, in one process on one device:

    7-band nc = 1 variable-coefficient matrix on n^3 (default 256)   against the CSR product of fasp_format_dstr_dcsr(A)
    the same pattern on m^3 (default 128) with nc = 3                against the BSR product of the converted matrix

    python tools/perf_str.py [--n 256] [--m 128] [--rounds 5] [--reps 20] [--out profiles/str_mxv.txt]

Each round times `reps` back-to-back launches of one product after two warm-up launches (HIP events inside the library's timers), the two
formats alternating; the figure reported is the median of the rounds' means.  Bytes are algorithmic: what the format has to move once
(matrix, x read once, y written once).  The read ceiling is measured in the same process (fasp_hip_measure_ceilings)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import faspsolver_amd as fa  # noqa: E402
from faspsolver_amd import _types as T  # noqa: E402

PEAK = 8000.0   # GB/s


def bands_7pt(n, nc, rng):
    """Variable-coefficient 7-band matrix on n^3, offsets in the order [-1, 1, -n, n, -n^2, n^2]; zeros where a grid line ends."""
    ngrid = n ** 3
    i = np.arange(ngrid)
    inside = {1: i % n < n - 1, n: (i // n) % n < n - 1, n * n: i // (n * n) < n - 1}
    offsets, bands = [], []
    diag = np.zeros((ngrid, nc, nc))
    for d in (1, n, n * n):
        k = np.where(inside[d], np.exp(rng.uniform(-1.0, 1.0, ngrid)), 0.0)[:ngrid - d]
        blk = (np.eye(nc) + 0.1 * rng.standard_normal((nc, nc)))[None] if nc > 1 else np.ones((1, 1, 1))
        b = -k[:, None, None] * blk
        diag[:ngrid - d] -= b
        diag[d:] -= b
        offsets += [-d, d]
        bands += [b.reshape(-1), b.reshape(-1).copy()]
    return offsets, diag.reshape(-1), bands


def to_bsr(n, nc, offsets, diag, bands):
    """The block CSR form of the band matrix: per grid point the diagonal block, then the bands that have a term, in storage order."""
    ngrid, nc2 = n ** 3, nc * nc
    i = np.arange(ngrid)
    cols = [i] + [i + o for o in offsets]
    ex = [np.ones(ngrid, dtype=bool)] + [(i + o >= 0) & (i + o < ngrid) for o in offsets]
    cnt = np.sum(ex, axis=0)
    ia = np.zeros(ngrid + 1, dtype=np.int32)
    np.cumsum(cnt, out=ia[1:])
    ja = np.empty(int(ia[-1]), dtype=np.int32)
    val = np.empty((int(ia[-1]), nc2))
    at = ia[:-1].astype(np.int64).copy()
    for k, (c, e) in enumerate(zip(cols, ex)):
        src = diag.reshape(-1, nc2) if k == 0 else bands[k - 1].reshape(-1, nc2)
        off = 0 if k == 0 else offsets[k - 1]
        rows = np.flatnonzero(e)
        ja[at[rows]] = c[rows]
        val[at[rows]] = src[rows + off] if off < 0 else src[rows]   # a lower band is stored by column
        at[rows] += 1
    return ia, ja, val.reshape(-1)


def line(name, nbytes, ms, read_gbs):
    gbs = nbytes / ms / 1e6
    return (f"  {name:34s} {nbytes / 1e9:7.3f} GB  {ms * 1e3:8.1f} us  {gbs / 1e3:6.3f} TB/s  {gbs / PEAK:5.3f} of 8 TB/s  "
            f"{gbs / read_gbs:5.3f} of the read ceiling")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--m", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "str_mxv.txt"))
    a = ap.parse_args()
    if not fa.available():
        sys.exit("perf_str: no HIP device (there is no CPU fallback and nothing to time)")
    L = fa.lib()
    ceil = (C.c_double * 3)()
    L.fasp_hip_measure_ceilings(ceil, 1 << 30, 10)
    read_gbs = ceil[0]
    out = [f"band SpMV of a structured matrix against the converted formats; {a.rounds} rounds x {a.reps} launches, median of the rounds",
           f"measured ceilings: read {ceil[0] / 1e3:.2f}, copy {ceil[1] / 1e3:.2f}, triad {ceil[2] / 1e3:.2f} TB/s"]
    rng = np.random.default_rng(7)

    # nc = 1 against plain CSR
    n = a.n
    offsets, diag, bands = bands_7pt(n, 1, rng)
    A, keep = T.as_str(n, n, n, 1, offsets, diag, bands)
    form = L.fasp_hip_str_form(C.byref(A))
    B = T.dCSRmat()
    assert L.fasp_format_dstr_dcsr(C.byref(A), C.byref(B)) == 0
    kind = C.c_int(-1)
    t_str, t_csr = [], []
    for _ in range(a.rounds):   # alternating
        t_str.append(L.fasp_hip_time_str_mxv(C.byref(A), a.reps))
        t_csr.append(L.fasp_hip_time_matrix(C.byref(B), 0, a.reps, C.byref(kind)))
    ngrid = n ** 3
    b_str = 8.0 * (7 * ngrid + 2 * ngrid)
    b_csr = 12.0 * B.nnz + 4.0 * (B.row + 1) + 16.0 * B.row
    out.append(f"nc = 1, {n}^3 = {ngrid} rows, 7 bands (form {form}), CSR of fasp_format_dstr_dcsr: {B.nnz} entries, kernel family {kind.value}")
    out.append(line("k_str_band (STR)", b_str, float(np.median(t_str)), read_gbs) + f"   rounds {[round(t * 1e3, 1) for t in t_str]}")
    out.append(line("CSR product of the converted matrix", b_csr, float(np.median(t_csr)), read_gbs) + f"   rounds {[round(t * 1e3, 1) for t in t_csr]}")
    out.append(f"  time ratio STR / CSR {np.median(t_str) / np.median(t_csr):.3f}; bytes ratio {b_str / b_csr:.3f}")
    L.fasp_dcsr_free(C.byref(B))
    del A, keep, diag, bands

    # nc = 3 against BSR
    m, nc = a.m, 3
    offsets, diag, bands = bands_7pt(m, nc, rng)
    A, keep = T.as_str(m, m, m, nc, offsets, diag, bands)
    form = L.fasp_hip_str_form(C.byref(A))
    ia, ja, val = to_bsr(m, nc, offsets, diag, bands)
    Bb, keepb = T.as_bsr(ia, ja, val, nc)
    t_str, t_bsr = [], []
    for _ in range(a.rounds):
        t_str.append(L.fasp_hip_time_str_mxv(C.byref(A), a.reps))
        t_bsr.append(L.fasp_hip_time_bsr_mxv(C.byref(Bb), a.reps))
    ngrid = m ** 3
    b_str = 8.0 * (7 * ngrid * nc * nc + 2 * ngrid * nc)
    b_bsr = Bb.NNZ * (8.0 * nc * nc + 4) + 4.0 * (Bb.ROW + 1) + 16.0 * Bb.ROW * nc
    out.append(f"nc = 3, {m}^3 = {ngrid} block rows, 7 bands (form {form}), BSR of the converted matrix: {Bb.NNZ} blocks")
    out.append(line("k_str_band (STR)", b_str, float(np.median(t_str)), read_gbs) + f"   rounds {[round(t * 1e3, 1) for t in t_str]}")
    out.append(line("BSR product of the converted matrix", b_bsr, float(np.median(t_bsr)), read_gbs) + f"   rounds {[round(t * 1e3, 1) for t in t_bsr]}")
    out.append(f"  time ratio STR / BSR {np.median(t_str) / np.median(t_bsr):.3f}; bytes ratio {b_str / b_bsr:.3f}")
    if min(t_str + t_bsr + t_csr) <= 0:
        sys.exit("perf_str: a timer failed")
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
