"""The fused update kernels of the safe-net Krylov solvers (csrc/safe_krylov.hip.h) through fasp_hip_safe_update_selftest: every output
vector has the bits of the reference's sequence over the existing BLAS-1 kernels, the sums are within the a-priori bound of any summation
order of their np.longdouble values, maxima and NaN counts are exact.  Sizes: 1 and 2 (tail only / one pair), 255 and 257 (around one
block), 1331 (odd, several blocks) and 524 289 = MAXGRID * BLOCK + 1 (a second grid-stride trip and an odd tail)."""
import numpy as np
import pytest

from _libs import sum_bound_ratio

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 255, 257, 1331, 2048 * 256 + 1)
ALPHA, OMEGA, BETA = 0.37, -0.61, 1.29


def vector(k, n, seed):
    """Input vector k of the selftest (include/fasp_hip_dev.h): splitmix64's finaliser of (i, seed, k) -> [-1, 1)."""
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed) * np.uint64(0xBF58476D1CE4E5B9) \
            + np.uint64(k) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(30); z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27); z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    v = (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 * 2.0 - 1.0
    if k == 0 and seed >= 1000:
        v[[0, n // 2, n - 1]] = np.nan
    return v


def expected(which, n, seed):
    """[(kind, operands)] of the step's scalars: ("sum", a, b) = a.b, ("max", a) = max|a| over the entries that are no NaN, ("nan", a)."""
    v = [vector(k, n, seed) for k in range(7)]
    if which == 0:
        uo, ro = v[0] + ALPHA * v[1], v[3] + (-ALPHA) * v[2]
        return [("sum", ro, ro), ("sum", uo, uo), ("sum", v[1], v[1]), ("max", uo), ("nan", uo)]
    if which == 2:
        spo = ALPHA * v[1] + OMEGA * v[2]
        uo, so = v[0] + spo, v[3] + (-OMEGA) * v[4]
        return [("sum", so, v[5]), ("sum", spo, spo), ("sum", uo, uo), ("sum", so, so), ("max", uo), ("nan", uo)]
    if which == 4:
        return [("sum", v[1], v[1]), ("sum", v[2], v[1])]
    if which == 5:
        xo = v[0] + v[1]
        return [("sum", xo, xo), ("max", xo), ("nan", xo)]
    return []


@pytest.mark.parametrize("seed", (7, 1007))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("which", range(6))
def test_fused_kernel_against_the_blas1_sequence(gpu, which, n, seed):
    mismatches, fused, seq = gpu.safe_update_selftest(which, n, seed)
    exp = expected(which, n, seed)
    assert mismatches == 0
    assert len(fused) == len(seq) == len(exp)
    ld = np.longdouble
    for q, e in enumerate(exp):
        for name, got in (("fused", fused[q]), ("sequence", seq[q])):
            if e[0] == "sum":
                prod = e[1].astype(ld) * e[2].astype(ld)
                if np.isnan(prod).any():
                    assert np.isnan(got), (q, name)
                    continue
                ratio = sum_bound_ratio(np.array([got]), np.array([prod.sum()]), np.array([np.abs(prod).sum()]), np.array([n]))
                assert ratio <= 1.0, (q, name, ratio)
            elif e[0] == "max":
                a = np.abs(e[1][~np.isnan(e[1])])
                assert got == (a.max() if len(a) else 0.0), (q, name)
            else:
                assert got == np.isnan(e[1]).sum(), (q, name)
    if seed >= 1000 and exp and exp[-1][0] == "nan":
        assert fused[-1] == len({0, n // 2, n - 1})
