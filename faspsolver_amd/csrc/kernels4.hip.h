// kernels4.hip.h -- k_csr_sell: value-indexed sliced-ELL row kernel (gfx950 / CDNA4, wave64).
//
// The levels k_csr_wstream2 serves (20-48 entries per row, no repeating rows) are bound by the x gathers of its phase 1:
// lane = entry, and 64 consecutive entries -- two rows in discovery order -- scatter over ~40 cache lines (DESIGN.md
// section 3.1a).  Two properties of a Galerkin operator on a regular grid are used here:
//   * lane = ROW: the k-th entries of 64 consecutive rows fall into ~13 cache lines of x, and a row's products are summed
//     by one lane in storage order -- the reference's left-to-right row sum (BlaSpmvCSR.c:242), bit for bit;
//   * few distinct values (P7(256) level 2: 8 245 doubles for 49.7 M entries): an entry is ONE 32-bit word, index into the
//     table of the exact doubles (kept in LDS) | column - smallest column of the slice.  4 bytes instead of 12.
// Stored form (device_csr.hip.h, build_sell): slices of 64 consecutive rows; word k of the 64 rows of a slice is contiguous
// (one coalesced 256-byte load per step, no staging); a slice is padded at the END of its rows to its longest row with the
// word 0 -- a valid (value 0, column base) pair that is fetched but never multiplied: a lane stops at its row's length.
#pragma once

#include "kernels2.hip.h"

namespace fasp {

constexpr int SELL_BLOCK = 1024;            // 16 wavefronts = 16 slices = one row window unit (DIST_WIN_ALIGN)
constexpr int SELL_NW    = SELL_BLOCK / 64;
constexpr int SELL_U     = 8;               // code words (and gathers) in flight per lane
constexpr int SELL_MAXV  = 9216;            // table entries: 72 KB of LDS, two workgroups per CU

// One wavefront per slice.  Pipeline of a wave: the code words of batch k + 1 are loaded (unit stride, independent of x)
// behind batch k's gathers, while its values come from LDS; the last batch of a slice looks ahead to the first batch of the
// NEXT slice, so that no load the loop waits for queues up behind the store of y.
template <int OP>
__global__ __launch_bounds__(SELL_BLOCK, 8) void k_csr_sell(CsrArgs a)
{
    if (a.stop && *a.stop) return;
    extern __shared__ __attribute__((aligned(16))) double sell_lds[];   // value table, then one slot per wave for the reduction
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nv = a.sell_nv;
    for (int i = threadIdx.x; i < nv; i += SELL_BLOCK) sell_lds[i] = a.sell_tab[i];
    __syncthreads();
    const double* tab = sell_lds;
    const int      obits = a.sell_obits;
    const unsigned omask = (1u << obits) - 1u;
    const int vmax = tile_vmax(a);
    const int G = gridDim.x;
    double dotacc = 0.0;

    // next slice of this wave: first row (-1: none) and row count, wave-uniform
    auto advance = [&](int& v, int& r0, int& nr) {
        for (;;) {
            r0 = -1; nr = 0;
            if (v >= vmax) return;
            const int t = tile_of(a, v);
            v += G;
            if (t >= a.ntiles) continue;
            const int rr = (t + a.tile0) * SELL_BLOCK + wave * 64;
            if (rr >= a.nrow) continue;
            r0 = rr; nr = min(64, a.nrow - rr);
            return;
        }
    };
    // the slice's first word row, width (its longest row), smallest column; the lane's row length
    auto meta = [&](int r0, int nr, int& p0, int& W, int& base, int& len) {
        p0 = W = base = len = 0;
        if (r0 < 0) return;
        const int s = r0 >> 6;
        p0 = a.sell_sptr[s]; W = a.sell_sptr[s + 1] - p0; base = a.sell_sbase[s];
        if (lane < nr) len = a.sell_rlen[r0 + lane];
    };
    unsigned c[SELL_U];
    // words k0 .. k0 + U of the lane (steps beyond the slice's width repeat its last word: in bounds, never used)
    auto load_codes = [&](unsigned* q, int p0, int W, int k0) {
        const unsigned* cp = a.sell_code + ((size_t)p0 << 6) + lane;
#pragma unroll
        for (int u = 0; u < SELL_U; ++u) q[u] = __builtin_nontemporal_load(cp + ((size_t)min(k0 + u, W - 1) << 6));
    };

    int v = blockIdx.x;
    int r0A, nrA, p0A, WA, baseA, lenA;
    advance(v, r0A, nrA);
    meta(r0A, nrA, p0A, WA, baseA, lenA);
    if (r0A >= 0 && WA > 0) load_codes(c, p0A, WA, 0);
    while (r0A >= 0) {
        int r0B, nrB, p0B, WB, baseB, lenB;
        advance(v, r0B, nrB);
        meta(r0B, nrB, p0B, WB, baseB, lenB);
        const int r = r0A + lane;
        double acc = ((OP == OP_JACOBI || OP == OP_L1DIAG) && lane < nrA) ? a.b[r] : 0.0;
        const bool haveB = r0B >= 0 && WB > 0;
        for (int k0 = 0; k0 < WA; k0 += SELL_U) {
            int    col[SELL_U];
            double xv[SELL_U], w[SELL_U];
#pragma unroll
            for (int u = 0; u < SELL_U; ++u) col[u] = baseA + (int)(c[u] & omask);
            unsigned dmask = 0u;   // OP_JACOBI: which of the batch is the row's diagonal (a bit each: the columns need not stay in registers)
            if (OP == OP_JACOBI) {
#pragma unroll
                for (int u = 0; u < SELL_U; ++u) dmask |= (col[u] == r ? 1u : 0u) << u;
            }
#pragma unroll
            for (int u = 0; u < SELL_U; ++u) xv[u] = a.x[col[u]];
            // look ahead BEHIND the gathers (the wait for x leaves these in flight) and unconditional (a load under a branch is waited
            // for at the join): the slice's next batch, or the next slice's first one, or -- nothing left --
            // this slice's last word row once more
            unsigned n[SELL_U];
            const bool more = k0 + SELL_U < WA;   // wave-uniform
            load_codes(n, more || !haveB ? p0A : p0B, more || !haveB ? WA : WB, more ? k0 + SELL_U : haveB ? 0 : WA - 1);
#pragma unroll
            for (int u = 0; u < SELL_U; ++u) w[u] = tab[c[u] >> obits];
#pragma unroll
            for (int u = 0; u < SELL_U; ++u) {
                const double pr = w[u] * xv[u];
                bool use = k0 + u < lenA;
                if (OP == OP_JACOBI) use = use && !((dmask >> u) & 1u);
                const double nxt = (OP == OP_JACOBI || OP == OP_L1DIAG) ? acc - pr : acc + pr;
                acc = use ? nxt : acc;
            }
#pragma unroll
            for (int u = 0; u < SELL_U; ++u) c[u] = n[u];
        }
        if (WA == 0 && haveB) load_codes(c, p0B, WB, 0);   // (a slice of empty rows has no last batch to look ahead from)
        if (lane < nrA) row_epilogue<OP>(a, r, acc, dotacc);
        r0A = r0B; nrA = nrB; p0A = p0B; WA = WB; baseA = baseB; lenA = lenB;
    }
    if (OP == OP_MXV_DOT || (OP == OP_JACOBI && a.partials)) {
        // deterministic: wave shuffle tree, then the 16 wave results in wave order
        double* red = sell_lds + nv;
        const double s = subwave_sum<64>(dotacc);
        __syncthreads();
        if (lane == 0) red[wave] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            double tot = red[0];
            for (int q = 1; q < SELL_NW; ++q) tot += red[q];
            a.partials[blockIdx.x] = tot;
        }
    }
}

}  // namespace fasp
