// kernels5.hip.h -- k_csr_rgroup: row groups that share their x gathers (gfx950 / CDNA4, wave64).
//
// The long-row levels (P7(256) levels 4-8: 190-1 360 entries per row) are bound by the texture-address pipe: k_csr_rows and k_csr_estream
// issue one gather of x per ENTRY, and a 64-lane gather costs about 45 cycles of that pipe.  In the brick
// numbering of these levels consecutive rows are graph neighbours and read mostly the same columns: the entries of 16 consecutive rows
// divided by the distinct columns of those rows is 5-9.  Here a GROUP of R consecutive rows is walked over the sorted union of its
// columns, lane = union column: ONE gather of x per union column serves up to R entries.
// Stored form (device_csr.hip.h, build_rgroup), per group:
//   * nch + 1 32-bit value offsets of its chunks (chunk = 64 consecutive union columns; relative to the group's first value), then
//   * one 32-bit word per union column: low 16 bits = column - the group's smallest column, high R bits = which rows of the group have an
//     entry there (bit 32 - R + r: row r);
//   * the values, no fill: chunk after chunk, inside a chunk row 0's values in union order, then row 1's, ... -- lane l finds its value of
//     row r at (start of row r in the chunk) + (lanes below l with bit r set): the set lanes of a row read CONSECUTIVE doubles of the slab.
//   * {word offset, value offset, smallest column, chunks} in the group table.
// One workgroup of NW waves (2, 4 or 8) per group, a wave owns a contiguous share of the chunks.  Pipeline of a wave: the words of chunk c + 2, the
// gather of chunk c + 1 and the 16-byte value loads of chunk c + 1 are issued in front of the arithmetic of chunk c (values from the wave's
// LDS slab, x and word in registers) and waited for behind it; registers are the second buffer of the values.  Loads beyond the group fall
// outside their buffer range: nothing is fetched, the word reads 0 -- no row, column offset 0: a valid gather that is never multiplied.
// Row sums: per wave, lane and row in union order; then per lane the NW waves' parts in wave order from LDS; then the DPP tree over the 64
// lanes (es_group_sum) -- no atomics, the association is fixed by the stored form and NW.  Not the reference's storage order (neither are k_csr_rows'
// and k_csr_estream's on these levels): 1e-13 of the row's absolute sum, tests/test_gpu_rgroup.py.
#pragma once

#include "kernels3.hip.h"

namespace fasp {

template <int R, int NW, int OP>
__global__ __launch_bounds__(NW * 64) void k_csr_rgroup(CsrArgs a)
{
    if (a.stop && *a.stop) return;
    constexpr int SLAB = 64 * R, NQ = SLAB / 128, SH = 32 - R;
    static_assert((R == 8 || R == 16) && (NW == 2 || NW == 4 || NW == 8), "rows per group, waves per group");
    extern __shared__ __attribute__((aligned(16))) double rg_lds[];   // NW slabs of SLAB doubles (after the loop: the waves' R row sums)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // blocks b and b + 8 share an XCD: an XCD's workgroups take one contiguous eighth of the groups (neighbouring groups share columns)
    const int per = (int)gridDim.x >> 3;
    const int g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3));
    if (g >= a.rg_ng) return;   // (the whole workgroup)
    const int woff = es_tab(a.rg_meta, 4 * g), voff = es_tab(a.rg_meta, 4 * g + 1), cbase = es_tab(a.rg_meta, 4 * g + 2), nch = es_tab(a.rg_meta, 4 * g + 3);
    const int len = es_tab(a.rg_meta, 4 * g + 4) - woff - (nch + 1);   // union columns
    const int* const coff = reinterpret_cast<const int*>(a.rg_code) + woff;
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned*>(a.rg_code) + woff + nch + 1, 0, len * 4, 0x00020000);
    double* const sv = rg_lds + wave * SLAB;
    const int c_lo = nch * wave / NW, c_hi = nch * (wave + 1) / NW;   // this wave's chunks

    auto load_word = [&](int c) { return (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rw, (c * 64 + lane) * 4, 0, 0); };
    f64x2_t qv[NQ];
    // n values from value vo on: 16 bytes per lane and piece, as many pieces as n needs (wave-uniform)
    auto stage_load = [&](int vo, int n) {
        const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(a.rg_val) + vo, 0, ((n + 1) & ~1) * 8, 0x00020000);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            if (q * 128 < n) qv[q] = __builtin_bit_cast(f64x2_t, __builtin_amdgcn_raw_buffer_load_b128(rv, (lane + 64 * q) * 16, 0, 0));
    };
    auto stage_store = [&](int n) {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            if (q * 128 < n) reinterpret_cast<f64x2_t*>(sv)[lane + 64 * q] = qv[q];
    };

    double acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    if (c_lo < c_hi) {
        int v0 = voff + es_tab(coff, c_lo), v1 = voff + es_tab(coff, c_lo + 1);
        unsigned wcur = load_word(c_lo), wnext = load_word(c_lo + 1);
        stage_load(v0, v1 - v0);
        double xcur = a.x[cbase + (int)(wcur & 0xffffu)];
        stage_store(v1 - v0);
        wave_order();
        for (int c = c_lo; c < c_hi; ++c) {
            const bool more = c + 1 < c_hi;
            const int  v2 = more ? voff + es_tab(coff, c + 2) : v1;
            // the next chunk, issued in front of this chunk's arithmetic, waited for behind it
            const unsigned wn2   = load_word(c + 2);
            const double   xnext = a.x[cbase + (int)(wnext & 0xffffu)];
            stage_load(v1, v2 - v1);
            // this chunk: row r's values lie behind those of the rows before it
            // Straight-line: all R reads of the slab are issued before the first product waits for one (under a branch per row the
            // compiler waits for every read where it is issued).  A lane without the bit reads a neighbour's value or what the slab
            // held -- inside the slab, never used: it adds +0.0, which leaves a sum that started from +0.0 as it is.
            int rb = 0;
            double vv[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const unsigned long long m = __builtin_amdgcn_ballot_w64(((wcur >> (SH + r)) & 1u) != 0u);
                const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                vv[r] = sv[rb + rank];
                rb += __builtin_popcountll(m);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double p = vv[r] * xcur;
                acc[r] = acc[r] + (((wcur >> (SH + r)) & 1u) != 0u ? p : 0.0);
            }
            wave_order();
            stage_store(v2 - v1);
            wave_order();
            wcur = wnext; wnext = wn2; xcur = xnext; v0 = v1; v1 = v2;
        }
    }
    // every wave leaves its R x 64 partial sums in its own slab; wave w then owns the rows w R / NW ..: per lane the NW waves' parts in wave
    // order, then the DPP tree over the 64 lanes (the total ends in lane 63) -- R / NW trees per wave instead of R
    wave_order();
#pragma unroll
    for (int r = 0; r < R; ++r) sv[r * 64 + lane] = acc[r];
    __syncthreads();
    constexpr int PP = R / NW > 0 ? R / NW : 1;   // rows per wave
    if (wave * PP < R) {                          // (R < NW: the last waves have no row)
#pragma unroll
        for (int j = 0; j < PP; ++j) {
            const int r = wave * PP + j;
            double s = rg_lds[r * 64 + lane];
#pragma unroll
            for (int q = 1; q < NW; ++q) s += rg_lds[q * SLAB + r * 64 + lane];
            s = es_group_sum<64>(s);
            const int row = g * R + r;
            if (lane == 63 && row < a.nrow) es_epilogue<OP>(a, row, s);
        }
    }
}

}  // namespace fasp
