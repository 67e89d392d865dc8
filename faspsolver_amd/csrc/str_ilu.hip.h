// str_ilu.hip.h -- the triangular solves of a structured ILU(0) / ILU(1) factor on the device: z = U^-1 L^-1 r.
// Part of the single translation unit solver.hip (included there after str.hip.h; not a stand-alone header).
//
// Reference: fasp_precond_dstr_ilu0 / _ilu1 (PreSTR.c:71 / :349) on a factor of fasp_ilu_dstr_setup0 / _setup1 (csrc/str_ilu_setup.cpp).
// Arithmetic: row i starts from its right-hand side and subtracts one term at a time in the reference's order,
//   L  -1, [1-nline,] -nline, [nline-nplane, 1-nplane,] -nplane        U  +1, [nline-1,] +nline, [nplane-nline, nplane-1,] +nplane
// (in brackets: ILU(1) only), acc_p = acc_p - (B x)_p with (B x)_p summed left to right from its first product (nc = 6: from 0.0, as
// fasp_blas_smat_mxv's general text does); U ends with z = D acc, D the inverted pivot block.  No fused multiply-add (-ffp-contract=off).
// A term is evaluated only where the point it reads is the row's GEOMETRIC neighbour: grid point i = x + gx (y + gy z), term (dx, dy, dz)
// reads (x + dx, y + dy, z + dz) and does not exist when that leaves the grid.  The reference evaluates every term whose index i + offset
// lies in 0 .. ngrid-1; the two agree because the host checks at bind time (str_ilu_describe) that every coefficient of the other kind is
// exactly 0.0 -- every grid-derived matrix gives that -- so z can differ from the reference's in the sign of a zero only.
//
// Layout: every evaluated band of both triangles in a StrBands store of its own (str_common.hip.h).  The offsets and the term geometry are
// a handful of integers in the kernel arguments.
//
// Schedule: level(i) = x + wy y + wz z with (wy, wz) = (1, 1) for ILU(0) and (2, 3) for ILU(1): every L term lowers the level by at least
// one (ILU(1): -1, -1, -2, -1, -2, -3).  L runs the levels upwards, U downwards.  Lane = (grid point, component p); a wavefront holds
// 64 / nc whole points, so that U's closing product D acc takes acc's other components by a shuffle.  Two forms of k_str_tri:
//   level   (k_str_tri_level)  one launch per level, the points of a level enumerated from (y, z), x = level - wy y - wz z.  No spins.
//   pipe    (k_str_tri_pipe)   3-D only.  A workgroup draws a z-plane from a ticket counter in z order and walks its in-plane levels
//           s = x + wy y with __syncthreads() between them; in-plane operands come from an LDS ring of the last three in-plane levels (indexed
//           by y), the operands of plane z -+ 1 from global memory, where the value is the flag: the output vector is prefilled with the
//           sentinel (all bits set), every result is published by one 8-byte agent-scope atomic store and consumed by agent-scope atomic
//           loads that spin while they see the sentinel -- the idiom of k_ilu_flow (ilu.hip.h).  The cross-plane loads of a point are issued
//           before its matrix values and its in-plane chain.  A plane waits only for the plane before it, which holds a lower ticket, drawn
//           by a workgroup that is running or has finished: no residency assumption, one workgroup is merely sequential.  Every spin is
//           bounded by flow_give_up (2 s, the error word, seq_err_check: the solve fails loudly, later applications use the level form);
//           a workgroup that saw the error word leaves at its next step.
// str_ilu_plan is the one place that chooses the form.

namespace fasp_str {

struct StrTriArgs {
    const double* band[6];   // term k's coefficients: the block of grid point i at i * NC * NC
    const double* diag;      // U: the inverted pivot blocks
    const double* in;        // right-hand side
    double*       out;       // solution; also what the terms read
    int           off[6];    // term k reads grid point i + off[k] ...
    int           dx[6], dy[6], dz[6];   // ... which is (x + dx, y + dy, z + dz)
    int           nt;        // terms; the last ncross of them leave the plane (dz != 0), the others do not
    int           ncross;
    int           gx, gy, gz, wy, wz;
    unsigned*     sync;      // pipe: [0] ticket, [1] error word, [6..7] host-mapped error word (flow_give_up)
};

template <int NC>
__device__ __forceinline__ double str_row_dot(const double* a, const double* x)
{
    double m = NC == 6 ? 0.0 + a[0] * x[0] : a[0] * x[0];
#pragma unroll
    for (int q = 1; q < NC; ++q) m = m + a[q] * x[q];
    return m;
}

__device__ __forceinline__ bool str_term_exists(const StrTriArgs& a, int k, int x, int y, int z)
{
    return (unsigned)(x + a.dx[k]) < (unsigned)a.gx && (unsigned)(y + a.dy[k]) < (unsigned)a.gy && (unsigned)(z + a.dz[k]) < (unsigned)a.gz;
}

// U: z_p = (D acc)_p, acc's components sit in the NC lanes of the point (lanes lp * NC .. + NC - 1 of this wavefront); every lane of the
// wavefront calls this.  L: acc itself.
template <int NC, bool UPPER>
__device__ __forceinline__ double str_tri_finish(const StrTriArgs& a, bool act, int i, int p, int lp, double acc)
{
    if (!UPPER) return acc;
    if (NC == 1) return act ? acc * a.diag[i] : 0.0;
    double v[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) v[q] = __shfl(acc, min(lp * NC + q, 63));
    if (!act) return 0.0;
    const double* d = a.diag + ((size_t)i * NC + p) * NC;
    double dv[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) dv[q] = d[q];
    return str_row_dot<NC>(dv, v);
}

// one level: the points (x, y, z) with x + wy y + wz z == lev, z in zlo .. zlo + npts / gy - 1, enumerated as pt = y + gy (z - zlo)
template <int NC, bool UPPER>
__global__ __launch_bounds__(256) void k_str_tri_level(const StrTriArgs a, int lev, int zlo, int npts)
{
    constexpr int PPW = 64 / NC, PPB = 4 * PPW;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int lp = lane / NC, p = lane - lp * NC;
    const int pt = (int)blockIdx.x * PPB + wave * PPW + lp;
    bool act = lp < PPW && pt < npts;
    int x = 0, y = 0, z = 0;
    if (act) {
        y = pt % a.gy; z = zlo + pt / a.gy;
        x = lev - a.wy * y - a.wz * z;
        act = (unsigned)x < (unsigned)a.gx;
    }
    const int i = act ? x + a.gx * (y + a.gy * z) : 0;
    double acc = act ? a.in[(size_t)i * NC + p] : 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (k < a.nt && act && str_term_exists(a, k, x, y, z)) {
            const double* __restrict__ B = a.band[k] + ((size_t)i * NC + p) * NC;
            const double* __restrict__ xs = a.out + (size_t)(i + a.off[k]) * NC;
            double av[NC], xv[NC];
#pragma unroll
            for (int q = 0; q < NC; ++q) { av[q] = __builtin_nontemporal_load(B + q); xv[q] = xs[q]; }
            acc = acc - str_row_dot<NC>(av, xv);
        }
    }
    const double res = str_tri_finish<NC, UPPER>(a, act, i, p, lp, acc);
    if (act) a.out[(size_t)i * NC + p] = res;
}

// planes pipelined over workgroups (header of this file).  Dynamic LDS: 3 * gy * NC doubles.
template <int NC, bool UPPER>
__global__ __launch_bounds__(256) void k_str_tri_pipe(const StrTriArgs a)
{
    typedef __attribute__((address_space(1))) unsigned long long gu64;
    typedef __attribute__((address_space(1))) unsigned gu32;
    extern __shared__ double s_ring[];   // [3][gy][NC]: in-plane level s of this plane lives in slot s % 3, by y
    __shared__ int s_ticket, s_abort[2];   // s_abort[step parity]: a lane of this step gave up (read after the step's barrier only)
    constexpr int PPW = 64 / NC, PPB = 4 * PPW;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int lp = lane / NC, p = lane - lp * NC, lpb = wave * PPW + lp;
    const bool lane_ok = lp < PPW;
    const int S = (a.gx - 1) + a.wy * (a.gy - 1);   // the last in-plane level
    const int ringlen = a.gy * NC, nin = a.nt - a.ncross;
    unsigned spins = 0, stepno = 0;
    unsigned long long t0 = 0;
    if (threadIdx.x == 0) { s_abort[0] = 0; s_abort[1] = 0; }
    for (;;) {
        if (threadIdx.x == 0) {
            int t = (int)__hip_atomic_fetch_add((gu32*)a.sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__hip_atomic_load((gu32*)(a.sync + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) t = a.gz;   // somebody gave up
            s_ticket = t;
        }
        __syncthreads();
        const int t = s_ticket;
        __syncthreads();
        if (t >= a.gz) break;
        const int z = UPPER ? a.gz - 1 - t : t;
        for (int st = 0; st <= S; ++st) {
            const int s = UPPER ? S - st : st;
            const int ylo = s > a.gx - 1 ? (s - (a.gx - 1) + a.wy - 1) / a.wy : 0, yhi = min(a.gy - 1, s / a.wy);
            double* const cur = s_ring + (s % 3) * ringlen;
            for (int y0 = ylo; y0 <= yhi; y0 += PPB) {   // (a level wider than the workgroup: its points are independent)
                const int  y = y0 + lpb;
                const bool act = lane_ok && y <= yhi;
                const int  x = s - a.wy * y;
                const int  i = act ? x + a.gx * (y + a.gy * z) : 0;
                // the operands of the neighbouring plane first: they have been on their way longest
                unsigned long long bits[3][NC];
                bool ex[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) ex[k] = k < a.nt && act && str_term_exists(a, k, x, y, z);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
#pragma unroll
                    for (int q = 0; q < NC; ++q) bits[c][q] = 0ull;
#pragma unroll
                    for (int k = 0; k < 6; ++k)
                        if (c < a.ncross && k == nin + c && ex[k]) {
#pragma unroll
                            for (int q = 0; q < NC; ++q)
                                bits[c][q] = __hip_atomic_load((gu64*)(a.out + (size_t)(i + a.off[k]) * NC + q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                }
                double acc = act ? a.in[(size_t)i * NC + p] : 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    if (!ex[k]) continue;
                    const double* __restrict__ B = a.band[k] + ((size_t)i * NC + p) * NC;
                    double av[NC], xv[NC];
#pragma unroll
                    for (int q = 0; q < NC; ++q) av[q] = __builtin_nontemporal_load(B + q);
                    if (k < nin) {   // in the plane: this workgroup's own earlier levels
                        const double* xs = s_ring + ((s + a.dx[k] + a.wy * a.dy[k]) % 3) * ringlen + (y + a.dy[k]) * NC;
#pragma unroll
                        for (int q = 0; q < NC; ++q) xv[q] = xs[q];
                    } else {
                        const int c = k - nin;
#pragma unroll
                        for (int q = 0; q < NC; ++q) {
                            unsigned long long b = 0ull;
#pragma unroll
                            for (int cc = 0; cc < 3; ++cc)
                                if (cc == c) b = bits[cc][q];
                            gu64* src = (gu64*)(a.out + (size_t)(i + a.off[k]) * NC + q);
                            while (b == ~0ull) {
                                if (flow_give_up(a.sync, spins, t0)) { s_abort[stepno & 1u] = 1; break; }
                                __builtin_amdgcn_s_sleep(1);
                                b = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            }
                            xv[q] = __longlong_as_double((long long)b);
                        }
                    }
                    acc = acc - str_row_dot<NC>(av, xv);
                }
                const double res = str_tri_finish<NC, UPPER>(a, act, i, p, lp, acc);
                if (act) {
                    cur[y * NC + p] = res;
                    __hip_atomic_store((gu64*)(a.out + (size_t)i * NC + p), (unsigned long long)__double_as_longlong(res), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            __syncthreads();
            if (s_abort[stepno & 1u]) return;   // (uniform: the next step writes the other word, which was found clear a step ago)
            ++stepno;
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// what a factor looks like to the device: geometry, the evaluated terms of both triangles, the schedule
struct StrIluDesc {
    int ngrid = 0, nc = 0, lfil = 0;
    int gx = 0, gy = 0, gz = 0, wy = 1, wz = 1;
    int nt = 0, ncross = 0;           // evaluated terms per triangle, those of them that leave the plane (the last ones)
    int slot[2][6];                   // [0: L, 1: U][k]: LU->offdiag slot
    int off[2][6], dx[2][6], dy[2][6], dz[2][6];
};

// Is LU a factor of fasp_ilu_dstr_setup0 (lfil 0) / _setup1 (lfil 1) the device can apply?  Fills D.  Pure host code.
// why (may be NULL): the reason when not.
static bool str_ilu_describe(const dSTRmat* LU, int lfil, StrIluDesc& D, const char** why)
{
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!LU || (lfil != 0 && lfil != 1) || LU->ngrid <= 0 || LU->nc < 1 || LU->nc > 7 || !LU->diag || !LU->offsets || !LU->offdiag) { *why = "not a factor (NULL or zeroed, or nc outside 1 .. 7)"; return false; }
    if ((long long)LU->ngrid * LU->nc * LU->nc > 0x7fffffffLL) { *why = "too large"; return false; }
    StrGrid G;
    if (!str_grid(LU, G, why)) return false;
    const int ngrid = LU->ngrid, nline = G.nline, nplane = G.nplane;
    D.ngrid = ngrid; D.nc = LU->nc; D.lfil = lfil;
    D.gx = G.gx; D.gy = G.gy; D.gz = G.gz;
    const bool three_d = D.gz > 1;
    D.wy = lfil ? 2 : 1; D.wz = lfil ? 3 : 1;
    // the L terms in the reference's order: (slot, dx, dy, dz); U: slot + 1, mirrored
    static const int T0[3][4] = {{0, -1, 0, 0}, {2, 0, -1, 0}, {4, 0, 0, -1}};
    static const int T1[6][4] = {{0, -1, 0, 0}, {2, 1, -1, 0}, {4, 0, -1, 0}, {6, 0, 1, -1}, {8, 1, 0, -1}, {10, 0, 0, -1}};
    const int nall = lfil ? 6 : 3, nband = lfil ? 12 : (three_d ? 6 : LU->nband);
    if (LU->nband != nband || (nband != 4 && nband != 6 && nband != 12)) { *why = "nband is not that of the fill level"; return false; }
    const int want0[6] = {-1, 1, -nline, nline, -nplane, nplane};
    const int want1[12] = {-1, 1, 1 - nline, nline - 1, -nline, nline, nline - nplane, nplane - nline, 1 - nplane, nplane - 1, -nplane, nplane};
    for (int b = 0; b < nband; ++b) {
        if (LU->offsets[b] != (lfil ? want1[b] : want0[b])) { *why = "offsets are not the factor's canonical ones"; return false; }
        if (ngrid - std::abs(LU->offsets[b]) > 0 && !LU->offdiag[b]) { *why = "a band is missing"; return false; }
    }
    D.nt = 0; D.ncross = 0;
    for (int k = 0; k < nall; ++k) {
        const int* T = lfil ? T1[k] : T0[k];
        if (T[0] >= nband) continue;                 // ILU(0) on a 2-D grid has no plane bands
        const bool evaluated = three_d || T[3] == 0; // on a 2-D grid the plane terms reach no geometric neighbour
        for (int u = 0; u < 2; ++u) {
            const int slot = T[0] + u, sg = u ? -1 : 1, dx = sg * T[1], dy = sg * T[2], dz = sg * T[3];
            if (!str_offgrid_coefficients_are_zero(LU, G, slot, dx, dy, dz, evaluated, why)) return false;
            if (evaluated) {
                const int k2 = D.nt;
                D.slot[u][k2] = slot; D.off[u][k2] = LU->offsets[slot]; D.dx[u][k2] = dx; D.dy[u][k2] = dy; D.dz[u][k2] = dz;
            }
        }
        if (evaluated) { ++D.nt; if (T[3] != 0) ++D.ncross; }
    }
    return true;
}

constexpr size_t STR_ILU_PIPE_LDS = 64 * 1024;   // the in-plane ring of the pipelined form at most

// The one place that chooses the form: 0 one launch per level, 1 planes pipelined over workgroups.
static int str_ilu_plan(const StrIluDesc& D)
{
    if (D.gz <= 1) return 0;                                                    // 2-D: nothing to pipeline
    if (sizeof(double) * 3 * (size_t)D.gy * D.nc > STR_ILU_PIPE_LDS) return 0;   // the ring of in-plane levels must fit
    if (g_tune.str_ilu_form == 0 || g_flow_disabled) return 0;
    return 1;   // (default and str_ilu_form 1: measured faster on every 3-D shape, profiles/str_ilu_apply.txt)
}

struct StrIluDev {
    StrIluDesc D;
    DevPool  pool;
    StrBands B[2][6];                     // [0: L, 1: U][k]: term k, a store of one band each (see the constructor)
    double*  diag = nullptr, *y = nullptr, *z = nullptr, *r = nullptr;
    unsigned* sync = nullptr;
    std::vector<int> lvl_zlo, lvl_npts;   // level launches: first plane and points enumerated (gy per plane) of each level
    bool ok = false;
    bool used_pipe = false;
    StrIluDev(const dSTRmat* LU, const StrIluDesc& desc) : D(desc)
    {
        if (ctx_init() < 0) return;
        const size_t nc2 = (size_t)D.nc * D.nc, n = (size_t)D.ngrid * D.nc;
        if (!pool.get(&diag, (size_t)D.ngrid * nc2) || !pool.get(&y, n) || !pool.get(&z, n) || !pool.get(&r, n) || !pool.get(&sync, 16)) return;
        if (hipMemcpy(diag, LU->diag, sizeof(double) * (size_t)D.ngrid * nc2, hipMemcpyHostToDevice) != hipSuccess) return;
        // One allocation per band, not one store over the 2 nt picks: with a triangle's bands exactly `stride` apart the level form measured
        // 1.7 % slower on P7(128), nc 1 (stride 16 MiB) and 1.6 % faster on P7(256) (profiles/str_refactor_ab.txt); this keeps both as they were.
        for (int u = 0; u < 2; ++u)
            for (int k = 0; k < D.nt; ++k)
                if (!B[u][k].init(pool, LU, {D.slot[u][k]})) return;
        if (!str_sync_words(sync)) return;
        str_diag_levels(D.gx, D.gy, D.gz, D.wy, D.wz, lvl_zlo, lvl_npts);
        ok = true;
    }
    // matrix values of both triangles and the pivots, the right-hand side read, y written and read, z written
    double bytes() const { return 8.0 * ((2.0 * D.nt + 1.0) * D.ngrid * D.nc * D.nc + 4.0 * D.ngrid * D.nc); }
};

template <int NC, bool UPPER>
static void str_tri_launch(StrIluDev& M, int form, const StrTriArgs& a)
{
    constexpr int PPB = 4 * (64 / NC);
    if (form == 1) {
        const int cap = g_tune.str_ilu_wgs > 0 ? g_tune.str_ilu_wgs : 2 * std::max(g_ctx.num_cu, 1);
        const size_t lds = sizeof(double) * 3 * (size_t)a.gy * NC;
        hipLaunchKernelGGL((k_str_tri_pipe<NC, UPPER>), dim3((unsigned)std::max(1, std::min(a.gz, cap))), dim3(256), lds, g_ctx.stream, a);
        return;
    }
    const int nlev = (int)M.lvl_zlo.size();
    for (int t = 0; t < nlev; ++t) {
        const int l = UPPER ? nlev - 1 - t : t, npts = M.lvl_npts[(size_t)l];
        hipLaunchKernelGGL((k_str_tri_level<NC, UPPER>), dim3((unsigned)((npts + PPB - 1) / PPB)), dim3(256), 0, g_ctx.stream, a, l, M.lvl_zlo[(size_t)l], npts);
    }
}

template <int NC>
static int str_tri_solve_nc(StrIluDev& M, int form, bool upper, const StrTriArgs& a)
{
    if (form == 1) {
        HIPCK(hipMemsetAsync(a.out, 0xFF, sizeof(double) * (size_t)M.D.ngrid * NC, g_ctx.stream));   // the sentinel: not yet computed
        HIPCK(hipMemsetAsync(M.sync, 0, 8, g_ctx.stream));                                             // ticket counter + error word
    }
    if (upper) str_tri_launch<NC, true>(M, form, a);
    else str_tri_launch<NC, false>(M, form, a);
    return hipGetLastError() == hipSuccess ? FASP_SUCCESS : ERROR_MISC;
}

// out = U^-1 L^-1 in (device vectors of ngrid nc, not the same; L's result goes through M.y)
static int str_ilu_apply(StrIluDev& M, const double* in, double* out)
{
    if (seq_err_pending()) return seq_err_check();
    const int form = str_ilu_plan(M.D);
    if (form == 1) M.used_pipe = true;
    for (int u = 0; u < 2; ++u) {
        StrTriArgs a{};
        for (int k = 0; k < M.D.nt; ++k) {
            a.band[k] = M.B[u][k].val; a.off[k] = M.D.off[u][k];
            a.dx[k] = M.D.dx[u][k]; a.dy[k] = M.D.dy[u][k]; a.dz[k] = M.D.dz[u][k];
        }
        a.diag = M.diag; a.in = u ? M.y : in; a.out = u ? out : M.y;
        a.nt = M.D.nt; a.ncross = M.D.ncross;
        a.gx = M.D.gx; a.gy = M.D.gy; a.gz = M.D.gz; a.wy = M.D.wy; a.wz = M.D.wz;
        a.sync = M.sync;
        const int st = str_for_nc(M.D.nc, [&](auto NC) { return str_tri_solve_nc<NC()>(M, form, u != 0, a); });
        if (st < 0) return st;
    }
    return FASP_SUCCESS;
}
}  // namespace fasp_str
