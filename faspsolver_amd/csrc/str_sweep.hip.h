// str_sweep.hip.h -- the smoothers of a structured matrix on the device: Jacobi, Gauss-Seidel and SOR in every order of the reference.
// Part of the single translation unit solver.hip (included there after str_ilu.hip.h; not a stand-alone header).
//
// Reference: ItrSmootherSTR.c (fasp_smoother_dstr_jacobi1 :92, _gs_ascend :322, _gs_descend :438, _gs_order :556, _gs_cf :680,
// _sor_ascend :981, _sor_descend :1102, _sor_order :1224, _sor_cf :1355).  Arithmetic: a visit of grid point i starts
// from b_i and subtracts the existing band terms in band STORAGE order, rhs_p = rhs_p - a_pq u_q with q ascending (blkcontr2 :1833), then
//   GS   nc = 1: u_i = rhs / diag_i (a division);  nc > 1: u_i = diaginv_i rhs summed as fasp_blas_smat_mxv does (str_row_dot)
//   SOR  nc = 1: u_i = (1 - w) u_i + w (rhs / diag_i);  nc > 1: aAxpby (:1876): w == 0: u_p (1 - w), otherwise t = (1 - w) / w,
//        u_p = u_p t, u_p = u_p + diaginv_pq rhs_q (q ascending), u_p = u_p w.  The reference's scalar _sor_cf closes the points of its SECOND
//        pass as Gauss-Seidel does (:1443); so does this file (bit 31 of a list entry).
//   Jacobi: every term reads the vector as it came in, then the closing step of GS.
// No fused multiply-add (-ffp-contract=off).
//
// Layout: the bands that have terms, in storage order, in a StrBands store (str_common.hip.h).  No matrix index arrays.  Lane = (grid point,
// component p); a wavefront holds 64 / nc whole points, so that the closing product takes rhs's other components by a shuffle (as k_str_tri).
//
// Forms of a GS / SOR sweep (str_sweep_plan is the one place that chooses):
//   level    ASCEND / DESCEND on a grid-like matrix.  Level x + y + z, one launch per level, the points of a level enumerated from (y, z), in
//            place: a point of level L reads new values at L - 1 and old values at L + 1, which are not yet written.
//   pipe     3-D, the schedule of k_str_tri_pipe: a ticket per z-plane, in-plane levels s = x + y with __syncthreads() between them, the new
//            in-plane operands (level s -+ 1) from an LDS ring of two levels indexed by y, the new operands of plane z -+ 1 from global memory
//            where the value is the flag.  A vector that is swept in place cannot be prefilled with the sentinel, so this form reads the old
//            operands from the input vector without a spin and writes the new values to a second vector prefilled with the sentinel; the
//            two change places after the sweep.  Every spin is bounded by flow_give_up; a plane waits only for the plane with the lower
//            ticket: no residency assumption.
//   ordered  every other sweep (a user's sequence, the C/F orders, a matrix that is not grid-like).  The host gives every visit of the
//            sequence a level (str_sweep_levels), sorts the visits stably by level into one list of 4 bytes per visit -- the only index
//            array -- and k_str_sweep_list runs one launch per level over its slice, in place.
// "Grid-like": the offsets of the bands that have terms are distinct members of {+-1, +-nline, +-nplane} (the rule of section 3.7) and every
// coefficient between two points that are not geometric neighbours is exactly 0.0 (checked on the host, str_sweep_describe).  Such a term is
// never evaluated: for finite u, rhs - 0 u is rhs (but for a rhs that is -0.0 at that moment: the sign of a zero).

namespace fasp_str {

enum : int { STR_SWEEP_JACOBI = 0, STR_SWEEP_GS = 1, STR_SWEEP_SOR = 2 };
enum : int { STR_SWF_LEVEL = 0, STR_SWF_PIPE = 1, STR_SWF_LIST = 2, STR_SWF_JACOBI = 3 };
enum : int { STR_ORDER_ASCEND = 12, STR_ORDER_DESCEND = 21, STR_ORDER_USER = 0 };

struct StrSweepArgs {
    const double* val;      // nb bands of `stride` doubles, storage order; the block of grid point i at i * NC * NC
    size_t        stride;
    const double* diag;     // NC == 1: the diagonal of A; NC > 1: the inverted diagonal blocks
    const double* b;
    const double* in;       // what the old operands are read from (pipe, Jacobi); == out in the in-place forms
    double*       out;
    const int*    terms;    // list, Jacobi: nb x {offset, dx, dy, dz}
    const int*    list;     // list: grid point of a visit, bit 31: close as Gauss-Seidel (header)
    int           nb, ngrid;
    int           geo;      // list: a term exists iff it reaches the geometric neighbour (grid-like matrix); 0: iff 0 <= i + offset < ngrid
    int           off[6], dx[6], dy[6], dz[6];   // level, pipe (nb <= 6)
    int           kind[6];  // pipe: 0 old operand (from `in`), 1 new, in the plane (LDS ring), 2 new, of the neighbouring plane (spin on `out`)
    int           kcross;   // pipe: the term of kind 2, or -1
    int           gx, gy, gz;
    double        w, omw, t;   // SOR: weight, 1 - w, (1 - w) / w
    unsigned*     sync;     // pipe: [0] ticket, [1] error word, [6..7] host-mapped error word (flow_give_up)
};

// rhs_p = rhs_p - a_pq u_q, q ascending (blkcontr2)
template <int NC>
__device__ __forceinline__ double str_sweep_sub(double rhs, const double* av, const double* xv)
{
#pragma unroll
    for (int q = 0; q < NC; ++q) rhs = rhs - av[q] * xv[q];
    return rhs;
}

__device__ __forceinline__ bool str_sweep_geo_exists(const StrSweepArgs& a, int k, int x, int y, int z)
{
    return (unsigned)(x + a.dx[k]) < (unsigned)a.gx && (unsigned)(y + a.dy[k]) < (unsigned)a.gy && (unsigned)(z + a.dz[k]) < (unsigned)a.gz;
}

// the closing step of a visit (header); rhs's components sit in the NC lanes of the point (lanes lp * NC .. + NC - 1 of this wavefront);
// every lane of the wavefront calls this.  uold: u_i,p before the visit (SOR).
template <int NC, bool SOR>
__device__ __forceinline__ double str_sweep_close(const StrSweepArgs& a, bool act, int i, int p, int lp, double rhs, double uold, bool as_gs)
{
    if (NC == 1) {
        if (!act) return 0.0;
        const double q = rhs / a.diag[i];
        if (!SOR || as_gs) return q;
        return a.omw * uold + a.w * q;
    }
    double v[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) v[q] = __shfl(rhs, min(lp * NC + q, 63));
    if (!act) return 0.0;
    const double* d = a.diag + ((size_t)i * NC + p) * NC;
    double dv[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) dv[q] = d[q];
    if (!SOR) return str_row_dot<NC>(dv, v);
    if (a.w == 0.0) return uold * a.omw;
    double y = uold * a.t;
#pragma unroll
    for (int q = 0; q < NC; ++q) y = y + dv[q] * v[q];
    return y * a.w;
}

// b_i minus the existing terms of grid point i in storage order, every operand from u; the terms from a.terms (any number of bands)
template <int NC>
__device__ __forceinline__ double str_sweep_rhs(const StrSweepArgs& a, bool act, int i, int p, const double* u)
{
    double rhs = act ? a.b[(size_t)i * NC + p] : 0.0;
    int x = 0, y = 0, z = 0;
    if (a.geo) { x = i % a.gx; const int r = i / a.gx; y = r % a.gy; z = r / a.gy; }
    const double* ap = a.val + ((size_t)i * NC + p) * NC;
    for (int k = 0; k < a.nb; ++k, ap += a.stride) {
        const int off = a.terms[4 * k];
        const bool ex = a.geo ? (unsigned)(x + a.terms[4 * k + 1]) < (unsigned)a.gx && (unsigned)(y + a.terms[4 * k + 2]) < (unsigned)a.gy &&
                                    (unsigned)(z + a.terms[4 * k + 3]) < (unsigned)a.gz
                              : (unsigned)(i + off) < (unsigned)a.ngrid;
        if (!(act && ex)) continue;
        const double* xs = u + (size_t)(i + off) * NC;
        double av[NC], xv[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) { av[q] = __builtin_nontemporal_load(ap + q); xv[q] = xs[q]; }
        rhs = str_sweep_sub<NC>(rhs, av, xv);
    }
    return rhs;
}

// Jacobi: one pass, out of place (in: the vector as it came in)
template <int NC>
__global__ __launch_bounds__(256) void k_str_jacobi(const StrSweepArgs a)
{
    constexpr int PPW = 64 / NC, PPB = 4 * PPW;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int lp = lane / NC, p = lane - lp * NC;
    const long long pt = (long long)blockIdx.x * PPB + wave * PPW + lp;
    const bool act = lp < PPW && pt < a.ngrid;
    const int i = act ? (int)pt : 0;
    const double rhs = str_sweep_rhs<NC>(a, act, i, p, a.in);
    const double res = str_sweep_close<NC, false>(a, act, i, p, lp, rhs, 0.0, false);
    if (act) a.out[(size_t)i * NC + p] = res;
}

// ordered form: the visits list[first .. first + count) of one level, in place
template <int NC, bool SOR>
__global__ __launch_bounds__(256) void k_str_sweep_list(const StrSweepArgs a, int first, int count)
{
    constexpr int PPW = 64 / NC, PPB = 4 * PPW;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int lp = lane / NC, p = lane - lp * NC;
    const long long pt = (long long)blockIdx.x * PPB + wave * PPW + lp;
    const bool act = lp < PPW && pt < count;
    const int e = act ? a.list[(size_t)first + (size_t)pt] : 0;
    const int i = e & 0x7fffffff;
    const double rhs = str_sweep_rhs<NC>(a, act, i, p, a.out);
    const double uold = SOR && act ? a.out[(size_t)i * NC + p] : 0.0;
    const double res = str_sweep_close<NC, SOR>(a, act, i, p, lp, rhs, uold, e < 0);
    if (act) a.out[(size_t)i * NC + p] = res;
}

// level form: the points (x, y, z) with x + y + z == lev, z in zlo .. zlo + npts / gy - 1, enumerated as pt = y + gy (z - zlo); in place
template <int NC, bool SOR>
__global__ __launch_bounds__(256) void k_str_sweep_level(const StrSweepArgs a, int lev, int zlo, int npts)
{
    constexpr int PPW = 64 / NC, PPB = 4 * PPW;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int lp = lane / NC, p = lane - lp * NC;
    const int pt = (int)blockIdx.x * PPB + wave * PPW + lp;
    bool act = lp < PPW && pt < npts;
    int x = 0, y = 0, z = 0;
    if (act) {
        y = pt % a.gy; z = zlo + pt / a.gy;
        x = lev - y - z;
        act = (unsigned)x < (unsigned)a.gx;
    }
    const int i = act ? x + a.gx * (y + a.gy * z) : 0;
    double rhs = act ? a.b[(size_t)i * NC + p] : 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (k < a.nb && act && str_sweep_geo_exists(a, k, x, y, z)) {
            const double* B = a.val + (size_t)k * a.stride + ((size_t)i * NC + p) * NC;
            const double* xs = a.out + (size_t)(i + a.off[k]) * NC;
            double av[NC], xv[NC];
#pragma unroll
            for (int q = 0; q < NC; ++q) { av[q] = __builtin_nontemporal_load(B + q); xv[q] = xs[q]; }
            rhs = str_sweep_sub<NC>(rhs, av, xv);
        }
    }
    const double uold = SOR && act ? a.out[(size_t)i * NC + p] : 0.0;
    const double res = str_sweep_close<NC, SOR>(a, act, i, p, lp, rhs, uold, false);
    if (act) a.out[(size_t)i * NC + p] = res;
}

// planes pipelined over workgroups (header of this file).  Dynamic LDS: 2 * gy * NC doubles.  DESC: planes and in-plane levels downwards.
template <int NC, bool SOR, bool DESC>
__global__ __launch_bounds__(256) void k_str_sweep_pipe(const StrSweepArgs a)
{
    typedef __attribute__((address_space(1))) unsigned long long gu64;
    typedef __attribute__((address_space(1))) unsigned gu32;
    extern __shared__ double s_swring[];   // [2][gy][NC]: in-plane level s of this plane lives in slot s & 1, by y
    __shared__ int s_ticket, s_abort[2];   // s_abort[step parity]: a lane of this step gave up (read after the step's barrier only)
    constexpr int PPW = 64 / NC, PPB = 4 * PPW;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int lp = lane / NC, p = lane - lp * NC, lpb = wave * PPW + lp;
    const bool lane_ok = lp < PPW;
    const int S = (a.gx - 1) + (a.gy - 1);   // the last in-plane level
    const int ringlen = a.gy * NC;
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
        const int z = DESC ? a.gz - 1 - t : t;
        for (int st = 0; st <= S; ++st) {
            const int s = DESC ? S - st : st;
            const int ylo = s > a.gx - 1 ? s - (a.gx - 1) : 0, yhi = min(a.gy - 1, s);
            double* const cur = s_swring + (s & 1) * ringlen;
            const double* const prev = s_swring + ((s & 1) ^ 1) * ringlen;   // level s -+ 1: the step before this one
            for (int y0 = ylo; y0 <= yhi; y0 += PPB) {   // (a level wider than the workgroup: its points are independent)
                const int  y = y0 + lpb;
                const bool act = lane_ok && y <= yhi;
                const int  x = s - y;
                const int  i = act ? x + a.gx * (y + a.gy * z) : 0;
                bool ex[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) ex[k] = k < a.nb && act && str_sweep_geo_exists(a, k, x, y, z);
                // the new operand of the neighbouring plane first: it has been on its way longest
                unsigned long long bits[NC];
#pragma unroll
                for (int q = 0; q < NC; ++q) bits[q] = 0ull;
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    if (k == a.kcross && ex[k]) {
#pragma unroll
                        for (int q = 0; q < NC; ++q)
                            bits[q] = __hip_atomic_load((gu64*)(a.out + (size_t)(i + a.off[k]) * NC + q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                double rhs = act ? a.b[(size_t)i * NC + p] : 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    if (!ex[k]) continue;
                    const double* B = a.val + (size_t)k * a.stride + ((size_t)i * NC + p) * NC;
                    double av[NC], xv[NC];
#pragma unroll
                    for (int q = 0; q < NC; ++q) av[q] = __builtin_nontemporal_load(B + q);
                    if (a.kind[k] == 1) {          // new, in the plane: this workgroup's own last level
                        const double* xs = prev + (y + a.dy[k]) * NC;
#pragma unroll
                        for (int q = 0; q < NC; ++q) xv[q] = xs[q];
                    } else if (a.kind[k] == 2) {   // new, of the plane before: the value is the flag
#pragma unroll
                        for (int q = 0; q < NC; ++q) {
                            unsigned long long bq = bits[q];
                            gu64* src = (gu64*)(a.out + (size_t)(i + a.off[k]) * NC + q);
                            while (bq == ~0ull) {
                                if (flow_give_up(a.sync, spins, t0)) { s_abort[stepno & 1u] = 1; break; }
                                __builtin_amdgcn_s_sleep(1);
                                bq = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            }
                            xv[q] = __longlong_as_double((long long)bq);
                        }
                    } else {                        // old: nobody writes `in` during this launch
                        const double* xs = a.in + (size_t)(i + a.off[k]) * NC;
#pragma unroll
                        for (int q = 0; q < NC; ++q) xv[q] = xs[q];
                    }
                    rhs = str_sweep_sub<NC>(rhs, av, xv);
                }
                const double uold = SOR && act ? a.in[(size_t)i * NC + p] : 0.0;
                const double res = str_sweep_close<NC, SOR>(a, act, i, p, lp, rhs, uold, false);
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
// what a matrix looks like to the sweeps: the bands that have terms, and whether it is grid-like (header)
struct StrSweepDesc {
    int ngrid = 0, nc = 0, nb = 0;
    std::vector<int> slot, off, dx, dy, dz;   // per band with terms, in storage order: A->offdiag index, offset, geometry (grid-like only)
    bool geo = false;
    const char* why = "";                      // why not grid-like
    int gx = 0, gy = 0, gz = 0;
};

// Fills D.  Negative: a matrix the library refuses (ERROR_INPUT_PAR).  Pure host code.
static int str_sweep_describe(const dSTRmat* A, StrSweepDesc& D)
{
    if (str_plan(A, nullptr) < 0) return ERROR_INPUT_PAR;
    if ((long long)A->ngrid * A->nc * A->nc > 0x7fffffffLL) return ERROR_INPUT_PAR;
    const int ngrid = A->ngrid;
    D.ngrid = ngrid; D.nc = A->nc;
    for (int b = 0; b < A->nband; ++b)
        if (std::llabs((long long)A->offsets[b]) < (long long)ngrid) { D.slot.push_back(b); D.off.push_back(A->offsets[b]); }
    D.nb = (int)D.slot.size();
    D.dx.assign((size_t)D.nb, 0); D.dy.assign((size_t)D.nb, 0); D.dz.assign((size_t)D.nb, 0);
    D.geo = false;
    StrGrid G;
    if (!str_grid(A, G, &D.why)) return FASP_SUCCESS;
    D.gx = G.gx; D.gy = G.gy; D.gz = G.gz;
    if (D.nb > 6) { D.why = "an offset outside {+-1, +-nline, +-nplane}"; return FASP_SUCCESS; }
    for (size_t k = 0; k < (size_t)D.nb; ++k)
        if (!G.classify(D.off[k], D.dx[k], D.dy[k], D.dz[k])) { D.why = "an offset outside {+-1, +-nline, +-nplane}"; return FASP_SUCCESS; }
    for (size_t k = 0; k < (size_t)D.nb; ++k)
        if (!str_offgrid_coefficients_are_zero(A, G, D.slot[k], D.dx[k], D.dy[k], D.dz[k], true, &D.why)) return FASP_SUCCESS;
    D.geo = true;
    return FASP_SUCCESS;
}

constexpr size_t STR_SWEEP_PIPE_LDS = 64 * 1024;   // the in-plane ring of the pipelined form at most
// The default of ASCEND / DESCEND on a 3-D grid-like matrix, by measurement (profiles/str_sweep.txt)
constexpr int STR_SWEEP_DEFAULT_3D = STR_SWF_PIPE;

// The one place that chooses the form of a GS / SOR sweep.  natural: ASCEND or DESCEND without a mark array.
static int str_sweep_plan(const StrSweepDesc& D, bool natural)
{
    if (!natural || !D.geo || g_tune.str_sweep_form == STR_SWF_LIST) return STR_SWF_LIST;
    if (D.gz <= 1) return STR_SWF_LEVEL;                                                      // 2-D: nothing to pipeline
    if (sizeof(double) * 2 * (size_t)D.gy * D.nc > STR_SWEEP_PIPE_LDS) return STR_SWF_LEVEL;   // the ring of in-plane levels must fit
    if (g_tune.str_sweep_form == STR_SWF_LEVEL || g_flow_disabled) return STR_SWF_LEVEL;
    if (g_tune.str_sweep_form == STR_SWF_PIPE) return STR_SWF_PIPE;
    return STR_SWEEP_DEFAULT_3D;
}

// the visits of a sweep in the reference's order: list entries (grid point, bit 31: close as Gauss-Seidel).  cf: the C/F form with
// FIRST = order, SECOND = -order; otherwise ASCEND / DESCEND (mark NULL) or the user's sequence (mark, checked by the caller).
static void str_sweep_visits(int ngrid, int order, const int* mark, bool cf, bool second_as_gs, std::vector<int>& seq)
{
    seq.clear();
    if (cf) {
        for (int i = 0; i < ngrid; ++i) if (mark[i] == order) seq.push_back(i);
        for (int i = 0; i < ngrid; ++i) if (mark[i] == -order) seq.push_back(second_as_gs ? (int)((unsigned)i | 0x80000000u) : i);
    } else if (mark) seq.assign(mark, mark + ngrid);
    else if (order == STR_ORDER_ASCEND) for (int i = 0; i < ngrid; ++i) seq.push_back(i);
    else for (int i = ngrid - 1; i >= 0; --i) seq.push_back(i);
}

// The levels of the visits (str_visit_levels): a visit writes its grid point and reads the points its existing terms reach -- the geometric
// neighbours of a grid-like matrix, otherwise those of the index rule.  Returns the number of levels.
static int str_sweep_levels(const StrSweepDesc& D, const std::vector<int>& seq, std::vector<int>& lev)
{
    auto writes = [&](size_t v, auto&& f) { f(seq[v] & 0x7fffffff); };
    auto reads = [&](size_t v, auto&& f) {
        const int i = seq[v] & 0x7fffffff, x = D.geo ? i % D.gx : 0, y = D.geo ? (i / D.gx) % D.gy : 0, z = D.geo ? i / (D.gx * D.gy) : 0;
        for (size_t k = 0; k < (size_t)D.nb; ++k) {
            const long long j = (long long)i + D.off[k];
            const bool ex = D.geo ? (unsigned)(x + D.dx[k]) < (unsigned)D.gx && (unsigned)(y + D.dy[k]) < (unsigned)D.gy && (unsigned)(z + D.dz[k]) < (unsigned)D.gz
                                  : j >= 0 && j < D.ngrid;
            if (ex) f((int)j);
        }
    };
    return str_visit_levels(D.ngrid, seq.size(), writes, reads, lev);
}

// a sweep resident on the device: matrix, plan and vectors uploaded once
struct StrSweepDev {
    StrSweepDesc D;
    int      kind = STR_SWEEP_GS, form = STR_SWF_LIST;
    bool     desc = false;
    double   w = 1.0;
    DevPool  pool;
    StrBands B;                           // the bands D.slot
    double*  diag = nullptr, *b = nullptr, *u = nullptr, *u2 = nullptr;
    int*     terms = nullptr, *list = nullptr;
    unsigned* sync = nullptr;
    std::vector<int> lvl_zlo, lvl_npts;   // level form: first plane and points enumerated (gy per plane) of each level
    std::vector<int> lvl_first;           // ordered form: the slice of each level in the list (nlev + 1 entries)
    int      kindk[6] = {}, kcross = -1;
    bool     ok = false, used_pipe = false;
    int      launches = 0, levels = 0, wgs = 0, visits = 0;
    // dg: the diagonal (nc == 1) or the inverted diagonal blocks; seq: the visits (ordered form only)
    StrSweepDev(const dSTRmat* A, const StrSweepDesc& desc_, int kind_, int form_, bool descending, double weight, const double* dg,
                const std::vector<int>& seq, const double* hb, const double* hu)
        : D(desc_), kind(kind_), form(form_), desc(descending), w(weight)
    {
        if (ctx_init() < 0) return;
        const size_t nc2 = (size_t)D.nc * D.nc, n = (size_t)D.ngrid * D.nc;
        if (!B.init(pool, A, D.slot)) return;
        if (!pool.get(&diag, B.stride) || !pool.get(&b, n) || !pool.get(&u, n) || !pool.get(&u2, n) || !pool.get(&sync, 16) ||
            !pool.get(&terms, 4 * (size_t)std::max(D.nb, 1)))
            return;
        std::vector<int> ht(4 * (size_t)std::max(D.nb, 1), 0);
        for (size_t k = 0; k < (size_t)D.nb; ++k) { ht[4 * k] = D.off[k]; ht[4 * k + 1] = D.dx[k]; ht[4 * k + 2] = D.dy[k]; ht[4 * k + 3] = D.dz[k]; }
        if (hipMemcpy(terms, ht.data(), sizeof(int) * ht.size(), hipMemcpyHostToDevice) != hipSuccess) return;
        if (hipMemcpy(diag, dg, sizeof(double) * (size_t)D.ngrid * nc2, hipMemcpyHostToDevice) != hipSuccess) return;
        if (hipMemcpy(b, hb, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess) return;
        if (hipMemcpy(u, hu, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess) return;
        if (!str_sync_words(sync)) return;
        if (form == STR_SWF_LEVEL || form == STR_SWF_PIPE) {
            str_diag_levels(D.gx, D.gy, D.gz, 1, 1, lvl_zlo, lvl_npts);
            const int nlev = (int)lvl_zlo.size();
            for (int k = 0; k < D.nb; ++k) {   // a term is new iff its partner lies one level towards where the sweep comes from
                const int step = D.dx[(size_t)k] + D.dy[(size_t)k] + D.dz[(size_t)k];
                const bool is_new = step == (desc ? 1 : -1);
                kindk[k] = !is_new ? 0 : D.dz[(size_t)k] != 0 ? 2 : 1;
                if (kindk[k] == 2) kcross = k;
            }
            levels = nlev; visits = D.ngrid;
        } else if (form == STR_SWF_LIST) {
            std::vector<int> lev, hl;
            const int nlev = str_sweep_levels(D, seq, lev);
            str_bucket_by_level(seq, lev, nlev, lvl_first, hl, nullptr);
            if (!pool.get(&list, hl.size())) return;
            if (!hl.empty() && hipMemcpy(list, hl.data(), sizeof(int) * hl.size(), hipMemcpyHostToDevice) != hipSuccess) return;
            levels = nlev; visits = (int)seq.size();
        } else {
            levels = 1; visits = D.ngrid;
        }
        if (hipDeviceSynchronize() != hipSuccess) return;
        ok = true;
    }

    StrSweepArgs args() const
    {
        StrSweepArgs a{};
        a.val = B.val; a.stride = B.stride; a.diag = diag; a.b = b; a.in = u; a.out = u;
        a.terms = terms; a.list = list; a.nb = D.nb; a.ngrid = D.ngrid; a.geo = D.geo ? 1 : 0;
        for (int k = 0; k < std::min(D.nb, 6); ++k) {
            a.off[k] = D.off[(size_t)k]; a.dx[k] = D.dx[(size_t)k]; a.dy[k] = D.dy[(size_t)k]; a.dz[k] = D.dz[(size_t)k]; a.kind[k] = kindk[k];
        }
        a.kcross = kcross;
        a.gx = D.gx; a.gy = D.gy; a.gz = D.gz;
        a.w = w; a.omw = 1.0 - w; a.t = w == 0.0 ? 0.0 : (1.0 - w) / w;
        a.sync = sync;
        return a;
    }

    template <int NC, bool SOR>
    int sweep_nc()
    {
        constexpr int PPB = 4 * (64 / NC);
        StrSweepArgs a = args();
        launches = 0; wgs = 0;
        auto grid_of = [&](long long pts) { const int g = (int)((pts + PPB - 1) / PPB); wgs = std::max(wgs, g); ++launches; return dim3((unsigned)g); };
        if (kind == STR_SWEEP_JACOBI) {
            a.in = u; a.out = u2; a.geo = 0;   // every term of the reference: 0 <= i + offset < ngrid
            hipLaunchKernelGGL((k_str_jacobi<NC>), grid_of(D.ngrid), dim3(256), 0, g_ctx.stream, a);
            std::swap(u, u2);
        } else if (form == STR_SWF_LIST) {
            for (size_t l = 0; l + 1 < lvl_first.size(); ++l) {
                const int first = lvl_first[l], count = lvl_first[l + 1] - first;
                hipLaunchKernelGGL((k_str_sweep_list<NC, SOR>), grid_of(count), dim3(256), 0, g_ctx.stream, a, first, count);
            }
        } else if (form == STR_SWF_LEVEL) {
            const int nlev = (int)lvl_zlo.size();
            for (int t = 0; t < nlev; ++t) {
                const int l = desc ? nlev - 1 - t : t, npts = lvl_npts[(size_t)l];
                hipLaunchKernelGGL((k_str_sweep_level<NC, SOR>), grid_of(npts), dim3(256), 0, g_ctx.stream, a, l, lvl_zlo[(size_t)l], npts);
            }
        } else {
            a.in = u; a.out = u2;
            HIPCK(hipMemsetAsync(u2, 0xFF, sizeof(double) * (size_t)D.ngrid * NC, g_ctx.stream));   // the sentinel: not yet computed
            HIPCK(hipMemsetAsync(sync, 0, 8, g_ctx.stream));                                        // ticket counter + error word
            const int cap = g_tune.str_sweep_wgs > 0 ? g_tune.str_sweep_wgs : 2 * std::max(g_ctx.num_cu, 1);
            const size_t lds = sizeof(double) * 2 * (size_t)D.gy * NC;
            wgs = std::max(1, std::min(D.gz, cap)); launches = 1;
            if (desc) hipLaunchKernelGGL((k_str_sweep_pipe<NC, SOR, true>), dim3((unsigned)wgs), dim3(256), lds, g_ctx.stream, a);
            else hipLaunchKernelGGL((k_str_sweep_pipe<NC, SOR, false>), dim3((unsigned)wgs), dim3(256), lds, g_ctx.stream, a);
            std::swap(u, u2);
            used_pipe = true;
        }
        return hipGetLastError() == hipSuccess ? FASP_SUCCESS : ERROR_MISC;
    }
    template <int NC> int sweep_k() { return kind == STR_SWEEP_SOR ? sweep_nc<NC, true>() : sweep_nc<NC, false>(); }

    // one sweep; the result is in u afterwards
    int sweep()
    {
        if (D.ngrid <= 0) return FASP_SUCCESS;
        if (form == STR_SWF_PIPE && seq_err_pending()) return seq_err_check();
        return str_for_nc(D.nc, [&](auto NC) { return sweep_k<NC()>(); });
    }
    // what a sweep moves at least: the matrix, the diagonal (blocks), b, u read and written
    double bytes() const { return 8.0 * (((double)D.nb + 1.0) * D.ngrid * D.nc * D.nc + 3.0 * D.ngrid * D.nc); }
};
}  // namespace fasp_str
