// ilu.hip.h -- application of an incomplete LU factor on the device (PreCSR.c:198 / :263 / :317, ItrSmootherCSR.c:1280),
// the residency of factors built by fasp_ilu_dcsr_setup (csrc/ilu_setup.cpp), fasp_ilu_data_free (PreDataInit.c:445) and the
// solver entry points around them (SolCSR.c:588 / :668).  Part of the single translation unit solver.hip (included inside its
// extern "C" block; the kernels and the C++ helpers sit in an extern "C++" block).
//
// The factor (MSR: ijlu / luval, see ilu_setup.cpp) is two triangular operators:
//   L: row i's entries in storage order up to the first one with column >= i; y_i = r_i - l_i1 y_c1 - l_i2 y_c2 - ...
//   U: row i's entries from the END of the row back to the first one with column <= i; z_i = (y_i - u_i1 z_c1 - ...) * luval[i]
// exactly the reference's loops: one product subtracted at a time in that order, the stored inverse pivot as a multiplier, no
// fused multiply-add (the build has -ffp-contract=off and nothing here asks for one), so z is bit for bit the reference's.
//
// Schedule (host, at upload): level(i) = 1 + the largest level of the rows i reads (0: reads none).  The rows of a level are
// independent; each level is cut into chunks of 64 rows (one wavefront, one row per lane, the sum chain of a row in its own
// lane), the last chunk of a level padded.  A chunk's entries are an ELL slab: entry k of its 64 rows at [base + 64 k, +64), so
// the lanes of a wavefront read consecutive addresses while every row is still summed in its own order.  Two forms:
//   level launches   one launch per level (k_ilu_level); the kernel boundary hands the level on.  The fallback, and the form
//                    the tests compare against.
//   single launch    (k_ilu_flow) every wavefront draws chunks in level order from a ticket counter; the output vector is
//                    filled with a sentinel (all bits set) first and each value is published by one 8-byte agent-scope store
//                    (the data is the flag: cdna_hip_programming.md Guideline 16, R2), read by agent-scope loads that spin
//                    while they see the sentinel.  A chunk only waits for rows of lower levels, which hold lower tickets,
//                    drawn by wavefronts that are running: no residency assumption.  Spins are bounded (flow_give_up: 2 s,
//                    then the error word, the solve fails loudly and later solves use level launches).  Known limit: a value
//                    whose bits are all set (a NaN with that payload, in the right-hand side or computed) is the sentinel
//                    itself, so a reader of it waits until flow_give_up; the default quiet NaN and infinities are not.
// The form follows the schedule's depth (single launch beyond ILU_FLOW_MIN_LEVELS levels); fasp_hip_tune("ilu_form", 0 / 1)
// forces one.  ILU(0) of P7(n) has 3 n - 2 levels per triangle: 766 at 256^3.
//
// Block factors (fasp_ilu_dbsr_setup, PreBSR.c:347) run through the same schedule with NB x NB blocks per entry (the kernels
// are templated on NB, NB = 1 being the scalar factor): see ilu_chunk for the slab layout and the order of operations.
//
// The smoother of the block AMG cycle (bsr_ilu_smooth, ItrSmootherBSR.c:1479: x = x + (LU)^-1 (b - A x)) runs on a factor the
// hierarchy owns and ends its U solve with the EPI form of the kernels: the lane that finishes z_row also writes
// x_row = x_row + z_row (0.0 + z_row from a zero guess), which saves the separate axpy pass and its read of z.

#ifndef ILU_FLOW_MIN_LEVELS
#define ILU_FLOW_MIN_LEVELS 24
#endif

extern "C++" {

struct IluArgs {
    const int*       rows;    // [nchunk * 64] row of each slot, -1: padding
    const int*       len;     // [nchunk * 64] entries of the slot's row
    const long long* cbase;   // [nchunk] first slab entry of the chunk
    const int*       cols;    // slab: column of entry k of slot s at cbase[c] + 64 k + lane
    const double*    vals;
    const double*    diag;    // U: luval[row] per slot; L: nullptr
    const double*    in;      // right-hand side (indexed by row)
    double*          out;     // solution (indexed by row)
    unsigned*        sync;    // single launch: [0] ticket, [1] error word, [6..7] host-mapped error word (flow_give_up)
    int              nchunk;
    double*          x;       // EPI kernels only: the iterate, x_row = x_row + out_row written with out_row
    int              x_zero;  // ... from a zero guess: x_row = 0.0 + out_row, x is not read
};

// one row of an NB x NB block times NB values, the row's elements 64 doubles apart (one slab plane each), summed left to
// right as fasp_blas_smat_mxv does; NB = 6 has no unrolled form there and starts from 0.0 (its default branch)
template <int NB>
__device__ __forceinline__ double ilu_block_row(const double* a, const double* x)
{
    double m = NB == 6 ? 0.0 + a[0] * x[0] : a[0] * x[0];
#pragma unroll
    for (int q = 1; q < NB; ++q) m = m + a[64 * q] * x[q];
    return m;
}

// One chunk of 64 (block) rows, one row per lane.  NB = 1: the scalar factor.  NB > 1: entry k of the chunk's rows is
// an NB x NB block whose element (p, q) lies at vals[(cbase + 64 k) NB^2 + (p NB + q) 64 + lane] (NB^2 planes, each one
// coalesced wavefront load); U's inverse diagonal blocks lie in NB^2 planes of 64 per chunk the same way.  Per entry the
// lane forms mult_p = (L_ij x_j)_p and subtracts it, acc_p = acc_p - mult_p (PreBSR.c:347); U ends with z = D^-1 acc.
// EPI (the last stage of the smoother, U only): the finished value is also added to the iterate, x = x + z -- a plain store:
// nobody waits for x; out still gets z (the single launch publishes it to the rows that spin on it).
template <int NB, bool HAS_D, bool SPIN, bool EPI = false>
__device__ __forceinline__ void ilu_chunk(const IluArgs& a, int c, int lane)
{
    typedef __attribute__((address_space(1))) unsigned long long gu64;
    constexpr int NB2 = NB * NB;
    const int s = c * 64 + lane;
    const int row = a.rows[s];
    if (row < 0) return;
    const int len = a.len[s];
    const long long e0 = a.cbase[c] + lane;
    const double* v = a.vals + a.cbase[c] * NB2 + lane;
    double acc[NB];
#pragma unroll
    for (int p = 0; p < NB; ++p) acc[p] = a.in[(long long)row * NB + p];
    unsigned spins = 0;
    unsigned long long t0 = 0;
    for (int k = 0; k < len; ++k) {
        const long long col = a.cols[e0 + 64ll * k];
        double x[NB];
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            if (SPIN) {   // each component is its own flag
                gu64* src = (gu64*)(a.out + col * NB + q);
                unsigned long long bits = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                while (bits == ~0ull) {
                    if (flow_give_up(a.sync, spins, t0)) break;
                    __builtin_amdgcn_s_sleep(1);
                    bits = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                x[q] = __longlong_as_double((long long)bits);
            } else {
                x[q] = a.out[col * NB + q];
            }
        }
        const double* vk = v + 64ll * NB2 * k;
#pragma unroll
        for (int p = 0; p < NB; ++p) acc[p] = acc[p] - ilu_block_row<NB>(vk + 64 * NB * p, x);
    }
    if (HAS_D) {
        const double* dk = a.diag + (long long)c * NB2 * 64 + lane;
        double z[NB];
#pragma unroll
        for (int p = 0; p < NB; ++p) z[p] = NB == 1 ? acc[0] * dk[0] : ilu_block_row<NB>(dk + 64 * NB * p, acc);
#pragma unroll
        for (int p = 0; p < NB; ++p) acc[p] = z[p];
    }
#pragma unroll
    for (int p = 0; p < NB; ++p) {
        double* dst = a.out + (long long)row * NB + p;
        if (SPIN) __hip_atomic_store((gu64*)dst, (unsigned long long)__double_as_longlong(acc[p]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else *dst = acc[p];
    }
    if (EPI) {
        double* xr = a.x + (long long)row * NB;
#pragma unroll
        for (int p = 0; p < NB; ++p) xr[p] = (a.x_zero ? 0.0 : xr[p]) + acc[p];   // 0.0 + (-0.0) = +0.0, as the reference's sum gives
    }
}

// one level: chunks [c0, c1), four wavefronts per workgroup, one chunk each
template <int NB, bool HAS_D, bool EPI = false>
__global__ __launch_bounds__(256) void k_ilu_level(IluArgs a, int c0, int c1)
{
    const int c = c0 + (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (c < c1) ilu_chunk<NB, HAS_D, false, EPI>(a, c, (int)(threadIdx.x & 63));
}

// all levels in one launch: wavefronts draw chunks in level order
template <int NB, bool HAS_D, bool EPI = false>
__global__ __launch_bounds__(256) void k_ilu_flow(IluArgs a)
{
    typedef __attribute__((address_space(1))) unsigned gu32;
    const int lane = (int)(threadIdx.x & 63);
    for (;;) {
        int c = 0;
        if (lane == 0) c = (int)__hip_atomic_fetch_add((gu32*)a.sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        c = __shfl(c, 0);
        if (c >= a.nchunk) break;
        ilu_chunk<NB, HAS_D, true, EPI>(a, c, lane);
    }
}

namespace {

// one triangle on the device
struct IluTri {
    int nlev = 0, nchunk = 0, maxlen = 0;
    long long nent = 0, nreal = 0;   // slab entries (padded) / actual entries
    std::vector<int> lvl_chunk;      // host: first chunk of each level, nlev + 1
    int *rows = nullptr, *len = nullptr, *cols = nullptr;
    long long* cbase = nullptr;
    double *vals = nullptr, *diag = nullptr;
};
struct IluDev {
    int      n = 0, nb = 1;   // (block) rows, block size (1: a scalar factor, or a block factor with nb = 1)
    IluTri   L, U;
    double  *y = nullptr, *r = nullptr, *z = nullptr;
    unsigned* sync = nullptr;
    std::vector<void*> owned;
};

void ilu_dev_destroy(IluDev* D)
{
    if (!D) return;
    for (void* p : D->owned) (void)hipFree(p);
    delete D;
}

template <class T>
bool ilu_put(IluDev* D, T** dst, const std::vector<T>& src, size_t count)
{
    void* p = nullptr;
    if (hipMalloc(&p, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) return false;
    D->owned.push_back(p);
    *dst = static_cast<T*>(p);
    if (!src.empty()) return hipMemcpy(p, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice) == hipSuccess;
    return true;
}

// the entries of row i that one triangle reads, in the order they are subtracted
void ilu_row_entries(const ILU_data* d, int i, bool upper, std::vector<int>& pos)
{
    pos.clear();
    const int n = d->row;
    const int b = d->ijlu[i], e = d->ijlu[i + 1];
    if (!upper) {
        if (i == 0) return;   // the reference starts the forward sweep at row 1
        for (int p = b; p < e && d->ijlu[p] < i; ++p) pos.push_back(p);
    } else {
        if (i == n - 1) return;   // ... and the backward sweep at row n - 2
        for (int p = e - 1; p >= b && d->ijlu[p] > i; --p) pos.push_back(p);
    }
}

int ilu_build_tri(IluDev* D, const ILU_data* d, bool upper, IluTri& T)
{
    const int n = d->row, nb2 = D->nb * D->nb;
    std::vector<int> level((size_t)n, 0), pos;
    int nlev = 0;
    for (int t = 0; t < n; ++t) {
        const int i = upper ? n - 1 - t : t;
        ilu_row_entries(d, i, upper, pos);
        int lv = 0;
        for (int p : pos) {
            const int c = d->ijlu[p];
            if (c < 0 || c >= n) return ERROR_DATA_STRUCTURE;
            lv = std::max(lv, level[(size_t)c] + 1);
        }
        level[(size_t)i] = lv;
        nlev = std::max(nlev, lv + 1);
    }
    // rows by level (ascending row index inside a level), cut into chunks of 64
    std::vector<int> cnt((size_t)nlev + 1, 0);
    for (int i = 0; i < n; ++i) ++cnt[(size_t)level[(size_t)i] + 1];
    std::vector<int> first((size_t)nlev + 1, 0);
    for (int l = 0; l < nlev; ++l) first[(size_t)l + 1] = first[(size_t)l] + cnt[(size_t)l + 1];
    std::vector<int> order((size_t)n);
    {
        std::vector<int> at(first.begin(), first.end() - 1);
        for (int i = 0; i < n; ++i) order[(size_t)at[(size_t)level[(size_t)i]]++] = i;
    }
    T.nlev = nlev;
    T.lvl_chunk.assign((size_t)nlev + 1, 0);
    for (int l = 0; l < nlev; ++l) T.lvl_chunk[(size_t)l + 1] = T.lvl_chunk[(size_t)l] + (cnt[(size_t)l + 1] + 63) / 64;
    T.nchunk = T.lvl_chunk[(size_t)nlev];
    const size_t nslot = (size_t)T.nchunk * 64;
    std::vector<int> rows(nslot, -1), len(nslot, 0);
    std::vector<long long> cbase((size_t)T.nchunk, 0);
    std::vector<double> diag(upper ? nslot * nb2 : 0, 0.0);   // NB^2 planes of 64 per chunk
    long long nent = 0;
    T.maxlen = 0; T.nreal = 0;
    for (int l = 0; l < nlev; ++l)
        for (int c = T.lvl_chunk[(size_t)l]; c < T.lvl_chunk[(size_t)l + 1]; ++c) {
            int kmax = 0;
            for (int lane = 0; lane < 64; ++lane) {
                const int q = first[(size_t)l] + (c - T.lvl_chunk[(size_t)l]) * 64 + lane;
                if (q >= first[(size_t)l + 1]) break;
                const int i = order[(size_t)q];
                ilu_row_entries(d, i, upper, pos);
                rows[(size_t)c * 64 + lane] = i;
                len[(size_t)c * 64 + lane] = (int)pos.size();
                if (upper)
                    for (int e = 0; e < nb2; ++e) diag[((size_t)c * nb2 + e) * 64 + lane] = d->luval[(size_t)i * nb2 + e];
                kmax = std::max(kmax, (int)pos.size());
                T.nreal += (long long)pos.size();
            }
            cbase[(size_t)c] = nent;
            nent += 64ll * kmax;
            T.maxlen = std::max(T.maxlen, kmax);
        }
    T.nent = nent;
    std::vector<int> cols((size_t)nent, 0);
    std::vector<double> vals((size_t)nent * nb2, 0.0);   // entry k, element el of a slot: ((cbase + 64 k) nb2 + el) 64 + lane
    for (int c = 0; c < T.nchunk; ++c)
        for (int lane = 0; lane < 64; ++lane) {
            const int i = rows[(size_t)c * 64 + lane];
            if (i < 0) continue;
            ilu_row_entries(d, i, upper, pos);
            for (size_t k = 0; k < pos.size(); ++k) {
                const size_t e = (size_t)cbase[(size_t)c] + 64 * k + (size_t)lane;
                cols[e] = d->ijlu[pos[k]];
                const size_t v0 = ((size_t)cbase[(size_t)c] + 64 * k) * nb2 + (size_t)lane;
                for (int el = 0; el < nb2; ++el) vals[v0 + 64 * (size_t)el] = d->luval[(size_t)pos[k] * nb2 + el];
            }
        }
    if (!ilu_put(D, &T.rows, rows, nslot) || !ilu_put(D, &T.len, len, nslot) || !ilu_put(D, &T.cbase, cbase, cbase.size()) ||
        !ilu_put(D, &T.cols, cols, cols.size()) || !ilu_put(D, &T.vals, vals, vals.size()))
        return ERROR_ALLOC_MEM;
    if (upper && !ilu_put(D, &T.diag, diag, diag.size())) return ERROR_ALLOC_MEM;
    return FASP_SUCCESS;
}

// the device copy of a factor with nb x nb blocks (nullptr: no device, or an inconsistent factor -- *st says which)
IluDev* ilu_upload(const ILU_data* d, int nb, int* st)
{
    *st = FASP_SUCCESS;
    if (ctx_init() < 0) { *st = ERROR_MISC; return nullptr; }
    if (!d || d->row <= 0 || !d->ijlu || !d->luval || nb < 1 || nb > 7) { *st = ERROR_INPUT_PAR; return nullptr; }
    IluDev* D = new IluDev;
    D->n = d->row;
    D->nb = nb;
    const size_t len = (size_t)D->n * nb;
    const std::vector<double> none;
    const std::vector<unsigned> sync0(16, 0u);
    int e = ilu_build_tri(D, d, false, D->L);
    if (e == FASP_SUCCESS) e = ilu_build_tri(D, d, true, D->U);
    if (e == FASP_SUCCESS && (!ilu_put(D, &D->y, none, len) || !ilu_put(D, &D->r, none, len) ||
                              !ilu_put(D, &D->z, none, len) || !ilu_put(D, &D->sync, sync0, sync0.size())))
        e = ERROR_ALLOC_MEM;
    if (e == FASP_SUCCESS) {
        const unsigned long long herr_addr = (unsigned long long)seq_err_device_word();
        if (hipMemcpy(D->sync + 6, &herr_addr, 8, hipMemcpyHostToDevice) != hipSuccess) e = ERROR_MISC;
    }
    if (e != FASP_SUCCESS) { ilu_dev_destroy(D); *st = e; return nullptr; }
    return D;
}

// the form the schedule's depth asks for when nothing forces one
bool ilu_auto_single(const IluTri& T) { return T.nlev > ILU_FLOW_MIN_LEVELS; }

bool ilu_single_launch(const IluTri& T)
{
    if (g_tune.ilu_form == 0 || g_flow_disabled) return false;
    if (g_tune.ilu_form == 1) return true;
    return ilu_auto_single(T);
}

// workgroups (four wavefronts, one chunk each) of the launch of chunks [c0, c1) of one level, and of the single launch
int ilu_level_grid(int c0, int c1) { return (c1 - c0 + 3) / 4; }
int ilu_flow_grid(const IluTri& T) { return std::max(1, std::min((T.nchunk + 3) / 4, 1024)); }

template <int NB>
void ilu_launch(const IluTri& T, bool upper, bool single, const IluArgs& a)
{
    const bool epi = upper && a.x != nullptr;
    if (single) {
        const int grid = ilu_flow_grid(T);
        if (epi) hipLaunchKernelGGL((k_ilu_flow<NB, true, true>), dim3(grid), dim3(256), 0, g_ctx.stream, a);
        else if (upper) hipLaunchKernelGGL((k_ilu_flow<NB, true>), dim3(grid), dim3(256), 0, g_ctx.stream, a);
        else hipLaunchKernelGGL((k_ilu_flow<NB, false>), dim3(grid), dim3(256), 0, g_ctx.stream, a);
        return;
    }
    for (int l = 0; l < T.nlev; ++l) {
        const int c0 = T.lvl_chunk[(size_t)l], c1 = T.lvl_chunk[(size_t)l + 1];
        const dim3 grid((unsigned)ilu_level_grid(c0, c1));
        if (epi) hipLaunchKernelGGL((k_ilu_level<NB, true, true>), grid, dim3(256), 0, g_ctx.stream, a, c0, c1);
        else if (upper) hipLaunchKernelGGL((k_ilu_level<NB, true>), grid, dim3(256), 0, g_ctx.stream, a, c0, c1);
        else hipLaunchKernelGGL((k_ilu_level<NB, false>), grid, dim3(256), 0, g_ctx.stream, a, c0, c1);
    }
}

// out = T^-1 in (in, out: device vectors of n nb, not the same).  x (U only, may be nullptr; not in or out): x = x + out
// written by the same kernels, x = 0.0 + out when x_zero.
int ilu_tri_solve(IluDev* D, const IluTri& T, bool upper, const double* in, double* out, double* x = nullptr, bool x_zero = false)
{
    IluArgs a{};
    a.rows = T.rows; a.len = T.len; a.cbase = T.cbase; a.cols = T.cols; a.vals = T.vals; a.diag = T.diag;
    a.in = in; a.out = out; a.sync = D->sync; a.nchunk = T.nchunk;
    a.x = upper ? x : nullptr; a.x_zero = x_zero ? 1 : 0;
    if (T.nchunk == 0) return FASP_SUCCESS;
    const bool single = ilu_single_launch(T);
    if (single) {
        HIPCK(hipMemsetAsync(out, 0xFF, sizeof(double) * (size_t)D->n * D->nb, g_ctx.stream));   // the sentinel: not yet computed
        HIPCK(hipMemsetAsync(D->sync, 0, 8, g_ctx.stream));                                       // ticket counter + error word
    }
    switch (D->nb) {
        case 1: ilu_launch<1>(T, upper, single, a); break;
        case 2: ilu_launch<2>(T, upper, single, a); break;
        case 3: ilu_launch<3>(T, upper, single, a); break;
        case 4: ilu_launch<4>(T, upper, single, a); break;
        case 5: ilu_launch<5>(T, upper, single, a); break;
        case 6: ilu_launch<6>(T, upper, single, a); break;
        case 7: ilu_launch<7>(T, upper, single, a); break;
        default: return ERROR_INPUT_PAR;
    }
    return hipGetLastError() == hipSuccess ? FASP_SUCCESS : ERROR_MISC;
}

// which: 0 both triangles (fasp_precond_ilu), 1 L only (_forward), 2 U only (_backward).  out: a device vector other than in
// (both triangles go through D->y).
int ilu_apply(IluDev* D, int which, const double* in, double* out)
{
    if (seq_err_pending()) return seq_err_check();
    if (which == 1) return ilu_tri_solve(D, D->L, false, in, out);
    if (which == 2) return ilu_tri_solve(D, D->U, true, in, out);
    const int st = ilu_tri_solve(D, D->L, false, in, D->y);
    return st < 0 ? st : ilu_tri_solve(D, D->U, true, D->y, out);
}

// factors made by fasp_ilu_dcsr_setup / fasp_ilu_dbsr_setup: device copy made at the first application, dropped by
// fasp_ilu_data_free.  block_nb records the kind: 0 a scalar factor, else the block size of a block factor (ILU_data.nb
// alone cannot tell: the scalar setup leaves it as the caller's struct held it).
struct IluEntry { ILU_data* d; IluDev* dev; int block_nb; };
std::vector<IluEntry> g_ilu_registry;

IluEntry* ilu_entry(const ILU_data* d)
{
    for (IluEntry& e : g_ilu_registry)
        if (e.d == d) return &e;
    return nullptr;
}

// the device copy to apply `d` with: resident (a registered factor of the kind the entry point asks for) or made for
// this use (*tmp owns it).  block: applied as a block factor (fasp_precond_dbsr_ilu and its kin), block size from the
// registry's record, else from d->nb.
IluDev* ilu_device_of(ILU_data* d, bool block, std::unique_ptr<IluDev, void (*)(IluDev*)>& tmp, int* st)
{
    *st = FASP_SUCCESS;
    IluEntry* e = ilu_entry(d);
    const bool same_kind = e && (e->block_nb > 0) == block;
    const int nb = !block ? 1 : same_kind ? e->block_nb : (d ? d->nb : 0);
    if (same_kind) {
        if (!e->dev) e->dev = ilu_upload(d, nb, st);
        return e->dev;
    }
    tmp.reset(ilu_upload(d, nb, st));
    return tmp.get();
}

int ilu_which(void (*fct)(double*, double*, void*))
{
    if (fct == fasp_precond_ilu) return 0;
    if (fct == fasp_precond_ilu_forward) return 1;
    if (fct == fasp_precond_ilu_backward) return 2;
    return -1;
}

void ilu_precond_host(const char* fn, int which, bool block, double* r, double* z, void* data)
{
    ILU_data* d = static_cast<ILU_data*>(data);
    if (ctx_init() < 0) die_no_device(fn);
    const int rows = d ? d->row : 0;
    if (!d || d->nwork < 2 * rows) {
        std::printf("### ERROR: Need %d memory, only %d available!\n", 2 * rows, d ? d->nwork : 0);
        std::exit(ERROR_ALLOC_MEM);
    }
    std::unique_ptr<IluDev, void (*)(IluDev*)> tmp(nullptr, ilu_dev_destroy);
    int st;
    IluDev* D = ilu_device_of(d, block, tmp, &st);
    const int m = D ? D->n * D->nb : 0;
    if (D) {
        st = hipMemcpyAsync(D->r, r, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, g_ctx.stream) == hipSuccess ? FASP_SUCCESS : ERROR_MISC;
        if (st >= 0) st = ilu_apply(D, which, D->r, D->z);
        if (hipStreamSynchronize(g_ctx.stream) != hipSuccess) st = ERROR_MISC;
        if (st >= 0) st = seq_err_check();
        if (st >= 0 && hipMemcpy(z, D->z, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost) != hipSuccess) st = ERROR_MISC;
    }
    if (st < 0) {
        std::fprintf(stderr, "### ERROR: %s: device ILU application failed (%d)\n", fn, st);
        std::exit(st);
    }
}

// Krylov plug-in: the preconditioner as a device operation (nullptr: pc is not an ILU preconditioner).  *tmp owns a
// per-solve copy; *st < 0: an ILU preconditioner that cannot be applied here.
IluDev* ilu_of_precond(precond* pc, int n, std::unique_ptr<IluDev, void (*)(IluDev*)>& tmp, int* which, int* st)
{
    *st = FASP_SUCCESS;
    if (!pc || !pc->data || !pc->fct) return nullptr;
    *which = ilu_which(pc->fct);
    if (*which < 0) return nullptr;
    ILU_data* d = static_cast<ILU_data*>(pc->data);
    if (d->row != n) { *st = ERROR_INPUT_PAR; return nullptr; }
    return ilu_device_of(d, false, tmp, st);
}

// the same for the block Krylov plug-in: fasp_precond_dbsr_ilu (*which = 0), n = block rows * nb of the system
IluDev* ilu_of_precond_bsr(precond* pc, int n, std::unique_ptr<IluDev, void (*)(IluDev*)>& tmp, int* which, int* st)
{
    *st = FASP_SUCCESS;
    *which = 0;
    if (!pc || !pc->data || pc->fct != fasp_precond_dbsr_ilu) return nullptr;
    IluDev* D = ilu_device_of(static_cast<ILU_data*>(pc->data), true, tmp, st);
    if (D && D->n * D->nb != n) { *st = ERROR_INPUT_PAR; return nullptr; }
    return D;
}
}  // namespace

namespace fasp {
void ilu_register_host(ILU_data* d, int block_nb)
{
    FASP_ENTRY();
    IluEntry* e = ilu_entry(d);
    if (e) { ilu_dev_destroy(e->dev); e->dev = nullptr; e->block_nb = block_nb; return; }   // set up again: the old device copy is stale
    g_ilu_registry.push_back(IluEntry{d, nullptr, block_nb});
}
}  // namespace fasp

namespace fasp_bsr {
// The ILU step of the block cycle on level `level` (fasp_smoother_dbsr_ilu, ItrSmootherBSR.c:1479) with the factor the
// hierarchy owns: r = b - A x by the level's residual kernel (a zero guess: r = b, no product), y = L^-1 r, then the U solve
// that writes z and x = x + z together.  fasp_hip_tune("ilu_smooth_fused", 0): the three passes it replaces (residual, both
// solves, axpy) -- the same bits, kept for the A/B measurement of tools/perf_bilu.py.
static int bsr_ilu_smooth(fasp_hip_amg_bsr* h, int level)
{
    BsrLevel& Lv = h->L[level];
    IluDev* D = Lv.ilu;
    if (!D || !Lv.replicated) return ERROR_INPUT_PAR;   // a triangular solve couples all rows: whole levels only
    if (seq_err_pending()) return seq_err_check();
    const bool zero = Lv.x_zero;
    const double* rhs = Lv.b;
    if (!zero) { bsr_resid(*Lv.A, Lv.x, Lv.b, D->r); rhs = D->r; }
    int st = ilu_tri_solve(D, D->L, false, rhs, D->y);
    if (st < 0) return st;
    if (g_tune.ilu_smooth_fused) {
        st = ilu_tri_solve(D, D->U, true, D->y, D->z, Lv.x, zero);
    } else {
        st = ilu_tri_solve(D, D->U, true, D->y, D->z);
        if (st >= 0 && zero) HIPCK(hipMemsetAsync(Lv.x, 0, sizeof(double) * Lv.n, g_ctx.stream));
        if (st >= 0) d_axpy(Lv.n, 1.0, D->z, Lv.x);
    }
    Lv.x_zero = false;
    return st;
}
}  // namespace fasp_bsr

}  // extern "C++"

// test entries (fasp_hip_dev.h): the host factor of a level of a block hierarchy, and the schedule of its device copy
int fasp_hip_bsr_amg_get_ilu(const fasp_hip_amg_bsr* h, int level, ILU_data* view)
{
    FASP_ENTRY();
    if (!h || !view || level < 0 || level >= (int)h->H.L.size()) return ERROR_INPUT_PAR;
    const HostLevelBSR& L = h->H.L[level];
    if (!L.LU) return 0;
    *view = L.LU->d;
    return 1;
}

int fasp_hip_bsr_amg_ilu_info(const fasp_hip_amg_bsr* h, int level, double info[6])
{
    FASP_ENTRY();
    if (!h || !info || level < 0 || level >= (int)h->H.L.size()) return ERROR_INPUT_PAR;
    for (int i = 0; i < 6; ++i) info[i] = 0.0;
    const IluDev* D = level < (int)h->L.size() ? h->L[level].ilu : nullptr;
    if (!D) return 0;
    info[0] = D->L.nlev; info[1] = D->U.nlev;
    info[2] = ilu_single_launch(D->L) ? 1 : 0; info[3] = ilu_single_launch(D->U) ? 1 : 0;
    info[4] = D->L.nchunk; info[5] = D->U.nchunk;
    return 1;
}

// measurement entry (fasp_hip_dev.h): microseconds per ILU smoothing step of the cycle on `level`, from a non-zero iterate
// (b_i = sin(0.37 i) + 0.1, x restored to zero afterwards), in the form fasp_hip_tune("ilu_smooth_fused", ..) selects
double fasp_hip_bsr_amg_ilu_smooth_time(fasp_hip_amg_bsr* h, int level, int reps)
{
    FASP_ENTRY();
    if (!h || level < 0 || level >= (int)h->L.size() || !h->L[level].ilu || reps <= 0) return -1.0;
    BsrLevel& Lv = h->L[level];
    std::vector<double> hb((size_t)Lv.n);
    for (size_t i = 0; i < hb.size(); ++i) hb[i] = std::sin(0.37 * (double)i) + 0.1;
    if (hipMemcpy(Lv.b, hb.data(), sizeof(double) * hb.size(), hipMemcpyHostToDevice) != hipSuccess) return -1.0;
    Lv.x_zero = true;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.0;
    if (bsr_ilu_smooth(h, level) < 0) return -1.0;   // warm-up; the timed steps start from its iterate
    (void)hipEventRecord(e0, g_ctx.stream);
    for (int i = 0; i < reps; ++i) (void)bsr_ilu_smooth(h, level);
    (void)hipEventRecord(e1, g_ctx.stream);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipMemsetAsync(Lv.b, 0, sizeof(double) * (size_t)Lv.nv, g_ctx.stream);
    (void)hipMemsetAsync(Lv.x, 0, sizeof(double) * (size_t)Lv.nv, g_ctx.stream);
    (void)hipStreamSynchronize(g_ctx.stream);
    if (seq_err_check() < 0) return -1.0;
    return 1000.0 * ms / reps;
}

void fasp_precond_ilu(double* r, double* z, void* data)
{
    FASP_ENTRY();
    ilu_precond_host(__func__, 0, false, r, z, data);
}
void fasp_precond_ilu_forward(double* r, double* z, void* data)
{
    FASP_ENTRY();
    ilu_precond_host(__func__, 1, false, r, z, data);
}
void fasp_precond_ilu_backward(double* r, double* z, void* data)
{
    FASP_ENTRY();
    ilu_precond_host(__func__, 2, false, r, z, data);
}
// PreBSR.c:347: z = (LU)^-1 r with a block factor (nb = 1: the scalar solves, whose arithmetic is the same)
void fasp_precond_dbsr_ilu(double* r, double* z, void* data)
{
    FASP_ENTRY();
    ilu_precond_host(__func__, 0, true, r, z, data);
}


// PreDataInit.c:445.  ILUtp: the columns of the matrix the factor was made of are numbered back (iperm is 1-based).
void fasp_ilu_data_free(ILU_data* iludata)
{
    FASP_ENTRY();
    if (!iludata) return;
    for (size_t q = 0; q < g_ilu_registry.size(); ++q)
        if (g_ilu_registry[q].d == iludata) {
            ilu_dev_destroy(g_ilu_registry[q].dev);
            g_ilu_registry.erase(g_ilu_registry.begin() + (long)q);
            break;
        }
    std::free(iludata->ijlu); iludata->ijlu = nullptr;
    std::free(iludata->luval); iludata->luval = nullptr;
    std::free(iludata->work); iludata->work = nullptr;
    std::free(iludata->ilevL); iludata->ilevL = nullptr;
    std::free(iludata->jlevL); iludata->jlevL = nullptr;
    std::free(iludata->ilevU); iludata->ilevU = nullptr;
    std::free(iludata->jlevU); iludata->jlevU = nullptr;
    if (iludata->type == ILUtp) {
        if (iludata->A) {
            const int nnz = iludata->A->nnz;
            const int* iperm = iludata->iperm;
            for (int k = 0; k < nnz; ++k) iludata->A->JA[k] = iperm[iludata->A->JA[k]] - 1;
        }
        std::free(iludata->iperm); iludata->iperm = nullptr;
    }
}

// device factors resident now (test entry, fasp_hip_dev.h)
int fasp_hip_ilu_resident_count(void)
{
    FASP_ENTRY();
    int c = 0;
    for (const IluEntry& e : g_ilu_registry) c += e.dev ? 1 : 0;
    return c;
}

// test entry (fasp_hip_dev.h): the schedule of one triangle (which: 1 L, 2 U) of a factor applied with nb x nb blocks, from a
// device copy made and freed here; nothing is launched.  info = {levels, chunks, slab entries, actual entries, longest row,
// single launch by the depth rule (whatever ilu_form forces), workgroups of the level launches summed, of the single launch}
int fasp_hip_ilu_schedule(ILU_data* iludata, int nb, int which, double info[8])
{
    FASP_ENTRY();
    if (!info) return ERROR_INPUT_PAR;
    for (int i = 0; i < 8; ++i) info[i] = 0.0;
    if (which != 1 && which != 2) return ERROR_INPUT_PAR;
    int st;
    std::unique_ptr<IluDev, void (*)(IluDev*)> D(ilu_upload(iludata, nb, &st), ilu_dev_destroy);
    if (!D) return st;
    const IluTri& T = which == 1 ? D->L : D->U;
    long long wgs = 0;
    for (int l = 0; l < T.nlev; ++l) wgs += ilu_level_grid(T.lvl_chunk[(size_t)l], T.lvl_chunk[(size_t)l + 1]);
    info[0] = T.nlev; info[1] = T.nchunk; info[2] = (double)T.nent; info[3] = (double)T.nreal; info[4] = T.maxlen;
    info[5] = ilu_auto_single(T) ? 1 : 0; info[6] = (double)wgs; info[7] = ilu_flow_grid(T);
    return FASP_SUCCESS;
}

// measurement entry (fasp_hip_dev.h): microseconds per solve of one triangle of a factor (which: 1 L, 2 U), the factor kept
// resident as a solve keeps it (a block factor of fasp_ilu_dbsr_setup is applied as one); info (may be NULL, 6 doubles) =
// {levels, single launch (1) or level launches (0), bytes moved per solve, slab entries, actual entries, longest row}
double fasp_hip_ilu_time(ILU_data* iludata, int which, int reps, double* info)
{
    FASP_ENTRY();
    if (!iludata || (which != 1 && which != 2) || reps <= 0) return -1.0;
    std::unique_ptr<IluDev, void (*)(IluDev*)> tmp(nullptr, ilu_dev_destroy);
    int st;
    const IluEntry* e = ilu_entry(iludata);
    IluDev* D = ilu_device_of(iludata, e && e->block_nb > 0, tmp, &st);
    if (!D) return -1.0;
    const IluTri& T = which == 1 ? D->L : D->U;
    const bool upper = which == 2;
    const size_t len = (size_t)D->n * D->nb;
    std::vector<double> h(len);
    for (size_t i = 0; i < len; ++i) h[i] = std::sin(0.37 * (double)i) + 0.1;
    if (hipMemcpy(D->r, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice) != hipSuccess) return -1.0;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.0;
    if (ilu_tri_solve(D, T, upper, D->r, D->z) < 0) return -1.0;   // warm-up
    (void)hipEventRecord(e0, g_ctx.stream);
    for (int i = 0; i < reps; ++i) (void)ilu_tri_solve(D, T, upper, D->r, D->z);
    (void)hipEventRecord(e1, g_ctx.stream);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (seq_err_check() < 0) return -1.0;
    if (info) {
        const bool single = ilu_single_launch(T);
        const double slots = 64.0 * T.nchunk, nb = D->nb, nb2 = nb * nb, vec = (double)D->n * nb;
        // slots: row + length (+ the inverse diagonal block); slab: column + block; the gathered operands; rhs read,
        // result written (+ the sentinel fill of the single launch)
        const double bytes = slots * (8.0 + (upper ? 8.0 * nb2 : 0.0)) + 8.0 * T.nchunk + (4.0 + 8.0 * nb2) * (double)T.nent +
                             8.0 * nb * (double)T.nreal + 16.0 * vec + (single ? 8.0 * vec : 0.0);
        info[0] = T.nlev; info[1] = single ? 1 : 0; info[2] = bytes; info[3] = (double)T.nent; info[4] = (double)T.nreal; info[5] = T.maxlen;
    }
    return 1000.0 * ms / reps;
}

// ItrSmootherCSR.c:1280: x = x + (LU)^-1 (b - A x)
void fasp_smoother_dcsr_ilu(dCSRmat* A, dvector* b, dvector* x, void* data)
{
    FASP_ENTRY();
    ILU_data* d = static_cast<ILU_data*>(data);
    if (ctx_init() < 0) die_no_device(__func__);
    const int m = A->row;
    if (!d || d->nwork < 3 * m) {
        std::printf("### ERROR: ILU needs %d memory, only %d available! [%s]\n", 3 * m, d ? d->nwork : 0, __func__);
        std::exit(ERROR_ALLOC_MEM);
    }
    if (d->row != m || A->col != m || b->row < m || x->row < m) {
        std::fprintf(stderr, "### ERROR: %s: inconsistent arguments\n", __func__);
        std::exit(ERROR_INPUT_PAR);
    }
    std::unique_ptr<IluDev, void (*)(IluDev*)> tmp(nullptr, ilu_dev_destroy);
    int st;
    IluDev* D = ilu_device_of(d, false, tmp, &st);
    TmpCSR dA(A);
    TmpVec db(b->val, (size_t)m), dx(x->val, (size_t)m);
    if (D && (!dA.ok || !db.d || !dx.d)) st = ERROR_ALLOC_MEM;
    if (D && st >= 0) {
        d_resid(dA.D, dx.d, db.d, D->r);          // zr = b - A x
        st = ilu_apply(D, 0, D->r, D->z);
        if (st >= 0) d_axpy(m, 1.0, D->z, dx.d);  // x = x + 1 z
        if (hipStreamSynchronize(g_ctx.stream) != hipSuccess) st = ERROR_MISC;
        if (st >= 0) st = seq_err_check();
        if (st >= 0) dx.get(x->val);
    }
    if (st < 0) {
        std::fprintf(stderr, "### ERROR: %s: device ILU smoother failed (%d)\n", __func__, st);
        std::exit(st);
    }
}

// ItrSmootherBSR.c:1479: x = x + (LU)^-1 (b - A x) with a block factor; the work space check is the reference's (5 m)
void fasp_smoother_dbsr_ilu(dBSRmat* A, dvector* b, dvector* x, void* data)
{
    FASP_ENTRY();
    ILU_data* d = static_cast<ILU_data*>(data);
    if (ctx_init() < 0) die_no_device(__func__);
    const int m = d && A ? A->ROW * d->nb : 0;
    if (!d || d->nwork < 5 * m) {
        std::printf("### ERROR: ILU needs %d memory, only %d available! [%s]\n", 5 * m, d ? d->nwork : 0, __func__);
        std::exit(ERROR_ALLOC_MEM);
    }
    std::unique_ptr<IluDev, void (*)(IluDev*)> tmp(nullptr, ilu_dev_destroy);
    int st;
    IluDev* D = ilu_device_of(d, true, tmp, &st);
    if (D && (D->n != A->ROW || D->nb != A->nb || A->COL != A->ROW || b->row < m || x->row < m)) {
        std::fprintf(stderr, "### ERROR: %s: inconsistent arguments\n", __func__);
        std::exit(ERROR_INPUT_PAR);
    }
    if (D) {
        TmpBSR dA(A);
        TmpVec db(b->val, (size_t)m), dx(x->val, (size_t)m);
        if (!dA.ok || !db.d || !dx.d) st = ERROR_ALLOC_MEM;
        if (st >= 0) {
            bsr_resid(dA, dx.d, db.d, D->r);          // zr = b - A x
            st = ilu_apply(D, 0, D->r, D->z);
            if (st >= 0) d_axpy(m, 1.0, D->z, dx.d);  // x = x + 1 z
            if (hipStreamSynchronize(g_ctx.stream) != hipSuccess) st = ERROR_MISC;
            if (st >= 0) st = seq_err_check();
            if (st >= 0) dx.get(x->val);
        }
    }
    if (st < 0) {
        std::fprintf(stderr, "### ERROR: %s: device ILU smoother failed (%d)\n", __func__, st);
        std::exit(st);
    }
}

// SolCSR.c:588 / :668: ILU setup of A (or of M) + fasp_solver_dcsr_itsolver with fasp_precond_ilu (applied in HBM).  No device:
// ERROR_MISC before any work; a partitioned run: ERROR_INPUT_PAR (one GPU, as the plug-in level).
extern "C++" {
namespace {
int krylov_ilu_common(const char* label, dCSRmat* A, dvector* b, dvector* x, ITS_param* itparam, ILU_param* iluparam, dCSRmat* M)
{
    if (!A || !b || !x || !itparam || !iluparam || !M) return ERROR_INPUT_PAR;
    if (ctx_init() < 0) {
        std::fprintf(stderr, "### ERROR: %s: no usable HIP device and no CPU fallback in libfasp_hip\n", label);
        return ERROR_MISC;
    }
    if (comm_size() > 1) return ERROR_INPUT_PAR;
    const double t0 = wall_seconds();
    ILU_data LU;
    std::memset(&LU, 0, sizeof(LU));
    int status = fasp_ilu_dcsr_setup(M, &LU, iluparam);
    if (status >= 0) status = fasp_mem_iludata_check(&LU);
    if (status >= 0) {
        precond pc{&LU, fasp_precond_ilu};
        status = fasp_solver_dcsr_itsolver(A, b, x, &pc, itparam);
        if (itparam->print_level >= PRINT_MIN)
            std::printf("%s_Krylov method%s costs %.4f seconds.\n",
                        iluparam->ILU_type == ILUt ? "ILUt" : iluparam->ILU_type == ILUtp ? "ILUtp" : "ILUk", M == A ? " totally" : "",
                        wall_seconds() - t0);
    }
    fasp_ilu_data_free(&LU);
    return status;
}
}  // namespace
}  // extern "C++"

int fasp_solver_dcsr_krylov_ilu(dCSRmat* A, dvector* b, dvector* x, ITS_param* itparam, ILU_param* iluparam)
{
    FASP_ENTRY();
    return krylov_ilu_common(__func__, A, b, x, itparam, iluparam, A);
}
int fasp_solver_dcsr_krylov_ilu_M(dCSRmat* A, dvector* b, dvector* x, ITS_param* itparam, ILU_param* iluparam, dCSRmat* M)
{
    FASP_ENTRY();
    return krylov_ilu_common(__func__, A, b, x, itparam, iluparam, M);
}

// SolBSR.c:286: block ILU setup + fasp_solver_dbsr_itsolver with fasp_precond_dbsr_ilu (applied in HBM by the block plug-in).
// No device: ERROR_MISC before any work; a partitioned run: ERROR_INPUT_PAR.
int fasp_solver_dbsr_krylov_ilu(dBSRmat* A, dvector* b, dvector* x, ITS_param* itparam, ILU_param* iluparam)
{
    FASP_ENTRY();
    if (!A || !b || !x || !itparam || !iluparam) return ERROR_INPUT_PAR;
    if (ctx_init() < 0) {
        std::fprintf(stderr, "### ERROR: %s: no usable HIP device and no CPU fallback in libfasp_hip\n", __func__);
        return ERROR_MISC;
    }
    if (comm_size() > 1) return ERROR_INPUT_PAR;
    const double t0 = wall_seconds();
    ILU_data LU;
    std::memset(&LU, 0, sizeof(LU));
    int status = fasp_ilu_dbsr_setup(A, &LU, iluparam);
    if (status >= 0) status = fasp_mem_iludata_check(&LU);
    if (status >= 0) {
        precond pc{&LU, fasp_precond_dbsr_ilu};
        status = fasp_solver_dbsr_itsolver(A, b, x, &pc, itparam);
        if (itparam->print_level > PRINT_NONE)
            std::printf("ILUk_Krylov method totally costs %.4f seconds\n", wall_seconds() - t0);
    }
    fasp_ilu_data_free(&LU);
    return status;
}
