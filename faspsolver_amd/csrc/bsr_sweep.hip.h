// bsr_sweep.hip.h -- the sequential block sweeps of a dBSRmat (Gauss-Seidel / SOR in ascending, descending or a user order:
// ItrSmootherBSR.c:410-1470) over the slab plan of bsr_sweep_plan.h, the resident handle around it (fasp_hip_bsr_smoother_*), the
// reference's entries on top of the handle and the opt-in use inside the block AMG cycle (fasp_hip_tune("bsr_cycle_sweep", 1)).
// Part of the single translation unit solver.hip (included inside its extern "C" block, behind ilu.hip.h; kernels and C++
// helpers sit in an extern "C++" block).
//
// The sweep is out of place: u_old is the caller's iterate and is never written, u_new receives every block row once.  Entry
// (i, j) reads u_new[j] when row j comes before row i in the visiting sequence (bit 31 of the stored column) and u_old[j]
// otherwise, which is what the reference's in-place loop reads.  One lane per block row, the row's entries in storage order in
// that lane -- old and new operands mixed in that order --, so every row is summed as the reference sums it:
//   per entry  s_r = A_r0 x_0 + A_r1 x_1 + ... (left to right), b_tmp_r -= s_r            fasp_blas_smat_ymAx / rhs -= val * u
//   GS         u_i = Dinv_i b_tmp  (fasp_blas_smat_mxv; nb = 1: rhs * diaginv[i])
//   SOR        fasp_blas_smat_aAxpby(w, Dinv_i, b_tmp, 1 - w, u_i)  (nb = 1: (1 - w) u_i + w (rhs * diaginv[i]))
//   identity   u_i = b_tmp  (the ...1 / _order2 entries: A scaled to identity diagonal blocks)
// No fused multiply-add (-ffp-contract=off), so u_new is the reference's result bit for bit.
//
// Layout as the block ILU solves' (ilu_chunk): chunks of 64 rows of one dependency level, a chunk's entry k in nb^2 planes of 64
// values, the inverse diagonal blocks in nb^2 planes per chunk -- every load of a wavefront is contiguous.  Two forms:
//   level launches  k_bsr_sweep_level: chunks [c0, c1) of one level per launch; the kernel boundary hands the level on.
//   single launch   k_bsr_sweep_flow: u_new is filled with the all-ones sentinel, wavefronts draw chunks in level order from a
//                   ticket counter, an operand read as new is an agent-scope relaxed load that spins while it sees the sentinel
//                   (each component its own flag), a finished component is published by one 8-byte agent-scope store.  A chunk
//                   waits only for rows of lower levels, which hold lower tickets drawn by wavefronts that are running: no
//                   residency assumption.  Spins are bounded by flow_give_up (2 s, the error word, seq_err_check: the call fails
//                   loudly, later calls take level launches).
// Form: fasp_hip_tune("bsr_sweep_form", -1 / 0 / 1) = by the plan, level launches, single launch.  The rule of -1 is read off
// profiles/bsr_sweep.txt (tools/perf_bsr_sweep.py): the single launch for plans deeper than BSR_SWEEP_FLOW_MIN_LEVELS levels whose
// levels hold at most BSR_SWEEP_FLOW_MAX_WIDTH chunks on average.  Measured: a hand-over from level to level costs the single launch
// 0.9 - 3.2 us on a chain of one-row levels and 3.6 - 5.2 us at 70 - 94 levels of 4 - 6 chunks (P7(24), P7(32): 1.0 - 1.35 x faster
// than a launch per level, 5.8 - 6.5 us each); with wider levels the waves that wait crowd the memory system -- P7(48), 13 chunks
// per level: 0.88 x; P7(64) and P7(128): 0.3 - 0.9 x -- and below some 50 levels the sentinel fill and the ticket counter are not
// paid back (P7(8) - P7(16) (x) B3: 0.8 x).

#ifndef BSR_SWEEP_FLOW_MIN_LEVELS
#define BSR_SWEEP_FLOW_MIN_LEVELS 64
#endif
#ifndef BSR_SWEEP_FLOW_MAX_WIDTH
#define BSR_SWEEP_FLOW_MAX_WIDTH 8   // chunks of 64 block rows per level, on average
#endif

extern "C++" {

enum { BSR_SW_GS = 0, BSR_SW_SOR = 1, BSR_SW_ID = 2 };

struct BsrSweepArgs {
    const int*       rows;    // [nchunk * 64] block row of each slot, -1: padding
    const int*       len;     // [nchunk * 64] off-diagonal entries of the slot's row
    const long long* cbase;   // [nchunk] first slab entry of the chunk
    const int*       cols;    // slab: column of entry k of a slot at cbase[c] + 64 k + lane, bit 31: reads u_new
    const double*    vals;
    const double*    dinv;    // nb^2 planes of 64 per chunk (GS, SOR)
    const double*    b;
    const double*    u_old;
    double*          u_new;
    unsigned*        sync;    // single launch: [0] ticket, [1] error word, [6..7] host-mapped error word (flow_give_up)
    int              nchunk;
    double           w;       // SOR weight
};

// (A x)_p of one block entry, the block's elements 64 doubles apart (one slab plane each): fasp_blas_smat_ymAx's sum, left to right
template <int NB>
__device__ __forceinline__ void bsr_sweep_prod(const double* vk, const double* x, double* m)
{
#pragma unroll
    for (int p = 0; p < NB; ++p) {
        const double* ap = vk + 64 * NB * p;
        double t = ap[0] * x[0];
#pragma unroll
        for (int q = 1; q < NB; ++q) t = t + ap[64 * q] * x[q];
        m[p] = t;
    }
}

// one operand of the single launch: an agent-scope load that spins while it sees the sentinel (each component is its own flag)
__device__ __forceinline__ double bsr_sweep_wait(const double* p, unsigned* sync, unsigned& spins, unsigned long long& t0)
{
    typedef __attribute__((address_space(1))) unsigned long long gu64;
    gu64* src = (gu64*)p;
    unsigned long long bits = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (bits == ~0ull) {
        if (flow_give_up(sync, spins, t0)) break;
        __builtin_amdgcn_s_sleep(1);
        bits = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return __longlong_as_double((long long)bits);
}

// rows of at most this many off-diagonal entries take the short-row path of the single launch; nb <= 4 only: with the products and
// the inverse block of nb >= 5 held in registers the path measured slower than the plain loop (P7(64) (x) B5: 9.6 against 6.0 ms)
template <int NB> struct BsrSweepShort { static constexpr int value = NB <= 4 ? 8 : 0; };

// One chunk of 64 block rows, one row per lane (layout: bsr_sweep_plan.h).  Per entry the lane forms s = A_ij x_j and subtracts it,
// b_tmp = b_tmp - s, in storage order; then the end of the row of KIND.
// SPIN (single launch), rows of at most BsrSweepShort entries: the products of the entries that read u_old and the inverse block are
// fetched and formed BEFORE the lane waits for its first u_new operand -- a product does not depend on b_tmp, only the subtractions
// are ordered, and they still run in storage order --, so that what follows the arrival of the last operand is one product, the
// subtractions and the end of the row: the chain from level to level carries no load of the matrix.
template <int NB, int KIND, bool SPIN>
__device__ __forceinline__ void bsr_sweep_chunk(const BsrSweepArgs& a, int c, int lane)
{
    typedef __attribute__((address_space(1))) unsigned long long gu64;
    constexpr int NB2 = NB * NB;
    constexpr int LM = BsrSweepShort<NB>::value > 0 ? BsrSweepShort<NB>::value : 1;
    const int s = c * 64 + lane;
    const int row = a.rows[s];
    if (row < 0) return;
    const int len = a.len[s];
    const long long e0 = a.cbase[c] + lane;
    const double* v = a.vals + a.cbase[c] * NB2 + lane;
    const double* dk = a.dinv + (long long)c * NB2 * 64 + lane;
    double bt[NB], dv[KIND == BSR_SW_ID ? 1 : NB2], own[NB];
#pragma unroll
    for (int p = 0; p < NB; ++p) bt[p] = a.b[(long long)row * NB + p];
    unsigned spins = 0;
    unsigned long long t0 = 0;
    const bool short_row = SPIN && BsrSweepShort<NB>::value > 0 && len <= LM;
    if (short_row) {
        int cw[LM];
#pragma unroll
        for (int k = 0; k < LM; ++k) cw[k] = k < len ? a.cols[e0 + 64ll * k] : 0;
        double m[LM][NB];
#pragma unroll
        for (int k = 0; k < LM; ++k) {
#pragma unroll
            for (int p = 0; p < NB; ++p) m[k][p] = 0.0;
            if (k < len && cw[k] >= 0) {
                double x[NB];
#pragma unroll
                for (int q = 0; q < NB; ++q) x[q] = a.u_old[(long long)cw[k] * NB + q];
                bsr_sweep_prod<NB>(v + 64ll * NB2 * k, x, m[k]);
            }
        }
        if (KIND != BSR_SW_ID) {
#pragma unroll
            for (int e = 0; e < NB2; ++e) dv[e] = dk[64 * e];
        }
        if (KIND == BSR_SW_SOR) {
#pragma unroll
            for (int p = 0; p < NB; ++p) own[p] = a.u_old[(long long)row * NB + p];
        }
#pragma unroll
        for (int k = 0; k < LM; ++k) {
            if (k < len) {
                if (cw[k] < 0) {
                    const long long col = cw[k] & 0x7fffffff;
                    double x[NB];
#pragma unroll
                    for (int q = 0; q < NB; ++q) x[q] = bsr_sweep_wait(a.u_new + col * NB + q, a.sync, spins, t0);
                    bsr_sweep_prod<NB>(v + 64ll * NB2 * k, x, m[k]);
                }
#pragma unroll
                for (int p = 0; p < NB; ++p) bt[p] -= m[k][p];
            }
        }
    } else {
        for (int k = 0; k < len; ++k) {
            const int cw = a.cols[e0 + 64ll * k];
            const long long col = cw & 0x7fffffff;
            double x[NB], m[NB];
            if (cw < 0) {
#pragma unroll
                for (int q = 0; q < NB; ++q) x[q] = SPIN ? bsr_sweep_wait(a.u_new + col * NB + q, a.sync, spins, t0) : a.u_new[col * NB + q];
            } else {
#pragma unroll
                for (int q = 0; q < NB; ++q) x[q] = a.u_old[col * NB + q];
            }
            bsr_sweep_prod<NB>(v + 64ll * NB2 * k, x, m);
#pragma unroll
            for (int p = 0; p < NB; ++p) bt[p] -= m[p];
        }
        if (KIND != BSR_SW_ID) {
#pragma unroll
            for (int e = 0; e < NB2; ++e) dv[e] = dk[64 * e];
        }
        if (KIND == BSR_SW_SOR) {
#pragma unroll
            for (int p = 0; p < NB; ++p) own[p] = a.u_old[(long long)row * NB + p];
        }
    }
    double z[NB];
    if (KIND == BSR_SW_ID) {
#pragma unroll
        for (int p = 0; p < NB; ++p) z[p] = bt[p];
    } else if (KIND == BSR_SW_GS) {   // fasp_blas_smat_mxv (nb = 6: its default branch, from 0.0; nb = 1: rhs * diaginv[i])
#pragma unroll
        for (int p = 0; p < NB; ++p) {
            double t = NB == 6 ? 0.0 + dv[NB * p] * bt[0] : dv[NB * p] * bt[0];
#pragma unroll
            for (int q = 1; q < NB; ++q) t = t + dv[NB * p + q] * bt[q];
            z[p] = t;
        }
    } else if (NB == 1) {
        z[0] = (1.0 - a.w) * own[0] + a.w * (bt[0] * dv[0]);   // ItrSmootherBSR.c:1166
    } else {   // fasp_blas_smat_aAxpby(w, Dinv, b_tmp, 1 - w, u), BlaSmallMat.c:1140
        const double w = a.w, omw = 1.0 - w;
        if (w == 0) {
#pragma unroll
            for (int p = 0; p < NB; ++p) z[p] = own[p] * omw;
        } else {
            const double tmp = omw / w;
#pragma unroll
            for (int p = 0; p < NB; ++p) {
                double yr = own[p];
                if (tmp != 1.0) yr *= tmp;
#pragma unroll
                for (int q = 0; q < NB; ++q) yr += dv[NB * p + q] * bt[q];
                if (w != 1.0) yr *= w;
                z[p] = yr;
            }
        }
    }
#pragma unroll
    for (int p = 0; p < NB; ++p) {
        double* dst = a.u_new + (long long)row * NB + p;
        if (SPIN) __hip_atomic_store((gu64*)dst, (unsigned long long)__double_as_longlong(z[p]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else *dst = z[p];
    }
}

// one level: chunks [c0, c1), four wavefronts per workgroup, one chunk each
template <int NB, int KIND>
__global__ __launch_bounds__(256) void k_bsr_sweep_level(BsrSweepArgs a, int c0, int c1)
{
    const int c = c0 + (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (c < c1) bsr_sweep_chunk<NB, KIND, false>(a, c, (int)(threadIdx.x & 63));
}

// all levels in one launch: wavefronts draw chunks in level order
template <int NB, int KIND>
__global__ __launch_bounds__(256) void k_bsr_sweep_flow(BsrSweepArgs a)
{
    typedef __attribute__((address_space(1))) unsigned gu32;
    const int lane = (int)(threadIdx.x & 63);
    for (;;) {
        int c = 0;
        if (lane == 0) c = (int)__hip_atomic_fetch_add((gu32*)a.sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        c = __shfl(c, 0);
        if (c >= a.nchunk) break;
        bsr_sweep_chunk<NB, KIND, true>(a, c, lane);
    }
}

namespace {

// the device copy of a plan
struct BsrSweepDev {
    int ROW = 0, nb = 0, nlev = 0, nchunk = 0, maxlen = 0;
    long long nent = 0, nreal = 0;
    std::vector<int> lvl_chunk;
    int *rows = nullptr, *len = nullptr, *cols = nullptr;
    long long* cbase = nullptr;
    double *vals = nullptr, *dinv = nullptr;
    unsigned* sync = nullptr;
    std::vector<void*> owned;
};

void bsr_sweep_dev_destroy(BsrSweepDev* D)
{
    if (!D) return;
    for (void* p : D->owned) (void)hipFree(p);
    delete D;
}

template <class T>
bool bsr_sweep_put(BsrSweepDev* D, T** dst, const std::vector<T>& src)
{
    void* p = nullptr;
    if (hipMalloc(&p, sizeof(T) * std::max<size_t>(src.size(), 1)) != hipSuccess) return false;
    D->owned.push_back(p);
    *dst = static_cast<T*>(p);
    if (!src.empty()) return hipMemcpy(p, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice) == hipSuccess;
    return true;
}

// plan of (A, seq) built on the host and uploaded; diaginv == NULL: a plan for the identity kind only
BsrSweepDev* bsr_sweep_upload(const dBSRmat* A, const std::vector<int>& seq, const double* diaginv, int* st)
{
    fasp::BsrSweepPlan P;
    *st = fasp::bsr_sweep_plan_build(A, seq, true, diaginv, P);
    if (*st < 0) return nullptr;
    if (ctx_init() < 0) { *st = ERROR_MISC; return nullptr; }
    BsrSweepDev* D = new BsrSweepDev;
    D->ROW = P.ROW; D->nb = P.nb; D->nlev = P.nlev; D->nchunk = P.nchunk; D->maxlen = P.maxlen; D->nent = P.nent; D->nreal = P.nreal;
    D->lvl_chunk = P.lvl_chunk;
    const std::vector<unsigned> sync0(16, 0u);
    bool ok = bsr_sweep_put(D, &D->rows, P.rows) && bsr_sweep_put(D, &D->len, P.len) && bsr_sweep_put(D, &D->cbase, P.cbase) &&
              bsr_sweep_put(D, &D->cols, P.cols) && bsr_sweep_put(D, &D->vals, P.vals) && bsr_sweep_put(D, &D->sync, sync0);
    if (ok && diaginv) ok = bsr_sweep_put(D, &D->dinv, P.dinv);
    if (!ok) { bsr_sweep_dev_destroy(D); *st = ERROR_ALLOC_MEM; return nullptr; }
    const unsigned long long herr_addr = (unsigned long long)seq_err_device_word();
    if (hipMemcpy(D->sync + 6, &herr_addr, 8, hipMemcpyHostToDevice) != hipSuccess) { bsr_sweep_dev_destroy(D); *st = ERROR_MISC; return nullptr; }
    return D;
}

bool bsr_sweep_single(const BsrSweepDev& D)
{
    if (g_tune.bsr_sweep_form == 0 || g_flow_disabled) return false;
    if (g_tune.bsr_sweep_form == 1) return true;
    return D.nlev > BSR_SWEEP_FLOW_MIN_LEVELS && (long long)D.nchunk <= (long long)BSR_SWEEP_FLOW_MAX_WIDTH * D.nlev;
}

template <int NB, int KIND>
void bsr_sweep_launch(const BsrSweepDev& D, bool single, const BsrSweepArgs& a)
{
    if (single) {
        const int grid = std::max(1, std::min((D.nchunk + 3) / 4, 1024));
        hipLaunchKernelGGL((k_bsr_sweep_flow<NB, KIND>), dim3(grid), dim3(256), 0, g_ctx.stream, a);
        return;
    }
    for (int l = 0; l < D.nlev; ++l) {
        const int c0 = D.lvl_chunk[(size_t)l], c1 = D.lvl_chunk[(size_t)l + 1];
        hipLaunchKernelGGL((k_bsr_sweep_level<NB, KIND>), dim3((unsigned)((c1 - c0 + 3) / 4)), dim3(256), 0, g_ctx.stream, a, c0, c1);
    }
}

template <int NB>
void bsr_sweep_launch_kind(const BsrSweepDev& D, int kind, bool single, const BsrSweepArgs& a)
{
    if (kind == BSR_SW_GS) bsr_sweep_launch<NB, BSR_SW_GS>(D, single, a);
    else if (kind == BSR_SW_SOR) bsr_sweep_launch<NB, BSR_SW_SOR>(D, single, a);
    else bsr_sweep_launch<NB, BSR_SW_ID>(D, single, a);
}

// One sweep: u_new = sweep(b, u_old); device vectors of ROW nb, u_old and u_new distinct.  *single_out (may be NULL): the form taken.
int bsr_sweep_run(BsrSweepDev* D, int kind, double w, const double* b, const double* u_old, double* u_new, int* single_out = nullptr)
{
    if (!D || kind < BSR_SW_GS || kind > BSR_SW_ID || (kind != BSR_SW_ID && !D->dinv) || u_old == u_new) return ERROR_INPUT_PAR;
    if (seq_err_pending()) return seq_err_check();
    const bool single = bsr_sweep_single(*D);
    if (single_out) *single_out = single ? 1 : 0;
    if (D->nchunk == 0) return FASP_SUCCESS;
    BsrSweepArgs a{};
    a.rows = D->rows; a.len = D->len; a.cbase = D->cbase; a.cols = D->cols; a.vals = D->vals; a.dinv = D->dinv;
    a.b = b; a.u_old = u_old; a.u_new = u_new; a.sync = D->sync; a.nchunk = D->nchunk; a.w = w;
    if (single) {
        HIPCK(hipMemsetAsync(u_new, 0xFF, sizeof(double) * (size_t)D->ROW * D->nb, g_ctx.stream));   // the sentinel: not yet computed
        HIPCK(hipMemsetAsync(D->sync, 0, 8, g_ctx.stream));                                           // ticket counter + error word
    }
    switch (D->nb) {
        case 1: bsr_sweep_launch_kind<1>(*D, kind, single, a); break;
        case 2: bsr_sweep_launch_kind<2>(*D, kind, single, a); break;
        case 3: bsr_sweep_launch_kind<3>(*D, kind, single, a); break;
        case 4: bsr_sweep_launch_kind<4>(*D, kind, single, a); break;
        case 5: bsr_sweep_launch_kind<5>(*D, kind, single, a); break;
        case 6: bsr_sweep_launch_kind<6>(*D, kind, single, a); break;
        case 7: bsr_sweep_launch_kind<7>(*D, kind, single, a); break;
        default: return ERROR_NUM_BLOCKS;
    }
    return hipGetLastError() == hipSuccess ? FASP_SUCCESS : ERROR_MISC;
}

// bytes one sweep moves at least: slots (row, length, inverse block), chunk bases, slab (column + block), gathered operands,
// b read, the row's own u_old (SOR), u_new written (+ the sentinel fill of the single launch)
double bsr_sweep_bytes(const BsrSweepDev& D, int kind, bool single)
{
    const double slots = 64.0 * D.nchunk, nb = D.nb, nb2 = nb * nb, vec = (double)D.ROW * nb;
    return slots * (8.0 + (kind != BSR_SW_ID ? 8.0 * nb2 : 0.0)) + 8.0 * D.nchunk + (4.0 + 8.0 * nb2) * (double)D.nent +
           8.0 * nb * (double)D.nreal + 16.0 * vec + (kind == BSR_SW_SOR ? 8.0 * vec : 0.0) + (single ? 8.0 * vec : 0.0);
}

}  // namespace
}  // extern "C++"

// ---------------------------------------------------------------------------
// the resident handle (fasp_hip.h)
// ---------------------------------------------------------------------------
struct fasp_hip_bsr_smoother {
    BsrSweepDev* D = nullptr;      // nullptr: nothing is swept (mark == NULL, order neither ASCEND nor DESCEND)
    int     ROW = 0, nb = 0;
    double *b = nullptr, *u0 = nullptr, *u1 = nullptr;
    int     last_form = -1;        // form of the last apply: 0 level launches, 1 single launch
    double  plan_ms = 0.0;         // host plan + upload
};

extern "C++" {
namespace {
// create with the checks of the public entry; need_dinv false: a handle for the identity kind only (no inverse blocks)
int bsr_smoother_create(fasp_hip_bsr_smoother** out, const dBSRmat* A, const double* diaginv, bool need_dinv, int order, const int* mark)
{
    if (!out) return ERROR_INPUT_PAR;
    *out = nullptr;
    if (!A) return ERROR_INPUT_PAR;
    if (A->nb < 1 || A->nb > 7) return ERROR_NUM_BLOCKS;
    if (A->ROW < 0 || A->ROW != A->COL || A->NNZ < 0 || A->storage_manner != 0 || !A->IA || (A->NNZ > 0 && (!A->JA || !A->val)))
        return ERROR_INPUT_PAR;
    std::vector<int> seq;
    const int sq = fasp::bsr_sweep_sequence(A->ROW, order, mark, seq);
    if (sq < 0) return sq;
    std::unique_ptr<fasp_hip_bsr_smoother> h(new fasp_hip_bsr_smoother);
    h->ROW = A->ROW; h->nb = A->nb;
    if (sq == 1) { *out = h.release(); return FASP_SUCCESS; }
    const double t0 = fasp::wall_seconds();
    std::vector<double> own;
    if (need_dinv && !diaginv) {
        own.resize((size_t)std::max(A->ROW, 1) * A->nb * A->nb);
        (void)fasp::bsr_diaginv(A, own.data());
        diaginv = own.data();
    }
    int st;
    h->D = bsr_sweep_upload(A, seq, need_dinv ? diaginv : nullptr, &st);
    if (!h->D) return st;
    const size_t n = (size_t)A->ROW * A->nb;
    double** v[] = {&h->b, &h->u0, &h->u1};
    for (double** q : v)
        if (hipMalloc(q, sizeof(double) * std::max<size_t>(n, 1)) != hipSuccess) {
            *q = nullptr;
            fasp_hip_bsr_smoother_destroy(h.release());
            return ERROR_ALLOC_MEM;
        }
    h->plan_ms = 1000.0 * (fasp::wall_seconds() - t0);
    *out = h.release();
    return FASP_SUCCESS;
}

// one sweep of the resident vectors: u0 -> u1, then the two change places
int bsr_smoother_sweep_resident(fasp_hip_bsr_smoother* h, int kind, double w)
{
    int single = 0;
    const int st = bsr_sweep_run(h->D, kind, w, h->b, h->u0, h->u1, &single);
    if (st < 0) return st;
    h->last_form = single;
    std::swap(h->u0, h->u1);
    return FASP_SUCCESS;
}
}  // namespace
}  // extern "C++"

int fasp_hip_bsr_smoother_create(fasp_hip_bsr_smoother** h, const dBSRmat* A, const double* diaginv, int order, const int* mark)
{
    FASP_ENTRY();
    return bsr_smoother_create(h, A, diaginv, true, order, mark);
}

void fasp_hip_bsr_smoother_destroy(fasp_hip_bsr_smoother* h)
{
    FASP_ENTRY();
    if (!h) return;
    if (g_ctx.ready) (void)hipStreamSynchronize(g_ctx.stream);
    bsr_sweep_dev_destroy(h->D);
    double* v[] = {h->b, h->u0, h->u1};
    for (double* q : v) if (q) (void)hipFree(q);
    delete h;
}

int fasp_hip_bsr_smoother_apply(fasp_hip_bsr_smoother* h, int kind, double weight, const dvector* b, dvector* u)
{
    FASP_ENTRY();
    if (!h || !b || !u || kind < BSR_SW_GS || kind > BSR_SW_ID) return ERROR_INPUT_PAR;
    const int n = h->ROW * h->nb;
    if (b->row < n || u->row < n || (n > 0 && (!b->val || !u->val))) return ERROR_INPUT_PAR;
    if (!h->D || n == 0) return FASP_SUCCESS;   // nothing is swept
    if (kind != BSR_SW_ID && !h->D->dinv) return ERROR_INPUT_PAR;
    const size_t bytes = sizeof(double) * (size_t)n;
    if (hipMemcpyAsync(h->b, b->val, bytes, hipMemcpyHostToDevice, g_ctx.stream) != hipSuccess ||
        hipMemcpyAsync(h->u0, u->val, bytes, hipMemcpyHostToDevice, g_ctx.stream) != hipSuccess)
        return ERROR_MISC;
    int st = bsr_smoother_sweep_resident(h, kind, weight);
    if (hipStreamSynchronize(g_ctx.stream) != hipSuccess) st = ERROR_MISC;
    if (st >= 0) st = seq_err_check();
    if (st >= 0 && hipMemcpy(u->val, h->u0, bytes, hipMemcpyDeviceToHost) != hipSuccess) st = ERROR_MISC;
    return st;
}

// measurement and test entries (fasp_hip_dev.h)
int fasp_hip_bsr_smoother_info(const fasp_hip_bsr_smoother* h, double info[6])
{
    FASP_ENTRY();
    if (!h || !info) return ERROR_INPUT_PAR;
    for (int i = 0; i < 6; ++i) info[i] = 0.0;
    info[4] = h->last_form;
    if (!h->D) return 0;
    info[0] = h->D->nlev; info[1] = h->D->nchunk; info[2] = (double)h->D->nent; info[3] = (double)(h->D->nent - h->D->nreal);
    info[5] = bsr_sweep_single(*h->D) ? 1 : 0;
    return 1;
}

int fasp_hip_bsr_sweep_plan(const dBSRmat* A, int order, const int* mark, long long info[6], int* level, int* lvl_chunk, int* rows,
                            int* len, long long* cbase, int* cols)
{
    if (!A || !info) return ERROR_INPUT_PAR;
    if (A->nb < 1 || A->nb > 7) return ERROR_NUM_BLOCKS;
    std::vector<int> seq;
    const int sq = fasp::bsr_sweep_sequence(A->ROW, order, mark, seq);
    if (sq < 0) return sq;
    for (int i = 0; i < 6; ++i) info[i] = 0;
    if (sq == 1) return 1;
    fasp::BsrSweepPlan P;
    const int st = fasp::bsr_sweep_plan_build(A, seq, false, nullptr, P);
    if (st < 0) return st;
    info[0] = P.nlev; info[1] = P.nchunk; info[2] = P.nent; info[3] = P.nreal; info[4] = P.maxlen; info[5] = P.ROW;
    if (level) std::copy(P.level.begin(), P.level.end(), level);
    if (lvl_chunk) std::copy(P.lvl_chunk.begin(), P.lvl_chunk.end(), lvl_chunk);
    if (rows) std::copy(P.rows.begin(), P.rows.end(), rows);
    if (len) std::copy(P.len.begin(), P.len.end(), len);
    if (cbase) std::copy(P.cbase.begin(), P.cbase.end(), cbase);
    if (cols) std::copy(P.cols.begin(), P.cols.end(), cols);
    return FASP_SUCCESS;
}

double fasp_hip_bsr_sweep_time(const dBSRmat* A, int order, const int* mark, int kind, double weight, int form, int reps, double* info)
{
    FASP_ENTRY();
    if (!A || reps <= 0 || form < -1 || form > 2 || kind < BSR_SW_GS || kind > BSR_SW_ID) return -1.0;
    if (form == 0 && (mark || (order != ASCEND && order != DESCEND) || kind == BSR_SW_ID)) return -1.0;   // k_bsr_seq_level: ascending / descending GS and SOR only
    const size_t n = (size_t)A->ROW * A->nb;
    std::vector<double> hb(n), dinv(std::max<size_t>(n * A->nb, 1));
    for (size_t i = 0; i < n; ++i) hb[i] = std::sin(0.37 * (double)i) + 0.1;
    if (A->nb < 1 || A->nb > 7 || fasp::bsr_diaginv(A, dinv.data()) < 0) return -1.0;
    hipEvent_t e0, e1;
    float ms = 0.f;
    if (form == 0) {   // the per-level launches of the cycle's default sweeps, in place
        TmpBSR M(A);
        if (!M.ok) return -1.0;
        TmpVec du(hb.data(), n), db(hb.data(), n), dd(dinv.data(), n * A->nb);
        if (!du.d || !db.d || !dd.d) return -1.0;
        DevLevel::Sched S;
        const double t0 = fasp::wall_seconds();
        if (bsr_seq_schedule(A->ROW, A->COL, A->NNZ, A->IA, A->JA, order == DESCEND, S) < 0) return -1.0;
        const double plan_ms = 1000.0 * (fasp::wall_seconds() - t0);
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { S.release(); return -1.0; }
        (void)bsr_seq_launch(M, S, db.d, dd.d, du.d, kind == BSR_SW_SOR, weight);   // warm-up
        (void)hipEventRecord(e0, g_ctx.stream);
        for (int i = 0; i < reps; ++i) (void)bsr_seq_launch(M, S, db.d, dd.d, du.d, kind == BSR_SW_SOR, weight);
        (void)hipEventRecord(e1, g_ctx.stream);
        (void)hipEventSynchronize(e1);
        (void)hipEventElapsedTime(&ms, e0, e1);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        if (info) {
            const double nb = A->nb, nb2 = nb * nb;
            info[0] = (double)S.ptr.size() - 1; info[1] = 0; info[2] = A->NNZ; info[3] = A->NNZ; info[4] = 0;
            info[5] = 4.0 * A->ROW + 8.0 * A->ROW + (4.0 + 8.0 * nb2 + 8.0 * nb) * (double)A->NNZ + 8.0 * nb2 * A->ROW + 24.0 * (double)n;
            info[6] = plan_ms; info[7] = 0;
        }
        S.release();
        return 1000.0 * ms / reps;
    }
    fasp_hip_bsr_smoother* h = nullptr;
    if (bsr_smoother_create(&h, A, dinv.data(), true, order, mark) < 0 || !h) return -1.0;
    if (!h->D) { fasp_hip_bsr_smoother_destroy(h); return -1.0; }
    const int saved = g_tune.bsr_sweep_form;
    if (form > 0) g_tune.bsr_sweep_form = form - 1;
    double us = -1.0;
    if (hipMemcpy(h->b, hb.data(), sizeof(double) * n, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(h->u0, hb.data(), sizeof(double) * n, hipMemcpyHostToDevice) == hipSuccess &&
        hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
        int st = bsr_smoother_sweep_resident(h, kind, weight);   // warm-up
        (void)hipEventRecord(e0, g_ctx.stream);
        for (int i = 0; i < reps && st >= 0; ++i) st = bsr_smoother_sweep_resident(h, kind, weight);
        (void)hipEventRecord(e1, g_ctx.stream);
        (void)hipEventSynchronize(e1);
        (void)hipEventElapsedTime(&ms, e0, e1);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        if (st >= 0 && seq_err_check() >= 0) us = 1000.0 * ms / reps;
        if (info) {
            info[0] = h->D->nlev; info[1] = h->D->nchunk; info[2] = (double)h->D->nent; info[3] = (double)h->D->nreal;
            info[4] = 1 + h->last_form; info[5] = bsr_sweep_bytes(*h->D, kind, h->last_form == 1); info[6] = h->plan_ms; info[7] = h->D->maxlen;
        }
    }
    g_tune.bsr_sweep_form = saved;
    fasp_hip_bsr_smoother_destroy(h);
    return us;
}

// ---------------------------------------------------------------------------
// the reference's entries (ItrSmootherBSR.c): host vectors, each one create + apply + destroy of the handle
// ---------------------------------------------------------------------------
extern "C++" {
namespace {
void bsr_smoother_oneshot(const char* fn, dBSRmat* A, dvector* b, dvector* u, int order, int* mark, const double* diaginv, bool own_dinv,
                          int kind, double w)
{
    if (!A || !b || !u || (kind != BSR_SW_ID && !own_dinv && !diaginv)) {
        std::fprintf(stderr, "### ERROR: %s: inconsistent arguments\n", fn);
        std::exit(ERROR_INPUT_PAR);
    }
    if (A->nb < 1 || A->nb > 7) {
        std::fprintf(stderr, "### ERROR: %s: nb = %d is illegal (1 .. 7)\n", fn, A->nb);
        std::exit(ERROR_NUM_BLOCKS);
    }
    if (!mark && order != ASCEND && order != DESCEND) return;   // as the reference: nothing is swept
    fasp_hip_bsr_smoother* h = nullptr;
    int st = ERROR_INPUT_PAR;
    const long long n = (long long)A->ROW * A->nb;
    if (A->ROW == A->COL && b->row >= n && u->row >= n) st = bsr_smoother_create(&h, A, diaginv, kind != BSR_SW_ID, order, mark);
    if (st == ERROR_MISC) die_no_device(fn);
    if (st == ERROR_INPUT_PAR || st == ERROR_DATA_STRUCTURE) {
        std::fprintf(stderr, "### ERROR: %s: inconsistent arguments\n", fn);
        std::exit(ERROR_INPUT_PAR);
    }
    if (st >= 0) st = fasp_hip_bsr_smoother_apply(h, kind, w, b, u);
    fasp_hip_bsr_smoother_destroy(h);
    if (st < 0) { std::fprintf(stderr, "### ERROR: %s: sweep failed (%d)\n", fn, st); std::exit(st); }
}
}  // namespace
}  // extern "C++"

// ItrSmootherBSR.c:163 (host): the diagonal blocks fetched (the last one a row stores) and inverted as fasp_smat_inv does
void fasp_smoother_dbsr_jacobi_setup(dBSRmat* A, double* diaginv)
{
    FASP_ENTRY();
    if (!A || !diaginv || fasp::bsr_diaginv(A, diaginv) < 0) {
        std::fprintf(stderr, "### ERROR: %s: nb is illegal (1 .. 7) or a NULL argument\n", __func__);
        std::exit(A && diaginv ? ERROR_NUM_BLOCKS : ERROR_INPUT_PAR);
    }
}
// ItrSmootherBSR.c:59
void fasp_smoother_dbsr_jacobi(dBSRmat* A, dvector* b, dvector* u)
{
    FASP_ENTRY();
    if (!A || !b || !u) { std::fprintf(stderr, "### ERROR: %s: inconsistent arguments\n", __func__); std::exit(ERROR_INPUT_PAR); }
    if (A->nb < 1 || A->nb > 7) { std::fprintf(stderr, "### ERROR: %s: nb = %d is illegal (1 .. 7)\n", __func__, A->nb); std::exit(ERROR_NUM_BLOCKS); }
    const long long n = (long long)A->ROW * A->nb;
    if (A->ROW != A->COL || b->row < n || u->row < n) { std::fprintf(stderr, "### ERROR: %s: inconsistent arguments\n", __func__); std::exit(ERROR_INPUT_PAR); }
    std::vector<double> dinv((size_t)std::max<long long>(n * A->nb, 1));
    (void)fasp::bsr_diaginv(A, dinv.data());
    fasp_smoother_dbsr_jacobi1(A, b, u, dinv.data());
}
void fasp_smoother_dbsr_gs(dBSRmat* A, dvector* b, dvector* u, int order, int* mark)
{
    FASP_ENTRY();
    bsr_smoother_oneshot(__func__, A, b, u, order, mark, nullptr, true, BSR_SW_GS, 0.0);
}
void fasp_smoother_dbsr_gs1(dBSRmat* A, dvector* b, dvector* u, int order, int* mark, double* diaginv)
{
    FASP_ENTRY();
    bsr_smoother_oneshot(__func__, A, b, u, order, mark, diaginv, false, BSR_SW_GS, 0.0);
}
void fasp_smoother_dbsr_gs_ascend(dBSRmat* A, dvector* b, dvector* u, double* diaginv)
{
    FASP_ENTRY();
    bsr_smoother_oneshot(__func__, A, b, u, ASCEND, nullptr, diaginv, false, BSR_SW_GS, 0.0);
}
void fasp_smoother_dbsr_gs_ascend1(dBSRmat* A, dvector* b, dvector* u)
{
    FASP_ENTRY();
    bsr_smoother_oneshot(__func__, A, b, u, ASCEND, nullptr, nullptr, false, BSR_SW_ID, 0.0);
}
void fasp_smoother_dbsr_gs_descend(dBSRmat* A, dvector* b, dvector* u, double* diaginv)
{
    FASP_ENTRY();
    bsr_smoother_oneshot(__func__, A, b, u, DESCEND, nullptr, diaginv, false, BSR_SW_GS, 0.0);
}
void fasp_smoother_dbsr_gs_descend1(dBSRmat* A, dvector* b, dvector* u)
{
    FASP_ENTRY();
    bsr_smoother_oneshot(__func__, A, b, u, DESCEND, nullptr, nullptr, false, BSR_SW_ID, 0.0);
}
void fasp_smoother_dbsr_gs_order1(dBSRmat* A, dvector* b, dvector* u, double* diaginv, int* mark)
{
    FASP_ENTRY();
    if (!mark) { std::fprintf(stderr, "### ERROR: %s: inconsistent arguments\n", __func__); std::exit(ERROR_INPUT_PAR); }
    bsr_smoother_oneshot(__func__, A, b, u, USERDEFINED, mark, diaginv, false, BSR_SW_GS, 0.0);
}
void fasp_smoother_dbsr_gs_order2(dBSRmat* A, dvector* b, dvector* u, int* mark, double* work)
{
    FASP_ENTRY();
    (void)work;   // the reference's b_tmp of nb doubles: the lanes keep theirs in registers
    if (!mark) { std::fprintf(stderr, "### ERROR: %s: inconsistent arguments\n", __func__); std::exit(ERROR_INPUT_PAR); }
    bsr_smoother_oneshot(__func__, A, b, u, USERDEFINED, mark, nullptr, false, BSR_SW_ID, 0.0);
}
void fasp_smoother_dbsr_sor(dBSRmat* A, dvector* b, dvector* u, int order, int* mark, double weight)
{
    FASP_ENTRY();
    bsr_smoother_oneshot(__func__, A, b, u, order, mark, nullptr, true, BSR_SW_SOR, weight);
}
void fasp_smoother_dbsr_sor1(dBSRmat* A, dvector* b, dvector* u, int order, int* mark, double* diaginv, double weight)
{
    FASP_ENTRY();
    bsr_smoother_oneshot(__func__, A, b, u, order, mark, diaginv, false, BSR_SW_SOR, weight);
}
void fasp_smoother_dbsr_sor_ascend(dBSRmat* A, dvector* b, dvector* u, double* diaginv, double weight)
{
    FASP_ENTRY();
    bsr_smoother_oneshot(__func__, A, b, u, ASCEND, nullptr, diaginv, false, BSR_SW_SOR, weight);
}
void fasp_smoother_dbsr_sor_descend(dBSRmat* A, dvector* b, dvector* u, double* diaginv, double weight)
{
    FASP_ENTRY();
    bsr_smoother_oneshot(__func__, A, b, u, DESCEND, nullptr, diaginv, false, BSR_SW_SOR, weight);
}
void fasp_smoother_dbsr_sor_order(dBSRmat* A, dvector* b, dvector* u, double* diaginv, int* mark, double weight)
{
    FASP_ENTRY();
    if (!mark) { std::fprintf(stderr, "### ERROR: %s: inconsistent arguments\n", __func__); std::exit(ERROR_INPUT_PAR); }
    bsr_smoother_oneshot(__func__, A, b, u, USERDEFINED, mark, diaginv, false, BSR_SW_SOR, weight);
}

// ---------------------------------------------------------------------------
// the block AMG cycle's sweeps through the plan: fasp_hip_tune("bsr_cycle_sweep", 1)
// ---------------------------------------------------------------------------
extern "C++" {
namespace fasp_bsr {
void bsr_level_sweeps_destroy(BsrLevel& Lv)
{
    for (BsrSweepDev*& D : Lv.sweep) { bsr_sweep_dev_destroy(D); D = nullptr; }
}
// One block Gauss-Seidel / SOR sweep of level `level`, ascending or descending, out of place through the level's second
// vector: x2 = sweep(b, x), then the two change places (as the block Jacobi sweep does).  The plan of a direction is built
// and uploaded at its first use and belongs to the level.
static int bsr_cycle_sweep(fasp_hip_amg_bsr* h, int level, bool descend, bool sor, double w)
{
    BsrLevel& Lv = h->L[level];
    BsrSweepDev*& D = Lv.sweep[descend ? 1 : 0];
    if (!D) {
        const HostLevelBSR& HL = h->H.L[level];
        const dBSRmat Av = HL.A.view();
        std::vector<int> seq;
        int st = fasp::bsr_sweep_sequence(Av.ROW, descend ? DESCEND : ASCEND, nullptr, seq);
        if (st < 0) return st;
        if (HL.diaginv.n < (size_t)Av.ROW * Av.nb * Av.nb) return ERROR_INPUT_PAR;
        D = bsr_sweep_upload(&Av, seq, HL.diaginv.data(), &st);
        if (!D) return st;
    }
    if (Lv.x_zero) { HIPCK(hipMemsetAsync(Lv.x, 0, sizeof(double) * Lv.n, g_ctx.stream)); Lv.x_zero = false; }
    const int st = bsr_sweep_run(D, sor ? BSR_SW_SOR : BSR_SW_GS, w, Lv.b, Lv.x, Lv.x2);
    if (st < 0) return st;
    std::swap(Lv.x, Lv.x2);
    return FASP_SUCCESS;
}
}  // namespace fasp_bsr
}  // extern "C++"
