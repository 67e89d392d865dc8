// rap.hip.h -- the Galerkin product C = R A P on the device (fasp_blas_dcsr_rap, base/src/BlaSpmvCSR.c:999), part of solver.hip.
//
// The result is the reference's byte for byte (the contract host_setup.cpp's galerkin_rap states): every row starts with the slot of
// its diagonal (0.0, only ever added to), the other columns follow in the order of first discovery of the loop j1 over R-row ic, j2
// over A-row i1, j3 over P-row i2; a contribution is (r*a)*p, a column's first contribution is assigned, later ones are added in
// the order of (j1, j2, j3).  Rows of C are independent: that is the parallelism.
//
// A fine row met a second time inside a coarse row discovers nothing (all its columns are in the row already) and contributes as
// the first time.  "Look the column up, append it when it is absent" therefore IS the reference's loop: the device kernels keep one
// open-addressing table per row, coarse column -> position in the row, and no "fine row seen" marker.  A position always comes from
// the row's own discovery counter, never from a table slot: hash function and probing cannot change the result.
//
// Two passes, as in the reference: a symbolic one counts the columns of every row (tables sized from the upper bound
// 1 + sum sum len P(i2), capped at nc, that k_rap_bounds computes), the numeric one writes C (tables sized from the counts).  The
// exclusive scans (row counts -> IA, table sizes -> arena offsets) run on the host between the passes.
//   form 0, k_rap_lane: one lane per coarse row, tables in a global arena, rows in batches that keep the arena within
//           fasp_hip_tune("rap_arena_kb") (a batch of one row is always allowed).
//   form 1, k_rap_wave: one wavefront per coarse row.  The (j1, j2) walk is uniform; the entries of P-row i2 go across the lanes,
//           64 a step.  Inside a P row the columns are distinct, so a step writes distinct slots and a slot's additions happen in step
//           order; new columns of a step take their positions from a ballot and a prefix count in lane (= j3) order.  Table and
//           accumulators live in LDS where the row fits (RAP_LENT entries), else in the arena / in C itself, with a fence between the
//           steps.  A P with a repeated column inside a row takes form 0.
// The product uses a stream and buffers of its own, touches no DevLevel, is synchronous at return and frees what it allocated: the
// setup may call it while the upload thread works on g_ctx.stream.
#pragma once

extern "C++" {
namespace fasp {

constexpr int RAP_LCAP = 2048;   // slots of form 1's LDS table (16 KiB); entries + 1 <= RAP_LCAP / 2
constexpr int RAP_LENT = 1023;   // entries of a row that fits: accumulators 8 KiB + columns 4 KiB beside the table, 28 KiB a workgroup

struct RapArgs {
    const int *Ri, *Rj, *Ai, *Aj, *Pi, *Pj;
    const double *Rv, *Av, *Pv;
    int nc, nf;
};

// slots of a row's table: a power of two, at least twice the entries it may hold
__host__ __device__ inline unsigned rap_cap(int need)
{
    unsigned c = 16;
    while (c < 2u * (unsigned)need + 2u) c <<= 1;
    return c;
}
__device__ __forceinline__ unsigned rap_hash(int c)
{
    unsigned h = (unsigned)c * 2654435761u;
    return h ^ (h >> 15);
}

// flag[0] |= 1: a row pointer or a column out of range; flag[1] |= 1 (dup != 0): a column repeated inside a row
__global__ __launch_bounds__(256) void k_rap_check(const int* ia, const int* ja, int nrow, int ncol, int nnz, int dup, int* flag)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nrow) return;
    const int b = ia[i], e = ia[i + 1];
    if (b < 0 || e < b || e > nnz) { atomicOr(&flag[0], 1); return; }
    bool bad = false, rep = false;
    for (int k = b; k < e; ++k) {
        const int c = ja[k];
        if (c < 0 || c >= ncol) bad = true;
        if (dup)
            for (int q = b; q < k; ++q) rep = rep || ja[q] == c;
    }
    if (bad) atomicOr(&flag[0], 1);
    if (rep) atomicOr(&flag[1], 1);
}

// need[ic] = min(1 + sum over (j1, j2) of len P(i2), nc): bounds the columns of row ic; *work += the uncapped sums
__global__ __launch_bounds__(256) void k_rap_bounds(RapArgs a, int* need, unsigned long long* work)
{
    const int ic = blockIdx.x * 256 + threadIdx.x;
    unsigned long long w = 0;
    if (ic < a.nc) {
        w = 1;
        for (int j1 = a.Ri[ic]; j1 < a.Ri[ic + 1]; ++j1) {
            const int i1 = a.Rj[j1];
            for (int j2 = a.Ai[i1]; j2 < a.Ai[i1 + 1]; ++j2) {
                const int i2 = a.Aj[j2];
                w += (unsigned long long)(a.Pi[i2 + 1] - a.Pi[i2]);
            }
        }
        need[ic] = (int)(w < (unsigned long long)a.nc ? w : (unsigned long long)a.nc);
    }
    for (int d = 32; d > 0; d >>= 1) w += __shfl_down(w, d, 64);
    if ((threadIdx.x & 63) == 0 && w) atomicAdd(work, w);
}

// form 0: lane = coarse row r0 + t.  The row's table (empty slots: key -1) starts at arena + off[ic].
template <bool NUM>
__global__ __launch_bounds__(256) void k_rap_lane(RapArgs a, int r0, int nrows, const int* __restrict__ need,
                                                  const unsigned long long* __restrict__ off, int2* arena, int* cnt,
                                                  const int* __restrict__ cia, int* Cj, double* Cv)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nrows) return;
    const int ic = r0 + t;
    int2* tab = arena + off[ic];
    const unsigned mask = rap_cap(need[ic]) - 1u;
    const int base = NUM ? cia[ic] : 0;
    int pos = 1;
    tab[rap_hash(ic) & mask] = make_int2(ic, 0);
    if (NUM) { Cj[base] = ic; Cv[base] = 0.0; }
    for (int j1 = a.Ri[ic]; j1 < a.Ri[ic + 1]; ++j1) {
        const double r = a.Rv[j1];
        const int    i1 = a.Rj[j1];
        for (int j2 = a.Ai[i1]; j2 < a.Ai[i1 + 1]; ++j2) {
            const double ra = r * a.Av[j2];
            const int    i2 = a.Aj[j2];
            for (int j3 = a.Pi[i2]; j3 < a.Pi[i2 + 1]; ++j3) {
                const int    c = a.Pj[j3];
                const double rap = ra * a.Pv[j3];
                for (unsigned s = rap_hash(c) & mask;; s = (s + 1u) & mask) {
                    const int2 e = tab[s];
                    if (e.x == c) {
                        if (NUM) Cv[base + e.y] += rap;
                        break;
                    }
                    if (e.x < 0) {
                        tab[s] = make_int2(c, pos);
                        if (NUM) { Cj[base + pos] = c; Cv[base + pos] = rap; }
                        ++pos;
                        break;
                    }
                }
            }
        }
    }
    if (!NUM) cnt[ic] = pos;
}

// between two steps of form 1: a later step reads what another lane of the wavefront wrote in an earlier one
__device__ __forceinline__ void rap_step_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

// form 1: workgroup b = one wavefront = coarse row rows[b].  LDS: table and accumulators in LDS (the row holds at most RAP_LENT
// entries); else the table at arena + off[b] and the accumulators in C itself.
template <bool NUM, bool LDS>
__global__ __launch_bounds__(64) void k_rap_wave(RapArgs a, const int* __restrict__ rows, const int* __restrict__ need,
                                                 const unsigned long long* __restrict__ off, int2* arena, int* cnt,
                                                 const int* __restrict__ cia, int* Cj, double* Cv)
{
    __shared__ int2   ltab[LDS ? RAP_LCAP : 1];
    __shared__ double lcv[(LDS && NUM) ? RAP_LENT + 1 : 1];
    __shared__ int    lcj[(LDS && NUM) ? RAP_LENT + 1 : 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int ic = rows[b];
    const unsigned cap = rap_cap(need[ic]), mask = cap - 1u;
    const int base = NUM ? cia[ic] : 0;
    int2*   tab = LDS ? ltab : arena + off[b];
    double* acc = LDS ? lcv : Cv + base;
    int*    col = LDS ? lcj : Cj + base;
    for (unsigned s = lane; s < cap; s += 64) tab[s] = make_int2(-1, -1);
    rap_step_fence();
    if (lane == 0) {
        tab[rap_hash(ic) & mask] = make_int2(ic, 0);
        if (NUM) { col[0] = ic; acc[0] = 0.0; }
    }
    rap_step_fence();
    int n = 1;   // columns of the row so far (uniform)
    for (int j1 = a.Ri[ic]; j1 < a.Ri[ic + 1]; ++j1) {
        const double r = a.Rv[j1];
        const int    i1 = a.Rj[j1];
        for (int j2 = a.Ai[i1]; j2 < a.Ai[i1 + 1]; ++j2) {
            const double ra = r * a.Av[j2];
            const int    i2 = a.Aj[j2];
            const int    pe = a.Pi[i2 + 1];
            for (int j0 = a.Pi[i2]; j0 < pe; j0 += 64) {
                const int  j3 = j0 + lane;
                const bool on = j3 < pe;
                int    c = -1, p = -1;
                double rap = 0.0;
                unsigned s = 0;
                if (on) {
                    c = a.Pj[j3];
                    rap = ra * a.Pv[j3];
                    for (s = rap_hash(c) & mask;; s = (s + 1u) & mask) {
                        const int k = tab[s].x;
                        if (k == c) { p = tab[s].y; break; }
                        if (k < 0) break;
                    }
                }
                const bool fresh = on && p < 0;
                const unsigned long long bal = __ballot(fresh);
                if (fresh) {   // position: the row's counter + the new columns of the lanes (= j3) before this one
                    p = n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
                    for (;; s = (s + 1u) & mask)   // another lane's new column may have taken the slot since the look-up
                        if (atomicCAS(&tab[s].x, -1, c) == -1) { tab[s].y = p; break; }
                    if (NUM) { col[p] = c; acc[p] = rap; }
                }
                else if (on && NUM) acc[p] += rap;
                n += __popcll(bal);
                rap_step_fence();
            }
        }
    }
    if (!NUM) { if (lane == 0) cnt[ic] = n; }
    else if (LDS)
        for (int q = lane; q < n; q += 64) { Cj[base + q] = col[q]; Cv[base + q] = acc[q]; }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
static int  g_rap_form = -1;          // fasp_hip_tune("rap_form"): -1 by the mean work per row, 0 lane per row, 1 wavefront per row
static int  g_rap_arena_kb = 262144;  // fasp_hip_tune("rap_arena_kb"): budget of the table arena, KiB
static int  g_device_rap = 0;         // fasp_hip_tune("device_rap"): the setups' Galerkin products on the device
static int  g_rap_info[4] = {-1, 0, 0, 0};
static long g_rap_count = 0;
constexpr double RAP_FORM1_MIN_WORK = 2048.0;   // automatic choice: form 1 from this mean of 1 + sum sum len P(i2) per row on (profiles/rap_device.txt: P7 level 1, 1 070 a row, is faster in form 0, level 2, 3 100, in form 1)

namespace {
struct RapDev {   // the product's own stream, events and buffers, all gone with it
    hipStream_t        s = nullptr;
    hipEvent_t         e0 = nullptr, e1 = nullptr;
    std::vector<void*> bufs;
    double             kernel_ms = 0.0;
    bool               bad = false;
    ~RapDev()
    {
        for (void* p : bufs) (void)hipFree(p);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (s) (void)hipStreamDestroy(s);
    }
    template <class T> T* alloc(size_t n)
    {
        void* p = nullptr;
        if (hipMalloc(&p, sizeof(T) * std::max<size_t>(n, 1)) != hipSuccess) { bad = true; return nullptr; }
        bufs.push_back(p);
        return static_cast<T*>(p);
    }
    void release(void* p)
    {
        for (auto& q : bufs)
            if (q == p) { (void)hipFree(p); q = bufs.back(); bufs.pop_back(); return; }
    }
    template <class T> T* up(const T* h, size_t n)
    {
        T* d = alloc<T>(n);
        if (d && n && hipMemcpyAsync(d, h, sizeof(T) * n, hipMemcpyHostToDevice, s) != hipSuccess) bad = true;
        return d;
    }
    template <class T> void down(T* h, const T* d, size_t n)
    {
        if (n && hipMemcpyAsync(h, d, sizeof(T) * n, hipMemcpyDeviceToHost, s) != hipSuccess) bad = true;
        if (hipStreamSynchronize(s) != hipSuccess) bad = true;
    }
    void tic() { (void)hipEventRecord(e0, s); }
    void toc()
    {
        (void)hipEventRecord(e1, s);
        if (hipEventSynchronize(e1) != hipSuccess) { bad = true; return; }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) kernel_ms += ms;
        if (hipGetLastError() != hipSuccess) bad = true;
    }
};

// One pass (symbolic or numeric) over all rows.  need[ic] bounds the entries of row ic's table.
struct RapPass {
    int form = 0, batches = 0, used_lds = 0;
};
template <bool NUM>
int rap_pass(RapDev& D, const RapArgs& a, int form, const std::vector<int>& need, const int* d_need, int* d_cnt, const int* d_cia,
             int* d_Cj, double* d_Cv, RapPass& out)
{
    const int nc = a.nc;
    const unsigned long long budget = std::max(1ull, (unsigned long long)std::max(g_rap_arena_kb, 1) * 1024ull / sizeof(int2));   // slots
    // rows that take the arena, in order; off: where a row's table starts inside its batch
    std::vector<int> glb, lds;
    if (form == 1)
        for (int ic = 0; ic < nc; ++ic) (need[(size_t)ic] <= RAP_LENT ? lds : glb).push_back(ic);
    const size_t ng = form == 1 ? glb.size() : (size_t)nc;
    std::vector<unsigned long long> off(std::max<size_t>(ng, 1));
    std::vector<size_t> bstart;   // first arena row of every batch (+ the end)
    unsigned long long fill = 0, largest = 0;
    for (size_t q = 0; q < ng; ++q) {
        const unsigned long long c = rap_cap(need[(size_t)(form == 1 ? glb[q] : (int)q)]);
        if (q == 0 || fill + c > budget) { bstart.push_back(q); fill = 0; }
        off[q] = fill;
        fill += c;
        largest = std::max(largest, fill);
    }
    bstart.push_back(ng);
    out.form = form; out.batches = (int)bstart.size() - 1; out.used_lds = lds.empty() ? 0 : 1;
    int2* arena = ng ? D.alloc<int2>((size_t)largest) : nullptr;
    unsigned long long* d_off = D.up(off.data(), ng);
    int *d_glb = nullptr, *d_lds = nullptr;
    if (form == 1) { d_glb = D.up(glb.data(), glb.size()); d_lds = D.up(lds.data(), lds.size()); }
    if (D.bad) return ERROR_ALLOC_MEM;
    D.tic();
    if (form == 1 && !lds.empty())
        hipLaunchKernelGGL((k_rap_wave<NUM, true>), dim3((unsigned)lds.size()), dim3(64), 0, D.s, a, d_lds, d_need, nullptr, nullptr, d_cnt, d_cia, d_Cj, d_Cv);
    for (size_t bi = 0; bi + 1 < bstart.size(); ++bi) {
        const size_t q0 = bstart[bi], q1 = bstart[bi + 1];
        if (q1 == q0) continue;
        if (form == 1)
            hipLaunchKernelGGL((k_rap_wave<NUM, false>), dim3((unsigned)(q1 - q0)), dim3(64), 0, D.s, a, d_glb + q0, d_need, d_off + q0, arena, d_cnt, d_cia, d_Cj, d_Cv);
        else {
            const unsigned long long slots = off[q1 - 1] + rap_cap(need[q1 - 1]);
            (void)hipMemsetAsync(arena, 0xff, (size_t)slots * sizeof(int2), D.s);
            hipLaunchKernelGGL((k_rap_lane<NUM>), dim3((unsigned)((q1 - q0 + 255) / 256)), dim3(256), 0, D.s, a, (int)q0, (int)(q1 - q0), d_need, d_off, arena, d_cnt, d_cia, d_Cj, d_Cv);
        }
    }
    D.toc();
    if (arena) D.release(arena);
    D.release(d_off);
    if (d_glb) D.release(d_glb);
    if (d_lds) D.release(d_lds);
    return D.bad ? ERROR_MISC : FASP_SUCCESS;
}
}  // namespace

// C = R A P.  alloc(nc, nnz, &ia, &ja, &val) provides the result's arrays (nc + 1, nnz, nnz).  kernel_ms (may be NULL): the
// kernels' time by events.  Returns FASP_SUCCESS, ERROR_INPUT_PAR (operands that are no CSR matrices), ERROR_ALLOC_MEM (more than
// 2^31 - 1 entries, or no memory), ERROR_MISC (a HIP call failed).
static int rap_device(const dCSRmat& R, const dCSRmat& A, const dCSRmat& P,
                      const std::function<bool(int, int, int**, int**, double**)>& alloc, double* kernel_ms)
{
    const int nc = R.row, nf = A.row;
    if (nc > 1000000000 || nc < 0 || nf < 0 || R.nnz < 0 || A.nnz < 0 || P.nnz < 0) return nc > 1000000000 ? ERROR_ALLOC_MEM : ERROR_INPUT_PAR;
    if ((R.nnz && (!R.JA || !R.val)) || (A.nnz && (!A.JA || !A.val)) || (P.nnz && (!P.JA || !P.val)) || !R.IA || !A.IA || !P.IA) return ERROR_INPUT_PAR;
    if (R.IA[nc] != R.nnz + R.IA[0] || A.IA[nf] != A.nnz + A.IA[0] || P.IA[nf] != P.nnz + P.IA[0] || R.IA[0] != 0 || A.IA[0] != 0 || P.IA[0] != 0) return ERROR_INPUT_PAR;
    (void)hipSetDevice(g_ctx.device);
    RapDev D;
    if (hipStreamCreateWithFlags(&D.s, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&D.e0) != hipSuccess || hipEventCreate(&D.e1) != hipSuccess) return ERROR_MISC;
    RapArgs a;
    a.nc = nc; a.nf = nf;
    a.Ri = D.up(R.IA, (size_t)nc + 1); a.Rj = D.up(R.JA, (size_t)R.nnz); a.Rv = D.up(R.val, (size_t)R.nnz);
    a.Ai = D.up(A.IA, (size_t)nf + 1); a.Aj = D.up(A.JA, (size_t)A.nnz); a.Av = D.up(A.val, (size_t)A.nnz);
    a.Pi = D.up(P.IA, (size_t)nf + 1); a.Pj = D.up(P.JA, (size_t)P.nnz); a.Pv = D.up(P.val, (size_t)P.nnz);
    int* d_flag = D.alloc<int>(2);
    unsigned long long* d_work = D.alloc<unsigned long long>(1);
    int* d_need = D.alloc<int>((size_t)nc);
    if (D.bad) return ERROR_ALLOC_MEM;
    (void)hipMemsetAsync(d_flag, 0, 2 * sizeof(int), D.s);
    (void)hipMemsetAsync(d_work, 0, sizeof(unsigned long long), D.s);
    D.tic();
    if (nc) hipLaunchKernelGGL(k_rap_check, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, D.s, a.Ri, a.Rj, nc, nf, R.nnz, 0, d_flag);
    if (nf) hipLaunchKernelGGL(k_rap_check, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, D.s, a.Ai, a.Aj, nf, nf, A.nnz, 0, d_flag);
    if (nf) hipLaunchKernelGGL(k_rap_check, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, D.s, a.Pi, a.Pj, nf, nc, P.nnz, 1, d_flag);
    D.toc();
    int flag[2] = {0, 0};
    D.down(flag, d_flag, 2);
    if (D.bad) return ERROR_MISC;
    if (flag[0]) return ERROR_INPUT_PAR;   // (nothing has walked the operands yet)
    std::vector<int> need((size_t)nc), cnt((size_t)nc);
    unsigned long long work = 0;
    D.tic();
    if (nc) hipLaunchKernelGGL(k_rap_bounds, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, D.s, a, d_need, d_work);
    D.toc();
    D.down(need.data(), d_need, (size_t)nc);
    D.down(&work, d_work, 1);
    if (D.bad) return ERROR_MISC;
    int form = g_rap_form >= 0 ? (g_rap_form ? 1 : 0) : (nc > 0 && (double)work >= RAP_FORM1_MIN_WORK * nc ? 1 : 0);
    if (flag[1]) form = 0;   // a column repeated inside a row of P: two lanes of one step would meet in one slot
    // symbolic pass: the columns of every row
    int* d_cnt = D.alloc<int>((size_t)nc);
    if (D.bad) return ERROR_ALLOC_MEM;
    RapPass ps, pn;
    int st = rap_pass<false>(D, a, form, need, d_need, d_cnt, nullptr, nullptr, nullptr, ps);
    if (st < 0) return st;
    D.down(cnt.data(), d_cnt, (size_t)nc);
    if (D.bad) return ERROR_MISC;
    long long total = 0;
    for (int ic = 0; ic < nc; ++ic) {
        if (cnt[(size_t)ic] < 1 || cnt[(size_t)ic] > need[(size_t)ic]) return ERROR_MISC;   // (a count beyond its bound: never write by it)
        total += cnt[(size_t)ic];
    }
    if (total > 2147483647LL) return ERROR_ALLOC_MEM;   // INT is 32-bit in the ABI
    int *ia = nullptr, *ja = nullptr;
    double* val = nullptr;
    if (!alloc(nc, (int)total, &ia, &ja, &val)) return ERROR_ALLOC_MEM;
    ia[0] = 0;
    for (int ic = 0; ic < nc; ++ic) ia[ic + 1] = ia[ic] + cnt[(size_t)ic];
    // numeric pass: tables sized from the counts
    int*    d_cia = D.up(ia, (size_t)nc + 1);
    int*    d_Cj = D.alloc<int>((size_t)total);
    double* d_Cv = D.alloc<double>((size_t)total);
    if (D.bad) return ERROR_ALLOC_MEM;
    if (hipMemcpyAsync(d_need, cnt.data(), sizeof(int) * (size_t)nc, hipMemcpyHostToDevice, D.s) != hipSuccess) return ERROR_MISC;
    st = rap_pass<true>(D, a, form, cnt, d_need, nullptr, d_cia, d_Cj, d_Cv, pn);
    if (st < 0) return st;
    D.down(ja, d_Cj, (size_t)total);
    D.down(val, d_Cv, (size_t)total);
    if (D.bad) return ERROR_MISC;
    g_rap_info[0] = form; g_rap_info[1] = std::max(ps.batches, pn.batches); g_rap_info[2] = (ps.used_lds || pn.used_lds) ? 1 : 0; g_rap_info[3] = nc;
    ++g_rap_count;
    if (kernel_ms) *kernel_ms = D.kernel_ms;
    return FASP_SUCCESS;
}

static bool rap_chains(const dCSRmat* R, const dCSRmat* A, const dCSRmat* P)
{
    return R->col == A->row && A->row == A->col && A->col == P->row && P->col == R->row;
}

// the setups' hook (fasp_internal.h): 1 = C formed on the device, 0 = the host is to form it
static int device_rap_hook(const HostCSR& R, const HostCSR& A, const HostCSR& P, HostCSR& C)
{
    if (!g_device_rap || comm_size() != 1) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return 0;
    if (ctx_init() < 0) return 0;
    const dCSRmat r = R.view(), m = A.view(), p = P.view();
    if (!rap_chains(&r, &m, &p)) return 0;
    const int st = rap_device(r, m, p, [&C](int nc, int nnz, int** ia, int** ja, double** val) {
        C.row = nc; C.col = nc; C.nnz = nnz;
        C.ia.alloc((size_t)nc + 1); C.ja.alloc((size_t)nnz); C.val.alloc((size_t)nnz);
        *ia = C.ia.data(); *ja = C.ja.data(); *val = C.val.data();
        return true;
    }, nullptr);
    if (st < 0) { std::printf("### ERROR: fasp_hip: the Galerkin product on the device failed (%d)\n", st); return st; }
    return 1;
}
[[maybe_unused]] static const bool g_rap_hook_set = (g_device_rap_hook = &device_rap_hook, true);

}  // namespace fasp
}  // extern "C++"

// ---- entries (include/fasp_hip.h, include/fasp_hip_dev.h) ----------------------------------------------------------------------
int fasp_hip_dcsr_rap(const dCSRmat* R, const dCSRmat* A, const dCSRmat* P, dCSRmat* RAP)
{
    FASP_ENTRY();
    if (RAP) std::memset(RAP, 0, sizeof(*RAP));
    if (!R || !A || !P || !RAP || !fasp::rap_chains(R, A, P)) return ERROR_INPUT_PAR;
    if (ctx_init() < 0) return ERROR_MISC;
    const int ncol = P->col;
    const int st = fasp::rap_device(*R, *A, *P, [RAP, ncol](int nc, int nnz, int** ia, int** ja, double** val) {
        RAP->row = nc; RAP->col = ncol; RAP->nnz = nnz;
        RAP->IA = (int*)fasp_mem_calloc((unsigned)nc + 1, sizeof(int));
        RAP->JA = (int*)fasp_mem_calloc((unsigned)nnz, sizeof(int));
        RAP->val = (double*)fasp_mem_calloc((unsigned)nnz, sizeof(double));
        *ia = RAP->IA; *ja = RAP->JA; *val = RAP->val;
        return true;
    }, nullptr);
    if (st < 0) { fasp_dcsr_free(RAP); std::memset(RAP, 0, sizeof(*RAP)); }
    return st;
}

// BlaSpmvCSR.c:999
void fasp_blas_dcsr_rap(const dCSRmat* R, const dCSRmat* A, const dCSRmat* P, dCSRmat* RAP)
{
    FASP_ENTRY();
    if (R && A && P && RAP && fasp::rap_chains(R, A, P) && ctx_init() < 0) die_no_device(__func__);
    const int st = fasp_hip_dcsr_rap(R, A, P, RAP);
    if (st < 0) {   // fasp_chkerr: the reference prints and exits
        std::printf("### ERROR: %s [%s]\n", st == ERROR_ALLOC_MEM ? "Cannot allocate memory!" : st == ERROR_INPUT_PAR ? "Wrong input parameters!" : "Unknown error!", __func__);
        std::exit(st);
    }
}

int fasp_hip_rap_info(int info[4])
{
    FASP_ENTRY();
    if (!info) return ERROR_INPUT_PAR;
    for (int i = 0; i < 4; ++i) info[i] = fasp::g_rap_info[i];
    return FASP_SUCCESS;
}

long fasp_hip_rap_device_count(void)
{
    FASP_ENTRY();
    return fasp::g_rap_count;
}

double fasp_hip_rap_time(const dCSRmat* R, const dCSRmat* A, const dCSRmat* P, int where, int reps)
{
    FASP_ENTRY();
    if (!R || !A || !P || !fasp::rap_chains(R, A, P) || where < 0 || where > 2 || reps <= 0) return -1.0;
    if (where == 0) {
        HostCSR r, a, p;
        auto view = [](HostCSR& H, const dCSRmat* M) {
            H.row = M->row; H.col = M->col; H.nnz = M->nnz;
            H.ia.view(M->IA, (size_t)M->row + 1); H.ja.view(M->JA, (size_t)M->nnz); H.val.view(M->val, (size_t)M->nnz);
        };
        view(r, R); view(a, A); view(p, P);
        HostThreads team;
        const double t0 = wall_seconds();
        try {
            for (int i = 0; i < reps; ++i) { HostCSR c; fasp::galerkin_rap_host(r, a, p, c); }
        } catch (const std::bad_alloc&) { return -1.0; }
        return (wall_seconds() - t0) / reps;
    }
    if (ctx_init() < 0) return -1.0;
    std::vector<int> ia, ja;
    std::vector<double> val;
    auto alloc = [&](int nc, int nnz, int** pia, int** pja, double** pval) {
        ia.resize((size_t)nc + 1); ja.resize((size_t)std::max(nnz, 1)); val.resize((size_t)std::max(nnz, 1));
        *pia = ia.data(); *pja = ja.data(); *pval = val.data();
        return true;
    };
    double ms = 0.0, ms_sum = 0.0;
    if (fasp::rap_device(*R, *A, *P, alloc, &ms) < 0) return -1.0;   // warm-up
    const double t0 = wall_seconds();
    for (int i = 0; i < reps; ++i) {
        if (fasp::rap_device(*R, *A, *P, alloc, &ms) < 0) return -1.0;
        ms_sum += ms;
    }
    return where == 1 ? (wall_seconds() - t0) / reps : 1e-3 * ms_sum / reps;
}
