// str_swz.hip.h -- the block Gauss-Seidel (Schwarz) smoother of a structured matrix on the device: patch factorisation and sweep.
// Part of the single translation unit solver.hip (included there after str_sweep.hip.h; not a stand-alone header).
//
// Reference: fasp_generate_diaginv_block (ItrSmootherSTR.c:1543), fasp_smoother_dstr_swz (:1665), fasp_smat_lu_decomp / _solve
// (BlaSmallMatLU.c:52 / :124).  DESIGN.md section 3.9.  The patch of grid point i is the member list [i, p_0, p_1, ...] of its neighbours that are
// not absent (< 0), k members, m = k nc rows.  Its matrix (m x m, row-major) holds every member's diagonal block on the diagonal, A(i, p) in block
// (0, a) and A(p, i) in block (a, 0) for member a >= 1 where a band has that offset, zeros elsewhere.  It is factored as the reference does: the
// pivot of column k is the first row j >= k of largest |a_jk|, the two whole rows change places, |a_kk| < 1e-20 stops the patch there, otherwise
// a_ik = a_ik / a_kk and a_ij = a_ij - a_ik a_kj.  A visit gathers the residual at the members, applies the interchanges, substitutes forward
// (x_k = x_k - x_i a_ki, i ascending) and backward (i = k + 1 .. m - 1 ascending, then the division) and adds the correction to u in member order.
//
// The reference recomputes the whole residual after every visit.  Every row of it is a fresh function of b and the current u, so nothing is
// kept here: a visit computes the residual rows of its members from b and u, in the arithmetic form fasp_blas_dstr_aAxpy(-1, A, u, .) has for
// this matrix (S / B / N / G, str.hip.h; the same walk over the TmpSTR bands as k_str_band).  No fused multiply-add (-ffp-contract=off).
//
// Schedule: writes(v) = the members of visit v, reads(v) = the members and every point a member's row has a term to whose coefficient block is
// not all 0.0 (for finite u such a product is a zero whichever u is read; the kernel still evaluates it, so only the sign of a zero can differ,
// as in section 3.8).  level(v) = 1 + the largest level among the earlier visits w with writes(w) and reads(v), reads(w) and writes(v), or
// writes(w) and writes(v) in common: one pass with two arrays per point (str_swz_levels).  Visits are sorted stably by level; one launch per
// level over its slice of the list, in place.
//
// Factors: stored in the order of the sorted list, every patch padded to ms^2 doubles (ms: the largest m), 64 patches interleaved: entry e of
// slot s at ((s / 64) ms^2 + e) 64 + s % 64; the pivots likewise.  A level reads one contiguous slab.  k_str_swz_factor: lane = patch, in place
// in that store -- the lanes of a wavefront touch consecutive doubles.  k_str_swz_level: lane = (visit, patch row): the residual rows, the
// interchanges and the forward substitution (column by column, which keeps every row's i-ascending order) run across the rows; the backward
// substitution is a serial chain by the reference's order of summation.  Factor, vector, members and pivots of a visit are staged in LDS.
// (Measured first: lane = visit with the vector in LDS as [row][lane] -- some 40 dependent memory round trips per visit, 50 us per level.)
// No matrix index arrays beyond neigh and the visit list.

namespace fasp_str {

constexpr int STR_SWZ_MAX_M = 64;   // rows of a patch at most: one wavefront per visit, its 64 x 64 factor 32 KB of LDS

struct StrSwzArgs {
    const double* val;      // TmpSTR: nb1 bands of `stride` doubles in walk order, the block of grid point i at i * NC * NC
    size_t        stride;
    const int*    offs;     // nb1 offsets in walk order (0: the diagonal)
    int           nb1, kdiag, form, ngrid;
    const int*    neigh;    // ngrid x nneigh, < 0: absent
    int           nneigh;
    const int*    list;     // grid point of every slot (the visits sorted by level)
    double*       fac;      // interleaved factors (header)
    int*          piv;      // interleaved pivots
    int           ms;       // the largest m
    const double* b;
    double*       u;
    unsigned*     count;    // [0] patches with a row interchange, [1] patches that stopped
};

__device__ __forceinline__ size_t swz_fac_at(const StrSwzArgs& a, int slot) { return (size_t)(slot >> 6) * (size_t)(a.ms * a.ms) * 64 + (size_t)(slot & 63); }
__device__ __forceinline__ size_t swz_piv_at(const StrSwzArgs& a, int slot) { return (size_t)(slot >> 6) * (size_t)a.ms * 64 + (size_t)(slot & 63); }

// row p of b_i - (A u)_i as fasp_blas_dstr_aAxpy(-1.0, A, u, r) on r = b computes it: the arithmetic of k_str_band with alpha = -1.  NB1 > 0: the
// number of walked bands is known at compile time (7 and 5: the canonical forms), the walk unrolls and the loads of all bands are in flight
// together; they never depend on whether the term exists (a missing term loads its padded zero and the row's own u), only the arithmetic does.
template <int NC, int NB1>
__device__ __forceinline__ double swz_resid_row(const StrSwzArgs& a, int i, int p)
{
    const double alpha = -1.0;
    const size_t r = (size_t)i * NC + p;
    double y = a.b[r];
    if (a.form == STR_G) y = y * (1.0 / alpha);
    double t = 0.0;
    bool   have = false;
    auto term = [&](int k) {
        const double* ap = a.val + (size_t)k * a.stride + r * NC;
        const int  j = i + a.offs[k];
        const bool ex = (unsigned)j < (unsigned)a.ngrid;
        const double* xp = a.u + (size_t)(ex ? j : i) * NC;
        double av[NC], xv[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) { av[q] = ap[q]; xv[q] = xp[q]; }
        if (!ex) return;
        if (a.form == STR_S) {
            const double pr = av[0] * xv[0];
            t = have ? t + pr : pr;
            have = true;
        } else if (a.form == STR_B) {
            double s = av[0] * xv[0];
#pragma unroll
            for (int q = 1; q < NC; ++q) s = s + av[q] * xv[q];
            y = y + alpha * s;
        } else if (a.form == STR_N) {
#pragma unroll
            for (int q = 0; q < NC; ++q) y = y + (alpha * av[q]) * xv[q];
        } else {
#pragma unroll
            for (int q = 0; q < NC; ++q) y = y + av[q] * xv[q];
        }
    };
    if constexpr (NB1 > 0) {
#pragma unroll
        for (int k = 0; k < NB1; ++k) term(k);
    } else {
        for (int k = 0; k < a.nb1; ++k) term(k);
    }
    if (a.form == STR_S) y = y + alpha * t;
    if (a.form == STR_G) y = y * alpha;
    return y;
}

// assemble and factor the patches of the slots [0, nslots): one lane per patch, in place in the interleaved store (zeroed by the host)
template <int NC>
__global__ __launch_bounds__(256) void k_str_swz_factor(const StrSwzArgs a, int nslots)
{
    const long long s64 = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s64 >= nslots) return;
    const int slot = (int)s64, i = a.list[slot];
    constexpr int NC2 = NC * NC;
    const int* nb = a.neigh + (size_t)i * a.nneigh;
    int k = 1;
    for (int l = 0; l < a.nneigh; ++l) k += nb[l] >= 0 ? 1 : 0;
    const int m = k * NC;
    double* F = a.fac + swz_fac_at(a, slot);
    int*    P = a.piv + swz_piv_at(a, slot);
#define SWZ_F(r, c) F[(size_t)((r) * m + (c)) * 64]
    const double* dg = a.val + (size_t)a.kdiag * a.stride;
    for (int j = 0; j < NC; ++j)
        for (int q = 0; q < NC; ++q) SWZ_F(j, q) = dg[(size_t)i * NC2 + j * NC + q];
    int at = 1;
    for (int l = 0; l < a.nneigh; ++l) {
        const int p = nb[l];
        if (p < 0) continue;
        const int r0 = at * NC;
        for (int j = 0; j < NC; ++j)
            for (int q = 0; q < NC; ++q) SWZ_F(r0 + j, r0 + q) = dg[(size_t)p * NC2 + j * NC + q];
        for (int kb = 0; kb < a.nb1; ++kb) {
            const int off = a.offs[kb];
            if (off == 0) continue;   // (the diagonal is one of the walked bands)
            const double* band = a.val + (size_t)kb * a.stride;
            if (off == p - i)         // A(i, p)
                for (int j = 0; j < NC; ++j)
                    for (int q = 0; q < NC; ++q) SWZ_F(j, r0 + q) = band[(size_t)i * NC2 + j * NC + q];
            if (off == i - p)         // A(p, i)
                for (int j = 0; j < NC; ++j)
                    for (int q = 0; q < NC; ++q) SWZ_F(r0 + j, q) = band[(size_t)p * NC2 + j * NC + q];
        }
        ++at;
    }
    bool swapped = false, stopped = false;
    for (int c = 0; c < m; ++c) {
        int    pk = c;
        double mx = fabs(SWZ_F(c, c));
        for (int j = c + 1; j < m; ++j) {
            const double v = fabs(SWZ_F(j, c));
            if (mx < v) { mx = v; pk = j; }
        }
        P[(size_t)c * 64] = pk;
        if (pk != c) {
            swapped = true;
            for (int j = 0; j < m; ++j) { const double v = SWZ_F(c, j); SWZ_F(c, j) = SWZ_F(pk, j); SWZ_F(pk, j) = v; }
        }
        const double d = SWZ_F(c, c);
        if (fabs(d) < 1e-20) { stopped = true; break; }
        for (int r = c + 1; r < m; ++r) SWZ_F(r, c) = SWZ_F(r, c) / d;
        for (int r = c + 1; r < m; ++r) {
            const double lrc = SWZ_F(r, c);
            for (int j = c + 1; j < m; ++j) SWZ_F(r, j) = SWZ_F(r, j) - lrc * SWZ_F(c, j);
        }
    }
#undef SWZ_F
    if (swapped) atomicAdd(a.count, 1u);
    if (stopped) atomicAdd(a.count + 1, 1u);
}

// the visits list[first .. first + count) of one level, in place.  W lanes per visit (W = 8, 16, 32 or 64 >= the largest m), lane = (visit, patch
// row), 64 / W visits per wavefront, one wavefront per workgroup (__syncthreads() is a wavefront barrier here).  Dynamic LDS: the factors of the
// wavefront's visits (64 W doubles), their vectors (64 doubles), members and pivots (64 ints each).
template <int NC, int NB1, int W>
__global__ __launch_bounds__(64) void k_str_swz_level(const StrSwzArgs a, int first, int count)
{
    constexpr int VPW = 64 / W;
    extern __shared__ double s_swz[];
    const int lane = (int)threadIdx.x, g = lane / W, r = lane - g * W;
    double* sF = s_swz + (size_t)g * W * W;                  // the visit's factor, row-major with stride m
    double* sx = s_swz + (size_t)64 * W + g * W;             // its vector
    int*    smem = reinterpret_cast<int*>(s_swz + (size_t)64 * W + 64) + g * W;   // its members
    int*    sP = smem + 64;                                  // its pivots
    const long long t = (long long)blockIdx.x * VPW + g;
    const bool vis = t < count;
    const int slot = vis ? first + (int)t : first, i = a.list[slot];
    const int* nb = a.neigh + (size_t)i * a.nneigh;
    // the members: entry 0 is the centre, entry l >= 1 neighbour l - 1; the absent ones are squeezed out with a ballot
    const unsigned long long grp = W == 64 ? ~0ull : ((1ull << (W & 63)) - 1ull) << (g * W);
    int k = 0;
    for (int base = 0; base <= a.nneigh; base += W) {
        const int l = base + r;
        const int cand = l == 0 ? i : l <= a.nneigh ? nb[l - 1] : -1;
        const unsigned long long mine = __ballot(cand >= 0) & grp;
        if (cand >= 0) smem[k + __popcll(mine & ((1ull << lane) - 1ull))] = cand;
        k += __popcll(mine);
    }
    const int m = k * NC, mm = m * m;
    const bool act = vis && r < m;
    // stage the factor and the pivots (the loads of a batch are in flight together)
    const double* F = a.fac + swz_fac_at(a, slot);
    for (int e0 = r; e0 < mm; e0 += 8 * W) {
        double tmp[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) tmp[q] = e0 + q * W < mm ? F[(size_t)(e0 + q * W) * 64] : 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) if (e0 + q * W < mm) sF[e0 + q * W] = tmp[q];
    }
    if (r < m) sP[r] = a.piv[swz_piv_at(a, slot) + (size_t)r * 64];
    __syncthreads();
    // the residual row of this lane, all rows before u changes
    const int am = r / NC, j = r - am * NC;
    double v = 0.0;
    if (act) {
        v = swz_resid_row<NC, NB1>(a, smem[am], j);
        // the interchanges b[k] <-> b[pivot[k]], k ascending (pivot[k] >= k, so they can all be applied before the substitution): where this row ends up
        int pos = r;
        for (int c = 0; c < m; ++c) { const int pk = sP[c]; pos = pos == c ? pk : pos == pk ? c : pos; }
        sx[pos] = v;
    }
    __syncthreads();
    if (act) v = sx[r];
    // L y = P b column by column: when column c is taken, row c is final; every row subtracts its terms with c ascending
    for (int c = 0; c + 1 < a.ms; ++c) {
        const double xc = __shfl(v, g * W + c);
        if (act && r > c) v = v - xc * sF[r * m + c];
    }
    if (act) sx[r] = v;
    __syncthreads();
    // U x = y: row k takes the terms i = k + 1 .. m - 1 ascending and cannot start before x[k + 1] is final: a serial chain
    for (int kk = a.ms - 1; kk >= 0; --kk) {
        if (act && r == kk) {
            const double* row = sF + kk * m;
            double x = sx[kk];
            for (int c = kk + 1; c < m; ++c) x = x - sx[c] * row[c];
            sx[kk] = x / row[kk];
        }
        __syncthreads();
    }
    // u[member] += e in member order: a point named more than once takes its corrections in that order, all from the lane of its first entry
    if (act) {
        const int p = smem[am];
        bool firstocc = true;
        for (int a2 = 0; a2 < am; ++a2) firstocc = firstocc && smem[a2] != p;
        if (firstocc) {
            double* up = a.u + (size_t)p * NC + j;
            double val = *up + sx[r];
            for (int a2 = am + 1; a2 < k; ++a2)
                if (smem[a2] == p) val = val + sx[a2 * NC + j];
            *up = val;
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
// everything the host decides before a device is touched: the checked neighbour set, the patch sizes, the visits and their levels
struct StrSwzPlan {
    int ngrid = 0, nc = 0, nneigh = 0, ms = 0;
    bool bad_matrix = false;
    std::vector<int> neigh;       // ngrid x nneigh
    std::vector<int> msize;       // m of every point's patch
    std::vector<int> seq, lev;    // the visits in the reference's order and the level of each
    std::vector<int> list;        // the visits sorted stably by level
    std::vector<int> lvl_first;   // the slice of every level in `list` (levels + 1 entries)
    int levels = 0, widest = 0;
};

// level of every visit (header, str_visit_levels); returns the number of levels
static int str_swz_levels(const dSTRmat* A, const StrSwzPlan& P, std::vector<int>& lev)
{
    const int ngrid = P.ngrid, nc2 = P.nc * P.nc, nband = A->nband;
    // the points every row has a term to whose coefficient block is not all 0.0
    std::vector<int> rd((size_t)std::max(ngrid, 1) * (size_t)std::max(nband, 1)), nrd((size_t)std::max(ngrid, 1), 0);
    for (int bnd = 0; bnd < nband; ++bnd)
        for (int i = 0; i < ngrid; ++i) {
            const double* c = str_block(A, bnd, i);
            if (c && !str_block_is_zero(c, nc2)) rd[(size_t)i * nband + nrd[(size_t)i]++] = i + A->offsets[bnd];
        }
    auto members = [&](size_t v, auto&& f) {
        const int i = P.seq[v];
        f(i);
        for (int l = 0; l < P.nneigh; ++l)
            if (P.neigh[(size_t)i * P.nneigh + l] >= 0) f(P.neigh[(size_t)i * P.nneigh + l]);
    };
    auto reads = [&](size_t v, auto&& f) {
        members(v, [&](int p) {
            f(p);
            for (int q = 0; q < nrd[(size_t)p]; ++q) f(rd[(size_t)p * nband + q]);
        });
    };
    return str_visit_levels(ngrid, P.seq.size(), members, reads, lev);
}

// Fills P.  fn: refusals are reported under this name.  with_levels false: the visits keep their order in one slice (factorisation only).
// Negative: refused (P.bad_matrix: a matrix the library refuses, as opposed to a refused neighbour set or order).  Pure host code.
static int str_swz_plan(const char* fn, const dSTRmat* A, const ivector* neigh, const ivector* order, bool with_levels, StrSwzPlan& P)
{
    if (str_plan(A, nullptr) < 0 || (long long)A->ngrid * A->nc * A->nc > 0x7fffffffLL) { P.bad_matrix = true; return ERROR_INPUT_PAR; }
    const int ngrid = A->ngrid, nc = A->nc;
    P.ngrid = ngrid; P.nc = nc;
    if (neigh && neigh->row != 0) {
        if (neigh->row < 0 || !neigh->val || ngrid <= 0 || neigh->row % ngrid) {
            std::fprintf(stderr, "### ERROR: %s: neigh needs a multiple of ngrid = %d entries (it has %d)\n", fn, ngrid, neigh->row);
            return ERROR_INPUT_PAR;
        }
        P.nneigh = neigh->row / ngrid;
        P.neigh.assign(neigh->val, neigh->val + neigh->row);
        for (int q = 0; q < neigh->row; ++q)
            if (P.neigh[(size_t)q] >= ngrid) {
                std::fprintf(stderr, "### ERROR: %s: neighbour %d of grid point %d is %d, outside 0 .. %d\n", fn, q % P.nneigh, q / P.nneigh, P.neigh[(size_t)q], ngrid - 1);
                return ERROR_INPUT_PAR;
            }
    }
    P.msize.assign((size_t)std::max(ngrid, 1), nc);
    P.ms = ngrid > 0 ? nc : 0;
    for (int i = 0; i < ngrid; ++i) {
        int k = 1;
        for (int l = 0; l < P.nneigh; ++l) k += P.neigh[(size_t)i * P.nneigh + l] >= 0 ? 1 : 0;
        if ((long long)k * nc > STR_SWZ_MAX_M) {
            std::fprintf(stderr, "### ERROR: %s: the patch of grid point %d has %d x %d rows, more than the %d this library serves\n", fn, i, k, nc, STR_SWZ_MAX_M);
            return ERROR_INPUT_PAR;
        }
        P.msize[(size_t)i] = k * nc;
        P.ms = std::max(P.ms, k * nc);
    }
    if (order) {
        if (order->row < ngrid || (ngrid > 0 && !order->val)) {
            std::fprintf(stderr, "### ERROR: %s: the order needs ngrid = %d entries (it has %d)\n", fn, ngrid, order->row);
            return ERROR_INPUT_PAR;
        }
        for (int q = 0; q < ngrid; ++q)
            if (order->val[q] < 0 || order->val[q] >= ngrid) {
                std::fprintf(stderr, "### ERROR: %s: entry %d of the order is %d, outside 0 .. %d\n", fn, q, order->val[q], ngrid - 1);
                return ERROR_INPUT_PAR;
            }
        P.seq.assign(order->val, order->val + ngrid);
    } else {
        P.seq.resize((size_t)ngrid);
        for (int i = 0; i < ngrid; ++i) P.seq[(size_t)i] = i;
    }
    if (with_levels) P.levels = str_swz_levels(A, P, P.lev);
    else { P.lev.assign(P.seq.size(), 0); P.levels = P.seq.empty() ? 0 : 1; }
    str_bucket_by_level(P.seq, P.lev, P.levels, P.lvl_first, P.list, &P.widest);
    return FASP_SUCCESS;
}

// Checks a caller's factors against the patches of P: the row fields, the pivots (k <= pivot[k] < m: what a finished factorisation leaves; a
// patch that stopped leaves zeros behind its last pivot), no 0.0 on U's diagonal.  Refused with a message under fn.
static int str_swz_check_factors(const char* fn, const StrSwzPlan& P, const dvector* diaginv, const ivector* pivot)
{
    if (!diaginv || !pivot) { std::fprintf(stderr, "### ERROR: %s: diaginv or pivot is NULL\n", fn); return ERROR_INPUT_PAR; }
    for (int i = 0; i < P.ngrid; ++i) {
        const int m = P.msize[(size_t)i];
        if (diaginv[i].row != m * m || pivot[i].row != m || !diaginv[i].val || !pivot[i].val) {
            std::fprintf(stderr, "### ERROR: %s: the factor of grid point %d does not fit its patch of %d rows (diaginv.row %d, pivot.row %d)\n", fn, i, m, diaginv[i].row, pivot[i].row);
            return ERROR_INPUT_PAR;
        }
        for (int k = 0; k < m; ++k) {
            if (pivot[i].val[k] < k || pivot[i].val[k] >= m) {
                std::fprintf(stderr, "### ERROR: %s: pivot %d of grid point %d is %d, outside %d .. %d (a factorisation that stopped?)\n", fn, k, i, pivot[i].val[k], k, m - 1);
                return ERROR_INPUT_PAR;
            }
            if (diaginv[i].val[(size_t)k * m + k] == 0.0) {
                std::fprintf(stderr, "### ERROR: %s: the factor of grid point %d has 0.0 on U's diagonal (row %d)\n", fn, i, k);
                return ERROR_INPUT_PAR;
            }
        }
    }
    return FASP_SUCCESS;
}

// a block Gauss-Seidel smoother resident on the device: band layout, neigh, visit list, factors and pivots; built once, applied many times
struct StrSwzDev {
    StrSwzPlan P;
    TmpSTR     M;
    int        kdiag = 0;
    int*       neigh = nullptr, *list = nullptr, *piv = nullptr;
    double*    fac = nullptr, *b = nullptr, *u = nullptr;
    unsigned*  count = nullptr;
    size_t     nslot64 = 0, nfac = 0, npiv = 0;
    DevPool    pool;
    bool       ok = false;
    int        st = ERROR_ALLOC_MEM;       // why not ok
    int        nswap = 0, nstopped = 0;    // patches with a row interchange, patches that stopped (device factorisation)
    int        launches = 0;
    // diaginv / pivot: a caller's factors (checked by str_swz_check_factors), repacked; both NULL: factored here, on the device
    StrSwzDev(const dSTRmat* A, StrSwzPlan&& plan, const dvector* diaginv, const ivector* pivot) : P(std::move(plan)), M(A)
    {
        if (!M.ok) { st = M.form < 0 ? ERROR_INPUT_PAR : g_ctx.ready ? ERROR_ALLOC_MEM : ERROR_MISC; return; }
        const size_t n = (size_t)P.ngrid * P.nc, nslots = P.list.size(), ms2 = (size_t)P.ms * P.ms;
        nslot64 = (nslots + 63) / 64 * 64;
        if (ms2 && nslot64 > (size_t)0x7fffffffffffLL / (8 * ms2)) return;
        nfac = nslot64 * ms2; npiv = nslot64 * (size_t)P.ms;
        for (int k = 0; k < M.nb; ++k) if (M.off[(size_t)k] == 0) kdiag = k;
        if (!pool.get(&neigh, P.neigh.size()) || !pool.get(&list, nslots) || !pool.get(&piv, npiv) || !pool.get(&fac, nfac) || !pool.get(&b, n) ||
            !pool.get(&u, n) || !pool.get(&count, 4))
            return;
        if (!P.neigh.empty() && hipMemcpy(neigh, P.neigh.data(), sizeof(int) * P.neigh.size(), hipMemcpyHostToDevice) != hipSuccess) return;
        if (nslots && hipMemcpy(list, P.list.data(), sizeof(int) * nslots, hipMemcpyHostToDevice) != hipSuccess) return;
        if (hipMemset(count, 0, sizeof(unsigned) * 4) != hipSuccess) return;
        if (diaginv) {
            std::vector<double> hf(std::max<size_t>(nfac, 1), 0.0);
            std::vector<int> hp(std::max<size_t>(npiv, 1), 0);
            for (size_t s = 0; s < nslots; ++s) {
                const int i = P.list[s], m = P.msize[(size_t)i];
                const size_t fb = (s >> 6) * ms2 * 64 + (s & 63), pb = (s >> 6) * (size_t)P.ms * 64 + (s & 63);
                for (int e = 0; e < m * m; ++e) hf[fb + (size_t)e * 64] = diaginv[i].val[e];
                for (int k = 0; k < m; ++k) hp[pb + (size_t)k * 64] = pivot[i].val[k];
            }
            if (nfac && hipMemcpy(fac, hf.data(), sizeof(double) * nfac, hipMemcpyHostToDevice) != hipSuccess) return;
            if (npiv && hipMemcpy(piv, hp.data(), sizeof(int) * npiv, hipMemcpyHostToDevice) != hipSuccess) return;
        } else if (factor() < 0) { st = ERROR_MISC; return; }
        ok = true; st = FASP_SUCCESS;
    }

    StrSwzArgs args(const double* rhs, double* sol) const
    {
        StrSwzArgs a{};
        a.val = M.val; a.stride = M.stride; a.offs = M.offs; a.nb1 = M.nb; a.kdiag = kdiag; a.form = M.form; a.ngrid = P.ngrid;
        a.neigh = neigh; a.nneigh = P.nneigh; a.list = list; a.fac = fac; a.piv = piv; a.ms = P.ms; a.b = rhs; a.u = sol; a.count = count;
        return a;
    }
    template <int NC> void factor_nc(const StrSwzArgs& a, int nslots)
    {
        hipLaunchKernelGGL((k_str_swz_factor<NC>), dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, g_ctx.stream, a, nslots);
    }
    // assemble and factor every patch on the device (asynchronous); counts() afterwards
    int launch_factor()
    {
        const int nslots = (int)P.list.size();
        if (nslots <= 0) return FASP_SUCCESS;
        HIPCK(hipMemsetAsync(fac, 0, sizeof(double) * nfac, g_ctx.stream));
        HIPCK(hipMemsetAsync(piv, 0, sizeof(int) * npiv, g_ctx.stream));
        HIPCK(hipMemsetAsync(count, 0, sizeof(unsigned) * 4, g_ctx.stream));
        const StrSwzArgs a = args(nullptr, nullptr);
        if (str_for_nc(P.nc, [&](auto NC) { factor_nc<NC()>(a, nslots); return 0; }) < 0) return ERROR_INPUT_PAR;
        return hipGetLastError() == hipSuccess ? FASP_SUCCESS : ERROR_MISC;
    }
    int counts()
    {
        unsigned hc[4] = {};
        HIPCK(hipStreamSynchronize(g_ctx.stream));
        HIPCK(hipMemcpy(hc, count, sizeof(hc), hipMemcpyDeviceToHost));
        nswap = (int)hc[0]; nstopped = (int)hc[1];
        return FASP_SUCCESS;
    }
    int factor() { const int s = launch_factor(); return s < 0 ? s : counts(); }

    template <int NC, int W> void sweep_w(const StrSwzArgs& a)
    {
        constexpr int VPW = 64 / W;
        const size_t lds = sizeof(double) * (64 * (size_t)W + 64) + sizeof(int) * 128;
        for (size_t l = 0; l + 1 < P.lvl_first.size(); ++l) {
            const int first = P.lvl_first[l], cnt = P.lvl_first[l + 1] - first;
            const dim3 grid((unsigned)((cnt + VPW - 1) / VPW)), block(64);
            if (M.form != STR_G && M.nb == 7) hipLaunchKernelGGL((k_str_swz_level<NC, 7, W>), grid, block, lds, g_ctx.stream, a, first, cnt);
            else if (M.form != STR_G && M.nb == 5) hipLaunchKernelGGL((k_str_swz_level<NC, 5, W>), grid, block, lds, g_ctx.stream, a, first, cnt);
            else hipLaunchKernelGGL((k_str_swz_level<NC, 0, W>), grid, block, lds, g_ctx.stream, a, first, cnt);
            ++launches;
        }
    }
    template <int NC> void sweep_nc(const StrSwzArgs& a)
    {
        if (P.ms <= 8) { if (NC <= 8) sweep_w<NC, 8>(a); }
        else if (P.ms <= 16) sweep_w<NC, 16>(a);
        else if (P.ms <= 32) sweep_w<NC, 32>(a);
        else sweep_w<NC, 64>(a);
    }
    // one sweep on device vectors, in place in sol
    int sweep(const double* rhs, double* sol)
    {
        if (P.ngrid <= 0) return FASP_SUCCESS;
        const StrSwzArgs a = args(rhs, sol);
        launches = 0;
        if (str_for_nc(P.nc, [&](auto NC) { sweep_nc<NC()>(a); return 0; }) < 0) return ERROR_INPUT_PAR;
        return hipGetLastError() == hipSuccess ? FASP_SUCCESS : ERROR_MISC;
    }
    // z = 0, one sweep with b = r: fasp_precond_dstr_blockgs on device vectors
    int precond(const double* r, double* z)
    {
        HIPCK(hipMemsetAsync(z, 0, sizeof(double) * (size_t)P.ngrid * P.nc, g_ctx.stream));
        return sweep(r, z);
    }
    // what a sweep moves at least: per visit its factor and pivots, the matrix rows, b and u of its members, u written
    double bytes() const
    {
        double s = 0.0;
        for (int i : P.list) { const double m = P.msize[(size_t)i]; s += 8.0 * m * m + 4.0 * m + 8.0 * m * ((double)M.nb * P.nc + 3.0) + 4.0 * (P.nneigh + 1); }
        return s;
    }
};

// factors that live on the device only (fasp_solver_dstr_krylov_blockgs): found through the address of the precond_data_str that stands for them
static std::vector<std::pair<const void*, StrSwzDev*>> g_swz_resident;
static StrSwzDev* str_swz_resident(const void* data)
{
    for (const auto& e : g_swz_resident) if (e.first == data) return e.second;
    return nullptr;
}
}  // namespace fasp_str
