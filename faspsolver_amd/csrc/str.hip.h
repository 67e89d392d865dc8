// str.hip.h -- structured (STR, dSTRmat) band operator: y = alpha A x + y without column indices.
// Part of the single translation unit solver.hip (included there after bsr.hip.h; not a stand-alone header).
//
// Reference: BlaSpmvSTR.c.  The reference has four arithmetic forms, chosen by (nband, nc, offsets); each of them is
// reproduced bit for bit by ONE kernel, k_str_band<NC, FORM, NB1, YIN>, that walks a row's bands in the order the form
// prescribes:
//   S  nc = 1, canonical             t = first existing product, t += the next ones; y = y + alpha t        (:420, :1121)
//   B  nc = 3, 5, canonical          per band: s = a_p0 x_0; s += a_pq x_q; y_p = y_p + alpha s             (:241, :265)
//   N  nc = 2, 4, 6, 7, canonical    per band, per q: y_p = y_p + (alpha a_pq) x_q                          (:294)
//   G  everything else               y_p = y_p (1/alpha); diagonal, then bands in storage order: y_p += a_pq x_q; y_p = y_p alpha  (:1760)
// "canonical": the offsets are the set {+-1, +-nx, +-nxy} (nband 6) or {+-1, +-nline} (nband 4; nline = nx, or ny when nx == 1)
// and the reference's row segments do not overlap (ngrid >= 2 nxy, resp. 2 nline); the walk is then by ascending offset,
// the diagonal between -1 and +1.  A band term exists for row i iff 0 <= i + offset < ngrid.
//
// Device layout: the walked bands (the diagonal is one of them) in a StrBands store (str_common.hip.h).  Lane = scalar row r = i * nc + p:
// the nc values of block row p are the nc doubles at r * nc, so a wave's loads of a band cover 64 * nc * 8 contiguous bytes; x is read as
// the contiguous run x[(i + offset) * nc ...], y is read and written once.  No column indices, no atomics, no pass per band.

namespace fasp_str {

enum StrForm : int { STR_S = 0, STR_B = 1, STR_N = 2, STR_G = 3 };

// Which form the product of A takes, and the walk: walk[k] = -1 for the diagonal, b for offdiag[b] (as str_block names them);
// bands that have no term at all (|offset| >= ngrid) are left out.  Negative: a matrix the library refuses (ERROR_INPUT_PAR).  Pure host code.
static int str_plan(const dSTRmat* A, std::vector<int>* walk)
{
    if (!A || A->nc < 1 || A->nc > 7 || A->nband < 0 || A->ngrid < 0) return ERROR_INPUT_PAR;
    if ((long long)A->ngrid * A->nc > 0x7fffffffLL) return ERROR_INPUT_PAR;
    if (A->ngrid > 0 && !A->diag) return ERROR_INPUT_PAR;
    if (A->nband > 0 && (!A->offsets || !A->offdiag)) return ERROR_INPUT_PAR;
    const int nband = A->nband, ngrid = A->ngrid;
    std::vector<int> sorted(A->offsets, A->offsets + nband);
    std::sort(sorted.begin(), sorted.end());
    for (int b = 0; b < nband; ++b) {
        if (sorted[b] == 0 || (b > 0 && sorted[b] == sorted[b - 1])) return ERROR_INPUT_PAR;
        const long long len = (long long)ngrid - std::llabs((long long)A->offsets[b]);
        if (len > 0 && !A->offdiag[b]) return ERROR_INPUT_PAR;
    }
    bool canonical = false;
    if (nband == 6) {
        const int nx = A->nx, nxy = A->nxy;
        canonical = nx > 1 && nxy > nx && (long long)ngrid >= 2LL * nxy && sorted[0] == -nxy && sorted[1] == -nx &&
                    sorted[2] == -1 && sorted[3] == 1 && sorted[4] == nx && sorted[5] == nxy;
    } else if (nband == 4) {
        const int nline = A->nx == 1 ? A->ny : A->nx;
        canonical = nline > 1 && (long long)ngrid >= 2LL * nline && sorted[0] == -nline && sorted[1] == -1 && sorted[2] == 1 &&
                    sorted[3] == nline;
    }
    if (walk) {
        walk->clear();
        if (canonical) {   // ascending offsets, the diagonal in the middle; every band has terms (ngrid >= 2 |offset|)
            for (int k = 0; k < nband; ++k) {
                if (k == nband / 2) walk->push_back(-1);
                for (int b = 0; b < nband; ++b)
                    if (A->offsets[b] == sorted[k]) walk->push_back(b);
            }
        } else {
            walk->push_back(-1);
            for (int b = 0; b < nband; ++b)
                if (std::llabs((long long)A->offsets[b]) < (long long)ngrid) walk->push_back(b);
        }
    }
    if (!canonical) return STR_G;
    return A->nc == 1 ? STR_S : (A->nc == 3 || A->nc == 5) ? STR_B : STR_N;
}

struct StrArgs {
    int           ngrid;    // grid points
    int           n;        // scalar rows, ngrid * nc
    int           nb1;      // walked bands, the diagonal included
    int           per_xcd;  // row tiles of an XCD's slab
    int           ntiles;   // row tiles of BLOCK rows
    const int*    offs;     // nb1 offsets in walk order (0: the diagonal)
    const double* val;      // nb1 bands of `stride` doubles
    size_t        stride;
    const double* x;
    const double* yin;      // YIN: the y the product is added to (may be yout)
    double*       yout;
    double        alpha, beta;   // beta = 1 / alpha (form G)
};

// NB1 > 0: the number of walked bands, known at compile time (7 and 5: the canonical forms), so that the walk unrolls and the loads of
// all bands are in flight together; NB1 == 0: a.nb1 bands.  Loads never depend on whether the term exists (the matrix slot of a
// missing term is a stored zero of the padded band, its x index is replaced by the row's own), the arithmetic does.
// The products and sums below must stay separate operations (-ffp-contract=off: the reference build has no fused multiply-add).
template <int NC, int FORM, int NB1, bool YIN>
__global__ __launch_bounds__(BLOCK) void k_str_band(const StrArgs a)
{
    // an XCD's workgroups (b, b + 8, ...) take one contiguous slab of row tiles: the +-nx / +-nxy neighbours of a slab's rows
    // lie in the same slab but for 2 nxy rows at its two ends, so x is fetched into one L2 only
    const int tile = (int)(blockIdx.x & 7u) * a.per_xcd + (int)(blockIdx.x >> 3);
    if (tile >= a.ntiles) return;
    const long long rr = (long long)tile * BLOCK + threadIdx.x;
    if (rr >= a.n) return;
    const int r = (int)rr, i = r / NC;
    const int nb1 = NB1 > 0 ? NB1 : a.nb1;
    double y = YIN ? a.yin[r] : 0.0;
    if (FORM == STR_G) y = y * a.beta;
    double t = 0.0;
    bool   have = false;
    const double* __restrict__ ap = a.val + (size_t)r * NC;
#pragma unroll
    for (int k = 0; k < nb1; ++k, ap += a.stride) {
        const int  j = i + a.offs[k];
        const bool ex = (unsigned)j < (unsigned)a.ngrid;
        const double* __restrict__ xp = a.x + (size_t)(ex ? j : i) * NC;
        double av[NC], xv[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) { av[q] = __builtin_nontemporal_load(ap + q); xv[q] = xp[q]; }
        if (!ex) continue;
        if (FORM == STR_S) {
            const double p = av[0] * xv[0];
            t = have ? t + p : p;
            have = true;
        } else if (FORM == STR_B) {
            double s = av[0] * xv[0];
#pragma unroll
            for (int q = 1; q < NC; ++q) s = s + av[q] * xv[q];
            y = y + a.alpha * s;
        } else if (FORM == STR_N) {
#pragma unroll
            for (int q = 0; q < NC; ++q) y = y + (a.alpha * av[q]) * xv[q];
        } else {
#pragma unroll
            for (int q = 0; q < NC; ++q) y = y + av[q] * xv[q];
        }
    }
    if (FORM == STR_S) y = y + a.alpha * t;
    if (FORM == STR_G) y = y * a.alpha;
    a.yout[r] = y;
}

// fasp_precond_dstr_diag (PreSTR.c:44): z_i = Dinv_i r_i as fasp_blas_smat_mxv (BlaSmallMat.c:238) sums it: left to right from the first
// product for nc = 2, 3, 4, 5, 7, from 0.0 for the general text (nc = 1, 6) -- the two differ in the sign of a zero only
__global__ __launch_bounds__(BLOCK) void k_str_dinv_apply(int n, int nc, const double* __restrict__ dinv, const double* __restrict__ b,
                                                           double* __restrict__ z)
{
    const bool from_zero = nc == 1 || nc == 6;
    for (int row = blockIdx.x * BLOCK + threadIdx.x; row < n; row += gridDim.x * BLOCK) {
        const int     br = row / nc, p = row - br * nc;
        const double* D = dinv + (size_t)br * nc * nc + p * nc;
        const double* bb = b + (size_t)br * nc;
        double s = D[0] * bb[0];
        if (from_zero) s = 0.0 + s;
        for (int c = 1; c < nc; ++c) s = s + D[c] * bb[c];
        z[row] = s;
    }
}

// device copy of a dSTRmat for the length of a call: the bands of str_plan's walk, the form, and the offsets where the kernel reads them
struct TmpSTR : StrBands {
    int     ngrid = 0, nc = 0, n = 0, form = ERROR_INPUT_PAR;
    int*    offs = nullptr;
    DevPool pool;
    bool    ok = false;
    explicit TmpSTR(const dSTRmat* A)
    {
        std::vector<int> walk;
        form = str_plan(A, &walk);
        if (form < 0 || ctx_init() < 0) return;
        ngrid = A->ngrid; nc = A->nc; n = ngrid * nc;
        if (!init(pool, A, walk) || !pool.get(&offs, off.size())) return;
        if (hipMemcpy(offs, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice) != hipSuccess) return;
        ok = true;
    }
    // matrix bytes + x + y written (+ y read) of one product
    double bytes(bool yin) const { return 8.0 * ((double)nb * ngrid * nc * nc + (double)n * (yin ? 3 : 2)); }
};

template <int NC, int FORM, int NB1>
static void launch_str_t(const StrArgs& a)
{
    const dim3 grid((unsigned)a.per_xcd * 8u), block(BLOCK);
    if (a.yin) hipLaunchKernelGGL((k_str_band<NC, FORM, NB1, true>), grid, block, 0, g_ctx.stream, a);
    else hipLaunchKernelGGL((k_str_band<NC, FORM, NB1, false>), grid, block, 0, g_ctx.stream, a);
}
template <int NC>
static void launch_str_nc(int form, const StrArgs& a)
{
    constexpr int CF = NC == 1 ? STR_S : (NC == 3 || NC == 5) ? STR_B : STR_N;   // the canonical form of this block width
    if (form == STR_G) launch_str_t<NC, STR_G, 0>(a);
    else if (a.nb1 == 7) launch_str_t<NC, CF, 7>(a);
    else launch_str_t<NC, CF, 5>(a);
}

// yout = alpha A x + yin (yin == nullptr: + 0, the reference's mxv on a cleared y); yin may be yout.  alpha == 0 in form G
// leaves y alone, as str_spaAxpy returns at once; the other forms do their arithmetic with alpha = 0 as the reference does.
static void str_aAxpy(const TmpSTR& M, double alpha, const double* x, const double* yin, double* yout)
{
    if (M.n <= 0) return;
    if (M.form == STR_G && alpha == 0.0) {
        if (yin && yin != yout) (void)hipMemcpyAsync(yout, yin, sizeof(double) * (size_t)M.n, hipMemcpyDeviceToDevice, g_ctx.stream);
        if (!yin) (void)hipMemsetAsync(yout, 0, sizeof(double) * (size_t)M.n, g_ctx.stream);
        return;
    }
    StrArgs a{};
    a.ngrid = M.ngrid; a.n = M.n; a.nb1 = M.nb; a.offs = M.offs; a.val = M.val; a.stride = M.stride;
    a.x = x; a.yin = yin; a.yout = yout; a.alpha = alpha; a.beta = 1.0 / alpha;
    a.ntiles = (int)(((long long)M.n + BLOCK - 1) / BLOCK);
    a.per_xcd = (a.ntiles + 7) / 8;
    (void)str_for_nc(M.nc, [&](auto NC) { launch_str_nc<NC()>(M.form, a); return 0; });
}
static void str_mxv(const TmpSTR& M, const double* x, double* y) { str_aAxpy(M, 1.0, x, nullptr, y); }
// r = b; r += (-1) A x: what the reference's solvers do (fasp_darray_cp, fasp_blas_dstr_aAxpy(-1.0, ...))
static void str_resid(const TmpSTR& M, const double* x, const double* b, double* r) { str_aAxpy(M, -1.0, x, b, r); }

[[noreturn]] static void die_str(const char* fn, int form)
{
    if (form < 0)
        std::fprintf(stderr, "### ERROR: %s: not a dSTRmat this library serves (1 <= nc <= 7, nband >= 0, offsets distinct and not 0)\n", fn);
    else
        std::fprintf(stderr, "### ERROR: %s: no usable HIP device and no CPU fallback in libfasp_hip\n", fn);
    std::exit(form < 0 ? ERROR_INPUT_PAR : ERROR_MISC);
}
}  // namespace fasp_str
using namespace fasp_str;
