// ilu_setup.cpp -- incomplete LU factorisation of a CSR matrix on the host (BlaILUSetupCSR.c:40 and its three kernels, BlaILU.c),
// the ILU parameter / data helpers (AuxParam.c:595, PreDataInit.c:411 / :445, AuxMemory.c:203).  Pure host code: no GPU needed.
//
// The factor is handed out in the reference's modified sparse row (MSR) layout, entry for entry:
//   ijlu[0 .. n]       row pointers into the same arrays (ijlu[0] = n + 1), row i = [ijlu[i], ijlu[i + 1]);
//   ijlu[p], luval[p]  (p >= n + 1) column and value of an off-diagonal entry: the row's L entries first (ascending columns
//                      for ILUk; for ILUt / ILUtp the order the largest-magnitude selection leaves), then its U entries;
//   luval[i]           (i < n) the inverse of the i-th pivot.
// All three factorisations build row i from row i of A and the finished rows above it (the IKJ form of Gaussian elimination):
// the row is scattered into a dense work row, the earlier rows are eliminated in ascending order of their index, and what
// survives the row's dropping rule is gathered into the factor.  ILUk drops by level of fill, ILUt by magnitude (relative to
// the row's mean absolute value) and by count, ILUtp additionally swaps columns for a larger pivot.  The order of every
// floating-point operation and of every stored entry is the reference's, so the arrays come out equal bit for bit.
//
// ILUtp renumbers the columns of the CALLER's A->JA in place on success (the Krylov method then runs on A with permuted
// columns, the solution comes out permuted); fasp_ilu_data_free undoes it.  That is the reference's contract and is kept.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fasp_internal.h"

namespace fasp {
void ilu_register_host(ILU_data* d);   // ilu.hip.h: factors built here are kept resident on the device once used
}

namespace {

// Outcome codes of a factorisation (the reference's ierr): 0 success, -1 a work row longer than n, -2 / -3 the L / U part
// overflows the iwk entries, -4 negative fill level, -5 a zero pivot (ILUk) or an all-zero row (ILUtp).
enum { FACT_OK = 0, FACT_LONG_ROW = -1, FACT_L_FULL = -2, FACT_U_FULL = -3, FACT_BAD_LFIL = -4, FACT_ZERO = -5 };

// Partial ordering by magnitude ("quick split"): afterwards the `keep` largest |v| of v[0 .. m) occupy v[0 .. keep), the
// element at keep - 1 separating the two groups.  One pivot pass per round, pivot = first element of the open window;
// the window shrinks towards keep - 1 until the pivot lands there.  keep outside [1, m]: nothing moves.
void split_by_magnitude(double* v, int* idx, int m, int keep)
{
    const int target = keep - 1;
    if (target < 0 || target > m - 1) return;
    int lo = 0, hi = m - 1;
    for (;;) {
        const double key = std::fabs(v[lo]);
        int mid = lo;
        for (int j = lo + 1; j <= hi; ++j)
            if (std::fabs(v[j]) > key) {
                ++mid;
                std::swap(v[mid], v[j]);
                std::swap(idx[mid], idx[j]);
            }
        std::swap(v[mid], v[lo]);
        std::swap(idx[mid], idx[lo]);
        if (mid == target) return;
        if (mid > target) hi = mid - 1;
        else lo = mid + 1;
    }
}

// The dense work row of step i.  Lower part: lc / lv (/ llev) in insertion order; upper part: uc / uv (/ ulev) with the
// pivot at index 0.  slot[c] = 1 + index of column c in its part (0: not present); columns < i live in the lower part.
struct WorkRow {
    std::vector<int>    lc, uc, llev, ulev, slot;
    std::vector<double> lv, uv;
    explicit WorkRow(int n) : slot((size_t)n, 0) {}
    void start(int i)
    {
        lc.clear(); lv.clear(); llev.clear();
        uc.assign(1, i); uv.assign(1, 0.0); ulev.assign(1, 0);
        slot[(size_t)i] = 1;
    }
    int add_lower(int c, double v, int lev) { lc.push_back(c); lv.push_back(v); llev.push_back(lev); slot[(size_t)c] = (int)lc.size(); return (int)lc.size(); }
    int add_upper(int c, double v, int lev) { uc.push_back(c); uv.push_back(v); ulev.push_back(lev); slot[(size_t)c] = (int)uc.size(); return (int)uc.size(); }
    // bring the smallest remaining lower column to position k (the first one of equal columns wins); returns that column
    int next_pivot_row(int k)
    {
        int best = k;
        for (int j = k + 1; j < (int)lc.size(); ++j)
            if (lc[(size_t)j] < lc[(size_t)best]) best = j;
        const int c = lc[(size_t)best];
        if (best != k) {
            const int other = lc[(size_t)k];
            std::swap(lc[(size_t)k], lc[(size_t)best]);
            std::swap(lv[(size_t)k], lv[(size_t)best]);
            std::swap(llev[(size_t)k], llev[(size_t)best]);
            slot[(size_t)other] = best + 1;
        }
        slot[(size_t)c] = 0;
        return c;
    }
    void clear_upper_slots() { for (int c : uc) slot[(size_t)c] = 0; }
};

// The MSR factor being written.  pos: next free entry.  ustart[i]: first U entry of row i.
struct Factor {
    int     n, iwk, pos;
    int*    ijlu;
    double* luval;
    std::vector<int> ustart, ulevel;   // ulevel: fill level of each stored U entry (ILUk only)
    Factor(int n_, int iwk_, int* ij, double* lu, bool levels) : n(n_), iwk(iwk_), pos(n_ + 1), ijlu(ij), luval(lu), ustart((size_t)n_, 0)
    {
        if (levels) ulevel.assign((size_t)std::max(iwk_, 1), 0);
        ijlu[0] = n_ + 1;
    }
};

// ---- ILU(k): level-of-fill dropping ----
int factor_iluk(const dCSRmat* A, int n, int lfil, Factor& F)
{
    if (lfil < 0) return FACT_BAD_LFIL;
    WorkRow W(n);
    for (int i = 0; i < n; ++i) {
        W.start(i);
        for (int k = A->IA[i]; k < A->IA[i + 1]; ++k) {
            const int c = A->JA[k];
            const double v = A->val[k];
            if (v == 0.0) continue;   // explicit zeros are not part of the pattern
            if (c < i) W.add_lower(c, v, 0);
            else if (c == i) { W.uv[0] = v; W.ulev[0] = 0; }
            else W.add_upper(c, v, 0);
        }
        for (int k = 0; k < (int)W.lc.size(); ++k) {
            const int r = W.next_pivot_row(k);
            const double mult = W.lv[(size_t)k] * F.luval[r];
            const int lev = W.llev[(size_t)k];
            if (lev > lfil) continue;
            for (int p = F.ustart[(size_t)r]; p < F.ijlu[r + 1]; ++p) {
                const double s = mult * F.luval[p];
                const int c = F.ijlu[p];
                const int at = W.slot[(size_t)c];
                const int flev = lev + F.ulevel[(size_t)p] + 1;
                if (c >= i) {
                    if (at == 0) {
                        if ((int)W.uc.size() + 1 > n) return FACT_LONG_ROW;
                        W.add_upper(c, -s, flev);
                    } else {
                        W.uv[(size_t)at - 1] = W.uv[(size_t)at - 1] - s;
                        W.ulev[(size_t)at - 1] = std::min(W.ulev[(size_t)at - 1], flev);
                    }
                } else {
                    if (at == 0) {
                        if ((int)W.lc.size() + 1 > n) return FACT_LONG_ROW;
                        W.add_lower(c, -s, flev);
                    } else {
                        W.lv[(size_t)at - 1] = W.lv[(size_t)at - 1] - s;
                        W.llev[(size_t)at - 1] = std::min(W.llev[(size_t)at - 1], flev);
                    }
                }
            }
            W.lv[(size_t)k] = mult;
        }
        W.clear_upper_slots();
        for (size_t k = 0; k < W.lc.size(); ++k) {
            if (F.pos >= F.iwk) return FACT_L_FULL;
            if (W.llev[k] <= lfil) { F.luval[F.pos] = W.lv[k]; F.ijlu[F.pos] = W.lc[k]; ++F.pos; }
        }
        F.ustart[(size_t)i] = F.pos;
        for (size_t k = 1; k < W.uc.size(); ++k) {
            if (F.pos >= F.iwk) return FACT_U_FULL;
            if (W.ulev[k] <= lfil) { F.ijlu[F.pos] = W.uc[k]; F.luval[F.pos] = W.uv[k]; F.ulevel[(size_t)F.pos] = W.ulev[k]; ++F.pos; }
        }
        if (W.uv[0] == 0.0) return FACT_ZERO;
        F.luval[i] = 1.0 / W.uv[0];
        F.ijlu[i + 1] = F.pos;
    }
    return FACT_OK;
}

// ---- ILUt (perm == nullptr) and ILUtp: threshold + count dropping, ILUtp with column pivoting ----
// perm: old_of_new / new_of_old column numbering (0-based), updated as pivots are chosen.  For ILUtp the factor stores
// ORIGINAL column numbers while it is built (the numbering keeps changing) and is renumbered once at the end.
int factor_ilut(const dCSRmat* A, int n, int lfil, double droptol, double permtol, int mbloc, Factor& F,
                std::vector<int>* old_of_new, std::vector<int>* new_of_old)
{
    if (lfil < 0) return FACT_BAD_LFIL;
    const bool pivoting = old_of_new != nullptr;
    std::vector<double> rowtol;
    if (!pivoting) {   // ILUt: every row's threshold up front (an empty row gives 0 / 0, as in the reference)
        rowtol.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            double s = 0.0;
            for (int k = A->IA[i]; k < A->IA[i + 1]; ++k) s = s + std::fabs(A->val[k]);
            s = s / (double)(A->IA[i + 1] - A->IA[i]);
            rowtol[(size_t)i] = s * droptol;
        }
    }
    auto cur = [&](int c) { return pivoting ? (*new_of_old)[(size_t)c] : c; };   // current number of an original column
    WorkRow W(n);
    for (int i = 0; i < n; ++i) {
        double rownorm = 0.0;   // ILUtp: mean |a_ij| of the row
        if (pivoting) {
            for (int k = A->IA[i]; k < A->IA[i + 1]; ++k) rownorm = rownorm + std::fabs(A->val[k]);
            if (rownorm == 0.0) return FACT_ZERO;
            rownorm = rownorm / (double)(A->IA[i + 1] - A->IA[i]);
        }
        W.start(i);
        for (int k = A->IA[i]; k < A->IA[i + 1]; ++k) {
            const int c = cur(A->JA[k]);
            const double v = A->val[k];
            if (c < i) W.add_lower(c, v, 0);
            else if (c == i) W.uv[0] = v;
            else W.add_upper(c, v, 0);
        }
        int kept = 0;   // multipliers kept so far, packed to the front of the lower part
        for (int k = 0; k < (int)W.lc.size(); ++k) {
            const int r = W.next_pivot_row(k);
            const double mult = W.lv[(size_t)k] * F.luval[r];
            if (std::fabs(mult) <= droptol) continue;
            for (int p = F.ustart[(size_t)r]; p < F.ijlu[r + 1]; ++p) {
                const double s = mult * F.luval[p];
                const int c = cur(F.ijlu[p]);
                const int at = W.slot[(size_t)c];
                if (c >= i) {
                    if (at == 0) {
                        if ((int)W.uc.size() + 1 > n) return FACT_LONG_ROW;
                        W.add_upper(c, -s, 0);
                    } else W.uv[(size_t)at - 1] = W.uv[(size_t)at - 1] - s;
                } else {
                    if (at == 0) {
                        if ((int)W.lc.size() + 1 > n) return FACT_LONG_ROW;
                        W.add_lower(c, -s, 0);
                    } else W.lv[(size_t)at - 1] = W.lv[(size_t)at - 1] - s;
                }
            }
            W.lv[(size_t)kept] = mult;
            W.lc[(size_t)kept] = r;
            ++kept;
        }
        W.clear_upper_slots();
        // L: the min(kept, lfil) largest multipliers
        const int nl = std::min(kept, lfil);
        split_by_magnitude(W.lv.data(), W.lc.data(), kept, nl);
        for (int k = 0; k < nl; ++k) {
            if (F.pos >= F.iwk) return FACT_L_FULL;
            F.luval[F.pos] = W.lv[(size_t)k];
            F.ijlu[F.pos] = pivoting ? (*old_of_new)[(size_t)W.lc[(size_t)k]] : W.lc[(size_t)k];
            ++F.pos;
        }
        F.ustart[(size_t)i] = F.pos;
        // U: drop below the row's threshold (order kept), then keep the largest
        const double utol = pivoting ? droptol * rownorm : rowtol[(size_t)i];
        int nu = 0;
        for (size_t k = 1; k < W.uc.size(); ++k)
            if (std::fabs(W.uv[k]) > utol) { ++nu; W.uv[(size_t)nu] = W.uv[k]; W.uc[(size_t)nu] = W.uc[k]; }
        const int ncut = std::min(nu + 1, lfil);   // the reference stores ncut - 1 entries of the upper part
        split_by_magnitude(W.uv.data() + 1, W.uc.data() + 1, nu, ncut);
        if (pivoting) {
            // the largest candidate among the kept ones replaces the pivot where it is permtol-times larger
            int best = 0;
            double big = std::fabs(W.uv[0]);
            const double big0 = big;
            const int i1 = i + 1;
            const int icut = i1 - 1 + mbloc - (i1 - 1) % mbloc;   // last column (1-based) of the pivot block
            for (int k = 1; k <= ncut - 1; ++k) {
                const double t = std::fabs(W.uv[(size_t)k]);
                if (t > big && t * permtol > big0 && W.uc[(size_t)k] + 1 <= icut) { best = k; big = t; }
            }
            std::swap(W.uv[0], W.uv[(size_t)best]);
            const int j = W.uc[(size_t)best];
            std::vector<int>& o = *old_of_new;
            std::vector<int>& q = *new_of_old;
            std::swap(o[(size_t)i], o[(size_t)j]);
            q[(size_t)o[(size_t)i]] = i;
            q[(size_t)o[(size_t)j]] = j;
        }
        if (ncut + F.pos + 1 > F.iwk) return FACT_U_FULL;
        for (int k = 1; k <= ncut - 1; ++k) {
            F.ijlu[F.pos] = pivoting ? (*old_of_new)[(size_t)W.uc[(size_t)k]] : W.uc[(size_t)k];
            F.luval[F.pos] = W.uv[(size_t)k];
            ++F.pos;
        }
        if (W.uv[0] == 0.0) W.uv[0] = pivoting ? (1.0e-4 + droptol) * rownorm : rowtol[(size_t)i];
        F.luval[i] = 1.0 / W.uv[0];
        F.ijlu[i + 1] = F.pos;
    }
    return FACT_OK;
}

const char* fact_message(int e)
{
    switch (e) {
        case FACT_LONG_ROW: return "a row of the factor grew beyond n entries (input matrix may be wrong)";
        case FACT_L_FULL: return "the L part does not fit in the allocated entries";
        case FACT_U_FULL: return "the U part does not fit in the allocated entries";
        case FACT_BAD_LFIL: return "negative level of fill";
        case FACT_ZERO: return "zero pivot or zero row";
        default: return "unknown";
    }
}

}  // namespace

extern "C" {

// AuxParam.c:595
void fasp_param_ilu_init(ILU_param* iluparam)
{
    if (!iluparam) return;
    iluparam->print_level = PRINT_NONE;
    iluparam->ILU_type = ILUk;
    iluparam->ILU_lfil = 2;
    iluparam->ILU_droptol = 0.001;
    iluparam->ILU_relax = 0;
    iluparam->ILU_permtol = 0.01;
}

// PreDataInit.c:411: iwk entries of ijlu / luval, nwork doubles of work, 2 row ints of iperm for ILUtp (all zeroed)
void fasp_ilu_data_create(const int iwk, const int nwork, ILU_data* iludata)
{
    iludata->ijlu = (int*)fasp_mem_calloc((unsigned)iwk, sizeof(int));
    if (iludata->type == ILUtp) iludata->iperm = (int*)fasp_mem_calloc((unsigned)iludata->row * 2, sizeof(int));
    iludata->luval = (double*)fasp_mem_calloc((unsigned)iwk, sizeof(double));
    iludata->work = (double*)fasp_mem_calloc((unsigned)nwork, sizeof(double));
}

// AuxMemory.c:203: the application needs 2 row doubles of work
short fasp_mem_iludata_check(const ILU_data* iludata)
{
    const int memneed = 2 * iludata->row;
    if (iludata->nwork >= memneed) return FASP_SUCCESS;
    std::printf("### ERROR: ILU needs %d RAM, only %d available!\n", memneed, iludata->nwork);
    return ERROR_ALLOC_MEM;
}

// BlaILUSetupCSR.c:40
short fasp_ilu_dcsr_setup(dCSRmat* A, ILU_data* iludata, ILU_param* iluparam)
{
    const int type = iluparam->ILU_type, n = A->col, nnz = A->nnz;
    const double droptol = iluparam->ILU_droptol, permtol = iluparam->ILU_permtol;
    const double t0 = fasp::wall_seconds();
    int lfil = iluparam->ILU_lfil, iwk;
    // entries allocated for the factor (the reference's sizing rules); ILUt / ILUtp keep at most n / 2 + 1 per part
    if (type == ILUt || type == ILUtp) { iwk = 100 * nnz; lfil = (int)std::floor(n * 0.5) + 1; }
    else iwk = lfil == 0 ? nnz + 500 : (lfil + 5) * nnz;
    const int nwork = 4 * n;

    iludata->A = A;
    iludata->row = iludata->col = n;
    iludata->ilevL = iludata->jlevL = nullptr;
    iludata->ilevU = iludata->jlevU = nullptr;
    iludata->iperm = nullptr;
    iludata->type = type;
    fasp_ilu_data_create(iwk, nwork, iludata);

    Factor F(n, iwk, iludata->ijlu, iludata->luval, type != ILUt && type != ILUtp);
    int err;
    if (type == ILUt) err = factor_ilut(A, n, lfil, droptol, permtol, n, F, nullptr, nullptr);
    else if (type == ILUtp) {
        std::vector<int> old_of_new((size_t)n), new_of_old((size_t)n);
        for (int j = 0; j < n; ++j) old_of_new[(size_t)j] = new_of_old[(size_t)j] = j;
        err = factor_ilut(A, n, lfil, droptol, permtol, n, F, &old_of_new, &new_of_old);
        if (err == FACT_OK) {   // the factor and the caller's A in the new column numbering
            for (int p = F.ijlu[0]; p < F.ijlu[n]; ++p) F.ijlu[p] = new_of_old[(size_t)F.ijlu[p]];
            for (int k = A->IA[0]; k < A->IA[n]; ++k) A->JA[k] = new_of_old[(size_t)A->JA[k]];
        }
        for (int j = 0; j < n; ++j) {   // kept 1-based, as the reference hands it out
            iludata->iperm[j] = old_of_new[(size_t)j] + 1;
            iludata->iperm[n + j] = new_of_old[(size_t)j] + 1;
        }
    } else err = factor_iluk(A, n, lfil, F);

    // nzlu: the first U entry of the last row (the last row has no U entries: the size of the factor)
    iludata->nzlu = err == FACT_OK ? F.ustart[(size_t)n - 1] : 0;
    iludata->nwork = nwork;
    if (err != FACT_OK) {
        std::printf("### ERROR: ILU setup failed (ierr=%d: %s)! [%s]\n", err, fact_message(err), __func__);
        return ERROR_SOLVER_ILUSETUP;
    }
    if (iwk < iludata->nzlu) {
        std::printf("### ERROR: ILU needs more RAM %d! [%s]\n", iwk - iludata->nzlu, __func__);
        return ERROR_SOLVER_ILUSETUP;
    }
    fasp::ilu_register_host(iludata);
    if (iluparam->print_level > PRINT_NONE)
        std::printf("%s setup costs %f seconds.\n", type == ILUt ? "ILUt" : type == ILUtp ? "ILUtp" : "ILUk", fasp::wall_seconds() - t0);
    return FASP_SUCCESS;
}

}  // extern "C"
