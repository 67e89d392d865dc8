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
// ilu.hip.h: factors built here are kept resident on the device once used.  block_nb: 0 for a factor of
// fasp_ilu_dcsr_setup, the block size for one of fasp_ilu_dbsr_setup (the registry's record of the kind)
void ilu_register_host(ILU_data* d, int block_nb);
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

// ---- block ILU(k) of a BSR matrix (BlaILUSetupBSR.c:55) ----
// Symbolic pass (the level-of-fill pattern of the block pattern, BlaILU.c:1372).  Row i starts from the off-diagonal
// columns of A's row i at level 0; its columns j < i are visited in ascending order (fill added on the way included), and
// each U entry (c, s2) of row j offers column c at level s1 + s2 + 1 (s1: level of (i, j)): a new column is taken when
// that level is <= lfil, an existing one keeps the smaller level.  The row is stored with ascending columns -- L entries,
// then U entries -- and the diagonal block at position i.  Returns nzlu, or -1 when more than iwk entries are needed,
// -2 for a row without its diagonal or with a repeated column.
int bsr_symbolic(const dBSRmat* A, int lfil, int iwk, std::vector<int>& ijlu, std::vector<int>& uptr)
{
    const int n = A->ROW;
    ijlu.assign((size_t)std::max(iwk, n + 1), 0);
    uptr.assign((size_t)n, 0);
    std::vector<int> level((size_t)std::max(iwk, n + 1), 0);   // level of each stored entry (position-indexed)
    std::vector<int> next((size_t)n + 1, n), rowlev((size_t)n, 0), mark((size_t)n, -1), cols;
    int nz = n + 1;
    ijlu[0] = n + 1;
    for (int i = 0; i < n; ++i) {
        cols.clear();
        bool diag = false;
        for (int k = A->IA[i]; k < A->IA[i + 1]; ++k) {
            const int c = A->JA[k];
            if (c < 0 || c >= n || mark[(size_t)c] == i) return -2;
            mark[(size_t)c] = i;
            if (c == i) diag = true;
            else { cols.push_back(c); rowlev[(size_t)c] = 0; }
        }
        if (!diag && !cols.empty()) return -2;
        std::sort(cols.begin(), cols.end());
        // the row as a sorted linked list: head -> next[] -> ... -> n
        int head = n;
        for (size_t q = cols.size(); q-- > 0;) { next[(size_t)cols[q]] = head; head = cols[q]; }
        int lower = 0, count = (int)cols.size();
        for (int j = head; j < i; j = next[(size_t)j]) {
            ++lower;
            if (lfil == 0) continue;
            int prev = j;
            const int s1 = rowlev[(size_t)j];
            for (int m = uptr[(size_t)j]; m < ijlu[(size_t)j + 1]; ++m) {
                const int c = ijlu[(size_t)m];
                const int lev = s1 + level[(size_t)m] + 1;
                if (mark[(size_t)c] != i) {
                    if (lev > lfil) continue;
                    mark[(size_t)c] = i;
                    rowlev[(size_t)c] = lev;
                    while (next[(size_t)prev] <= c) prev = next[(size_t)prev];   // U columns of row j ascend: insert after prev
                    next[(size_t)c] = next[(size_t)prev];
                    next[(size_t)prev] = c;
                    prev = c;
                    ++count;
                } else if (c != i) {
                    rowlev[(size_t)c] = std::min(rowlev[(size_t)c], lev);
                }
            }
        }
        if (nz + count > iwk) return -1;
        uptr[(size_t)i] = nz + lower;
        for (int j = head; j < n; j = next[(size_t)j]) {
            ijlu[(size_t)nz] = j;
            level[(size_t)nz] = rowlev[(size_t)j];
            ++nz;
        }
        ijlu[(size_t)i + 1] = nz;
    }
    return nz;
}

// c = a b for nb x nb blocks in fasp_blas_smat_mul's order: each entry summed left to right; nb = 6 (no unrolled form in
// the reference) starts from 0.0 and accumulates, as its default branch does
void block_mul(const double* a, const double* b, double* c, int nb)
{
    for (int i = 0; i < nb; ++i)
        for (int j = 0; j < nb; ++j) {
            double s = nb == 6 ? 0.0 + a[i * nb] * b[j] : a[i * nb] * b[j];
            for (int k = 1; k < nb; ++k) s = s + a[i * nb + k] * b[k * nb + j];
            c[i * nb + j] = s;
        }
}

// fasp_smat_inv_nc3 (BlaSmallMatInv.c:67): cofactors over the determinant, the identity for a near-singular block
void block_inv3(double* a)
{
    const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7], a8 = a[8];
    const double M0 = a4 * a8 - a5 * a7, M3 = a2 * a7 - a1 * a8, M6 = a1 * a5 - a2 * a4;
    const double M1 = a5 * a6 - a3 * a8, M4 = a0 * a8 - a2 * a6, M7 = a2 * a3 - a0 * a5;
    const double M2 = a3 * a7 - a4 * a6, M5 = a1 * a6 - a0 * a7, M8 = a0 * a4 - a1 * a3;
    const double det = a0 * M0 + a3 * M3 + a6 * M6;
    if (std::fabs(det) < fasp::SMALLREAL) {
        std::printf("### WARNING: Matrix is nearly singular, det = %e! Ignore.\n", det);
        for (int e = 0; e < 9; ++e) a[e] = e % 4 == 0 ? 1.0 : 0.0;
        return;
    }
    const double det_inv = 1.0 / det;
    a[0] = M0 * det_inv; a[1] = M3 * det_inv; a[2] = M6 * det_inv;
    a[3] = M1 * det_inv; a[4] = M4 * det_inv; a[5] = M7 * det_inv;
    a[6] = M2 * det_inv; a[7] = M5 * det_inv; a[8] = M8 * det_inv;
}

// Numeric pass (BlaILUSetupBSR.c:819): block IKJ elimination on the symbolic pattern.  Row k: A's blocks scattered onto
// the pattern (zeros elsewhere); for each L block in storage order, L_kj = L_kj U_jj^-1, then U_ks -= L_kj U_js for every
// U block of row j whose column row k holds; finally the diagonal block is inverted (nb = 1: 1 / d; nb = 3: the closed
// form; otherwise the pivoted Gauss-Jordan).  Returns the status of the LAST pivoted inverse (the reference's loop
// overwrites it), FASP_SUCCESS when there is none.
int bsr_numeric(const dBSRmat* A, const int* ijlu, const int* uptr, double* luval)
{
    const int n = A->ROW, nb = A->nb, nb2 = nb * nb;
    std::vector<int> pos((size_t)n, 0);
    std::vector<double> mult((size_t)nb2), upd((size_t)nb2);
    int status = FASP_SUCCESS;
    for (int k = 0; k < n; ++k) {
        for (int p = ijlu[k]; p < ijlu[k + 1]; ++p) {
            pos[(size_t)ijlu[p]] = p;
            std::fill(luval + (size_t)p * nb2, luval + (size_t)(p + 1) * nb2, 0.0);
        }
        std::fill(luval + (size_t)k * nb2, luval + (size_t)(k + 1) * nb2, 0.0);
        pos[(size_t)k] = k;
        for (int q = A->IA[k]; q < A->IA[k + 1]; ++q)
            std::memcpy(luval + (size_t)pos[(size_t)A->JA[q]] * nb2, A->val + (size_t)q * nb2, sizeof(double) * nb2);
        for (int p = ijlu[k]; p < uptr[k]; ++p) {
            const int j = ijlu[p];
            double* L = luval + (size_t)p * nb2;
            block_mul(L, luval + (size_t)j * nb2, mult.data(), nb);
            std::memcpy(L, mult.data(), sizeof(double) * nb2);
            for (int s = uptr[j]; s < ijlu[j + 1]; ++s) {
                const int at = pos[(size_t)ijlu[s]];
                if (at == 0) continue;
                block_mul(mult.data(), luval + (size_t)s * nb2, upd.data(), nb);
                double* U = luval + (size_t)at * nb2;
                for (int e = 0; e < nb2; ++e) U[e] -= upd[(size_t)e];
            }
        }
        for (int p = ijlu[k]; p < ijlu[k + 1]; ++p) pos[(size_t)ijlu[p]] = 0;
        pos[(size_t)k] = 0;
        double* D = luval + (size_t)k * nb2;
        if (nb == 1) D[0] = 1.0 / D[0];
        else if (nb == 3) block_inv3(D);
        else {
            status = fasp::smat_invp(D, nb);
            if (status < 0) std::printf("### WARNING: The matrix is nearly singular!\n");
        }
    }
    return status;
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

namespace fasp {
void smat_mul(const double* a, const double* b, double* c, int n) { block_mul(a, b, c, n); }
}

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
    fasp::ilu_register_host(iludata, 0);
    if (iluparam->print_level > PRINT_NONE)
        std::printf("%s setup costs %f seconds.\n", type == ILUt ? "ILUt" : type == ILUtp ? "ILUtp" : "ILUk", fasp::wall_seconds() - t0);
    return FASP_SUCCESS;
}

// BlaILUSetupBSR.c:55.  Every ILU_type gives ILUk(ILU_lfil) (ILUt / ILUtp parameters are not read).  The factor is MSR over
// block rows: ijlu as for the scalar factor, luval[p * nb^2 ..] the nb x nb block of entry p (row-major), luval[i * nb^2 ..]
// the INVERSE of the i-th diagonal block.  Failure: ERROR_SOLVER_ILUSETUP (the pattern needs more than (lfil + 2) NNZ
// entries, or a pivoted block inverse failed on the last block row).
short fasp_ilu_dbsr_setup(dBSRmat* A, ILU_data* iludata, ILU_param* iluparam)
{
    const double t0 = fasp::wall_seconds();
    const int lfil = iluparam->ILU_lfil;
    iludata->type = 0;
    iludata->iperm = nullptr;
    iludata->A = nullptr;
    iludata->ilevL = iludata->jlevL = nullptr;
    iludata->ilevU = iludata->jlevU = nullptr;
    iludata->ijlu = nullptr; iludata->luval = nullptr; iludata->work = nullptr;
    iludata->nzlu = 0; iludata->nwork = 0;
    if (!A || !A->IA || !A->JA || !A->val || A->ROW <= 0 || A->ROW != A->COL || A->nb < 1 || A->nb > 7 || lfil < 0) {
        std::printf("### ERROR: ILU setup needs a square BSR matrix with 1 <= nb <= 7 and lfil >= 0! [%s]\n", __func__);
        return ERROR_SOLVER_ILUSETUP;
    }
    const int n = A->ROW, nb = A->nb, nb2 = nb * nb;
    iludata->row = iludata->col = n;
    iludata->nb = nb;
    const long long iwk_ll = (long long)(lfil + 2) * A->NNZ;
    const int iwk = (int)std::min<long long>(iwk_ll, 0x7fffffffLL);

    std::vector<int> ijlu, uptr;
    const int nzlu = bsr_symbolic(A, lfil, iwk, ijlu, uptr);
    if (nzlu < 0) {
        if (nzlu == -1) std::printf("### ERROR: More storage needed! [fasp_symbfactor]\n");
        else std::printf("### ERROR: Missing diagonal block or repeated column in a block row! [fasp_symbfactor]\n");
        std::printf("### ERROR: ILU setup failed (ierr=%d)! [%s]\n", nzlu == -1 ? 1 : 2, __func__);
        return ERROR_SOLVER_ILUSETUP;
    }
    iludata->luval = (double*)fasp_mem_calloc((unsigned)nzlu * (unsigned)nb2, sizeof(double));
    const int status = bsr_numeric(A, ijlu.data(), uptr.data(), iludata->luval);
    if (status < 0) {
        std::printf("### ERROR: ILU factorization failed! [%s]\n", __func__);
        return ERROR_SOLVER_ILUSETUP;
    }
    iludata->nzlu = nzlu;
    iludata->nwork = 20 * n * nb;
    iludata->ijlu = (int*)fasp_mem_calloc((unsigned)nzlu, sizeof(int));
    std::memcpy(iludata->ijlu, ijlu.data(), sizeof(int) * (size_t)nzlu);
    iludata->work = (double*)fasp_mem_calloc((unsigned)iludata->nwork, sizeof(double));
    fasp::ilu_register_host(iludata, nb);
    if (iluparam->print_level > PRINT_NONE)
        std::printf("BSR ILU(%d)-seq setup costs %f seconds.\n", lfil, fasp::wall_seconds() - t0);
    return (short)status;
}

}  // extern "C"
