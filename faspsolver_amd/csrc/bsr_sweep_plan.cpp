// bsr_sweep_plan.cpp -- host builder of the plan of a sequential block sweep (bsr_sweep_plan.h has the layout and the rule).
#include "bsr_sweep_plan.h"

#include <algorithm>

namespace fasp {

int bsr_sweep_sequence(int ROW, int order, const int* mark, std::vector<int>& seq)
{
    seq.clear();
    if (ROW < 0) return ERROR_INPUT_PAR;
    if (!mark) {
        if (order != ASCEND && order != DESCEND) return 1;
        seq.resize((size_t)ROW);
        for (int t = 0; t < ROW; ++t) seq[(size_t)t] = order == ASCEND ? t : ROW - 1 - t;
        return FASP_SUCCESS;
    }
    std::vector<char> seen((size_t)std::max(ROW, 1), 0);
    for (int t = 0; t < ROW; ++t) {
        const int i = mark[t];
        if (i < 0 || i >= ROW || seen[(size_t)i]) return ERROR_INPUT_PAR;
        seen[(size_t)i] = 1;
    }
    seq.assign(mark, mark + ROW);
    return FASP_SUCCESS;
}

int bsr_sweep_plan_build(const dBSRmat* A, const std::vector<int>& seq, bool with_values, const double* diaginv, BsrSweepPlan& P)
{
    if (!A) return ERROR_INPUT_PAR;
    if (A->nb < 1 || A->nb > 7) return ERROR_NUM_BLOCKS;
    if (A->ROW < 0 || A->ROW != A->COL || A->NNZ < 0 || A->storage_manner != 0 || !A->IA || (A->NNZ > 0 && !A->JA) ||
        (with_values && A->NNZ > 0 && !A->val) || (int)seq.size() != A->ROW)
        return ERROR_INPUT_PAR;
    const int n = A->ROW, nb = A->nb, nb2 = nb * nb;
    const int *ia = A->IA, *ja = A->JA;
    if (ia[0] != 0 || ia[n] != A->NNZ) return ERROR_DATA_STRUCTURE;
    for (int i = 0; i < n; ++i)
        if (ia[i + 1] < ia[i]) return ERROR_DATA_STRUCTURE;
    for (int k = 0; k < A->NNZ; ++k)
        if (ja[k] < 0 || ja[k] >= n) return ERROR_DATA_STRUCTURE;
    P = BsrSweepPlan();
    P.ROW = n; P.nb = nb;
    std::vector<int> pos((size_t)n, 0);
    for (int t = 0; t < n; ++t) pos[(size_t)seq[(size_t)t]] = t;
    // levels, in visiting order: every row a row reads as new has been given its level
    P.level.assign((size_t)n, 0);
    std::vector<int> olen((size_t)n, 0);   // off-diagonal entries per row
    int nlev = 0;
    for (int t = 0; t < n; ++t) {
        const int i = seq[(size_t)t];
        int lv = 0, cnt = 0;
        for (int k = ia[i]; k < ia[i + 1]; ++k) {
            const int j = ja[k];
            if (j == i) continue;
            ++cnt;
            if (pos[(size_t)j] < t) lv = std::max(lv, P.level[(size_t)j] + 1);
        }
        P.level[(size_t)i] = lv;
        olen[(size_t)i] = cnt;
        nlev = std::max(nlev, lv + 1);
    }
    P.nlev = nlev;
    // rows by level (ascending row index inside a level), cut into chunks of 64
    std::vector<int> first((size_t)nlev + 1, 0);
    for (int i = 0; i < n; ++i) ++first[(size_t)P.level[(size_t)i] + 1];
    for (int l = 0; l < nlev; ++l) first[(size_t)l + 1] += first[(size_t)l];
    std::vector<int> by_level((size_t)n);
    {
        std::vector<int> at(first.begin(), first.end() - 1);
        for (int i = 0; i < n; ++i) by_level[(size_t)at[(size_t)P.level[(size_t)i]]++] = i;
    }
    P.lvl_chunk.assign((size_t)nlev + 1, 0);
    for (int l = 0; l < nlev; ++l)
        P.lvl_chunk[(size_t)l + 1] = P.lvl_chunk[(size_t)l] + (first[(size_t)l + 1] - first[(size_t)l] + 63) / 64;
    P.nchunk = P.lvl_chunk[(size_t)nlev];
    const size_t nslot = (size_t)P.nchunk * 64;
    P.rows.assign(nslot, -1);
    P.len.assign(nslot, 0);
    P.cbase.assign((size_t)P.nchunk, 0);
    if (diaginv) P.dinv.assign(nslot * nb2, 0.0);
    long long nent = 0;
    for (int l = 0; l < nlev; ++l)
        for (int c = P.lvl_chunk[(size_t)l]; c < P.lvl_chunk[(size_t)l + 1]; ++c) {
            int kmax = 0;
            for (int lane = 0; lane < 64; ++lane) {
                const int q = first[(size_t)l] + (c - P.lvl_chunk[(size_t)l]) * 64 + lane;
                if (q >= first[(size_t)l + 1]) break;
                const int i = by_level[(size_t)q];
                P.rows[(size_t)c * 64 + lane] = i;
                P.len[(size_t)c * 64 + lane] = olen[(size_t)i];
                kmax = std::max(kmax, olen[(size_t)i]);
                P.nreal += olen[(size_t)i];
                if (diaginv)
                    for (int e = 0; e < nb2; ++e) P.dinv[((size_t)c * nb2 + e) * 64 + lane] = diaginv[(size_t)i * nb2 + e];
            }
            P.cbase[(size_t)c] = nent;
            nent += 64ll * kmax;
            P.maxlen = std::max(P.maxlen, kmax);
        }
    P.nent = nent;
    P.cols.assign((size_t)nent, -1);
    if (with_values) P.vals.assign((size_t)nent * nb2, 0.0);
    for (int c = 0; c < P.nchunk; ++c)
        for (int lane = 0; lane < 64; ++lane) {
            const int i = P.rows[(size_t)c * 64 + lane];
            if (i < 0) continue;
            size_t k = 0;
            for (int p = ia[i]; p < ia[i + 1]; ++p) {
                const int j = ja[p];
                if (j == i) continue;
                const size_t e = (size_t)P.cbase[(size_t)c] + 64 * k + (size_t)lane;
                P.cols[e] = pos[(size_t)j] < pos[(size_t)i] ? (j | BSR_SWEEP_NEW) : j;
                if (with_values) {
                    const size_t v0 = ((size_t)P.cbase[(size_t)c] + 64 * k) * nb2 + (size_t)lane;
                    for (int el = 0; el < nb2; ++el) P.vals[v0 + 64 * (size_t)el] = A->val[(size_t)p * nb2 + el];
                }
                ++k;
            }
        }
    return FASP_SUCCESS;
}

}  // namespace fasp
