// bsr_sweep_plan.h -- the plan of one sequential block sweep (Gauss-Seidel / SOR family of ItrSmootherBSR.c) over a dBSRmat
// in a given visiting sequence: dependency levels, chunks of 64 block rows, ELL slab planes.  Host code only (bsr_sweep_plan.cpp);
// the kernels that walk it are in bsr_sweep.hip.h.
//
// pos(i) = the place of block row i in the sequence.  The sweep is out of place: entry (i, j), j != i, reads u_new[j] when
// pos(j) < pos(i) and u_old[j] otherwise, so only true dependences remain: level(i) = 1 + max level(j) over the entries that
// read u_new, 0 without one.  The rows of a level (ascending row index) are cut into chunks of 64, the last chunk of a level
// padded.  Slot s = 64 c + lane of chunk c holds row rows[s] (-1: padding) with len[s] off-diagonal entries in the row's storage
// order k = IA[i] .. IA[i+1]-1 (diagonal entries j == i are skipped, however many the row stores).  Entry k of the slot:
//   cols[cbase[c] + 64 k + lane]                         column j, bit 31 set when the entry reads u_new; -1: padding
//   vals[(cbase[c] + 64 k) nb^2 + 64 (p nb + q) + lane]  element (p, q) of the block (nb^2 planes of 64)
// and the inverse diagonal block of the slot's row: dinv[(c nb^2 + p nb + q) 64 + lane].
#ifndef FASP_BSR_SWEEP_PLAN_H
#define FASP_BSR_SWEEP_PLAN_H

#include <vector>

#include "../../include/fasp_hip.h"

namespace fasp {

constexpr int BSR_SWEEP_NEW = (int)0x80000000;   // bit 31 of a stored column: the entry reads u_new

struct BsrSweepPlan {
    int ROW = 0, nb = 0, nlev = 0, nchunk = 0, maxlen = 0;
    long long nent = 0, nreal = 0;      // slab entries (padded) / actual off-diagonal entries
    std::vector<int> level;             // [ROW]
    std::vector<int> lvl_chunk;         // [nlev + 1] first chunk of each level
    std::vector<int> rows, len;         // [nchunk * 64]
    std::vector<long long> cbase;       // [nchunk]
    std::vector<int> cols;              // [nent]
    std::vector<double> vals;           // [nent * nb^2]       (with_values)
    std::vector<double> dinv;           // [nchunk * 64 * nb^2] (diaginv given)
};

// The visiting sequence of (order, mark) as the reference's _gs1 / _sor1 dispatch it: mark != NULL wins (it must be a permutation
// of 0 .. ROW-1), else ASCEND / DESCEND.  Returns FASP_SUCCESS and seq (ROW entries); 1 with seq empty when nothing is swept
// (mark == NULL, any other order); ERROR_INPUT_PAR for a mark that is no permutation.
int bsr_sweep_sequence(int ROW, int order, const int* mark, std::vector<int>& seq);

// The plan of A (square, 1 <= nb <= 7, columns inside 0 .. ROW-1) over seq.  with_values: the slab values from A->val;
// diaginv (may be NULL): ROW inverse diagonal blocks, row-major, laid out in planes.  ERROR_NUM_BLOCKS for nb outside 1 .. 7,
// ERROR_INPUT_PAR / ERROR_DATA_STRUCTURE for an inconsistent matrix.  Touches no device.
int bsr_sweep_plan_build(const dBSRmat* A, const std::vector<int>& seq, bool with_values, const double* diaginv, BsrSweepPlan& P);

}  // namespace fasp
#endif
