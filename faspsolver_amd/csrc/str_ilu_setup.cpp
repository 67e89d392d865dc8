// str_ilu_setup.cpp -- incomplete LU factorisation of a structured matrix on the host, fasp_ilu_dstr_setup0 / _setup1
// (BlaILUSetupSTR.c:38 / :333), and the host form of the two preconditioners made of it, fasp_precond_dstr_ilu0 / _ilu1
// (PreSTR.c:71 / :349).  Pure host code: no GPU needed.  DESIGN.md section 3.7.
//
// The factor is a dSTRmat LU: diag holds the inverted pivot blocks, offdiag the L and U bands, L_k in slot 2 k, U_k in slot 2 k + 1:
//   ILU(0)  offsets -1, +1, -nline, +nline [, -nplane, +nplane]                      (nband 4 on a 2-D grid, 6 on a 3-D one)
//   ILU(1)  offsets -1, +1, 1-nline, nline-1, -nline, +nline, nline-nplane, nplane-nline, 1-nplane, nplane-1, -nplane, +nplane
// nline / nplane by the reference's rule: nx == 1 -> (ny, ngrid), ny == 1 or nz == 1 -> (nx, ngrid), else (nx, nx ny).
// Every floating-point operation is the reference's, in its order: the scalar texts (nc = 1) as written there, the block texts
// through its small-matrix product (each entry summed left to right; nc = 6 from 0.0) and its inverses -- fasp_smat_inv
// everywhere but in setup0 with nc = 5, which calls the 5 x 5 closed form (inv5_closed below).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fasp_internal.h"

using namespace fasp;

namespace {

// fasp_smat_inv_nc5 (BlaSmallMatInv.c:170) as tables.  det = sum_k det_k a[5 k]; det_k is the sum of four groups
// o (m0 (p0 q0 - r0 s0) + m1 (p1 q1 - r1 s1) + m2 (p2 q2 - r2 s2)), a row of kDet5 being {o, m0, p0, q0, r0, s0, m1, ...}.
// Entry e of the adjugate is the sum of four groups o (+- f f f +- f f f ...), coded in kAdj5 entry after entry as
// o, number of terms, then per term: 1 (added) or 0 (subtracted), number of factors, the factors -- every product taken
// left to right, the terms summed left to right; the entry is then multiplied by 1 / det.  The groups are the reference's as
// they stand, which is not everywhere the adjugate (one term of entry 10 has six factors, one of entry 19 four, entry 22
// has a group of seven terms): the bytes of the factor are the contract, so they are kept.  The reference also prints a
// check of the product after every call; that is not reproduced.
const unsigned char kDet5[5][4][16] = {
    {{6,12,18,24,19,23,17,14,23,13,24,22,13,19,14,18}, {11,7,19,23,18,24,17,8,24,9,23,22,9,18,8,19}, {16,7,13,24,14,23,12,9,23,8,24,22,8,14,9,13}, {21,17,9,13,8,14,7,14,18,13,19,12,8,19,9,18}},
    {{1,22,14,18,13,19,12,19,23,18,24,17,13,24,14,23}, {11,17,4,23,3,24,2,18,24,19,23,22,3,19,4,18}, {16,12,3,24,4,23,2,14,23,13,24,22,4,13,3,14}, {21,2,13,19,14,18,12,4,18,3,19,17,3,14,4,13}},
    {{1,7,18,24,19,23,17,9,23,8,24,22,8,19,9,18}, {6,2,19,23,18,24,17,3,24,4,23,22,4,18,3,19}, {16,2,8,24,9,23,7,4,23,3,24,22,3,9,4,8}, {21,7,3,19,4,18,2,9,18,8,19,17,4,8,3,9}},
    {{1,12,8,24,9,23,7,14,23,13,24,22,9,13,8,14}, {6,2,13,24,14,23,12,4,23,3,24,22,3,14,4,13}, {11,7,3,24,4,23,2,9,23,8,24,22,4,8,3,9}, {21,2,8,14,9,13,7,4,13,3,14,12,3,9,4,8}},
    {{1,7,13,19,14,18,12,9,18,8,19,17,8,14,9,13}, {6,12,3,19,4,18,17,4,13,3,14,2,14,18,13,19}, {11,2,8,19,9,18,7,4,18,3,19,17,3,9,4,8}, {16,7,3,14,4,13,2,9,13,8,14,12,4,8,3,9}},
};
const unsigned char kAdj5[3204] = {
    6,6,1,3,12,18,24,0,3,12,19,23,0,3,17,13,24,1,3,17,14,23,1,3,22,13,19,0,3,22,14,18,11,6,1,3,7,19,23,0,
    3,7,18,24,1,3,17,8,24,0,3,17,9,23,0,3,22,8,19,1,3,22,9,18,16,6,1,3,7,13,24,0,3,7,14,23,0,3,12,8,
    24,1,3,12,9,23,1,3,22,8,14,0,3,22,9,13,21,6,1,3,7,14,18,0,3,7,13,19,1,3,12,8,19,0,3,12,9,18,0,3,
    17,8,14,1,3,17,9,13,1,6,1,3,12,19,23,0,3,12,18,24,1,3,22,14,18,0,3,17,14,23,0,3,22,13,19,1,3,17,13,24,
    11,6,1,3,22,3,19,1,3,2,18,24,0,3,17,3,24,0,3,22,4,18,0,3,2,19,23,1,3,17,4,23,16,6,1,3,12,3,24,0,
    3,12,4,23,0,3,22,3,14,1,3,2,14,23,1,3,22,4,13,0,3,2,13,24,21,6,1,3,12,4,18,0,3,12,3,19,0,3,2,14,
    18,0,3,17,4,13,1,3,2,13,19,1,3,17,3,14,1,6,1,3,7,18,24,0,3,7,19,23,0,3,17,8,24,1,3,17,9,23,1,3,
    22,8,19,0,3,22,9,18,6,6,1,3,2,19,23,0,3,2,18,24,1,3,17,3,24,0,3,17,4,23,0,3,22,3,19,1,3,22,4,18,
    16,6,1,3,2,8,24,0,3,2,9,23,0,3,7,3,24,1,3,7,4,23,1,3,22,3,9,0,3,22,4,8,21,6,1,3,2,9,18,0,
    3,2,8,19,1,3,7,3,19,0,3,7,4,18,0,3,17,3,9,1,3,17,4,8,1,6,1,3,12,8,24,0,3,12,9,23,1,3,7,14,
    23,0,3,7,13,24,1,3,22,9,13,0,3,22,8,14,6,6,1,3,12,4,23,0,3,12,3,24,1,3,22,3,14,0,3,22,4,13,1,3,
    2,13,24,0,3,2,14,23,11,6,1,3,7,3,24,0,3,7,4,23,1,3,22,4,8,0,3,22,3,9,1,3,2,9,23,0,3,2,8,24,
    21,6,1,3,12,3,9,0,3,12,4,8,1,3,2,8,14,0,3,2,9,13,1,3,7,4,13,0,3,7,3,14,1,6,1,3,7,13,19,0,
    3,7,14,18,0,3,12,8,19,1,3,12,9,18,1,3,17,8,14,0,3,17,9,13,6,6,1,3,2,14,18,0,3,2,13,19,1,3,12,3,
    19,0,3,12,4,18,0,3,17,3,14,1,3,17,4,13,11,6,1,3,2,8,19,0,3,2,9,18,0,3,7,3,19,1,3,7,4,18,1,3,
    17,3,9,0,3,17,4,8,16,6,1,3,2,9,13,0,3,2,8,14,1,3,7,3,14,0,3,7,4,13,0,3,12,3,9,1,3,12,4,8,
    5,6,1,3,12,19,23,0,3,12,18,24,1,3,22,14,18,0,3,22,13,19,1,3,17,13,24,0,3,17,14,23,20,6,1,3,12,9,18,0,
    3,12,8,19,1,3,7,13,19,0,3,18,7,14,1,3,17,8,14,0,3,9,17,13,15,6,1,3,22,9,13,0,3,12,9,23,1,3,12,24,
    8,1,3,7,14,23,0,3,24,7,13,0,3,22,14,8,10,6,1,3,18,7,24,0,3,18,22,9,0,3,17,8,24,1,3,17,9,23,1,3,
    22,8,19,0,3,19,23,7,2,6,1,3,19,23,10,0,3,14,23,15,0,3,18,24,10,1,3,18,14,20,0,3,13,19,20,1,3,24,13,15,
    12,6,1,3,18,0,24,0,3,18,20,4,1,3,3,19,20,0,3,19,23,0,1,3,4,23,15,0,3,24,15,3,17,6,1,3,4,13,20,0,
    3,13,24,0,1,3,14,23,0,0,3,3,14,20,1,3,24,3,10,0,3,4,23,10,22,6,1,3,14,15,3,0,3,18,14,0,1,3,18,4,
    10,0,3,4,13,15,1,3,13,19,0,0,3,3,19,10,0,6,1,3,18,9,22,0,3,18,24,7,1,3,19,23,7,0,3,9,23,17,1,3,
    24,8,17,0,3,8,19,22,5,6,1,3,2,18,24,0,3,2,19,23,1,3,17,4,23,0,3,17,3,24,1,3,22,3,19,0,3,22,4,18,
    15,6,1,3,4,8,22,0,3,3,9,22,0,3,24,8,2,1,3,9,23,2,0,3,4,23,7,1,3,24,3,7,20,6,1,3,18,4,7,0,
    3,18,9,2,1,3,9,3,17,0,3,4,8,17,1,3,8,19,2,0,3,3,19,7,0,6,1,3,12,9,23,0,3,12,24,8,1,3,22,14,
    8,0,3,7,14,23,1,3,24,7,13,0,3,9,22,13,5,6,1,3,12,3,24,0,3,12,4,23,0,3,22,3,14,1,3,2,14,23,0,3,
    2,13,24,1,3,22,4,13,10,6,1,3,22,9,3,0,3,4,22,8,1,3,4,7,23,0,3,2,9,23,1,3,24,2,8,0,3,7,24,3,
    20,6,1,3,7,14,3,0,3,4,7,13,1,3,9,2,13,1,3,12,4,8,0,3,12,9,3,0,3,2,14,8,0,6,1,3,12,8,19,0,
    3,12,18,9,1,3,18,7,14,0,3,8,17,14,1,3,17,13,9,0,3,7,13,19,5,6,1,3,2,13,19,0,3,2,14,18,0,3,12,3,
    19,1,3,12,4,18,1,3,17,3,14,0,3,17,4,13,10,6,1,3,18,2,9,0,3,18,7,4,1,3,3,7,19,0,3,2,8,19,1,3,
    17,8,4,0,3,3,17,9,15,6,1,3,8,2,14,0,3,12,8,4,1,3,12,3,9,0,3,3,7,14,1,3,7,13,4,0,3,2,13,9,
    5,6,1,3,18,24,11,0,3,24,13,16,1,3,14,23,16,0,3,19,23,11,1,3,13,19,21,0,3,18,14,21,10,6,1,3,19,23,6,0,
    3,9,23,16,1,3,24,8,16,0,3,8,19,21,1,3,18,9,21,0,3,18,24,6,15,6,1,3,24,13,6,0,3,14,23,6,0,3,24,8,
    11,1,3,9,23,11,1,3,14,8,21,0,3,13,9,21,20,6,1,3,18,14,6,0,3,18,9,11,1,3,8,19,11,0,3,13,19,6,1,3,
    9,13,16,0,3,14,8,16,4,6,1,3,21,13,15,0,3,11,23,15,1,3,16,23,10,0,3,13,16,20,1,3,18,11,20,0,3,18,21,10,
    14,6,1,3,18,0,21,0,3,1,18,20,1,3,16,3,20,0,3,23,0,16,1,3,1,23,15,0,3,21,3,15,19,6,1,3,1,13,20,0,
    3,1,23,10,1,3,23,0,11,1,3,21,3,10,0,3,11,3,20,0,3,13,0,21,24,6,1,3,13,0,16,0,3,18,0,11,1,3,11,3,
    15,1,3,1,18,10,0,3,1,13,15,0,3,16,3,10,4,6,1,3,5,21,18,0,3,18,20,6,1,3,20,16,8,0,3,5,16,23,1,3,
    15,6,23,0,3,21,15,8,9,6,1,3,1,20,18,0,3,1,15,23,1,3,0,16,23,0,3,18,0,21,0,3,20,16,3,1,3,15,21,3,
    19,6,1,3,20,6,3,0,3,5,21,3,1,3,0,21,8,0,3,23,0,6,1,3,1,5,23,0,3,1,20,8,24,6,1,3,1,15,8,0,
    3,0,16,8,1,3,18,0,6,0,3,1,5,18,1,3,5,16,3,0,3,6,15,3,0,6,1,3,24,11,8,0,3,6,24,13,1,3,21,9,
    13,0,3,11,9,23,1,3,14,6,23,0,3,14,21,8,1,6,1,3,5,13,24,0,3,5,14,23,1,3,14,20,8,1,3,10,9,23,0,3,
    24,10,8,0,3,20,9,13,3,6,1,3,6,10,24,0,3,10,9,21,1,3,5,14,21,0,3,5,24,11,1,3,20,9,11,0,3,14,6,20,
    4,6,1,3,5,11,23,0,3,5,21,13,1,3,21,10,8,0,3,6,10,23,1,3,20,6,13,0,3,11,20,8,0,6,1,3,13,19,6,0,
    3,14,18,6,0,3,11,19,8,1,3,14,16,8,1,3,11,18,9,0,3,13,16,9,1,6,1,3,14,18,5,0,3,13,19,5,1,3,10,19,
    8,0,3,14,15,8,0,3,10,18,9,1,3,13,15,9,3,6,1,3,11,19,5,0,3,11,15,9,1,3,10,16,9,0,3,10,19,6,1,3,
    14,15,6,0,3,14,16,5,4,6,1,3,11,15,8,0,3,11,18,5,1,3,13,16,5,0,3,13,15,6,1,3,10,18,6,0,3,10,16,8,
    5,6,1,3,19,22,11,0,3,24,17,11,1,3,12,24,16,0,3,22,14,16,0,3,12,19,21,1,3,17,14,21,10,6,1,3,24,17,6,0,
    3,19,22,6,0,3,24,7,16,1,3,22,9,16,1,3,19,7,21,0,3,17,9,21,15,6,1,3,22,14,6,0,3,9,22,11,1,3,24,7,
    11,0,3,12,24,6,0,3,7,14,21,1,3,12,9,21,20,6,1,3,12,19,6,0,3,17,14,6,0,3,19,7,11,1,3,9,17,11,1,3,
    7,14,16,0,3,12,9,16,0,6,1,3,11,17,24,0,3,11,19,22,0,3,12,16,24,1,3,12,19,21,1,3,14,16,22,0,3,14,17,21,
    1,6,1,3,10,19,22,0,3,10,17,24,1,3,12,15,24,0,3,12,19,20,0,3,14,15,22,1,3,14,17,20,2,6,1,3,10,16,24,0,
    3,10,19,21,0,3,11,15,24,1,3,11,19,20,1,3,14,15,21,0,3,14,16,20,4,5,1,6,10,17,21,11,15,22,0,3,11,17,20,0,
    3,12,15,21,1,3,12,16,20,0,3,10,16,22,0,6,1,3,21,9,17,0,3,6,24,17,1,3,19,6,22,0,4,0,16,9,22,1,3,24,
    16,7,0,3,19,21,7,1,6,1,3,5,24,17,0,3,5,19,22,1,3,19,20,7,0,3,20,9,17,1,3,15,9,22,0,3,24,15,7,2,
    6,1,3,5,19,21,0,3,19,6,20,0,3,5,24,16,1,3,24,6,15,0,3,15,9,21,1,3,20,9,16,4,7,1,3,16,5,22,0,3,
    6,15,22,1,3,20,6,17,0,3,5,21,17,0,3,6,15,22,1,3,21,15,7,0,3,16,20,7,0,6,1,3,12,24,6,0,3,14,22,6,
    0,3,11,24,7,1,3,14,21,7,1,3,11,22,9,0,3,12,21,9,1,6,1,3,14,22,5,0,3,12,24,5,1,3,10,24,7,0,3,14,
    20,7,0,3,10,22,9,1,3,12,20,9,2,6,1,3,11,24,5,0,3,11,20,9,1,3,14,20,6,0,3,14,21,5,1,3,10,21,9,0,
    3,10,24,6,4,6,1,3,11,20,7,0,3,11,22,5,1,3,12,21,5,1,3,10,22,6,0,3,12,20,6,0,3,10,21,7,0,6,1,3,
    12,16,9,0,3,6,12,19,1,3,6,17,14,0,3,17,11,9,1,3,11,7,19,0,3,16,7,14,1,6,1,3,5,12,19,0,3,5,17,14,
    0,3,12,15,9,1,3,17,10,9,1,3,15,7,14,0,3,10,7,19,2,6,1,3,11,15,9,0,3,5,11,19,1,3,5,16,14,0,3,6,
    15,14,1,3,6,10,19,0,3,16,10,9,4,6,1,3,5,17,11,0,3,5,12,16,1,3,12,6,15,1,3,10,7,16,0,3,17,6,10,0,
    3,15,7,11,5,6,1,3,12,18,21,0,3,12,23,16,1,3,22,13,16,0,3,18,22,11,1,3,23,17,11,0,3,17,13,21,15,6,1,3,
    12,23,6,0,3,12,8,21,1,3,8,22,11,0,3,23,7,11,1,3,7,13,21,0,3,22,13,6,20,6,1,3,12,8,16,0,3,12,18,6,
    1,3,18,7,11,0,3,8,17,11,1,3,17,13,6,0,3,7,13,16,10,6,1,3,17,8,21,0,3,22,8,16,0,3,18,7,21,1,3,18,
    22,6,1,3,23,7,16,0,3,23,17,6,0,6,1,3,12,23,16,0,3,12,18,21,1,3,17,13,21,1,3,18,22,11,0,3,23,17,11,0,
    3,22,13,16,1,6,1,3,12,18,20,0,3,12,23,15,1,3,22,13,15,1,3,23,17,10,0,3,17,13,20,0,3,18,22,10,2,6,1,3,
    18,21,10,0,3,18,11,20,0,3,21,13,15,1,3,16,13,20,0,3,23,16,10,1,3,23,11,15,3,6,1,3,17,11,20,0,3,12,16,20,
    1,3,12,21,15,0,3,21,17,10,0,3,22,11,15,1,3,16,22,10,0,6,1,3,18,21,7,0,3,18,6,22,1,3,23,6,17,1,3,16,
    8,22,0,3,21,8,17,0,3,23,16,7,1,6,1,3,5,18,22,0,3,5,23,17,0,3,15,8,22,1,3,20,8,17,0,3,18,20,7,1,
    3,23,15,7,3,6,1,3,16,20,7,1,3,6,15,22,0,3,6,20,17,0,3,5,16,22,1,3,5,21,17,0,3,21,15,7,2,6,1,3,
    5,23,16,0,3,5,18,21,1,3,18,6,20,1,3,15,8,21,0,3,20,8,16,0,3,23,6,15,0,6,1,3,12,21,8,0,3,22,11,8,
    1,3,11,7,23,0,3,6,12,23,0,3,21,7,13,1,3,6,22,13,1,6,1,3,5,12,23,0,3,5,22,13,0,3,10,7,23,1,3,20,
    7,13,1,3,22,10,8,0,3,12,20,8,2,6,1,3,5,21,13,1,3,11,20,8,1,3,6,10,23,0,3,5,11,23,0,3,21,10,8,0,
    3,6,20,13,3,6,1,3,5,22,11,0,3,5,12,21,1,3,10,7,21,0,3,22,6,10,0,3,20,7,11,1,3,12,6,20,0,6,1,3,
    17,11,8,0,3,11,7,18,1,3,6,12,18,0,3,12,16,8,1,3,16,7,13,0,3,6,17,13,1,6,1,3,5,17,13,0,3,5,12,18,
    1,3,10,7,18,1,3,12,15,8,0,3,17,10,8,0,3,15,7,13,2,6,1,3,5,11,18,0,3,5,16,13,1,3,16,10,8,1,3,6,
    15,13,0,3,11,15,8,0,3,6,10,18,3,6,1,3,5,12,16,1,3,17,6,10,0,3,5,17,11,0,3,12,6,15,0,3,10,7,16,1,
    3,15,7,11,
};

void inv5_closed(double* a)
{
    double c[25];
    std::memcpy(c, a, sizeof(c));
    double det = 0.0;
    for (int k = 0; k < 5; ++k) {
        double dk = 0.0;
        for (int g = 0; g < 4; ++g) {
            const unsigned char* t = kDet5[k][g];
            double in = 0.0;
            for (int m = 0; m < 3; ++m) {
                const unsigned char* u = t + 1 + 5 * m;
                const double v = c[u[0]] * (c[u[1]] * c[u[2]] - c[u[3]] * c[u[4]]);
                in = m == 0 ? v : in + v;
            }
            const double gv = c[t[0]] * in;
            dk = g == 0 ? gv : dk + gv;
        }
        const double dv = dk * c[5 * k];
        det = k == 0 ? dv : det + dv;
    }
    if (std::fabs(det) < SMALLREAL) {
        std::printf("### WARNING: Matrix is nearly singular, det = %e! Ignore.\n", det);
        for (int e = 0; e < 25; ++e) a[e] = e % 6 == 0 ? 1.0 : 0.0;
        return;
    }
    const double det_inv = 1 / det;
    const unsigned char* t = kAdj5;
    for (int e = 0; e < 25; ++e) {
        double v = 0.0;
        for (int g = 0; g < 4; ++g) {
            const double o = c[*t++];
            const int nterm = *t++;
            double in = 0.0;
            for (int m = 0; m < nterm; ++m) {
                const bool add = *t++ != 0;
                const int nf = *t++;
                double pr = c[*t++];
                for (int f = 1; f < nf; ++f) pr = pr * c[*t++];
                in = m == 0 ? (add ? pr : -pr) : (add ? in + pr : in - pr);
            }
            const double gv = o * in;
            v = g == 0 ? gv : v + gv;
        }
        a[e] = v * det_inv;
    }
}

// the reference's line and plane strides (BlaILUSetupSTR.c:63, PreSTR.c:93)
void str_lines(const dSTRmat* A, int* nline, int* nplane)
{
    if (A->nx == 1) { *nline = A->ny; *nplane = A->ngrid; }
    else if (A->ny == 1 || A->nz == 1) { *nline = A->nx; *nplane = A->ngrid; }
    else { *nline = A->nx; *nplane = A->nxy; }
}

void lu_zero(dSTRmat* LU) { std::memset(LU, 0, sizeof(*LU)); }

// what both set-ups refuse before they allocate: false after the message, LU zeroed
bool str_ilu_usable(const dSTRmat* A, dSTRmat* LU, const char* fn, int nline, int nplane)
{
    lu_zero(LU);
    if (A->nband != 4 && A->nband != 6) {
        std::printf("%s: number of bands for structured ILU is illegal!\n", fn);
        return false;
    }
    if (A->nc < 1 || A->nc > 7) {
        std::printf("### ERROR: Block size %d is not served (1 .. 7)! [%s]\n", A->nc, fn);
        return false;
    }
    if (nline < 2 || nline >= A->ngrid || A->ngrid % nline != 0 || nplane % nline != 0 || A->ngrid % nplane != 0 || !A->diag || !A->offsets || !A->offdiag) {
        std::printf("### ERROR: Degenerate grid for ILU! [%s]\n", fn);
        return false;
    }
    if (A->nband == 4 && nplane != A->ngrid) {   // a 2-D stencil on a 3-D grid: the reference walks the missing plane bands
        std::printf("### ERROR: Illegal offset for ILU! [%s]\n", fn);
        return false;
    }
    return true;
}

// y = y - x over a block (fasp_blas_darray_axpy with a = -1: y += (-1) x, the same bits)
inline void sub_block(const double* x, double* y, int nc2) { for (int e = 0; e < nc2; ++e) y[e] = y[e] - x[e]; }

// the diagonal block product of the block texts: c = A b, each entry from its first product (nc = 6, which has no unrolled
// form in fasp_blas_smat_mxv: from 0.0)
inline void mxv_block(const double* a, const double* b, double* c, int nc)
{
    for (int p = 0; p < nc; ++p) {
        double s = nc == 6 ? 0.0 + a[p * nc] * b[0] : a[p * nc] * b[0];
        for (int q = 1; q < nc; ++q) s = s + a[p * nc + q] * b[q];
        c[p] = s;
    }
}

// one triangular term of the block texts: acc = acc - B x (fasp_blas_smat_mxv into tc, fasp_blas_darray_axpy(-1))
inline void term_block(const double* B, const double* x, double* acc, int nc)
{
    double tc[7];
    mxv_block(B, x, tc, nc);
    for (int p = 0; p < nc; ++p) acc[p] = acc[p] - tc[p];
}

}  // namespace

extern "C" {

// BlaILUSetupSTR.c:38
void fasp_ilu_dstr_setup0(dSTRmat* A, dSTRmat* LU)
{
    if (!A || !LU) return;
    int nline, nplane;
    str_lines(A, &nline, &nplane);
    if (!str_ilu_usable(A, LU, __func__, nline, nplane)) return;
    const int nc = A->nc, nc2 = nc * nc, ngrid = A->ngrid, nband = A->nband;
    int LUoffsets[6] = {-1, 1, -nline, nline, -nplane, nplane};
    const double* a[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // A's bands in canonical order
    for (int b = 0; b < nband; ++b) {
        int k = -1;
        for (int c = 0; c < nband; ++c)
            if (A->offsets[b] == LUoffsets[c]) k = c;
        if (k < 0 || a[k] || (ngrid - std::abs(A->offsets[b]) > 0 && !A->offdiag[b])) {
            std::printf("### ERROR: Illegal offset for ILU! [%s]\n", __func__);
            return;
        }
        a[k] = A->offdiag[b] ? A->offdiag[b] : A->diag;   // (an empty band: never read, but taken)
    }
    // LU carries the canonical offsets whatever A's storage order is (the reference labels LU with A's and fills it canonically)
    fasp_dstr_alloc(A->nx, A->ny, A->nz, A->nxy, ngrid, nband, nc, LUoffsets, LU);
    std::memcpy(LU->diag, A->diag, sizeof(double) * (size_t)ngrid * nc2);
    for (int k = 0; k < nband; ++k) {
        const int len = ngrid - std::abs(LUoffsets[k]);
        if (len > 0) std::memcpy(LU->offdiag[k], a[k], sizeof(double) * (size_t)len * nc2);
    }
    double* const d = LU->diag;
    double** const o = LU->offdiag;
    const double* const diag = A->diag;
    if (nc == 1) {
        d[0] = 1.0 / d[0];
        for (int i = 1; i < ngrid; ++i) {
            o[0][i - 1] = a[0][i - 1] * d[i - 1];
            if (i >= nline) o[2][i - nline] = a[2][i - nline] * d[i - nline];
            if (i >= nplane) o[4][i - nplane] = a[0][i - nplane] * d[i - nplane];   // the reference's text: the -1 band of A (:144)
            d[i] = diag[i] - o[0][i - 1] * o[1][i - 1];
            if (i >= nline) d[i] = d[i] - o[2][i - nline] * o[3][i - nline];
            if (i >= nplane) d[i] = d[i] - o[4][i - nplane] * o[5][i - nplane];
            d[i] = 1.0 / d[i];
        }
        return;
    }
    auto inv = [nc](double* m) { if (nc == 5) inv5_closed(m); else (void)smat_inv(m, nc); };
    double smat[49];
    inv(d);
    for (int i = 1; i < ngrid; ++i) {
        const size_t i1 = (size_t)(i - 1) * nc2, ii = (size_t)i * nc2;
        const size_t ix = i >= nline ? (size_t)(i - nline) * nc2 : 0, ixy = i >= nplane ? (size_t)(i - nplane) * nc2 : 0;
        smat_mul(a[0] + i1, d + i1, o[0] + i1, nc);
        if (i >= nline) smat_mul(a[2] + ix, d + ix, o[2] + ix, nc);
        if (i >= nplane) smat_mul(a[4] + ixy, d + ixy, o[4] + ixy, nc);
        smat_mul(o[0] + i1, o[1] + i1, smat, nc);
        for (int e = 0; e < nc2; ++e) d[ii + e] = diag[ii + e] - smat[e];   // (-1) smat + diag
        if (i >= nline) { smat_mul(o[2] + ix, o[3] + ix, smat, nc); sub_block(smat, d + ii, nc2); }
        if (i >= nplane) { smat_mul(o[4] + ixy, o[5] + ixy, smat, nc); sub_block(smat, d + ii, nc2); }
        inv(d + ii);
    }
}

// BlaILUSetupSTR.c:333.  L bands alpha1 .. alpha6 = slots 0, 2, 4, 6, 8, 10 (offsets -1, 1-nline, -nline, nline-nplane,
// 1-nplane, -nplane), U bands beta1 .. beta6 = slots 1, 3, .., 11 (their mirrors).
void fasp_ilu_dstr_setup1(dSTRmat* A, dSTRmat* LU)
{
    if (!A || !LU) return;
    int nline, nplane;
    str_lines(A, &nline, &nplane);
    if (!str_ilu_usable(A, LU, __func__, nline, nplane)) return;
    const int nc = A->nc, nc2 = nc * nc, ngrid = A->ngrid, nband = A->nband;
    const int canon[6] = {-1, 1, -nline, nline, -nplane, nplane};
    for (int b = 0; b < nband; ++b)
        if (A->offsets[b] != canon[b] || (ngrid - std::abs(canon[b]) > 0 && !A->offdiag[b])) {   // the reference reads A->offdiag[0 .. 5] as these
            std::printf("### ERROR: Illegal offset for ILU! [%s]\n", __func__);
            return;
        }
    int LUoffsets[12] = {-1, 1, 1 - nline, nline - 1, -nline, nline, nline - nplane, nplane - nline, 1 - nplane, nplane - 1, -nplane, nplane};
    fasp_dstr_alloc(A->nx, A->ny, A->nz, A->nxy, ngrid, 12, nc, LUoffsets, LU);
    double* const d = LU->diag;
    double** const o = LU->offdiag;
    double** const a = A->offdiag;
    if (nband == 6 && ngrid - nplane > 0) std::memcpy(o[11], a[5], sizeof(double) * (size_t)(ngrid - nplane) * nc2);
    std::memcpy(d, A->diag, sizeof(double) * nc2);

    if (nc == 1) {
        double t;
        d[0] = 1.0 / d[0];
        o[1][0] = a[1][0];
        o[5][0] = a[3][0];
        o[3][0] = 0;
        o[7][0] = 0;
        if (o[9]) o[9][0] = 0;
        for (int i = 1; i < ngrid; ++i) {
            const int i1 = i - 1, ix = i - nline, ixy = i - nplane, ix1 = ix + 1, ixyx = ixy + nline, ixy1 = ixy + 1;
            if (ixy >= 0) o[10][ixy] = a[4][ixy] * d[ixy];
            if (ixy1 >= 0) {
                t = 0;
                if (ixy >= 0) t -= o[10][ixy] * o[1][ixy];
                o[8][ixy1] = t * d[ixy1];
            }
            if (ixyx >= 0) {
                t = 0;
                if (ixy >= 0) t -= o[10][ixy] * o[5][ixy];
                if (ixy1 >= 0) t -= o[8][ixy1] * o[3][ixy1];
                o[6][ixyx] = t * d[ixyx];
            }
            if (ix >= 0) {
                t = a[2][ix];
                if (ixy >= 0) t -= o[10][ixy] * o[7][ixy];
                o[4][ix] = t * d[ix];
            }
            if (ix1 >= 0) {
                t = 0;
                if (ix >= 0) t -= o[4][ix] * o[1][ix];
                if (ixy1 >= 0) t -= o[8][ixy1] * o[7][ixy1];
                o[2][ix1] = t * d[ix1];
            }
            t = a[0][i1];
            if (ix >= 0) t -= o[4][ix] * o[3][ix];
            if (ixy >= 0) t -= o[10][ixy] * o[9][ixy];
            o[0][i1] = t * d[i1];
            if (i + 1 < ngrid) {
                t = a[1][i];
                if (ix1 >= 0) t -= o[2][ix1] * o[5][ix1];
                if (ixy1 >= 0) t -= o[8][ixy1] * o[11][ixy1];
                o[1][i] = t;
            }
            if (i + nline - 1 < ngrid) {
                t = -o[0][i1] * o[5][i1];
                if (ixyx >= 0) t -= o[6][ixyx] * o[9][ixyx];
                o[3][i] = t;
            }
            if (i + nline < ngrid) {
                t = a[3][i];
                if (ixyx >= 0) t -= o[6][ixyx] * o[11][ixyx];
                o[5][i] = t;
            }
            if (i + nplane - nline < ngrid) {
                t = 0;
                if (ix1 >= 0) t -= o[2][ix1] * o[9][ix1];
                if (ix >= 0) t -= o[4][ix] * o[11][ix];
                o[7][i] = t;
            }
            if (i + nplane - 1 < ngrid) o[9][i] = -o[0][i1] * o[11][i1];
            d[i] = A->diag[i] - o[0][i1] * o[1][i1];
            if (ix1 >= 0) d[i] -= o[2][ix1] * o[3][ix1];
            if (ix >= 0) d[i] -= o[4][ix] * o[5][ix];
            if (ixyx >= 0) d[i] -= o[6][ixyx] * o[7][ixyx];
            if (ixy1 >= 0) d[i] -= o[8][ixy1] * o[9][ixy1];
            if (ixy >= 0) d[i] -= o[10][ixy] * o[11][ixy];
            d[i] = 1.0 / d[i];
        }
        return;
    }

    // the block texts (nc = 3, 5, 7 and the general one are the same operations; all invert with fasp_smat_inv)
    double smat[49], tc[49];
    auto mul = [nc](const double* x, const double* y, double* z) { smat_mul(x, y, z, nc); };
    auto mulsub = [&](const double* x, const double* y, double* z) { smat_mul(x, y, smat, nc); sub_block(smat, z, nc2); };
    (void)smat_inv(d, nc);
    std::memcpy(o[1], a[1], sizeof(double) * nc2);
    std::memcpy(o[5], a[3], sizeof(double) * nc2);
    for (int i = 1; i < ngrid; ++i) {
        const int i1 = i - 1, ix = i - nline, ixy = i - nplane, ix1 = ix + 1, ixyx = ixy + nline, ixy1 = ixy + 1;
        const long long ic = (long long)i * nc2, i1c = (long long)i1 * nc2, ixc = (long long)ix * nc2, ix1c = (long long)ix1 * nc2,
                        ixyc = (long long)ixy * nc2, ixy1c = (long long)ixy1 * nc2, ixyxc = (long long)ixyx * nc2;
        if (ixy >= 0) mul(a[4] + ixyc, d + ixyc, o[10] + ixyc);
        if (ixy1 >= 0) {
            std::fill(tc, tc + nc2, 0.0);
            if (ixy >= 0) mulsub(o[10] + ixyc, o[1] + ixyc, tc);
            mul(tc, d + ixy1c, o[8] + ixy1c);
        }
        if (ixyx >= 0) {
            std::fill(tc, tc + nc2, 0.0);
            if (ixy >= 0) mulsub(o[10] + ixyc, o[5] + ixyc, tc);
            if (ixy1 >= 0) mulsub(o[8] + ixy1c, o[3] + ixy1c, tc);
            mul(tc, d + ixyxc, o[6] + ixyxc);
        }
        if (ix >= 0) {
            std::memcpy(tc, a[2] + ixc, sizeof(double) * nc2);
            if (ixy >= 0) mulsub(o[10] + ixyc, o[7] + ixyc, tc);
            mul(tc, d + ixc, o[4] + ixc);
        }
        if (ix1 >= 0) {
            std::fill(tc, tc + nc2, 0.0);
            if (ix >= 0) mulsub(o[4] + ixc, o[1] + ixc, tc);
            if (ixy1 >= 0) mulsub(o[8] + ixy1c, o[7] + ixy1c, tc);
            mul(tc, d + ix1c, o[2] + ix1c);
        }
        std::memcpy(tc, a[0] + i1c, sizeof(double) * nc2);
        if (ix >= 0) mulsub(o[4] + ixc, o[3] + ixc, tc);
        if (ixy >= 0) mulsub(o[10] + ixyc, o[9] + ixyc, tc);
        mul(tc, d + i1c, o[0] + i1c);
        if (i + 1 < ngrid) {
            std::memcpy(o[1] + ic, a[1] + ic, sizeof(double) * nc2);
            if (ix1 >= 0) mulsub(o[2] + ix1c, o[5] + ix1c, o[1] + ic);
            if (ixy1 >= 0) mulsub(o[8] + ixy1c, o[11] + ixy1c, o[1] + ic);
        }
        if (i + nline - 1 < ngrid) {
            mulsub(o[0] + i1c, o[5] + i1c, o[3] + ic);
            if (ixyx >= 0) mulsub(o[6] + ixyxc, o[9] + ixyxc, o[3] + ic);
        }
        if (i + nline < ngrid) {
            std::memcpy(o[5] + ic, a[3] + ic, sizeof(double) * nc2);
            if (ixyx >= 0) mulsub(o[6] + ixyxc, o[11] + ixyxc, o[5] + ic);
        }
        if (i + nplane - nline < ngrid) {
            if (ix1 >= 0) mulsub(o[2] + ix1c, o[9] + ix1c, o[7] + ic);
            if (ix >= 0) mulsub(o[4] + ixc, o[11] + ixc, o[7] + ic);
        }
        if (i + nplane - 1 < ngrid) mulsub(o[0] + i1c, o[11] + i1c, o[9] + ic);
        smat_mul(o[0] + i1c, o[1] + i1c, smat, nc);
        for (int e = 0; e < nc2; ++e) d[ic + e] = A->diag[ic + e] - smat[e];
        if (ix1 >= 0) mulsub(o[2] + ix1c, o[3] + ix1c, d + ic);
        if (ix >= 0) mulsub(o[4] + ixc, o[5] + ixc, d + ic);
        if (ixyx >= 0) mulsub(o[6] + ixyxc, o[7] + ixyxc, d + ic);
        if (ixy1 >= 0) mulsub(o[8] + ixy1c, o[9] + ixy1c, d + ic);
        if (ixy >= 0) mulsub(o[10] + ixyc, o[11] + ixyc, d + ic);
        (void)smat_inv(d + ic, nc);
    }
}

// PreSTR.c:71: z = U^-1 L^-1 r with an ILU(0) factor (data: the dSTRmat of fasp_ilu_dstr_setup0).  L terms -1, -nline,
// -nplane, U terms +1, +nline, +nplane, one product subtracted at a time, the inverted pivot as the multiplier.
void fasp_precond_dstr_ilu0(double* r, double* z, void* data)
{
    const dSTRmat* LU = static_cast<const dSTRmat*>(data);
    if (!LU || LU->ngrid <= 0 || !LU->diag || !LU->offdiag) return;
    int nline, nplane;
    str_lines(LU, &nline, &nplane);
    const int m = LU->ngrid, nc = LU->nc, nc2 = nc * nc;
    double** const o = LU->offdiag;
    const double* const d = LU->diag;
    std::vector<double> zzv((size_t)m * nc);
    double* const zz = zzv.data();
    if (nc == 1) {
        zz[0] = r[0];
        for (int i = 1; i < m; ++i) {
            zz[i] = r[i] - o[0][i - 1] * zz[i - 1];
            if (i >= nline) zz[i] = zz[i] - o[2][i - nline] * zz[i - nline];
            if (i >= nplane) zz[i] = zz[i] - o[4][i - nplane] * zz[i - nplane];
        }
        z[m - 1] = zz[m - 1] * d[m - 1];
        for (int i = m - 2; i >= 0; --i) {
            zz[i] = zz[i] - o[1][i] * z[i + 1];
            if (i < m - nline) zz[i] = zz[i] - o[3][i] * z[i + nline];
            if (i < m - nplane) zz[i] = zz[i] - o[5][i] * z[i + nplane];
            z[i] = zz[i] * d[i];
        }
        return;
    }
    std::memcpy(zz, r, sizeof(double) * (size_t)m * nc);
    for (int i = 1; i < m; ++i) {
        double* acc = zz + (size_t)i * nc;
        term_block(o[0] + (size_t)(i - 1) * nc2, zz + (size_t)(i - 1) * nc, acc, nc);
        if (i >= nline) term_block(o[2] + (size_t)(i - nline) * nc2, zz + (size_t)(i - nline) * nc, acc, nc);
        if (i >= nplane) term_block(o[4] + (size_t)(i - nplane) * nc2, zz + (size_t)(i - nplane) * nc, acc, nc);
    }
    mxv_block(d + (size_t)(m - 1) * nc2, zz + (size_t)(m - 1) * nc, z + (size_t)(m - 1) * nc, nc);
    for (int i = m - 2; i >= 0; --i) {
        double* acc = zz + (size_t)i * nc;
        const size_t ic2 = (size_t)i * nc2;
        term_block(o[1] + ic2, z + (size_t)(i + 1) * nc, acc, nc);
        if (i < m - nline) term_block(o[3] + ic2, z + (size_t)(i + nline) * nc, acc, nc);
        if (i < m - nplane) term_block(o[5] + ic2, z + (size_t)(i + nplane) * nc, acc, nc);
        mxv_block(d + ic2, acc, z + (size_t)i * nc, nc);
    }
}

// PreSTR.c:349: the same with an ILU(1) factor (fasp_ilu_dstr_setup1).  L terms -1, 1-nline, -nline, nline-nplane, 1-nplane,
// -nplane, U terms +1, nline-1, +nline, nplane-nline, nplane-1, +nplane.
void fasp_precond_dstr_ilu1(double* r, double* z, void* data)
{
    const dSTRmat* LU = static_cast<const dSTRmat*>(data);
    if (!LU || LU->ngrid <= 0 || !LU->diag || !LU->offdiag || LU->nband != 12) return;
    int nline, nplane;
    str_lines(LU, &nline, &nplane);
    const int m = LU->ngrid, nc = LU->nc, nc2 = nc * nc;
    double** const o = LU->offdiag;
    const double* const d = LU->diag;
    const int back[6] = {1, nline - 1, nline, nplane - nline, nplane - 1, nplane};   // distance of term k, L behind and U ahead
    std::vector<double> zzv((size_t)m * nc);
    double* const zz = zzv.data();
    if (nc == 1) {
        zz[0] = r[0];
        for (int i = 1; i < m; ++i) {
            zz[i] = r[i] - o[0][i - 1] * zz[i - 1];
            for (int k = 1; k < 6; ++k)
                if (i >= back[k]) zz[i] = zz[i] - o[2 * k][i - back[k]] * zz[i - back[k]];
        }
        z[m - 1] = zz[m - 1] * d[m - 1];
        for (int i = m - 2; i >= 0; --i) {
            zz[i] = zz[i] - o[1][i] * z[i + 1];
            for (int k = 1; k < 6; ++k)
                if (i + back[k] < m) zz[i] = zz[i] - o[2 * k + 1][i] * z[i + back[k]];
            z[i] = d[i] * zz[i];
        }
        return;
    }
    std::memcpy(zz, r, sizeof(double) * (size_t)m * nc);
    for (int i = 1; i < m; ++i) {
        double* acc = zz + (size_t)i * nc;
        for (int k = 0; k < 6; ++k)
            if (i >= back[k]) term_block(o[2 * k] + (size_t)(i - back[k]) * nc2, zz + (size_t)(i - back[k]) * nc, acc, nc);
    }
    mxv_block(d + (size_t)(m - 1) * nc2, zz + (size_t)(m - 1) * nc, z + (size_t)(m - 1) * nc, nc);
    for (int i = m - 2; i >= 0; --i) {
        double* acc = zz + (size_t)i * nc;
        for (int k = 0; k < 6; ++k)
            if (i + back[k] < m) term_block(o[2 * k + 1] + (size_t)i * nc2, z + (size_t)(i + back[k]) * nc, acc, nc);
        mxv_block(d + (size_t)i * nc2, acc, z + (size_t)i * nc, nc);
    }
}

}  // extern "C"
