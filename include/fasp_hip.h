/*
 * fasp_hip.h -- C-ABI of the MI355X-native AMG-preconditioned Krylov path.
 *
 * This header is the drop-in boundary of libfasp_hip.so.  Every type below is
 * layout-identical to the SERIAL (non-OpenMP) build of the reference headers,
 * and every `fasp_*` entry point keeps the reference's name, argument order,
 * argument meaning and return convention, so that a program compiled against
 * the reference's own `fasp.h` / `fasp_functs.h` can be linked against this
 * library instead of libfasp for the path listed here.
 *
 *   reference type / function                       reference location
 *   ------------------------------------------------------------------------
 *   INT = int, REAL = double, SHORT = short         base/include/fasp.h:71-75
 *   dCSRmat  {row,col,nnz,IA,JA,val}                base/include/fasp.h:151-180
 *   dvector / ivector                               base/include/fasp.h:354-376
 *   ITS_param                                       base/include/fasp.h:386-398
 *   AMG_param                                       base/include/fasp.h:455-595
 *   precond {data,fct}                              base/include/fasp.h:1095-1103
 *   fasp_param_amg_init                             base/src/AuxParam.c:431
 *   fasp_param_solver_init                          base/src/AuxParam.c:572
 *   fasp_solver_dcsr_krylov_amg                     base/src/SolCSR.c:476
 *   fasp_blas_dcsr_mxv / _aAxpy                     base/src/BlaSpmvCSR.c:242 / :494
 *   fasp_blas_darray_{dotprod,norm2,norminf,axpy,axpby}
 *                                                   base/src/BlaArray.c:771/691/719/90/620
 *   fasp_smoother_dcsr_jacobi                       base/src/ItrSmootherCSR.c:98
 *   fasp_solver_d{csr,bsr,str}_sp{cg,bcgs,minres,gmres,vgmres}
 *                                                   base/src/KrySPcg.c, KrySPbcgs.c, KrySPminres.c, KrySPgmres.c, KrySPvgmres.c
 *   fasp_solver_dcsr_itsolver_s / _krylov_s         base/src/SolCSR.c:163 / :295
 *
 * The `fasp_hip_*` functions are extensions (no reference counterpart): they
 * expose the device-resident objects behind fasp_solver_dcsr_krylov_amg so a
 * caller can set the hierarchy up once and solve many times, bind a GPU, join
 * an RCCL communicator and read timing / roofline counters.
 *
 * No torch types, no C++ types: plain pointers and sizes only.
 */
#ifndef FASP_HIP_H
#define FASP_HIP_H

#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* constants (values of base/include/fasp_const.h)                          */
/* ------------------------------------------------------------------------ */
#define FASP_SUCCESS            0
#define ERROR_OPEN_FILE       (-10)
#define ERROR_WRONG_FILE      (-11)
#define ERROR_INPUT_PAR       (-13)
#define ERROR_MAT_SIZE        (-15)
#define ERROR_NUM_BLOCKS      (-18)
#define ERROR_MISC            (-19)
#define ERROR_ALLOC_MEM       (-20)
#define ERROR_DATA_STRUCTURE  (-21)
#define ERROR_AMG_INTERP_TYPE (-30)
#define ERROR_AMG_SMOOTH_TYPE (-31)
#define ERROR_AMG_COARSE_TYPE (-32)
#define ERROR_AMG_SETUP       (-39)
#define ERROR_SOLVER_TYPE     (-40)
#define ERROR_SOLVER_PRECTYPE (-41)
#define ERROR_SOLVER_STAG     (-42)
#define ERROR_SOLVER_SOLSTAG  (-43)
#define ERROR_SOLVER_TOLSMALL (-44)
#define ERROR_SOLVER_ILUSETUP (-45)
#define ERROR_SOLVER_MISC     (-46)
#define ERROR_SOLVER_MAXIT    (-48)
#define ERROR_SOLVER_EXIT     (-49)
#define ERROR_UNKNOWN         (-99)

#define PRINT_NONE 0
#define PRINT_MIN  1
#define PRINT_SOME 2
#define PRINT_MORE 4
#define PRINT_MOST 8
#define PRINT_ALL  10

#define SOLVER_DEFAULT 0
#define SOLVER_CG      1
#define SOLVER_BiCGstab 2
#define SOLVER_MinRes  3
#define SOLVER_GMRES   4
#define SOLVER_VGMRES  5
#define SOLVER_VFGMRES 6
#define SOLVER_GCG     7
#define SOLVER_GCR     8

#define STOP_REL_RES     1
#define STOP_REL_PRECRES 2
#define STOP_MOD_REL_RES 3

#define PREC_NULL 0
#define PREC_DIAG 1
#define PREC_AMG  2
#define PREC_FMG  3
#define PREC_ILU     4
#define PREC_SCHWARZ 5

#define CLASSIC_AMG 1
#define SA_AMG      2
#define UA_AMG      3

#define V_CYCLE       1
#define W_CYCLE       2
#define AMLI_CYCLE    3
#define NL_AMLI_CYCLE 4
#define VW_CYCLE      12
#define WV_CYCLE      21

#define SMOOTHER_JACOBI  1
#define SMOOTHER_GS      2
#define SMOOTHER_SGS     3
#define SMOOTHER_CG      4
#define SMOOTHER_SOR     5
#define SMOOTHER_SSOR    6
#define SMOOTHER_GSOR    7
#define SMOOTHER_SGSOR   8
#define SMOOTHER_POLY    9
#define SMOOTHER_L1DIAG  10
#define SMOOTHER_JACOBIF 11
#define SMOOTHER_GSF     12

#define COARSE_RS  1
#define COARSE_RSP 2
#define COARSE_CR  3
#define COARSE_AC  4
#define COARSE_MIS 5

#define INTERP_DIR 1
#define INTERP_STD 2
#define INTERP_ENG 3
#define INTERP_RDC 4
#define INTERP_EXT 6

#define NO_ORDER 0
#define CF_ORDER 1

#define PAIRWISE 1
#define VMB      2

#define FASP_ILUk 1
/* ILU_param.ILU_type (fasp_const.h:149-151) */
#define ILUk  1
#define ILUt  2
#define ILUtp 3

/* ------------------------------------------------------------------------ */
/* types (serial layout of base/include/fasp.h; sizes checked in tests)     */
/* ------------------------------------------------------------------------ */

/* fasp.h:151  sizeof == 40 */
typedef struct dCSRmat {
    int     row;
    int     col;
    int     nnz;
    int*    IA;  /* row+1 row pointers, 0-based */
    int*    JA;  /* nnz column indices, unsorted within a row */
    double* val; /* nnz values */
} dCSRmat;

/* fasp_block.h:34  sizeof == 48.  Block CSR: ROW x COL blocks of nb x nb, NNZ stored blocks,
 * val[NNZ*nb*nb] with every block row-major (storage_manner 0). */
typedef struct dBSRmat {
    int     ROW;
    int     COL;
    int     NNZ;
    int     nb;
    int     storage_manner;
    double* val;
    int*    IA;
    int*    JA;
} dBSRmat;

/* fasp.h:316  sizeof == 64.  Structured (banded block) matrix on an nx x ny x nz grid: ngrid = nxy * nz grid points, nc x nc
 * blocks (row-major), a diagonal of ngrid blocks and nband off-diagonal bands.  Band b with offset d = offsets[b] holds the
 * ngrid - |d| blocks A(i, i + d); a lower band (d < 0) is indexed by its column: offdiag[b][k] is A(k - d, k). */
typedef struct dSTRmat {
    int      nx;
    int      ny;
    int      nz;
    int      nxy;
    int      nc;
    int      ngrid;
    double*  diag;
    int      nband;
    int*     offsets;
    double** offdiag;
} dSTRmat;

/* fasp.h:354  sizeof == 16 */
typedef struct dvector {
    int     row;
    double* val;
} dvector;

/* fasp.h:368  sizeof == 16 */
typedef struct ivector {
    int  row;
    int* val;
} ivector;

/* fasp.h:386  sizeof == 40 */
typedef struct {
    short  print_level;
    short  itsolver_type;
    short  decoup_type;
    short  precond_type;
    short  stop_type;
    int    restart;
    int    maxit;
    double tol;
    double abstol;
} ITS_param;

/* fasp.h:455  sizeof == 224 */
typedef struct {
    short   AMG_type;
    short   print_level;
    int     maxit;
    double  tol;
    short   max_levels;
    int     coarse_dof;
    short   cycle_type;
    double  quality_bound;
    short   smoother;
    short   smooth_order;
    short   presmooth_iter;
    short   postsmooth_iter;
    double  relaxation;
    short   polynomial_degree;
    short   coarse_solver;
    short   coarse_scaling;
    short   amli_degree;
    double* amli_coef;
    short   nl_amli_krylov_type;
    short   coarsening_type;
    short   aggregation_type;
    short   aggregation_norm_type;
    short   interpolation_type;
    double  strong_threshold;
    double  max_row_sum;
    double  truncation_threshold;
    int     aggressive_level;
    int     aggressive_path;
    int     pair_number;
    double  strong_coupled;
    int     max_aggregation;
    double  tentative_smooth;
    short   smooth_filter;
    short   smooth_restriction;
    short   ILU_levels;
    short   ILU_type;
    int     ILU_lfil;
    double  ILU_droptol;
    double  ILU_relax;
    double  ILU_permtol;
    int     SWZ_levels;
    int     SWZ_mmsize;
    int     SWZ_maxlvl;
    int     SWZ_type;
    int     SWZ_blksolver;
    double  theta;
} AMG_param;

/* fasp.h:1095  sizeof == 16 */
typedef struct {
    void* data;
    void (*fct)(double*, double*, void*);
} precond;

/* ---- reference-layout data of the AMG preconditioner (fasp.h:596-981, serial build without UMFPACK / MUMPS /
 * PARDISO / MULTI_COLOR_ORDER).  Field order and types are the reference's, so code compiled against fasp.h and
 * code compiled against this header agree on every offset (sizes pinned in tests/golden/abi.npz:
 * AMG_data 1104 bytes, precond_data 152 bytes).  ILU_param / ILU_data are those of the ILU preconditioner below
 * (fasp_ilu_dcsr_setup); the ILU / Schwarz smoother and direct-solver members of AMG_data are carried for layout only:
 * those smoothers and coarse solvers are out of scope here and stay zero. ---- */
typedef struct {            /* fasp.h:404  ILU_param */
    short  print_level;
    short  ILU_type;
    int    ILU_lfil;
    double ILU_droptol;
    double ILU_relax;
    double ILU_permtol;
} ILU_param;
typedef struct SWZ_param_ { /* fasp.h:430  SWZ_param */
    short print_level;
    short SWZ_type;
    int   SWZ_maxlvl;
    int   SWZ_mmsize;
    int   SWZ_blksolver;
} SWZ_param;
typedef struct { int job; } Mumps_data;            /* fasp.h:596 */
typedef struct { void* pt[64]; } Pardiso_data;     /* fasp.h:623 */
typedef struct {            /* fasp.h:651  ILU_data */
    dCSRmat* A;
    int      type, row, col, nzlu;
    int*     ijlu;
    double*  luval;
    int      nb, nwork;
    double*  work;
    int*     iperm;
    int      ncolors;
    int     *ic, *icmap, *uptr;
    int      nlevL, nlevU;
    int     *ilevL, *ilevU, *jlevL, *jlevU;
} ILU_data;
typedef struct {            /* fasp.h:724  SWZ_data */
    dCSRmat  A;
    int      nblk;
    int     *iblock, *jblock;
    double*  rhsloc;
    dvector  rhsloc1, xloc1;
    double  *au, *al;
    int      SWZ_type, blk_solver, memt;
    int*     mask;
    int      maxbs;
    int*     maxa;
    dCSRmat* blk_data;
    Mumps_data*        mumps;
    struct SWZ_param_* swzparam;
} SWZ_data;
typedef struct {            /* fasp.h:804  AMG_data: one per level, mgl[0 .. num_levels) */
    short        max_levels;
    short        num_levels;
    dCSRmat      A, R, P;          /* host copies of this level's operators (this library: views of its own hierarchy) */
    dvector      b, x;             /* host vectors of this level (scratch of the reference's cycle; unused by the device cycle) */
    void*        Numeric;
    Pardiso_data pdata;
    ivector      cfmark;
    int          ILU_levels;
    ILU_data     LU;
    int          near_kernel_dim;
    double**     near_kernel_basis;
    int          SWZ_levels;
    SWZ_data     Schwarz;
    dvector      w;
    Mumps_data   mumps;
    int          cycle_type;
    int         *ic, *icmap;
    int          colors;
    double       weight;
} AMG_data;
typedef struct {            /* fasp.h:894  precond_data */
    short     AMG_type, print_level;
    int       maxit;
    short     max_levels;
    double    tol;
    short     cycle_type, smoother, smooth_order, presmooth_iter, postsmooth_iter;
    double    relaxation;
    short     polynomial_degree, coarsening_type, coarse_solver, coarse_scaling, amli_degree, nl_amli_krylov_type;
    double    tentative_smooth;
    double*   amli_coef;
    AMG_data* mgl_data;
    ILU_data* LU;
    dCSRmat  *A, *A_nk, *P_nk, *R_nk;
    dvector   r;
    double*   w;
} precond_data;

/* fasp_block.h:255  data of the block-diagonal preconditioner */
typedef struct {
    int     nb;
    dvector diag;   /* ROW inverse diagonal blocks of nb*nb doubles */
} precond_diag_bsr;

/* fasp.h:1074  data of the block-diagonal preconditioner of a dSTRmat */
typedef struct {
    int     nc;
    dvector diag;   /* ngrid inverse diagonal blocks of nc*nc doubles */
} precond_diag_str;

/* fasp.h:984  data of the preconditioners of a dSTRmat (the reference's CPR-type preconditioners); fasp_precond_dstr_blockgs reads
 * A_str, diaginv, pivot, order and neigh, the other members are carried for layout only */
typedef struct {
    short     AMG_type, print_level;
    int       maxit;
    short     max_levels;
    double    tol;
    short     cycle_type, smoother, presmooth_iter, postsmooth_iter, coarsening_type;
    double    relaxation;
    short     coarse_scaling;
    AMG_data* mgl_data;
    ILU_data* LU;
    short     scaled;
    dCSRmat*  A;
    dSTRmat  *A_str, *SS_str;
    dvector*  diaginv;    /* ngrid factored patches (fasp_generate_diaginv_block) */
    ivector*  pivot;      /* ... and their pivots */
    dvector*  diaginvS;
    ivector*  pivotS;
    ivector*  order;      /* the visiting sequence, NULL: natural */
    ivector*  neigh;      /* ngrid * nneigh neighbours, < 0: absent; NULL: none */
    dvector   r;
    double*   w;
} precond_data_str;

/* fasp.h:1109  matrix-free operator: y = A x through a function pointer */
typedef struct {
    void* data;
    void (*fct)(const void*, const double*, double*);
} mxv_matfree;
#define MAT_FREE 0
#define MAT_CSR  1
#define MAT_BSR  2
#define MAT_STR  3

/* ------------------------------------------------------------------------ */
/* reference entry points kept by this library                              */
/* ------------------------------------------------------------------------ */

/* AuxParam.c:431 -- defaults: classical AMG, GS smoother with C/F order, V(1,1),
 * coarse_dof 500, max_levels 20, theta 0.3, max_row_sum 0.9, trunc 0.2 ... */
void fasp_param_amg_init(AMG_param* amgparam);

/* AuxParam.c:572 -- defaults: CG, AMG precond, STOP_REL_RES, maxit 500,
 * restart 25, tol 1e-6, abstol 1e-18 */
void fasp_param_solver_init(ITS_param* itsparam);

/* SolCSR.c:476 -- the drop-in entry point.  Host arrays in, host arrays out.
 * Deep-copies A, builds the AMG hierarchy (host), uploads it, runs the whole
 * Krylov loop on the bound MI355X, copies x back, frees everything.
 * Returns the iteration count (>=0) or a negative ERROR_* code.  Parameter
 * combinations this library has no device path for (ILU/Schwarz smoothers,
 * AMLI cycles, direct coarse solvers, ...) return an error; they never fall
 * back to a CPU solve. */
int fasp_solver_dcsr_krylov_amg(dCSRmat* A, dvector* b, dvector* x,
                                ITS_param* itparam, AMG_param* amgparam);

/* Kernel-level operators of the path, same names and semantics as the
 * reference, host pointers in/out (upload -> HIP kernel -> download).  They
 * exist so the reference's own call sites / tests of these operators can be
 * pointed at the device kernels; hot loops use the handle API below instead. */
void   fasp_blas_dcsr_mxv(const dCSRmat* A, const double* x, double* y);              /* BlaSpmvCSR.c:242 */
void   fasp_blas_dcsr_aAxpy(const double alpha, const dCSRmat* A, const double* x,
                            double* y);                                               /* BlaSpmvCSR.c:494 */
double fasp_blas_darray_dotprod(const int n, const double* x, const double* y);       /* BlaArray.c:771 */
double fasp_blas_darray_norm2(const int n, const double* x);                          /* BlaArray.c:691 */
double fasp_blas_darray_norminf(const int n, const double* x);                        /* BlaArray.c:719 */
void   fasp_blas_darray_axpy(const int n, const double a, const double* x, double* y); /* BlaArray.c:90 */
void   fasp_blas_darray_axpby(const int n, const double a, const double* x,
                              const double b, double* y);                             /* BlaArray.c:620 */
/* the Galerkin product RAP = R A P on the device, the reference's result byte for byte (IA, JA, val; every row starts with its
 * diagonal slot, the other columns in discovery order).  Host arrays in and out; RAP's arrays are allocated with fasp_mem_calloc
 * (release them with fasp_dcsr_free).  Wrong dimensions or more than 2^31 - 1 entries: prints "### ERROR: ..." and exits with the
 * status, as fasp_chkerr does. */
void   fasp_blas_dcsr_rap(const dCSRmat* R, const dCSRmat* A, const dCSRmat* P, dCSRmat* RAP);   /* BlaSpmvCSR.c:999 */
/* the remaining kernel-level names of the path, host arrays in and out */
double fasp_blas_dcsr_vmv(const dCSRmat* A, const double* x, const double* y);           /* BlaSpmvCSR.c:839  y' A x */
void   fasp_blas_dcsr_mxv_agg(const dCSRmat* A, const double* x, double* y);             /* BlaSpmvCSR.c:438  unit entries, val unread */
void   fasp_blas_dcsr_aAxpy_agg(const double alpha, const dCSRmat* A, const double* x,
                                double* y);                                              /* BlaSpmvCSR.c:727 */
void   fasp_blas_darray_ax(const int n, const double a, double* x);                      /* BlaArray.c:43 */
void   fasp_blas_darray_axpyz(const int n, const double a, const double* x,
                              const double* y, double* z);                               /* BlaArray.c:403 */
double fasp_blas_darray_norm1(const int n, const double* x);                             /* BlaArray.c:663 */
void   fasp_darray_cp(const int n, const double* x, double* y);                          /* AuxArray.c:210 */
void   fasp_darray_set(const int n, double* x, const double val);                        /* AuxArray.c:41 */
short  fasp_dvec_isnan(const dvector* u);                                                /* AuxVector.c:39 */
void   fasp_smoother_dcsr_jacobi(dvector* u, const int i_1, const int i_n, const int s,
                                 dCSRmat* A, dvector* b, int L, const double w);      /* ItrSmootherCSR.c:98 */

/* Block (BSR) operators of config 3, same conventions (host pointers, device kernels).
 * nb <= 7: every block contributes y_r += (A_r0 x_0 + A_r1 x_1 + ...), inner sum first, exactly
 * as fasp_blas_smat_ypAx (BlaSmallMat.c:779). */
void   fasp_blas_dbsr_mxv(const dBSRmat* A, const double* x, double* y);              /* BlaSpmvBSR.c:1055 */
void   fasp_blas_dbsr_aAxpy(const double alpha, const dBSRmat* A, const double* x,
                            double* y);                                               /* BlaSpmvBSR.c:514 */
dvector fasp_dbsr_getdiaginv(const dBSRmat* A);                                       /* BlaSparseBSR.c:543 (host; nb <= 3) */
void   fasp_smoother_dbsr_jacobi1(dBSRmat* A, dvector* b, dvector* u, double* diaginv); /* ItrSmootherBSR.c:263 */
/* mean milliseconds per launch of the BSR SpMV kernel on a resident copy of A (HIP events) */
double fasp_hip_time_bsr_mxv(const dBSRmat* A, int reps);

/* Structured (STR) matrices, BlaSparseSTR.c:41-162, BlaFormat.c:119, BlaSpmvSTR.c:61/:131 -- the reference's third Krylov format.
 * create / alloc / free / cp / fasp_format_dstr_dcsr are host code (no GPU needed; arrays from fasp_mem_calloc, B's CSR arrays
 * are released with fasp_dcsr_free; fasp_dstr_cp copies into an allocated B as the reference does).  The two products take host
 * vectors of ngrid*nc doubles and run k_str_band on the device: no column indices, and the reference's result bit for bit in each of
 * its four arithmetic forms.  fasp_blas_dstr_mxv clears and writes exactly ngrid*nc entries of y (the reference
 * clears ngrid*nc*nc, BlaSpmvSTR.c:135).  A matrix with nc outside 1..7, nband < 0, an offset of 0 or a repeated offset: message and
 * exit(ERROR_INPUT_PAR); a band with |offset| >= ngrid is legal and empty. */
dSTRmat fasp_dstr_create(const int nx, const int ny, const int nz, const int nc, const int nband, int* offsets);
void    fasp_dstr_alloc(const int nx, const int ny, const int nz, const int nxy, const int ngrid, const int nband,
                        const int nc, int* offsets, dSTRmat* A);
void    fasp_dstr_free(dSTRmat* A);
void    fasp_dstr_cp(const dSTRmat* A, dSTRmat* B);
short   fasp_format_dstr_dcsr(const dSTRmat* A, dCSRmat* B);
void    fasp_blas_dstr_aAxpy(const double alpha, const dSTRmat* A, const double* x, double* y);
void    fasp_blas_dstr_mxv(const dSTRmat* A, const double* x, double* y);

/* ini front-end: fasp_param_input (AuxInput.c:86) + fasp_param_init (AuxParam.c:34) for the two parameter
 * structs of this path -- same keywords, value formats, defaults and range check as the reference's
 * ini files (test/ini/, .dat).  fname == NULL: defaults.  Returns 0, ERROR_OPEN_FILE (-10) or
 * ERROR_INPUT_PAR; pure host code. */
int  fasp_hip_param_input(const char* fname, ITS_param* itsparam, AMG_param* amgparam);
/* Readers of the reference's ASCII data formats (base/src/BlaIO.c:164, :938, :807).  Same formats and
 * messages; an error code is returned where the reference exits.  Arrays are malloc-family
 * allocations: release with fasp_hip_free_system / fasp_hip_free_bsr / free(). */
int  fasp_dcsrvec_read2(const char* filemat, const char* filerhs, dCSRmat* A, dvector* b);
int  fasp_dvec_read(const char* filename, dvector* b);
int  fasp_dbsr_read(const char* filename, dBSRmat* A);
/* BlaIO.c:699: "nx ny nz / nc / nband / n diag.. / offset n band.." per band; release with fasp_dstr_free */
int  fasp_dstr_read(const char* filename, dSTRmat* A);
/* coordinate formats (BlaIO.c:332 0-based, :384 / :514 / :567 1-based, :624 one triangle of a
 * symmetric MatrixMarket file) and the writers that pair with the readers (:1388, :1623, :1145) */
int  fasp_dcoo_read(const char* filename, dCSRmat* A);
int  fasp_dcoo_read1(const char* filename, dCSRmat* A);
int  fasp_dcoo_shift_read(const char* filename, dCSRmat* A);
int  fasp_dmtx_read(const char* filename, dCSRmat* A);
int  fasp_dmtxsym_read(const char* filename, dCSRmat* A);
int  fasp_dvec_write(const char* filename, dvector* vec);
int  fasp_dcsr_write_coo(const char* filename, const dCSRmat* A);
int  fasp_dcsrvec_write2(const char* filemat, const char* filerhs, dCSRmat* A, dvector* b);
void fasp_hip_free_bsr(dBSRmat* A);
/* Fortran-style wrapper, SolWrapper.c:261: parameters from "ini/amg.dat" in the working directory */
void fasp_fwrapper_dcsr_krylov_amg_(int* n, int* nnz, int* ia, int* ja, double* a, double* b, double* u,
                                    double* tol, int* maxit, int* ptrlvl);
/* SolWrapper.c:136 (AMG as the solver) and :397 (block matrix: UA-AMG + VFGMRES) */
void fasp_fwrapper_dcsr_amg_(int* n, int* nnz, int* ia, int* ja, double* a, double* b, double* u,
                             double* tol, int* maxit, int* ptrlvl);
void fasp_fwrapper_dbsr_krylov_amg_(int* n, int* nnz, int* nb, int* ia, int* ja, double* a, double* b,
                                    double* u, double* tol, int* maxit, int* ptrlvl);

/* AMG-preconditioned Krylov solve on a block matrix -- replaces base/src/SolBSR.c:349.
 * Unsmoothed aggregation (PreAMGSetupUABSR.c:55, VMB on the condensed matrix, identity-block
 * prolongation, block Galerkin product) on the host, block-Jacobi V/W cycle
 * (PreMGCycle.c:287) with GMRES(25) on the coarsest level and PCG / VGMRES / VFGMRES
 * (KryPcg.c:386, KryPvgmres.c:416, KryPvfgmres.c:386) on the device.  Returns the iteration
 * count or a negative ERROR_* code; unsupported parameters are refused, never run on the CPU. */
int fasp_solver_dbsr_krylov_amg(dBSRmat* A, dvector* b, dvector* x, ITS_param* itparam,
                                AMG_param* amgparam);

/* Resident form of the block path (extension): setup + upload once, solve many times. */
typedef struct fasp_hip_amg_bsr fasp_hip_amg_bsr;
int  fasp_hip_bsr_amg_create(fasp_hip_amg_bsr** h, const dBSRmat* A, AMG_param* amgparam);
int  fasp_hip_bsr_amg_create_host(fasp_hip_amg_bsr** h, const dBSRmat* A, AMG_param* amgparam); /* no GPU needed */
void fasp_hip_bsr_amg_destroy(fasp_hip_amg_bsr* h);
int  fasp_hip_bsr_amg_num_levels(const fasp_hip_amg_bsr* h);
/* which: 0 = A_l, 1 = P_l, 2 = R_l; the view aliases host memory owned by the handle */
int  fasp_hip_bsr_amg_get_matrix(const fasp_hip_amg_bsr* h, int level, int which, dBSRmat* view);
const double* fasp_hip_bsr_amg_get_diaginv(const fasp_hip_amg_bsr* h, int level);

/* ------------------------------------------------------------------------ */
/* extensions: device binding, resident hierarchy, instrumentation          */
/* ------------------------------------------------------------------------ */

/* Bind the calling process to one GPU (default: device 0 on first use). */
int fasp_hip_set_device(int device);
/* Number of visible GPUs, or a negative ERROR_* code. */
int fasp_hip_device_count(void);
/* PCI bus id of the device this process is bound to into out (cap >= 16); returns the device index or a negative ERROR_* code. */
int fasp_hip_device_identity(char* out, int cap);
/* 1 when a gfx950 device is usable, else 0 (never initialises a fallback). */
int fasp_hip_available(void);

typedef struct fasp_hip_amg fasp_hip_amg; /* opaque: host + device hierarchy */

/* Host setup (classical RS, bit-compatible with PreAMGSetupRS.c:52) followed by
 * upload of every level's A/R/P to HBM.  A is deep-copied.  amgparam is
 * mutated exactly as the reference mutates it (tentative_smooth = 1.0 ...). */
int fasp_hip_amg_create(fasp_hip_amg** out, const dCSRmat* A, AMG_param* amgparam);
/* The two halves of fasp_hip_amg_create: host setup only (needs no GPU; the handle
 * can be inspected with the getters below) and the upload to the bound GPU. */
int fasp_hip_amg_create_host(fasp_hip_amg** out, const dCSRmat* A, AMG_param* amgparam);
int fasp_hip_amg_upload(fasp_hip_amg* h);
/* One host setup per node: the process that ran fasp_hip_amg_create_host publishes the host
 * hierarchy (and the parameters as the setup left them) in the POSIX shared-memory segment /<name>; the other ranks
 * of the node attach to it -- a host-only handle whose arrays are read-only views of the segment -- and call
 * fasp_hip_amg_upload, which extracts and uploads the rows they own.  unpublish removes the name once every rank has
 * attached (the mapping of an attached handle lives until fasp_hip_amg_destroy). */
int fasp_hip_amg_publish(const fasp_hip_amg* h, const char* name);
int fasp_hip_amg_attach(fasp_hip_amg** out, const char* name);
int fasp_hip_amg_unpublish(const char* name);
void fasp_hip_amg_destroy(fasp_hip_amg* h);

/* Hierarchy inspection (parity tests compare these with the oracle). */
int fasp_hip_amg_num_levels(const fasp_hip_amg* h);
/* host-only round-trip check of the lossless matrix coding applied at upload:
 * *kind = 5 row-pattern coded, 4 byte-dictionary coded, 0 stays plain CSR; returns 0 if exact */
int  fasp_hip_coding_selftest(const dCSRmat* A, int* kind);
/* kernel family that serves y = M x on operator `which` (0 A, 1 P, 2 R) of a level -- 0: sub-wavefront per row (or its
 * entry-parallel form), 2: wave-level stream, 4: byte-dictionary coded, 5: row-pattern coded (6, 9: its pair sweeps for square
 * and rectangular operators), 7, 8, 10, 11: the second-generation plain kernels (fasp_hip_dev.h lists them) -- and the matrix
 * bytes one pass of it reads; evaluated under the tune keys in force, from the plan the launch itself executes */
int  fasp_hip_amg_kernel_info(const fasp_hip_amg* h, int level, int which, int* kind, double* matrix_bytes);
/* which: 0 = A_l, 1 = P_l, 2 = R_l.  Returns host views owned by the handle. */
int fasp_hip_amg_get_matrix(const fasp_hip_amg* h, int level, int which, dCSRmat* view);
int fasp_hip_amg_get_cfmark(const fasp_hip_amg* h, int level, ivector* view);

/* Per-solve statistics filled by fasp_hip_solve. */
typedef struct {
    int    iters;            /* return value of the Krylov method */
    int    nhist;            /* entries written to hist */
    double relres;           /* final relative residual (as printed by ITS_FINAL) */
    double absres;           /* final ||r||_2 */
    double normr0;           /* max(1e-20, ||r0||_2) */
    double solve_seconds;    /* wall time of the Krylov loop, device-synchronised */
    double upload_seconds;   /* H2D of b, x0 and D2H of x */
    double spmv_ms;          /* mean duration of the level-0 A*p kernel (HIP events) */
    long long spmv_launches; /* number of launches averaged in spmv_ms */
    long long coarse_iters;  /* total coarsest-level SPCG iterations */
    long long vcycles;       /* number of multigrid cycles executed */
} fasp_hip_stats;

/* Krylov solve on a resident hierarchy.  hist (may be NULL) receives the
 * absolute residual norms ||r_k||_2, k = 0..iters, up to hist_cap entries. */
int fasp_hip_solve(fasp_hip_amg* h, const dvector* b, dvector* x, const ITS_param* itparam,
                   double* hist, int hist_cap, fasp_hip_stats* stats);

int fasp_hip_bsr_solve(fasp_hip_amg_bsr* h, const dvector* b, dvector* x, const ITS_param* itparam,
                       double* hist, int hist_cap, fasp_hip_stats* stats);
/* one process per GPU (fasp_hip_comm_init before the create call): block rows of level 0 this rank owns --
 * info[0] = 1 if level 0 is whole on every rank, [1] first owned block row, [2] owned block rows, [3] ghost blocks,
 * [4] first level kept whole, [5] block size.  fasp_hip_bsr_solve takes the GLOBAL b and x; a rank fills its rows of x. */
int fasp_hip_bsr_dist_info(const fasp_hip_amg_bsr* h, int* info);

/* The same solve in three steps, for callers that keep b and x resident in HBM:
 * upload the right-hand side / initial guess (x == NULL: zeros), run the Krylov loop on
 * the resident vectors, download the solution. */
int fasp_hip_set_rhs(fasp_hip_amg* h, const dvector* b);
int fasp_hip_set_guess(fasp_hip_amg* h, const dvector* x);
int fasp_hip_solve_resident(fasp_hip_amg* h, const ITS_param* itparam, double* hist, int hist_cap,
                            fasp_hip_stats* stats);
int fasp_hip_get_solution(fasp_hip_amg* h, dvector* x);
int fasp_hip_device_synchronize(void);

/* AMG as a stand-alone solver -- replaces base/src/SolAMG.c:49 (+ PreMGSolve.c:49): setup,
 * then multigrid cycles until ||b - A x|| / ||b|| < param->tol or param->maxit cycles.
 * Returns the cycle count or a negative ERROR_* code (a failed setup returns its code; the
 * reference's CPU GMRES fallback does not exist here). */
int fasp_solver_amg(dCSRmat* A, dvector* b, dvector* x, AMG_param* param);
/* One full-multigrid cycle as the solver -- replaces base/src/SolFAMG.c:41 (void there; the status is an
 * extension).  x: initial guess in, result out.  itparam->precond_type = PREC_FMG selects the same cycle as
 * the preconditioner of fasp_solver_dcsr_krylov_amg (SolCSR.c:537). */
int fasp_solver_famg(const dCSRmat* A, const dvector* b, dvector* x, AMG_param* param);
/* the same iteration on a resident hierarchy; param == NULL: the parameters of the setup */
int fasp_hip_amg_solve(fasp_hip_amg* h, const dvector* b, dvector* x, const AMG_param* param,
                       double* hist, int hist_cap, fasp_hip_stats* stats);

/* ---- plug-in level (fasp.h:1095-1103): Krylov methods with a caller-supplied preconditioner ---- */
/* KryPcg.c:96, KryPvgmres.c:66, KryPvfgmres.c:67 -- same arguments, return values and
 * safeguards; SpMV, BLAS-1 and orthogonalisation run on the device.  pc == NULL: no
 * preconditioner.  pc->fct == fasp_hip_precond_fct: the whole iteration stays in HBM.
 * Any other pc->fct is called as a host function on host copies of r and z (one PCIe round
 * trip per application) -- e.g. a reference preconditioner kept on the CPU.  fasp_precond_swz, fasp_precond_ilu / _forward /
 * _backward are recognised by their address and applied on the device (triangular solves in HBM). */
int fasp_solver_dcsr_pcg(dCSRmat* A, dvector* b, dvector* u, precond* pc, const double tol,
                         const double abstol, const int MaxIt, const short StopType, const short PrtLvl);
int fasp_solver_dcsr_pbcgs(dCSRmat* A, dvector* b, dvector* u, precond* pc, const double tol,
                           const double abstol, const int MaxIt, const short StopType, const short PrtLvl); /* KryPbcgs.c:62 */
/* Solver-level entry points next to the AMG drop-in (SolCSR.c:56/:245/:333, SolBSR.c:64/:145/:186): dispatch on
 * itsolver_type with a caller's preconditioner, without one, or with the (block-)diagonal one.  fasp_precond_diag
 * (PreCSR.c:172) and fasp_precond_dbsr_diag (PreBSR.c:49) are host functions usable anywhere a `precond` is; handed
 * to this library's Krylov methods they are recognised by their address and applied on the device. */
void fasp_precond_diag(double* r, double* z, void* data);        /* data: dvector* of diagonal entries */
void fasp_precond_dbsr_diag(double* r, double* z, void* data);   /* data: precond_diag_bsr* */
int  fasp_solver_dcsr_itsolver(dCSRmat* A, dvector* b, dvector* x, precond* pc, ITS_param* itparam);
int  fasp_solver_dcsr_krylov(dCSRmat* A, dvector* b, dvector* x, ITS_param* itparam);
int  fasp_solver_dcsr_krylov_diag(dCSRmat* A, dvector* b, dvector* x, ITS_param* itparam);
int  fasp_solver_dbsr_itsolver(dBSRmat* A, dvector* b, dvector* x, precond* pc, ITS_param* itparam);
int  fasp_solver_dbsr_krylov(dBSRmat* A, dvector* b, dvector* x, ITS_param* itparam);
int  fasp_solver_dbsr_krylov_diag(dBSRmat* A, dvector* b, dvector* x, ITS_param* itparam);
/* The same for structured matrices (KryPcg.c:970, KryPbcgs.c:1027, KryPgmres.c:998, KryPvgmres.c:1116, KryPminres.c:876;
 * SolSTR.c:51/:132/:175; PreSTR.c:44).  One GPU; the operator is uploaded once as index-free bands and the iteration stays in
 * HBM.  fasp_precond_dstr_diag (data: precond_diag_str*) is recognised by its address and applied on the device, any other
 * preconditioner is called on host copies.  fasp_solver_dstr_itsolver dispatches CG, BiCGstab, GMRES and VGMRES as the reference
 * does (anything else: ERROR_SOLVER_TYPE).  ERROR_INPUT_PAR: a NULL pointer, nc outside 1..7, nband < 0, an offset of 0 or a
 * repeated one, vectors of another length than ngrid*nc, more than one rank. */
void fasp_precond_dstr_diag(double* r, double* z, void* data);
int  fasp_solver_dstr_pcg(dSTRmat* A, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                          const int MaxIt, const short StopType, const short PrtLvl);
int  fasp_solver_dstr_pbcgs(dSTRmat* A, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                            const int MaxIt, const short StopType, const short PrtLvl);
int  fasp_solver_dstr_pminres(dSTRmat* A, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                              const int MaxIt, const short StopType, const short PrtLvl);
int  fasp_solver_dstr_pgmres(dSTRmat* A, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                             const int MaxIt, const short restart, const short StopType, const short PrtLvl);
int  fasp_solver_dstr_pvgmres(dSTRmat* A, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                              const int MaxIt, const short restart, const short StopType, const short PrtLvl);
int  fasp_solver_dstr_itsolver(dSTRmat* A, dvector* b, dvector* x, precond* pc, ITS_param* itparam);
int  fasp_solver_dstr_krylov(dSTRmat* A, dvector* b, dvector* x, ITS_param* itparam);
int  fasp_solver_dstr_krylov_diag(dSTRmat* A, dvector* b, dvector* x, ITS_param* itparam);
/* Structured ILU(0) / ILU(1).  fasp_ilu_dstr_setup0 / _setup1 (BlaILUSetupSTR.c:38 / :333) are host
 * code (no GPU needed): LU is allocated with fasp_mem_calloc, released with fasp_dstr_free, and equals the reference's factor
 * byte for byte for nc 1 .. 7.  A has 4 bands {+-1, +-nline} on a 2-D grid or 6 bands {+-1, +-nline, +-nplane} on a 3-D one;
 * setup0 takes them in any storage order and always labels LU with the canonical order -1, +1, -nline, +nline, -nplane, +nplane,
 * setup1 takes the canonical order only.  Refused, with a message and LU zeroed (null arrays, ngrid 0): another nband, another
 * offset, nline < 2 or a grid of one line, nc outside 1 .. 7.
 * fasp_precond_dstr_ilu0 / _ilu1 (PreSTR.c:71 / :349; data: the dSTRmat LU) are host functions too.  Handed to an STR Krylov
 * method they are recognised by their address: the factor is uploaded once per solve and both triangular solves run on the
 * device (k_str_tri) with the reference's result.  A factor with a non-zero coefficient between grid points that are not
 * geometric neighbours (no grid-derived matrix has one) is applied through the host function instead.
 * fasp_solver_dstr_krylov_ilu (SolSTR.c:236): ILU_lfil 0 or 1 (else the reference's message and ERROR_MISC), setup, solve, LU
 * freed; a refused setup returns ERROR_INPUT_PAR. */
void fasp_ilu_dstr_setup0(dSTRmat* A, dSTRmat* LU);                 /* BlaILUSetupSTR.c:38 */
void fasp_ilu_dstr_setup1(dSTRmat* A, dSTRmat* LU);                 /* BlaILUSetupSTR.c:333 */
void fasp_precond_dstr_ilu0(double* r, double* z, void* data);      /* PreSTR.c:71 */
void fasp_precond_dstr_ilu1(double* r, double* z, void* data);      /* PreSTR.c:349 */
int  fasp_solver_dstr_krylov_ilu(dSTRmat* A, dvector* b, dvector* x, ITS_param* itparam, ILU_param* iluparam);   /* SolSTR.c:236 */
/* The structured smoothers (ItrSmootherSTR.c): one sweep on the device, host vectors of ngrid*nc, one-shot
 * (upload, sweep, download) as fasp_smoother_dcsr_gs, with the reference's result bit for bit.  Orders, as _gs1 / _sor1 dispatch them:
 * mark == NULL: ASCEND or DESCEND, any other order does nothing; mark != NULL: USERDEFINED -- mark is the visiting sequence of the
 * ngrid points -- and any other order is the C/F form with FIRST = order, SECOND = -order: the points marked FIRST ascending, then those
 * marked SECOND; points marked neither are not visited (the _cf entries take this form whatever `order` is).  The entries without the
 * trailing 1 invert the diagonal blocks on the host for nc > 1 (fasp_smat_inv); the others take them as diaginv (NULL for nc = 1).
 * The reference's scalar fasp_smoother_dstr_sor_cf closes the points of its SECOND pass without the weight (ItrSmootherSTR.c:1443); so
 * does this one.  nc < 1: the reference's message, nothing done.  Refused with a message, u untouched: a USERDEFINED sequence with an
 * entry outside 0 .. ngrid-1 or a point named twice; NULL diaginv with nc > 1 where it is an argument.  nc > 7 and any matrix
 * fasp_hip_str_form refuses end the process like the other STR entries. */
#ifndef ASCEND
#define ASCEND      12   /* fasp_const.h: the orders of the structured smoothers */
#define DESCEND     21
#define USERDEFINED 0
#define CPFIRST     1
#define FPFIRST     (-1)
#endif
void fasp_smoother_dstr_jacobi(dSTRmat* A, dvector* b, dvector* u);                                                   /* ItrSmootherSTR.c:43 */
void fasp_smoother_dstr_jacobi1(dSTRmat* A, dvector* b, dvector* u, double* diaginv);                                 /* ItrSmootherSTR.c:92 */
void fasp_smoother_dstr_gs(dSTRmat* A, dvector* b, dvector* u, const int order, int* mark);                           /* ItrSmootherSTR.c:217 */
void fasp_smoother_dstr_gs1(dSTRmat* A, dvector* b, dvector* u, const int order, int* mark, double* diaginv);         /* ItrSmootherSTR.c:277 */
void fasp_smoother_dstr_gs_ascend(dSTRmat* A, dvector* b, dvector* u, double* diaginv);                               /* ItrSmootherSTR.c:322 */
void fasp_smoother_dstr_gs_descend(dSTRmat* A, dvector* b, dvector* u, double* diaginv);                              /* ItrSmootherSTR.c:438 */
void fasp_smoother_dstr_gs_order(dSTRmat* A, dvector* b, dvector* u, double* diaginv, int* mark);                     /* ItrSmootherSTR.c:556 */
void fasp_smoother_dstr_gs_cf(dSTRmat* A, dvector* b, dvector* u, double* diaginv, int* mark, const int order);       /* ItrSmootherSTR.c:680 */
void fasp_smoother_dstr_sor(dSTRmat* A, dvector* b, dvector* u, const int order, int* mark, const double weight);     /* ItrSmootherSTR.c:873 */
void fasp_smoother_dstr_sor1(dSTRmat* A, dvector* b, dvector* u, const int order, int* mark, double* diaginv, const double weight);   /* ItrSmootherSTR.c:935 */
void fasp_smoother_dstr_sor_ascend(dSTRmat* A, dvector* b, dvector* u, double* diaginv, double weight);               /* ItrSmootherSTR.c:981 */
void fasp_smoother_dstr_sor_descend(dSTRmat* A, dvector* b, dvector* u, double* diaginv, double weight);              /* ItrSmootherSTR.c:1102 */
void fasp_smoother_dstr_sor_order(dSTRmat* A, dvector* b, dvector* u, double* diaginv, int* mark, double weight);     /* ItrSmootherSTR.c:1224 */
void fasp_smoother_dstr_sor_cf(dSTRmat* A, dvector* b, dvector* u, double* diaginv, int* mark, const int order, const double weight);   /* ItrSmootherSTR.c:1355 */

/* The block Gauss-Seidel (Schwarz) smoother and preconditioner of a structured matrix.  The patch of grid point i is
 * [i, neigh[i * nneigh + 0 .. nneigh)] without the absent entries (< 0; nneigh = neigh->row / ngrid, neigh == NULL: none), m = members * nc
 * rows; a point may be named twice or name itself.  order: the visiting sequence (ngrid entries, a point may come twice), NULL: natural.
 * fasp_generate_diaginv_block assembles and factors every patch on the device (LU with row interchanges, fasp_smat_lu_decomp) and delivers
 * the reference's host layout and bytes: diaginv[i].row = m_i^2, pivot[i].row = m_i, all values carved in order from one zero-initialised
 * fasp_mem_calloc block of ((nneigh+1) nc)^2 ngrid doubles / (nneigh+1) nc ngrid ints (diaginv[0].val and pivot[0].val are the bases); a patch
 * whose factorisation stops (a pivot below 1e-20) holds what the reference leaves.  fasp_smoother_dstr_swz: one sweep, one-shot (upload, the
 * caller's factors repacked, sweep, download), the reference's result bit for bit.  fasp_precond_dstr_blockgs (data: precond_data_str*):
 * z = 0 and one sweep with b = r; handed to an STR Krylov method it is recognised by its address and stays on the device, called directly
 * (also from inside another preconditioner of a running solve) it is one-shot.  fasp_solver_dstr_krylov_blockgs factors on the device (the
 * factors are never downloaded), solves with fasp_solver_dstr_itsolver and prints the reference's lines.
 * nc < 1: the reference's message, nothing done.  nc > 7 and any matrix fasp_hip_str_form refuses end the process like the other STR entries
 * (the solver entry returns ERROR_INPUT_PAR).  Refused with a message, u / z untouched (the solver entry: ERROR_INPUT_PAR): a neigh entry >=
 * ngrid, neigh->row no multiple of ngrid, an order of fewer than ngrid entries or with an entry outside 0 .. ngrid-1, a patch of more than
 * 64 rows, factors whose row fields or pivots (k <= pivot[k] < m) do not fit the patches, a factorisation that stopped or a factor with 0.0 on
 * U's diagonal (the reference would go on with the correction of the visit before).  A factor store that does not fit: ERROR_ALLOC_MEM. */
void fasp_generate_diaginv_block(dSTRmat* A, ivector* neigh, dvector* diaginv, ivector* pivot);                                          /* ItrSmootherSTR.c:1543 */
void fasp_smoother_dstr_swz(dSTRmat* A, dvector* b, dvector* u, dvector* diaginv, ivector* pivot, ivector* neigh, ivector* order);      /* ItrSmootherSTR.c:1665 */
void fasp_precond_dstr_blockgs(double* r, double* z, void* data);                                                                       /* PreSTR.c:1715 */
int  fasp_solver_dstr_krylov_blockgs(dSTRmat* A, dvector* b, dvector* x, ITS_param* itparam, ivector* neigh, ivector* order);           /* SolSTR.c:323 */

/* Matrix-free interface (SolMatFree.c:58/:157/:201; KryPcg.c:1260, KryPbcgs.c:1349, KryPgcg.c:213,
 * KryPgmres.c:1309, KryPvgmres.c:1468, KryPvfgmres.c:1026, KryPminres.c:1283 -- the reference keeps older texts of
 * CG, GMRES and MinRes for this interface; they are what runs here).  fasp_solver_matfree_init(MAT_CSR | MAT_BSR | MAT_STR)
 * installs fasp_hip_mxv_csr / _bsr / _str: such an operator is uploaded once and the iteration stays in HBM.
 * Any other mf->fct is called as a host function on host copies (one PCIe round trip per product).
 * fasp_solver_pminres: the reference's restart branches skip the preconditioner when one is given and dereference
 * pc == NULL otherwise (KryPminres.c:1524, :1605); here both cases take tz = tp there (krylov.hip.h). */
void fasp_hip_mxv_csr(const void* A, const double* x, double* y);
void fasp_hip_mxv_bsr(const void* A, const double* x, double* y);
void fasp_hip_mxv_str(const void* A, const double* x, double* y);   /* MAT_STR: a dSTRmat, treated like the two above */
void fasp_solver_matfree_init(int matrix_format, mxv_matfree* mf, void* A);
int  fasp_solver_pcg(mxv_matfree* mf, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                     const int MaxIt, const short StopType, const short PrtLvl);
int  fasp_solver_pbcgs(mxv_matfree* mf, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                       const int MaxIt, const short StopType, const short PrtLvl);
int  fasp_solver_pgcg(mxv_matfree* mf, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                      const int MaxIt, const short StopType, const short PrtLvl);
int  fasp_solver_pminres(mxv_matfree* mf, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                         const int MaxIt, const short StopType, const short PrtLvl);
int  fasp_solver_pgmres(mxv_matfree* mf, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                        const int MaxIt, const short restart, const short StopType, const short PrtLvl);
int  fasp_solver_pvgmres(mxv_matfree* mf, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                         const int MaxIt, short restart, const short StopType, const short PrtLvl);
int  fasp_solver_pvfgmres(mxv_matfree* mf, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                          const int MaxIt, const short restart, const short StopType, const short PrtLvl);
int  fasp_solver_itsolver(mxv_matfree* mf, dvector* b, dvector* x, precond* pc, ITS_param* itparam);
int  fasp_solver_krylov(mxv_matfree* mf, dvector* b, dvector* x, ITS_param* itparam);

int fasp_solver_dcsr_pminres(dCSRmat* A, dvector* b, dvector* u, precond* pc, const double tol,
                             const double abstol, const int MaxIt, const short StopType, const short PrtLvl); /* KryPminres.c:61 */
int fasp_solver_dcsr_pgcg(dCSRmat* A, dvector* b, dvector* u, precond* pc, const double tol,
                          const double abstol, const int MaxIt, const short StopType, const short PrtLvl);    /* KryPgcg.c:60 */
int fasp_solver_dcsr_pgcr(dCSRmat* A, dvector* b, dvector* x, precond* pc, const double tol,
                          const double abstol, const int MaxIt, const short restart,
                          const short StopType, const short PrtLvl);                      /* KryPgcr.c:55 */
int fasp_solver_dcsr_pgmres(dCSRmat* A, dvector* b, dvector* x, precond* pc, const double tol,
                            const double abstol, const int MaxIt, const short restart,
                            const short StopType, const short PrtLvl);                    /* KryPgmres.c:66 */
int fasp_solver_dcsr_pvgmres(dCSRmat* A, dvector* b, dvector* x, precond* pc, const double tol,
                             const double abstol, const int MaxIt, const short restart,
                             const short StopType, const short PrtLvl);
int fasp_solver_dcsr_pvfgmres(dCSRmat* A, dvector* b, dvector* x, precond* pc, const double tol,
                              const double abstol, const int MaxIt, const short restart,
                              const short StopType, const short PrtLvl);
/* ---- the Krylov methods with a safety net (KrySP*.c) and their dispatchers (SolCSR.c:163 / :295) ----
 * The best iterate seen so far is kept and handed back when the iteration breaks down, produces a NaN, or ends (also at MaxIt) on an
 * iterate that is worse by more than tol * STAG_RATIO; "### WARNING: Discard current iteration. Restore iteration %d!" says so.  The
 * reference's prototypes (no abstol), return codes and printed lines.  All three stop types.  `pc`: as for the non-safe entries of the
 * format -- a device AMG handle, fasp_precond_ilu, the (block-)diagonal and Schwarz preconditioners and the structured ILU / block
 * Gauss-Seidel ones stay in HBM, any other pc->fct is called on the host.  One GPU (several ranks: message, ERROR_INPUT_PAR).  Without
 * a usable device these entries print why and return ERROR_MISC with x untouched (no CPU fallback).  fasp_solver_dcsr_itsolver_s takes
 * SOLVER_CG, _BiCGstab, _MinRes, _GMRES and _VGMRES; any other itsolver_type: "Unknown iterative solver type", ERROR_SOLVER_TYPE, before
 * any work.  fasp_solver_dcsr_krylov_s: the same with pc = NULL and the timing line. */
int fasp_solver_dcsr_spcg(const dCSRmat* A, const dvector* b, dvector* u, precond* pc, const double tol, const int MaxIt,
                          const short StopType, const short PrtLvl);                      /* KrySPcg.c:60 */
int fasp_solver_dcsr_spbcgs(const dCSRmat* A, const dvector* b, dvector* u, precond* pc, const double tol, const int MaxIt,
                            const short StopType, const short PrtLvl);                    /* KrySPbcgs.c:61 */
int fasp_solver_dcsr_spminres(const dCSRmat* A, const dvector* b, dvector* u, precond* pc, const double tol, const int MaxIt,
                              const short StopType, const short PrtLvl);                  /* KrySPminres.c:60 */
int fasp_solver_dcsr_spgmres(const dCSRmat* A, const dvector* b, dvector* x, precond* pc, const double tol, const int MaxIt,
                             short restart, const short StopType, const short PrtLvl);    /* KrySPgmres.c:66 */
int fasp_solver_dcsr_spvgmres(const dCSRmat* A, const dvector* b, dvector* x, precond* pc, const double tol, const int MaxIt,
                              short restart, const short StopType, const short PrtLvl);   /* KrySPvgmres.c:68 */
int fasp_solver_dcsr_itsolver_s(dCSRmat* A, dvector* b, dvector* x, precond* pc, ITS_param* itparam);   /* SolCSR.c:163 */
int fasp_solver_dcsr_krylov_s(dCSRmat* A, dvector* b, dvector* x, ITS_param* itparam);                  /* SolCSR.c:295 */
int fasp_solver_dbsr_spbcgs(const dBSRmat* A, const dvector* b, dvector* u, precond* pc, const double tol, const int MaxIt,
                            const short StopType, const short PrtLvl);                    /* KrySPbcgs.c:452 */
int fasp_solver_dbsr_spgmres(const dBSRmat* A, const dvector* b, dvector* x, precond* pc, const double tol, const int MaxIt,
                             short restart, const short StopType, const short PrtLvl);    /* KrySPgmres.c:409 */
int fasp_solver_dbsr_spvgmres(const dBSRmat* A, const dvector* b, dvector* x, precond* pc, const double tol, const int MaxIt,
                              short restart, const short StopType, const short PrtLvl);   /* KrySPvgmres.c:449 */
int fasp_solver_dstr_spcg(const dSTRmat* A, const dvector* b, dvector* u, precond* pc, const double tol, const int MaxIt,
                          const short StopType, const short PrtLvl);                      /* KrySPcg.c:726 */
int fasp_solver_dstr_spbcgs(const dSTRmat* A, const dvector* b, dvector* u, precond* pc, const double tol, const int MaxIt,
                            const short StopType, const short PrtLvl);                    /* KrySPbcgs.c:1234 */
int fasp_solver_dstr_spminres(const dSTRmat* A, const dvector* b, dvector* u, precond* pc, const double tol, const int MaxIt,
                              const short StopType, const short PrtLvl);                  /* KrySPminres.c:962 */
int fasp_solver_dstr_spgmres(const dSTRmat* A, const dvector* b, dvector* x, precond* pc, const double tol, const int MaxIt,
                             short restart, const short StopType, const short PrtLvl);    /* KrySPgmres.c:1095 */
int fasp_solver_dstr_spvgmres(const dSTRmat* A, const dvector* b, dvector* x, precond* pc, const double tol, const int MaxIt,
                              short restart, const short StopType, const short PrtLvl);   /* KrySPvgmres.c:1210 */
/* ---- the reference's own preconditioner objects (relink-only callers: tutorial/main/poisson-pcg.c:81,91) ----
 * fasp_precond_setup (PreCSR.c:46): PREC_AMG / PREC_FMG build the hierarchy on the host, upload it, and hand out
 * precond{data = precond_data*, fct = fasp_precond_amg | _amli | _namli | _famg}; mgl_data[l].A / P / R / cfmark show
 * the host hierarchy (read-only views owned by the library), b / x / w are allocated as the reference's setup
 * leaves them.  PREC_DIAG gives fasp_precond_diag on a copy of the diagonal, PREC_ILU gives
 * precond{data = ILU_data*, fct = fasp_precond_ilu} from fasp_ilu_dcsr_setup (PreCSR.c:130), PREC_NULL returns NULL;
 * PREC_SCHWARZ is out of scope: message + exit, as fasp_chkerr does.
 * fasp_precond_amg (PreCSR.c:416): z = B r for host vectors r, z -- pcdata->maxit cycles from a zero guess, cycle /
 * smoother parameters re-read from pcdata at every call (fasp_param_prec_to_amg).  Handed to this library's Krylov
 * methods these functions are recognised by their address and the whole iteration stays in HBM.
 * fasp_amg_data_create / _free (PreDataInit.c:64 / :101): a hierarchy obtained from fasp_precond_setup is released
 * together with its device copy; an AMG_data the caller filled itself is freed field by field like the reference. */
AMG_data* fasp_amg_data_create(short max_levels);
void      fasp_amg_data_free(AMG_data* mgl, AMG_param* param);
precond*  fasp_precond_setup(const short precond_type, AMG_param* amgparam, ILU_param* iluparam, dCSRmat* A);
void      fasp_precond_amg(double* r, double* z, void* data);
void      fasp_precond_famg(double* r, double* z, void* data);    /* PreCSR.c:450 */
void      fasp_precond_amli(double* r, double* z, void* data);    /* PreCSR.c:484 */
void      fasp_precond_namli(double* r, double* z, void* data);   /* PreCSR.c:518 */
void      fasp_param_amg_to_prec(precond_data* pcdata, const AMG_param* amgparam);   /* AuxParam.c:782 */
void      fasp_param_prec_to_amg(AMG_param* amgparam, const precond_data* pcdata);   /* AuxParam.c:816 */
/* the small host utilities such callers use around the solver (AuxMemory.c:152, AuxVector.c:105/:222/:145,
 * BlaSparseCSR.c:184/:34) */
void    fasp_mem_free(void* mem);
void*   fasp_mem_calloc(const unsigned int size, const unsigned int type);
void    fasp_dvec_alloc(const int m, dvector* u);
void    fasp_dvec_set(int n, dvector* x, const double val);
void    fasp_dvec_free(dvector* u);
dvector fasp_dvec_create(const int m);
dCSRmat fasp_dcsr_create(const int m, const int n, const int nnz);
void    fasp_dcsr_free(dCSRmat* A);
/* stand-alone sweeps of the other hot-path smoothers (ItrSmootherCSR.c:251 / :932 / :1509), host vectors in and
 * out, the sweep itself on the device by level scheduling (same result as the sequential sweep) */
void fasp_smoother_dcsr_gs(dvector* u, const int i_1, const int i_n, const int s, dCSRmat* A, dvector* b, int L);
void fasp_smoother_dcsr_sor(dvector* u, const int i_1, const int i_n, const int s, dCSRmat* A, dvector* b, int L,
                            const double w);
void fasp_smoother_dcsr_L1diag(dvector* u, const int i_1, const int i_n, const int s, dCSRmat* A, dvector* b, int L);

/* ---- ILU preconditioner (BlaILUSetupCSR.c, PreCSR.c:198-360, SolCSR.c:588/:668) ----
 * fasp_ilu_dcsr_setup: ILUk / ILUt / ILUtp factorisation on the HOST, output equal to the reference's entry for entry
 * (MSR factor in ijlu / luval, luval[i] = inverse pivot, nzlu, iperm, work, status ERROR_SOLVER_ILUSETUP on failure).
 * ILUtp renumbers the columns of A->JA in place, as the reference does; fasp_ilu_data_free renumbers them back.
 * fasp_param_ilu_init, fasp_ilu_data_create, fasp_mem_iludata_check need no GPU either.
 * fasp_precond_ilu / _forward / _backward: z = (LU)^-1 r, L^-1 r, U^-1 r for host vectors, computed on the device by
 * level-scheduled triangular solves with the reference's order of operations (bit for bit the same z).  A factor made
 * by fasp_ilu_dcsr_setup is uploaded at its first application and stays resident until fasp_ilu_data_free; any other
 * ILU_data is uploaded for each call.  Without a device they refuse to run (no CPU fallback).
 * fasp_solver_dcsr_krylov_ilu(_M): setup (of A, or of M) + fasp_solver_dcsr_itsolver with that preconditioner, every
 * itsolver_type; the preconditioner stays in HBM.  fasp_smoother_dcsr_ilu (ItrSmootherCSR.c:1280): x += (LU)^-1 (b - A x).
 * Block ILU (BlaILUSetupBSR.c:55, PreBSR.c:347, SolBSR.c:286, ItrSmootherBSR.c:1479): fasp_ilu_dbsr_setup is block ILUk
 * (ILU_lfil; every ILU_type) on the HOST, equal to the reference's bytes (luval holds nb x nb blocks, the diagonal ones
 * inverted), 1 <= nb <= 7; it needs no GPU.  fasp_precond_dbsr_ilu applies it with block triangular solves on the device
 * (bit for bit the reference's z; resident from the first application until fasp_ilu_data_free, as above), the block
 * Krylov methods recognise it and keep it in HBM; fasp_solver_dbsr_krylov_ilu = setup + fasp_solver_dbsr_itsolver.
 * ILU as a smoother of the block AMG cycle: AMG_param.ILU_levels > 0 with fasp_solver_dbsr_krylov_amg, the fasp_hip_bsr_*
 * handles and fasp_hip_bsr_precond_setup factors the levels below ILU_levels on the host (PreAMGSetupUABSR.c:149-179) and
 * smooths them on the device with one ILU step + block Gauss-Seidel sweeps (PreMGCycle.c:321-326); one GPU only.  The
 * scalar AMG cycle (fasp_solver_dcsr_krylov_amg with ILU_levels > 0) stays out of scope (Schwarz smoothing inside the scalar cycles, SWZ_levels > 0, is served: DESIGN.md section 3.11); structured ILU: fasp_ilu_dstr_setup0 / _setup1 above. */
void  fasp_param_ilu_init(ILU_param* iluparam);                                     /* AuxParam.c:595 */
void  fasp_ilu_data_create(const int iwk, const int nwork, ILU_data* iludata);      /* PreDataInit.c:411 */
void  fasp_ilu_data_free(ILU_data* iludata);                                        /* PreDataInit.c:445 */
short fasp_mem_iludata_check(const ILU_data* iludata);                              /* AuxMemory.c:203 */
short fasp_ilu_dcsr_setup(dCSRmat* A, ILU_data* iludata, ILU_param* iluparam);      /* BlaILUSetupCSR.c:40 */
void  fasp_precond_ilu(double* r, double* z, void* data);                           /* PreCSR.c:198 */
void  fasp_precond_ilu_forward(double* r, double* z, void* data);                   /* PreCSR.c:263 */
void  fasp_precond_ilu_backward(double* r, double* z, void* data);                  /* PreCSR.c:317 */
int   fasp_solver_dcsr_krylov_ilu(dCSRmat* A, dvector* b, dvector* x, ITS_param* itparam, ILU_param* iluparam);
int   fasp_solver_dcsr_krylov_ilu_M(dCSRmat* A, dvector* b, dvector* x, ITS_param* itparam, ILU_param* iluparam,
                                    dCSRmat* M);
void  fasp_smoother_dcsr_ilu(dCSRmat* A, dvector* b, dvector* x, void* data);
/* SolWrapper.c:195: ILUk(2)-preconditioned VFGMRES on a caller's CSR arrays (Fortran calling convention) */
void  fasp_fwrapper_dcsr_krylov_ilu_(int* n, int* nnz, int* ia, int* ja, double* a, double* b, double* u,
                                     double* tol, int* maxit, int* ptrlvl);
short fasp_ilu_dbsr_setup(dBSRmat* A, ILU_data* iludata, ILU_param* iluparam);      /* BlaILUSetupBSR.c:55 */
void  fasp_precond_dbsr_ilu(double* r, double* z, void* data);                      /* PreBSR.c:347 */
int   fasp_solver_dbsr_krylov_ilu(dBSRmat* A, dvector* b, dvector* x, ITS_param* itparam, ILU_param* iluparam);
void  fasp_smoother_dbsr_ilu(dBSRmat* A, dvector* b, dvector* x, void* data);       /* ItrSmootherBSR.c:1479 */
/* SolWrapper.c:326: ILUk(0)-preconditioned VFGMRES on a caller's BSR arrays (Fortran calling convention) */
void  fasp_fwrapper_dbsr_krylov_ilu_(int* n, int* nnz, int* nb, int* ia, int* ja, double* a, double* b, double* u,
                                     double* tol, int* maxit, int* ptrlvl);

/* The block (BSR) smoothers (ItrSmootherBSR.c): one sweep on the device, host vectors of ROW*nb, with the reference's
 * result bit for bit.  Orders, as _gs1 / _sor1 dispatch them: a non-NULL mark wins -- it is the visiting sequence, a permutation of
 * 0 .. ROW-1 --, else ASCEND or DESCEND; mark == NULL with any other order does nothing.  _jacobi, _gs and _sor invert the diagonal blocks on
 * the host (fasp_smat_inv; 1.0 / d for nb = 1; the last diagonal block a row stores counts), the others take them as diaginv; the entries
 * ending in 1 (_gs_ascend1, _gs_descend1) and _gs_order2 assume identity diagonal blocks (`work` is not used).  Off-diagonal entries are
 * taken in storage order, columns need not be sorted, rows may be empty.  A: square, storage_manner 0.  Every entry is create + apply +
 * destroy of the handle below.  Ends the process with a message: nb outside 1 .. 7 (ERROR_NUM_BLOCKS), a mark that is not a permutation,
 * ROW != COL, a b or u shorter than ROW*nb, a NULL argument (ERROR_INPUT_PAR), no usable device (ERROR_MISC: there is no CPU fallback).
 * fasp_smoother_dbsr_jacobi_setup is host code. */
void fasp_smoother_dbsr_jacobi(dBSRmat* A, dvector* b, dvector* u);                                                  /* ItrSmootherBSR.c:59 */
void fasp_smoother_dbsr_jacobi_setup(dBSRmat* A, double* diaginv);                                                   /* ItrSmootherBSR.c:163 */
void fasp_smoother_dbsr_gs(dBSRmat* A, dvector* b, dvector* u, int order, int* mark);                                /* ItrSmootherBSR.c:410 */
void fasp_smoother_dbsr_gs1(dBSRmat* A, dvector* b, dvector* u, int order, int* mark, double* diaginv);              /* ItrSmootherBSR.c:520 */
void fasp_smoother_dbsr_gs_ascend(dBSRmat* A, dvector* b, dvector* u, double* diaginv);                              /* ItrSmootherBSR.c:552 */
void fasp_smoother_dbsr_gs_ascend1(dBSRmat* A, dvector* b, dvector* u);                                              /* ItrSmootherBSR.c:619 */
void fasp_smoother_dbsr_gs_descend(dBSRmat* A, dvector* b, dvector* u, double* diaginv);                             /* ItrSmootherBSR.c:683 */
void fasp_smoother_dbsr_gs_descend1(dBSRmat* A, dvector* b, dvector* u);                                             /* ItrSmootherBSR.c:751 */
void fasp_smoother_dbsr_gs_order1(dBSRmat* A, dvector* b, dvector* u, double* diaginv, int* mark);                   /* ItrSmootherBSR.c:816 */
void fasp_smoother_dbsr_gs_order2(dBSRmat* A, dvector* b, dvector* u, int* mark, double* work);                      /* ItrSmootherBSR.c:888 */
void fasp_smoother_dbsr_sor(dBSRmat* A, dvector* b, dvector* u, int order, int* mark, double weight);                /* ItrSmootherBSR.c:959 */
void fasp_smoother_dbsr_sor1(dBSRmat* A, dvector* b, dvector* u, int order, int* mark, double* diaginv, double weight);   /* ItrSmootherBSR.c:1075 */
void fasp_smoother_dbsr_sor_ascend(dBSRmat* A, dvector* b, dvector* u, double* diaginv, double weight);              /* ItrSmootherBSR.c:1115 */
void fasp_smoother_dbsr_sor_descend(dBSRmat* A, dvector* b, dvector* u, double* diaginv, double weight);             /* ItrSmootherBSR.c:1234 */
void fasp_smoother_dbsr_sor_order(dBSRmat* A, dvector* b, dvector* u, double* diaginv, int* mark, double weight);    /* ItrSmootherBSR.c:1358 */
/* The resident form for a caller that smooths with one matrix many times (a precond.fct callback): the sweep plan of
 * (A, order, mark) is built and uploaded once.  fasp_hip_bsr_smoother_create: diaginv = the ROW inverse diagonal blocks, or NULL to have them
 * computed as _gs does; returns FASP_SUCCESS, ERROR_NUM_BLOCKS (nb outside 1 .. 7), ERROR_INPUT_PAR (a NULL pointer, ROW != COL, storage_manner
 * != 0, a mark that is not a permutation), ERROR_DATA_STRUCTURE (IA / JA inconsistent), ERROR_MISC (no device), ERROR_ALLOC_MEM; *h is NULL
 * unless it succeeds.  The checks come before any device work.  A is not needed after the call.  fasp_hip_bsr_smoother_apply: one sweep,
 * u = sweep(b, u) on host vectors; kind 0 Gauss-Seidel, 1 SOR with `weight`, 2 the identity-diagonal form; ERROR_INPUT_PAR for a b or u
 * shorter than ROW*nb or another kind; ERROR_MISC for a device failure.  A handle of (mark NULL, order neither ASCEND nor DESCEND) sweeps
 * nothing. */
typedef struct fasp_hip_bsr_smoother fasp_hip_bsr_smoother;
int  fasp_hip_bsr_smoother_create(fasp_hip_bsr_smoother** h, const dBSRmat* A, const double* diaginv, int order, const int* mark);
int  fasp_hip_bsr_smoother_apply(fasp_hip_bsr_smoother* h, int kind, double weight, const dvector* b, dvector* u);
void fasp_hip_bsr_smoother_destroy(fasp_hip_bsr_smoother* h);

/* The overlapping (multiplicative) Schwarz method of a CSR matrix.  The host side needs no GPU and leaves the
 * reference's arrays, entry order included: fasp_dcsr_sympart (1.0 A + 0.0 A^T: the symmetrised pattern with A's values), fasp_dcsr_shift,
 * fasp_sparse_mis (A 1-based; the greedy pass in natural order) and fasp_swz_dcsr_setup, which reads swzdata->A (1-BASED, square) and fills
 * nblk, iblock, jblock, maxbs, mask, maxa, blk_data, rhsloc1, xloc1, SWZ_type and swzparam; the members the reference leaves uninitialised
 * (mumps, au, al, rhsloc, memt, blk_solver) are zeroed.  Refused with a message and ERROR_INPUT_PAR before any device work: a block of more
 * than 256 rows, SWZ_maxlvl < 0, A.row != A.col.  SWZ_blksolver is accepted with any value and ignored: the device always solves a block
 * directly, by a dense LU with row interchanges (the reference build without UMFPACK / MUMPS solves it with GMRES to 1e-8; with a direct
 * solver compiled in it is exact as here).  SWZ_mmsize is never read, as in the reference.
 * fasp_dcsr_swz_forward / _backward: one sweep over the blocks 0 .. nblk-1 / in reverse on host vectors; for each block
 * rhs_i = b[k_i] - sum val x[k_j] over the entries of row k_i outside the block, the block solve, x[k_i] = u_i.  The first sweep of an
 * SWZ_data uploads it and factors every block on the device; the copy stays resident, found by the struct's address, until
 * fasp_swz_data_free.  A block whose factorisation meets a pivot below 1e-20 is refused (exit with ERROR_INPUT_PAR from the void entries,
 * that code from the solver), its index printed; a factor store that does not fit the device: ERROR_ALLOC_MEM.
 * fasp_precond_swz (data: SWZ_data*): z = 0, b = r, then backward (SWZ_type 2), forward and backward (3) or forward (anything else).
 * Handed to one of this library's CSR Krylov methods it is recognised by its address and the whole iteration stays in HBM; called
 * directly (a foreign Krylov method) it stages r and z per application.  fasp_solver_dcsr_krylov_swz: sympart, shift, setup, solve, free.
 * Without a device the computing entries refuse to run (ERROR_MISC).  Schwarz smoothing inside the scalar AMG cycles (AMG_param.SWZ_levels > 0)
 * uses the same setup and sweeps on the levels below SWZ_levels; a BSR hierarchy refuses it. */
void    fasp_param_swz_init(SWZ_param* swzparam);                                           /* AuxParam.c:617 */
dCSRmat fasp_dcsr_sympart(dCSRmat* A);                                                      /* BlaSparseCSR.c:1357 */
void    fasp_dcsr_shift(dCSRmat* A, const int offset);                                      /* BlaSparseCSR.c:1212 */
ivector fasp_sparse_mis(dCSRmat* A);                                                        /* BlaSparseUtil.c:907 */
int     fasp_swz_dcsr_setup(SWZ_data* swzdata, SWZ_param* swzparam);                        /* BlaSchwarzSetup.c:46 */
void    fasp_dcsr_swz_forward(SWZ_data* swzdata, SWZ_param* swzparam, dvector* x, dvector* b);   /* BlaSchwarzSetup.c:218 */
void    fasp_dcsr_swz_backward(SWZ_data* swzdata, SWZ_param* swzparam, dvector* x, dvector* b);  /* BlaSchwarzSetup.c:328 */
void    fasp_precond_swz(double* r, double* z, void* data);                                 /* PreCSR.c:371 */
void    fasp_swz_data_free(SWZ_data* swzdata);                                              /* PreDataInit.c:494 */
int     fasp_solver_dcsr_krylov_swz(dCSRmat* A, dvector* b, dvector* x, ITS_param* itparam, SWZ_param* schparam);   /* SolCSR.c:401 */

/* The AMG preconditioner as a `precond` -- the role of fasp_precond_setup(PREC_AMG, ..)
 * (PreCSR.c:46) + fasp_precond_amg (PreCSR.c:416).  The returned object can be handed to the
 * functions above or to the REFERENCE's own CPU Krylov methods (they only call pc->fct). */
precond* fasp_hip_precond_setup(dCSRmat* A, AMG_param* amgparam);
void     fasp_hip_precond_fct(double* r, double* z, void* data);
void     fasp_hip_precond_free(precond* pc);

/* The same plug-in level for block matrices (KryPcg.c:386, KryPbcgs.c:400, KryPgmres.c:357,
 * KryPvgmres.c:416, KryPvfgmres.c:386; PreBSR.c:1149 for the preconditioner action). */
int fasp_solver_dbsr_pcg(dBSRmat* A, dvector* b, dvector* u, precond* pc, const double tol,
                         const double abstol, const int MaxIt, const short StopType, const short PrtLvl);
int fasp_solver_dbsr_pbcgs(dBSRmat* A, dvector* b, dvector* u, precond* pc, const double tol,
                           const double abstol, const int MaxIt, const short StopType, const short PrtLvl);
int fasp_solver_dbsr_pgmres(dBSRmat* A, dvector* b, dvector* x, precond* pc, const double tol,
                            const double abstol, const int MaxIt, const short restart,
                            const short StopType, const short PrtLvl);
int fasp_solver_dbsr_pvgmres(dBSRmat* A, dvector* b, dvector* x, precond* pc, const double tol,
                             const double abstol, const int MaxIt, const short restart,
                             const short StopType, const short PrtLvl);
int fasp_solver_dbsr_pvfgmres(dBSRmat* A, dvector* b, dvector* x, precond* pc, const double tol,
                              const double abstol, const int MaxIt, const short restart,
                              const short StopType, const short PrtLvl);
precond* fasp_hip_bsr_precond_setup(dBSRmat* A, AMG_param* amgparam);
void     fasp_hip_bsr_precond_fct(double* r, double* z, void* data);
void     fasp_hip_bsr_precond_free(precond* pc);

/* One application of the AMG preconditioner z = B r (PreCSR.c:416) on the
 * resident hierarchy; host vectors in/out. */
int fasp_hip_precond_amg(fasp_hip_amg* h, const double* r, double* z);

/* Synthetic input of the headline benchmark: 3-D 7-point FD Poisson on the
 * unit cube, nx*ny*nz interior points, lexicographic, x fastest; row layout and
 * values as produced by test/src/FdmPoisson.c:439 + :731 of the reference.
 * A, b, u are allocated with malloc and released by fasp_hip_free_system. */
int  fasp_hip_poisson7pt(int nx, int ny, int nz, dCSRmat* A, dvector* b, dvector* u_exact);
/* Synthetic input of config 5: Q1 trilinear FE matrix (27-point stencil) of
 * -div(diag(kx,ky,kz) grad u) = 1 on the unit cube, n^3 interior nodes.  The reference has no
 * 3-D FE generator; this one is ours.  Free with fasp_hip_free_system. */
int  fasp_hip_aniso27pt(int n, double kx, double ky, double kz, dCSRmat* A, dvector* b);
void fasp_hip_free_system(dCSRmat* A, dvector* b, dvector* u);

/* Multi-GPU (1-D row partition, RCCL over xGMI).  The unique id is produced on
 * rank 0 and distributed by the caller (e.g. torch.distributed broadcast). */
#define FASP_HIP_UNIQUE_ID_BYTES 128
int fasp_hip_comm_unique_id(char* id_out);
int fasp_hip_comm_init(int rank, int nranks, const char* id);
int fasp_hip_comm_finalize(void);
/* Validation transport: host-staged through the POSIX shared-memory segment /<name>, so
 * several processes sharing ONE GPU can run the distributed solver (tests only). */
int fasp_hip_comm_init_shm(int rank, int nranks, const char* name);
/* Peer windows (round 4; csrc/comm_ipc.h): every rank maps every peer's uncached device window through hipIpc handles exchanged
 * in the shared-memory segment /<name>; a halo exchange is one kernel that stores this rank's boundary entries straight into the
 * neighbours' mailboxes (xGMI stores between the GPUs of a node) and polls / copies its own; the Krylov scalars are reduced the
 * same way, summed in rank order.  At most 8 ranks (one node); ranks may also share one GPU (validation).  FASP_HIP_IPC_CAP =
 * doubles per mailbox (default 524 288). */
int fasp_hip_comm_init_ipc(int rank, int nranks, const char* name);
int fasp_hip_comm_rank(void);
int fasp_hip_comm_size(void);

/* Measurement and test entries (kernel timers, run-time switches of the A/B identity tests, partition inspection, self-tests):
 * include/fasp_hip_dev.h -- in the library, but not part of the drop-in boundary. */

/* Library/version string. */
const char* fasp_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FASP_HIP_H */
