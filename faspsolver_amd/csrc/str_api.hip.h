// str_api.hip.h -- the structured-matrix (dSTRmat) entry points of the C ABI.
// Part of the single translation unit solver.hip (included there inside extern "C"; not a stand-alone header).

// ---- host code: BlaSparseSTR.c:41-162, BlaFormat.c:119 ---------------------------------------------
namespace {
void str_alloc_arrays(dSTRmat* A, const int* offsets)
{
    const unsigned nc2 = (unsigned)(A->nc * A->nc);
    A->offsets = (int*)fasp_mem_calloc((unsigned)std::max(A->nband, 0), sizeof(int));
    for (int b = 0; b < A->nband; ++b) A->offsets[b] = offsets[b];
    A->diag = (double*)fasp_mem_calloc((unsigned)A->ngrid * nc2, sizeof(double));
    A->offdiag = (double**)fasp_mem_calloc((unsigned)std::max(A->nband, 0), sizeof(double*));
    for (int b = 0; b < A->nband; ++b) {
        const int len = A->ngrid - std::abs(offsets[b]);
        A->offdiag[b] = len > 0 ? (double*)fasp_mem_calloc((unsigned)len * nc2, sizeof(double)) : nullptr;
    }
}
}  // namespace

dSTRmat fasp_dstr_create(const int nx, const int ny, const int nz, const int nc, const int nband, int* offsets)  // BlaSparseSTR.c:41
{
    FASP_ENTRY();
    dSTRmat A;
    A.nx = nx; A.ny = ny; A.nz = nz; A.nc = nc; A.nxy = nx * ny; A.ngrid = A.nxy * nz; A.nband = nband;
    str_alloc_arrays(&A, offsets);
    return A;
}
void fasp_dstr_alloc(const int nx, const int ny, const int nz, const int nxy, const int ngrid, const int nband, const int nc,
                     int* offsets, dSTRmat* A)  // BlaSparseSTR.c:93
{
    FASP_ENTRY();
    A->nx = nx; A->ny = ny; A->nz = nz; A->nxy = nxy; A->ngrid = ngrid; A->nband = nband; A->nc = nc;
    str_alloc_arrays(A, offsets);
}
// BlaSparseSTR.c:136; the reference leaves the offdiag pointer array itself allocated, here it is released too
void fasp_dstr_free(dSTRmat* A)
{
    FASP_ENTRY();
    if (!A) return;
    fasp_mem_free(A->offsets); A->offsets = nullptr;
    fasp_mem_free(A->diag); A->diag = nullptr;
    if (A->offdiag)
        for (int b = 0; b < A->nband; ++b) fasp_mem_free(A->offdiag[b]);
    fasp_mem_free(A->offdiag); A->offdiag = nullptr;
    A->nx = A->ny = A->nz = A->nxy = 0;
    A->ngrid = A->nband = A->nc = 0;
}
void fasp_dstr_cp(const dSTRmat* A, dSTRmat* B)  // BlaSparseSTR.c:162: B's arrays exist already
{
    FASP_ENTRY();
    const size_t nc2 = (size_t)A->nc * A->nc;
    B->nx = A->nx; B->ny = A->ny; B->nz = A->nz; B->nxy = A->nxy; B->ngrid = A->ngrid; B->nc = A->nc; B->nband = A->nband;
    if (A->nband > 0) std::memcpy(B->offsets, A->offsets, sizeof(int) * (size_t)A->nband);
    if (A->ngrid > 0) std::memcpy(B->diag, A->diag, sizeof(double) * (size_t)A->ngrid * nc2);
    for (int b = 0; b < A->nband; ++b) {
        const int len = A->ngrid - std::abs(A->offsets[b]);
        if (len > 0) std::memcpy(B->offdiag[b], A->offdiag[b], sizeof(double) * (size_t)len * nc2);
    }
}

// BlaFormat.c:119.  Scalar row (i, p) holds, block after block, the nc entries of block row p of: the diagonal block, then every band
// that has a term in grid row i, in storage order; in the rows p >= 1 the first entry and entry p change places afterwards, which
// puts the row's own diagonal entry first.  IA, JA, val as the reference builds them, byte for byte.
short fasp_format_dstr_dcsr(const dSTRmat* A, dCSRmat* B)
{
    FASP_ENTRY();
    if (!B || str_plan(A, nullptr) < 0) return ERROR_INPUT_PAR;
    const int nc = A->nc, ngrid = A->ngrid, nband = A->nband, rows = nc * ngrid;
    int* ia = (int*)fasp_mem_calloc((unsigned)rows + 1, sizeof(int));
    long long nnz = 0;
    for (int i = 0; i < ngrid; ++i) {
        int blocks = 1;
        for (int b = 0; b < nband; ++b) blocks += str_block(A, b, i) ? 1 : 0;
        for (int p = 0; p < nc; ++p) {
            nnz += (long long)nc * blocks;
            if (nnz > 0x7fffffffLL) { fasp_mem_free(ia); return ERROR_INPUT_PAR; }
            ia[(size_t)i * nc + p + 1] = (int)nnz;
        }
    }
    int*    ja = (int*)fasp_mem_calloc((unsigned)nnz, sizeof(int));
    double* av = (double*)fasp_mem_calloc((unsigned)nnz, sizeof(double));
    for (int i = 0; i < ngrid; ++i) {
        int block = 0;
        for (int b = -1; b < nband; ++b) {
            const double* src = str_block(A, b, i);   // (b == -1: the diagonal block)
            if (!src) continue;
            const int col0 = (i + (b < 0 ? 0 : A->offsets[b])) * nc;
            for (int p = 0; p < nc; ++p) {
                const size_t at = (size_t)ia[(size_t)i * nc + p] + (size_t)block * nc;
                for (int q = 0; q < nc; ++q) { ja[at + q] = col0 + q; av[at + q] = src[p * nc + q]; }
            }
            ++block;
        }
        for (int p = 1; p < nc; ++p) {
            const size_t at = (size_t)ia[(size_t)i * nc + p];
            std::swap(ja[at], ja[at + p]);
            std::swap(av[at], av[at + p]);
        }
    }
    B->row = rows; B->col = rows; B->nnz = (int)nnz; B->IA = ia; B->JA = ja; B->val = av;
    return FASP_SUCCESS;
}

int fasp_hip_str_form(const dSTRmat* A)
{
    FASP_ENTRY();
    return str_plan(A, nullptr);
}

// ---- the products, host vectors in and out (one-shot upload, as fasp_blas_dcsr_mxv) -----------------
void fasp_blas_dstr_aAxpy(const double alpha, const dSTRmat* A, const double* x, double* y)  // BlaSpmvSTR.c:61
{
    FASP_ENTRY();
    TmpSTR M(A);
    if (!M.ok) die_str(__func__, M.form);
    TmpVec dx(x, (size_t)M.n), dy(y, (size_t)M.n);
    str_aAxpy(M, alpha, dx.d, dy.d, dy.d);
    dy.get(y);
}
void fasp_blas_dstr_mxv(const dSTRmat* A, const double* x, double* y)  // BlaSpmvSTR.c:131 (which clears ngrid*nc*nc entries of y; here ngrid*nc)
{
    FASP_ENTRY();
    TmpSTR M(A);
    if (!M.ok) die_str(__func__, M.form);
    TmpVec dx(x, (size_t)M.n), dy(nullptr, (size_t)M.n);
    str_mxv(M, dx.d, dy.d);
    dy.get(y);
}
double fasp_hip_time_str_mxv(const dSTRmat* A, int reps)
{
    FASP_ENTRY();
    TmpSTR M(A);
    if (!M.ok || reps <= 0) return -1.0;
    TmpVec dx(nullptr, (size_t)M.n), dy(nullptr, (size_t)M.n);
    if (!dx.d || !dy.d) return -1.0;
    (void)hipMemsetAsync(dx.d, 0, sizeof(double) * dx.n, g_ctx.stream);
    str_mxv(M, dx.d, dy.d); str_mxv(M, dx.d, dy.d);
    double ms = -1.0;
    return time_reps(reps, [&] { str_mxv(M, dx.d, dy.d); return 0; }, &ms) < 0 ? -1.0 : ms;
}

// ---- structured ILU on the device: the dev entries (fasp_hip_dev.h) -------------------------------------
int fasp_hip_str_ilu_form(const dSTRmat* LU, int lfil)
{
    FASP_ENTRY();
    StrIluDesc D;
    const char* why = "";
    if (!str_ilu_describe(LU, lfil, D, &why)) {
        std::printf("fasp_hip_str_ilu_form: the ILU(%d) factor is not applied on the device: %s\n", lfil, why);
        return -1;
    }
    return str_ilu_plan(D);
}
int fasp_hip_str_ilu_apply(const dSTRmat* LU, int lfil, const double* r, double* z)
{
    FASP_ENTRY();
    StrIluDesc D;
    if (!r || !z || !str_ilu_describe(LU, lfil, D, nullptr)) return ERROR_INPUT_PAR;
    if (ctx_init() < 0) return ERROR_MISC;
    StrIluDev M(LU, D);
    if (!M.ok) return ERROR_ALLOC_MEM;
    const size_t n = (size_t)D.ngrid * D.nc;
    if (hipMemcpy(M.r, r, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess) return ERROR_MISC;
    int st = str_ilu_apply(M, M.r, M.z);
    if (hipStreamSynchronize(g_ctx.stream) != hipSuccess) st = ERROR_MISC;
    if (st >= 0 && hipMemcpy(z, M.z, sizeof(double) * n, hipMemcpyDeviceToHost) != hipSuccess) st = ERROR_MISC;
    const int err = seq_err_check();
    return st < 0 ? st : err;
}
double fasp_hip_time_str_ilu(const dSTRmat* LU, int lfil, int reps)
{
    FASP_ENTRY();
    StrIluDesc D;
    if (reps <= 0 || !str_ilu_describe(LU, lfil, D, nullptr) || ctx_init() < 0) return -1.0;
    StrIluDev M(LU, D);
    if (!M.ok) return -1.0;
    const size_t n = (size_t)D.ngrid * D.nc;
    std::vector<double> hr(n);
    for (size_t i = 0; i < n; ++i) hr[i] = std::sin(0.37 * (double)i) + 0.1;
    if (hipMemcpy(M.r, hr.data(), sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess) return -1.0;
    if (str_ilu_apply(M, M.r, M.z) < 0) return -1.0;   // warm-up
    double ms = -1.0;
    const int st = time_reps(reps, [&] { return str_ilu_apply(M, M.r, M.z); }, &ms);
    if (seq_err_check() < 0 || st < 0) return -1.0;
    return ms;
}

// PreSTR.c:44 (host arrays): z_i = Dinv_i r_i, summed as fasp_blas_smat_mxv does (BlaSmallMat.c:238: from the first product for
// nc = 2, 3, 4, 5, 7, from 0.0 in its general text)
void fasp_precond_dstr_diag(double* r, double* z, void* data)
{
    FASP_ENTRY();
    const precond_diag_str* d = static_cast<const precond_diag_str*>(data);
    const int  nc = d->nc, nc2 = nc * nc, m = d->diag.row / nc2;
    const bool from_zero = !(nc == 2 || nc == 3 || nc == 4 || nc == 5 || nc == 7);
    for (int i = 0; i < m; ++i)
        for (int p = 0; p < nc; ++p) {
            const double* D = d->diag.val + (size_t)i * nc2 + p * nc;
            double s = D[0] * r[(size_t)i * nc];
            if (from_zero) s = 0.0 + s;
            for (int c = 1; c < nc; ++c) s = s + D[c] * r[(size_t)i * nc + c];
            z[(size_t)i * nc + p] = s;
        }
}

// ---- Krylov methods with a caller's preconditioner: KryPcg.c:970, KryPbcgs.c:1027, KryPgmres.c:998, KryPvgmres.c:1116, KryPminres.c:876
int fasp_solver_dstr_pcg(dSTRmat* A, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                         const int MaxIt, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_STR, K_CG, A, b, u, pc, {tol, abstol, MaxIt, 0, StopType, PrtLvl});
}
int fasp_solver_dstr_pbcgs(dSTRmat* A, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                           const int MaxIt, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_STR, K_BiCGstab, A, b, u, pc, {tol, abstol, MaxIt, 0, StopType, PrtLvl});
}
int fasp_solver_dstr_pminres(dSTRmat* A, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                             const int MaxIt, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_STR, K_MinRes, A, b, u, pc, {tol, abstol, MaxIt, 0, StopType, PrtLvl});
}
int fasp_solver_dstr_pgmres(dSTRmat* A, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                            const int MaxIt, const short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_STR, K_GMRES, A, b, x, pc, {tol, abstol, MaxIt, restart, StopType, PrtLvl});
}
int fasp_solver_dstr_pvgmres(dSTRmat* A, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                             const int MaxIt, const short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_STR, K_VGMRES, A, b, x, pc, {tol, abstol, MaxIt, restart, StopType, PrtLvl});
}

// SolSTR.c:51: CG, BiCGstab, GMRES, VGMRES
int fasp_solver_dstr_itsolver(dSTRmat* A, dvector* b, dvector* x, precond* pc, ITS_param* itparam)
{
    FASP_ENTRY();
    if (!itparam) return ERROR_INPUT_PAR;
    const short prtlvl = itparam->print_level, stop_type = itparam->stop_type, restart = (short)itparam->restart;
    const int MaxIt = itparam->maxit;
    const double tol = itparam->tol, abstol = itparam->abstol, t0 = wall_seconds();
    int iter;
    its_check(tol, MaxIt);
    switch (itparam->itsolver_type) {
        case SOLVER_CG: iter = fasp_solver_dstr_pcg(A, b, x, pc, tol, abstol, MaxIt, stop_type, prtlvl); break;
        case SOLVER_BiCGstab: iter = fasp_solver_dstr_pbcgs(A, b, x, pc, tol, abstol, MaxIt, stop_type, prtlvl); break;
        case SOLVER_GMRES: iter = fasp_solver_dstr_pgmres(A, b, x, pc, tol, abstol, MaxIt, restart, stop_type, prtlvl); break;
        case SOLVER_VGMRES: iter = fasp_solver_dstr_pvgmres(A, b, x, pc, tol, abstol, MaxIt, restart, stop_type, prtlvl); break;
        default:
            std::printf("### ERROR: Unknown iterative solver type %d! [%s]\n", itparam->itsolver_type, __func__);
            return ERROR_SOLVER_TYPE;
    }
    print_itsolver_time(prtlvl, iter, wall_seconds() - t0);
    return iter;
}
// SolSTR.c:132
int fasp_solver_dstr_krylov(dSTRmat* A, dvector* b, dvector* x, ITS_param* itparam)
{
    FASP_ENTRY();
    if (!itparam) return ERROR_INPUT_PAR;
    const double t0 = wall_seconds();
    const int status = fasp_solver_dstr_itsolver(A, b, x, nullptr, itparam);
    if (itparam->print_level >= PRINT_MIN) std::printf("Krylov method totally costs %.4f seconds.\n", wall_seconds() - t0);
    return status;
}
// SolSTR.c:175: the diagonal blocks inverted on the host as fasp_smat_inv does (bsr_diaginv on the block diagonal)
int fasp_solver_dstr_krylov_diag(dSTRmat* A, dvector* b, dvector* x, ITS_param* itparam)
{
    FASP_ENTRY();
    if (!itparam || str_plan(A, nullptr) < 0) return ERROR_INPUT_PAR;
    const double t0 = wall_seconds();
    const int ngrid = A->ngrid, nc2 = A->nc * A->nc;
    std::vector<double> dv((size_t)std::max(ngrid, 1) * nc2, 0.0);
    std::vector<int> ia((size_t)ngrid + 1), ja((size_t)std::max(ngrid, 1));
    for (int i = 0; i <= ngrid; ++i) ia[(size_t)i] = i;
    for (int i = 0; i < ngrid; ++i) ja[(size_t)i] = i;
    dBSRmat D{ngrid, ngrid, ngrid, A->nc, 0, A->diag, ia.data(), ja.data()};   // the block diagonal as a BSR matrix
    const int st = bsr_diaginv(&D, dv.data());
    if (st < 0) return st;
    precond_diag_str diag;
    diag.nc = A->nc; diag.diag.row = ngrid * nc2; diag.diag.val = dv.data();
    precond pc{&diag, fasp_precond_dstr_diag};
    const int status = fasp_solver_dstr_itsolver(A, b, x, &pc, itparam);
    if (itparam->print_level >= PRINT_MIN) std::printf("Diag_Krylov method totally costs %.4f seconds.\n", wall_seconds() - t0);
    return status;
}
// SolSTR.c:236: structured ILU(0) / ILU(1) factorisation on the host, then the Krylov method with both triangular solves on the
// device (bind_ilu_str).  A refused factorisation (LU zeroed) ends the call; the reference would iterate on it.
int fasp_solver_dstr_krylov_ilu(dSTRmat* A, dvector* b, dvector* x, ITS_param* itparam, ILU_param* iluparam)
{
    FASP_ENTRY();
    if (!itparam || !iluparam || !A) return ERROR_INPUT_PAR;
    const short prtlvl = itparam->print_level;
    const int ILU_lfil = iluparam->ILU_lfil;
    if (ILU_lfil != 0 && ILU_lfil != 1) {
        std::printf("### ERROR: Illegal level of ILU fill-in (>1)! [%s]\n", __func__);
        return ERROR_MISC;
    }
    if (ctx_init() < 0) die_no_device(__func__);
    if (str_plan(A, nullptr) < 0) return ERROR_INPUT_PAR;
    const double t0 = wall_seconds();
    dSTRmat LU;
    if (ILU_lfil == 0) fasp_ilu_dstr_setup0(A, &LU);
    else fasp_ilu_dstr_setup1(A, &LU);
    const double setup_time = wall_seconds() - t0;
    if (LU.ngrid <= 0 || !LU.diag) return ERROR_INPUT_PAR;
    if (prtlvl > PRINT_NONE) std::printf("Structrued ILU(%d) setup costs %f seconds.\n", ILU_lfil, setup_time);
    precond pc{&LU, ILU_lfil == 0 ? fasp_precond_dstr_ilu0 : fasp_precond_dstr_ilu1};
    const double t1 = wall_seconds();
    const int status = fasp_solver_dstr_itsolver(A, b, x, &pc, itparam);
    if (prtlvl >= PRINT_MIN) {
        const double solve_time = wall_seconds() - t1;
        std::printf("Iterative solver costs %f seconds.\n", solve_time);
        std::printf("ILU_Krylov method totally costs %.4f seconds.\n", setup_time + solve_time);
    }
    fasp_dstr_free(&LU);
    return status;
}

// ---- the smoothers: ItrSmootherSTR.c (csrc/str_sweep.hip.h) ------------------------------------------------------
namespace {
struct StrSweepPrep {
    StrSweepDesc D;
    bool bad_matrix = false;   // a matrix the library refuses (as opposed to a refused sequence or a missing diaginv)
    bool todo = false, natural = false, cf = false, desc = false;
    int  form = STR_SWF_LIST;
    std::vector<int> seq;       // the visits of the ordered form
    std::vector<double> dinv;   // the diagonal blocks inverted here
    const double* dg = nullptr;   // what the closing step uses: A's diagonal (nc == 1) or inverted blocks
};

// Everything a sweep needs that the host decides: the dispatch of _gs1 / _sor1 (ItrSmootherSTR.c:277 / :935) on (order, mark) -- cf_entry:
// the C/F form whatever `order` is, as the _cf entries are called --, the checks, the form (str_sweep_plan) and the visits.  fn: refusals
// of a sequence or of a missing diaginv are reported under this name.  need_diag: resolve P.dg (invert: the blocks are inverted here
// when diaginv is NULL, as the entries without the trailing 1 do with fasp_smat_inv).
int str_sweep_prepare(const char* fn, const dSTRmat* A, int kind, int order, const int* mark, bool cf_entry, const double* diaginv, bool invert,
                      bool need_diag, StrSweepPrep& P)
{
    if (str_sweep_describe(A, P.D) < 0 || kind < STR_SWEEP_JACOBI || kind > STR_SWEEP_SOR) { P.bad_matrix = true; return ERROR_INPUT_PAR; }
    const int ngrid = P.D.ngrid, nc = P.D.nc;
    if (kind == STR_SWEEP_JACOBI) { P.todo = true; P.form = STR_SWF_JACOBI; }
    else {
        if (cf_entry && !mark) { std::fprintf(stderr, "### ERROR: %s: the C/F order needs a mark array\n", fn); return ERROR_INPUT_PAR; }
        P.cf = mark && (cf_entry || order != STR_ORDER_USER);
        P.natural = !mark && (order == STR_ORDER_ASCEND || order == STR_ORDER_DESCEND);
        P.desc = P.natural && order == STR_ORDER_DESCEND;
        P.todo = mark || P.natural;
        if (!P.todo) return FASP_SUCCESS;   // mark == NULL and neither ASCEND nor DESCEND: the reference does nothing
        if (mark && !P.cf) {
            std::vector<char> seen((size_t)std::max(ngrid, 1), 0);
            for (int q = 0; q < ngrid; ++q) {
                if (mark[q] < 0 || mark[q] >= ngrid || seen[(size_t)mark[q]]) {
                    std::fprintf(stderr, "### ERROR: %s: the user-defined order is not a sequence of all %d grid points (entry %d: %d)\n", fn, ngrid, q, mark[q]);
                    return ERROR_INPUT_PAR;
                }
                seen[(size_t)mark[q]] = 1;
            }
        }
        P.form = str_sweep_plan(P.D, P.natural);
        if (P.form == STR_SWF_LIST) str_sweep_visits(ngrid, order, mark, P.cf, kind == STR_SWEEP_SOR && nc == 1, P.seq);
    }
    if (!need_diag) return FASP_SUCCESS;
    if (nc == 1) P.dg = A->diag;
    else if (diaginv) P.dg = diaginv;
    else if (invert) {
        const size_t nc2 = (size_t)nc * nc;
        P.dinv.assign(A->diag, A->diag + (size_t)ngrid * nc2);
        for (int i = 0; i < ngrid; ++i) (void)smat_inv(P.dinv.data() + (size_t)i * nc2, nc);
        P.dg = P.dinv.data();
    } else {
        std::fprintf(stderr, "### ERROR: %s: nc = %d needs the inverted diagonal blocks (diaginv is NULL)\n", fn, nc);
        return ERROR_INPUT_PAR;
    }
    return FASP_SUCCESS;
}

// nsweeps sweeps on a resident copy, host vectors in and out.  reps > 0: `reps` further sweeps are timed with HIP events into *ms.
int str_sweep_run(const char* fn, const dSTRmat* A, int kind, int order, const int* mark, bool cf_entry, double w, const double* diaginv, bool invert,
                  const double* b, double* u, int nsweeps, int* info, int reps, double* ms, bool* bad_matrix)
{
    StrSweepPrep P;
    const int st0 = str_sweep_prepare(fn, A, kind, order, mark, cf_entry, diaginv, invert, true, P);
    if (bad_matrix) *bad_matrix = P.bad_matrix;
    if (info) std::fill(info, info + 8, 0);
    if (st0 < 0) return st0;
    if (!P.todo || P.D.ngrid == 0 || nsweeps <= 0) return FASP_SUCCESS;
    if (ctx_init() < 0) return ERROR_MISC;
    StrSweepDev M(A, P.D, kind, P.form, P.desc, w, P.dg, P.seq, b, u);
    if (!M.ok) return ERROR_ALLOC_MEM;
    int st = FASP_SUCCESS;
    for (int s = 0; s < nsweeps && st >= 0; ++s) st = M.sweep();
    if (reps > 0 && ms && st >= 0) st = time_reps(reps, [&] { return M.sweep(); }, ms);
    if (hipStreamSynchronize(g_ctx.stream) != hipSuccess && st >= 0) st = ERROR_MISC;
    if (M.used_pipe && seq_err_check() < 0 && st >= 0) st = ERROR_MISC;   // a poll of the pipelined form that ran out
    if (st >= 0 && hipMemcpy(u, M.u, sizeof(double) * (size_t)P.D.ngrid * P.D.nc, hipMemcpyDeviceToHost) != hipSuccess) st = ERROR_MISC;
    if (info) {
        info[0] = P.form; info[1] = M.launches; info[2] = M.levels; info[3] = M.wgs; info[4] = M.visits; info[5] = P.D.geo ? 1 : 0;
    }
    return st;
}

// the public smoothers: one-shot, host vectors, void as in the reference
void str_smoother_public(const char* fn, dSTRmat* A, dvector* b, dvector* u, int kind, int order, int* mark, bool cf_entry, double w,
                         double* diaginv, bool invert)
{
    if (!A || !b || !u || !b->val || !u->val) { std::fprintf(stderr, "### ERROR: %s: NULL argument\n", fn); return; }
    if (A->nc < 1) { std::printf("### ERROR: nc is illegal! [%s]\n", fn); std::fflush(stdout); return; }
    const long long n = (long long)A->ngrid * A->nc;
    if (A->ngrid > 0 && (b->row < n || u->row < n)) { std::fprintf(stderr, "### ERROR: %s: b and u need ngrid * nc = %lld entries\n", fn, n); return; }
    bool bad_matrix = false;
    const int st = str_sweep_run(fn, A, kind, order, mark, cf_entry, w, diaginv, invert, b->val, u->val, 1, nullptr, 0, nullptr, &bad_matrix);
    if (bad_matrix) die_str(fn, ERROR_INPUT_PAR);
    if (st == ERROR_INPUT_PAR) return;   // a refused sequence or a missing diaginv: said above, u untouched
    if (st == ERROR_MISC && !g_ctx.ready) die_str(fn, 0);
    if (st < 0) { std::fprintf(stderr, "### ERROR: %s: sweep failed (%d)\n", fn, st); std::exit(st); }
}
}  // namespace

void fasp_smoother_dstr_jacobi(dSTRmat* A, dvector* b, dvector* u)  // ItrSmootherSTR.c:43
{
    FASP_ENTRY();
    str_smoother_public(__func__, A, b, u, STR_SWEEP_JACOBI, 0, nullptr, false, 1.0, nullptr, true);
}
void fasp_smoother_dstr_jacobi1(dSTRmat* A, dvector* b, dvector* u, double* diaginv)  // :92
{
    FASP_ENTRY();
    str_smoother_public(__func__, A, b, u, STR_SWEEP_JACOBI, 0, nullptr, false, 1.0, diaginv, false);
}
void fasp_smoother_dstr_gs(dSTRmat* A, dvector* b, dvector* u, const int order, int* mark)  // :217
{
    FASP_ENTRY();
    str_smoother_public(__func__, A, b, u, STR_SWEEP_GS, order, mark, false, 1.0, nullptr, true);
}
void fasp_smoother_dstr_gs1(dSTRmat* A, dvector* b, dvector* u, const int order, int* mark, double* diaginv)  // :277
{
    FASP_ENTRY();
    str_smoother_public(__func__, A, b, u, STR_SWEEP_GS, order, mark, false, 1.0, diaginv, false);
}
void fasp_smoother_dstr_gs_ascend(dSTRmat* A, dvector* b, dvector* u, double* diaginv)  // :322
{
    FASP_ENTRY();
    str_smoother_public(__func__, A, b, u, STR_SWEEP_GS, STR_ORDER_ASCEND, nullptr, false, 1.0, diaginv, false);
}
void fasp_smoother_dstr_gs_descend(dSTRmat* A, dvector* b, dvector* u, double* diaginv)  // :438
{
    FASP_ENTRY();
    str_smoother_public(__func__, A, b, u, STR_SWEEP_GS, STR_ORDER_DESCEND, nullptr, false, 1.0, diaginv, false);
}
void fasp_smoother_dstr_gs_order(dSTRmat* A, dvector* b, dvector* u, double* diaginv, int* mark)  // :556
{
    FASP_ENTRY();
    if (!mark) { std::fprintf(stderr, "### ERROR: %s: the user-defined order needs a mark array\n", __func__); return; }
    str_smoother_public(__func__, A, b, u, STR_SWEEP_GS, STR_ORDER_USER, mark, false, 1.0, diaginv, false);
}
void fasp_smoother_dstr_gs_cf(dSTRmat* A, dvector* b, dvector* u, double* diaginv, int* mark, const int order)  // :680
{
    FASP_ENTRY();
    str_smoother_public(__func__, A, b, u, STR_SWEEP_GS, order, mark, true, 1.0, diaginv, false);
}
void fasp_smoother_dstr_sor(dSTRmat* A, dvector* b, dvector* u, const int order, int* mark, const double weight)  // :873
{
    FASP_ENTRY();
    str_smoother_public(__func__, A, b, u, STR_SWEEP_SOR, order, mark, false, weight, nullptr, true);
}
void fasp_smoother_dstr_sor1(dSTRmat* A, dvector* b, dvector* u, const int order, int* mark, double* diaginv, const double weight)  // :935
{
    FASP_ENTRY();
    str_smoother_public(__func__, A, b, u, STR_SWEEP_SOR, order, mark, false, weight, diaginv, false);
}
void fasp_smoother_dstr_sor_ascend(dSTRmat* A, dvector* b, dvector* u, double* diaginv, double weight)  // :981
{
    FASP_ENTRY();
    str_smoother_public(__func__, A, b, u, STR_SWEEP_SOR, STR_ORDER_ASCEND, nullptr, false, weight, diaginv, false);
}
void fasp_smoother_dstr_sor_descend(dSTRmat* A, dvector* b, dvector* u, double* diaginv, double weight)  // :1102
{
    FASP_ENTRY();
    str_smoother_public(__func__, A, b, u, STR_SWEEP_SOR, STR_ORDER_DESCEND, nullptr, false, weight, diaginv, false);
}
void fasp_smoother_dstr_sor_order(dSTRmat* A, dvector* b, dvector* u, double* diaginv, int* mark, double weight)  // :1224
{
    FASP_ENTRY();
    if (!mark) { std::fprintf(stderr, "### ERROR: %s: the user-defined order needs a mark array\n", __func__); return; }
    str_smoother_public(__func__, A, b, u, STR_SWEEP_SOR, STR_ORDER_USER, mark, false, weight, diaginv, false);
}
void fasp_smoother_dstr_sor_cf(dSTRmat* A, dvector* b, dvector* u, double* diaginv, int* mark, const int order, const double weight)  // :1355
{
    FASP_ENTRY();
    str_smoother_public(__func__, A, b, u, STR_SWEEP_SOR, order, mark, true, weight, diaginv, false);
}

// ---- the dev entries of the sweeps (fasp_hip_dev.h) -------------------------------------------------------------------------------------
int fasp_hip_str_sweep(const dSTRmat* A, int kind, int order, const int* mark, double weight, const double* diaginv, const double* b, double* u,
                       int nsweeps, int* info)
{
    FASP_ENTRY();
    if (!A || !b || !u || nsweeps < 0) return ERROR_INPUT_PAR;
    return str_sweep_run(__func__, A, kind, order, mark, false, weight, diaginv, true, b, u, nsweeps, info, 0, nullptr, nullptr);
}
int fasp_hip_str_sweep_form(const dSTRmat* A, int order, const int* mark)
{
    FASP_ENTRY();
    StrSweepPrep P;
    const int st = str_sweep_prepare(__func__, A, STR_SWEEP_GS, order, mark, false, nullptr, false, false, P);
    if (st < 0) return st;
    if (!P.todo) { std::printf("fasp_hip_str_sweep_form: mark is NULL and the order is neither ASCEND nor DESCEND: nothing is swept\n"); return -1; }
    if (!P.D.geo) std::printf("fasp_hip_str_sweep_form: not the geometric form: %s\n", P.D.why);
    else if (!P.natural) std::printf("fasp_hip_str_sweep_form: not the geometric form: the order is a sequence or a C/F marking\n");
    std::fflush(stdout);
    return P.form;
}
int fasp_hip_str_sweep_levels(const dSTRmat* A, int order, const int* mark, int* visit, int* level, int cap)
{
    FASP_ENTRY();
    StrSweepPrep P;
    const int st = str_sweep_prepare(__func__, A, STR_SWEEP_GS, order, mark, false, nullptr, false, false, P);
    if (st < 0) return st;
    if (!P.todo) return 0;
    if (P.form != STR_SWF_LIST) str_sweep_visits(P.D.ngrid, order, mark, P.cf, false, P.seq);
    std::vector<int> lev;
    (void)str_sweep_levels(P.D, P.seq, lev);
    for (size_t v = 0; v < P.seq.size() && (int)v < cap; ++v) {
        if (visit) visit[v] = P.seq[v] & 0x7fffffff;
        if (level) level[v] = lev[v];
    }
    return (int)P.seq.size();
}
double fasp_hip_time_str_sweep(const dSTRmat* A, int kind, int order, const int* mark, double weight, int reps)
{
    FASP_ENTRY();
    if (!A || reps <= 0 || A->ngrid <= 0 || A->nc < 1 || A->nc > 7) return -1.0;
    const size_t n = (size_t)A->ngrid * A->nc;
    std::vector<double> hb(n), hu(n, 0.0);
    for (size_t i = 0; i < n; ++i) hb[i] = std::sin(0.37 * (double)i) + 0.1;
    double ms = -1.0;
    const int st = str_sweep_run(__func__, A, kind, order, mark, false, weight, nullptr, true, hb.data(), hu.data(), 1, nullptr, reps, &ms, nullptr);
    return st < 0 ? -1.0 : ms;
}

// ---- block Gauss-Seidel (Schwarz): ItrSmootherSTR.c:1543 / :1665, PreSTR.c:1715, SolSTR.c:323 (csrc/str_swz.hip.h) ----
namespace {
// what every entry checks first.  0: go on; 1: nothing to do, said (nc < 1: the reference's message); a matrix the library refuses ends the process
int str_swz_gate(const char* fn, const dSTRmat* A)
{
    if (!A) { std::fprintf(stderr, "### ERROR: %s: NULL argument\n", fn); return 1; }
    if (A->nc < 1) { std::printf("### ERROR: nc is illegal! [%s]\n", fn); std::fflush(stdout); return 1; }
    if (str_plan(A, nullptr) < 0) die_str(fn, ERROR_INPUT_PAR);
    return 0;
}
void str_swz_fail(const char* fn, int st)
{
    if (st == ERROR_MISC && !g_ctx.ready) die_str(fn, 0);
    std::fprintf(stderr, "### ERROR: %s: failed (%d)\n", fn, st);
    std::exit(st);
}
int str_swz_refuse_stopped(const char* fn, const StrSwzDev& M)
{
    if (!M.nstopped) return FASP_SUCCESS;
    std::fprintf(stderr, "### ERROR: %s: the factorisation of %d patch(es) stopped at a pivot below 1e-20\n", fn, M.nstopped);
    return ERROR_INPUT_PAR;
}
// one sweep (zero_u: from u = 0) with the resident object M on host vectors
int str_swz_oneshot(StrSwzDev& M, const double* b, double* u, bool zero_u)
{
    const size_t n = (size_t)M.P.ngrid * M.P.nc;
    HIPCK(hipMemcpyAsync(M.b, b, sizeof(double) * n, hipMemcpyHostToDevice, g_ctx.stream));
    if (zero_u) HIPCK(hipMemsetAsync(M.u, 0, sizeof(double) * n, g_ctx.stream));
    else HIPCK(hipMemcpyAsync(M.u, u, sizeof(double) * n, hipMemcpyHostToDevice, g_ctx.stream));
    const int st = M.sweep(M.b, M.u);
    HIPCK(hipStreamSynchronize(g_ctx.stream));
    if (st < 0) return st;
    HIPCK(hipMemcpy(u, M.u, sizeof(double) * n, hipMemcpyDeviceToHost));
    return FASP_SUCCESS;
}
void str_swz_info(const StrSwzDev& M, int* info)
{
    if (!info) return;
    info[0] = M.P.levels; info[1] = M.launches; info[2] = (int)M.P.seq.size(); info[3] = M.P.widest; info[4] = M.P.ms; info[5] = M.nswap;
    info[6] = M.nstopped; info[7] = 0;
}
}  // namespace

void fasp_generate_diaginv_block(dSTRmat* A, ivector* neigh, dvector* diaginv, ivector* pivot)  // ItrSmootherSTR.c:1543
{
    FASP_ENTRY();
    if (str_swz_gate(__func__, A)) return;
    if (!diaginv || !pivot) { std::fprintf(stderr, "### ERROR: %s: NULL argument\n", __func__); return; }
    StrSwzPlan P;
    if (str_swz_plan(__func__, A, neigh, nullptr, false, P) < 0) return;   // said; diaginv and pivot untouched
    const int ngrid = P.ngrid, nc = P.nc;
    const size_t w = ((size_t)P.nneigh + 1) * nc, nd = w * w * (size_t)ngrid, np = w * (size_t)ngrid;
    if (nd > 0xffffffffull) { std::fprintf(stderr, "### ERROR: %s: the factors do not fit one fasp_mem_calloc block\n", __func__); return; }
    if (ctx_init() < 0) die_str(__func__, 0);
    const std::vector<int> msize = P.msize;
    const int ms = P.ms;
    StrSwzDev M(A, std::move(P), nullptr, nullptr);
    if (!M.ok) str_swz_fail(__func__, M.st);
    std::vector<double> hf(std::max<size_t>(M.nfac, 1));
    std::vector<int> hp(std::max<size_t>(M.npiv, 1));
    if ((M.nfac && hipMemcpy(hf.data(), M.fac, sizeof(double) * M.nfac, hipMemcpyDeviceToHost) != hipSuccess) ||
        (M.npiv && hipMemcpy(hp.data(), M.piv, sizeof(int) * M.npiv, hipMemcpyDeviceToHost) != hipSuccess)) str_swz_fail(__func__, ERROR_MISC);
    double* temp = (double*)fasp_mem_calloc((unsigned)nd, sizeof(double));
    int*    tmp = (int*)fasp_mem_calloc((unsigned)np, sizeof(int));
    size_t mem_inv = 0, mem_pivot = 0;
    const size_t ms2 = (size_t)ms * ms;
    for (int i = 0; i < ngrid; ++i) {   // (the list of a factorisation-only plan is the natural order: slot i is point i)
        const int m = msize[(size_t)i];
        const size_t s = (size_t)i, fb = (s >> 6) * ms2 * 64 + (s & 63), pb = (s >> 6) * (size_t)ms * 64 + (s & 63);
        diaginv[i].row = m * m; diaginv[i].val = temp + mem_inv;
        pivot[i].row = m; pivot[i].val = tmp + mem_pivot;
        for (int e = 0; e < m * m; ++e) diaginv[i].val[e] = hf[fb + (size_t)e * 64];
        for (int k = 0; k < m; ++k) pivot[i].val[k] = hp[pb + (size_t)k * 64];
        mem_inv += (size_t)m * m; mem_pivot += (size_t)m;
    }
}

void fasp_smoother_dstr_swz(dSTRmat* A, dvector* b, dvector* u, dvector* diaginv, ivector* pivot, ivector* neigh, ivector* order)  // ItrSmootherSTR.c:1665
{
    FASP_ENTRY();
    if (str_swz_gate(__func__, A)) return;
    if (!b || !u || !b->val || !u->val) { std::fprintf(stderr, "### ERROR: %s: NULL argument\n", __func__); return; }
    const long long n = (long long)A->ngrid * A->nc;
    if (A->ngrid > 0 && (b->row < n || u->row < n)) { std::fprintf(stderr, "### ERROR: %s: b and u need ngrid * nc = %lld entries\n", __func__, n); return; }
    StrSwzPlan P;
    if (str_swz_plan(__func__, A, neigh, order, true, P) < 0 || str_swz_check_factors(__func__, P, diaginv, pivot) < 0) return;   // said, u untouched
    if (P.ngrid == 0) return;
    if (ctx_init() < 0) die_str(__func__, 0);
    StrSwzDev M(A, std::move(P), diaginv, pivot);
    if (!M.ok) str_swz_fail(__func__, M.st);
    const int st = str_swz_oneshot(M, b->val, u->val, false);
    if (st < 0) str_swz_fail(__func__, st);
}

void fasp_precond_dstr_blockgs(double* r, double* z, void* data)  // PreSTR.c:1715
{
    FASP_ENTRY();
    const precond_data_str* d = static_cast<const precond_data_str*>(data);
    if (!r || !z || !d) { std::fprintf(stderr, "### ERROR: %s: NULL argument\n", __func__); return; }
    if (str_swz_gate(__func__, d->A_str)) return;
    if (d->A_str->ngrid == 0) return;
    if (StrSwzDev* R = str_swz_resident(data)) {   // factors that live on the device (fasp_solver_dstr_krylov_blockgs)
        const int st = str_swz_oneshot(*R, r, z, true);
        if (st < 0) str_swz_fail(__func__, st);
        return;
    }
    StrSwzPlan P;
    if (str_swz_plan(__func__, d->A_str, d->neigh, d->order, true, P) < 0 || str_swz_check_factors(__func__, P, d->diaginv, d->pivot) < 0) return;   // said, z untouched
    if (ctx_init() < 0) die_str(__func__, 0);
    StrSwzDev M(d->A_str, std::move(P), d->diaginv, d->pivot);
    if (!M.ok) str_swz_fail(__func__, M.st);
    const int st = str_swz_oneshot(M, r, z, true);
    if (st < 0) str_swz_fail(__func__, st);
}

// SolSTR.c:323: every patch factored on the device (the factors stay there), then the Krylov method with the sweep bound (bind_blockgs_str)
int fasp_solver_dstr_krylov_blockgs(dSTRmat* A, dvector* b, dvector* x, ITS_param* itparam, ivector* neigh, ivector* order)
{
    FASP_ENTRY();
    if (!itparam || !A || !b || !x) return ERROR_INPUT_PAR;
    const short prtlvl = itparam->print_level;
    if (A->nc < 1) { std::printf("### ERROR: nc is illegal! [%s]\n", __func__); std::fflush(stdout); return ERROR_INPUT_PAR; }
    if (str_plan(A, nullptr) < 0) return ERROR_INPUT_PAR;
    StrSwzPlan P;
    if (str_swz_plan(__func__, A, neigh, order, true, P) < 0) return ERROR_INPUT_PAR;
    if (ctx_init() < 0) die_no_device(__func__);
    const double t0 = wall_seconds();
    StrSwzDev M(A, std::move(P), nullptr, nullptr);
    if (!M.ok) return M.st;
    if (str_swz_refuse_stopped(__func__, M) < 0) return ERROR_INPUT_PAR;
    precond_data_str pcdata{};
    pcdata.A_str = A; pcdata.order = order; pcdata.neigh = neigh;   // diaginv, pivot: NULL -- the factors are M's
    precond pc{&pcdata, fasp_precond_dstr_blockgs};
    const double setup_time = wall_seconds() - t0;
    if (prtlvl > PRINT_NONE) std::printf("Preconditioner setup costs %f seconds.\n", setup_time);
    const double t1 = wall_seconds();
    g_swz_resident.emplace_back(&pcdata, &M);
    const int status = fasp_solver_dstr_itsolver(A, b, x, &pc, itparam);
    g_swz_resident.pop_back();
    if (prtlvl >= PRINT_MIN) {
        const double solve_time = wall_seconds() - t1;
        std::printf("Iterative solver costs %.4f seconds\n", solve_time);
        std::printf("BlockGS_Krylov method totally costs %.4f seconds\n", setup_time + solve_time);
    }
    return status;
}

// ---- the dev entries of the block Gauss-Seidel sweep (fasp_hip_dev.h) --------------------------------------------------------------------
namespace {
struct StrSwzRaw {   // (neigh, nneigh, order) of a dev entry as the ivectors the plan takes
    ivector nv{0, nullptr}, ov{0, nullptr};
    StrSwzRaw(const dSTRmat* A, const int* neigh, int nneigh, const int* order)
    {
        const long long ngrid = A ? A->ngrid : 0;
        if (neigh && nneigh > 0 && ngrid * nneigh <= 0x7fffffffLL) { nv.row = (int)(ngrid * nneigh); nv.val = const_cast<int*>(neigh); }
        if (order) { ov.row = (int)ngrid; ov.val = const_cast<int*>(order); }
    }
    const ivector* n() const { return nv.val ? &nv : nullptr; }
    const ivector* o() const { return ov.val ? &ov : nullptr; }
};
}  // namespace

int fasp_hip_str_swz(const dSTRmat* A, const int* neigh, int nneigh, const int* order, const double* b, double* u, int nsweeps, int* info)
{
    FASP_ENTRY();
    if (info) std::fill(info, info + 8, 0);
    if (!A || !b || !u || nsweeps < 0 || nneigh < 0) return ERROR_INPUT_PAR;
    const StrSwzRaw raw(A, neigh, nneigh, order);
    StrSwzPlan P;
    if (str_swz_plan(__func__, A, raw.n(), raw.o(), true, P) < 0) return ERROR_INPUT_PAR;
    if (P.ngrid == 0) return FASP_SUCCESS;
    if (ctx_init() < 0) return ERROR_MISC;
    StrSwzDev M(A, std::move(P), nullptr, nullptr);
    if (!M.ok) return M.st;
    str_swz_info(M, info);
    if (str_swz_refuse_stopped(__func__, M) < 0) return ERROR_INPUT_PAR;
    const size_t n = (size_t)M.P.ngrid * M.P.nc;
    HIPCK(hipMemcpy(M.b, b, sizeof(double) * n, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(M.u, u, sizeof(double) * n, hipMemcpyHostToDevice));
    int st = FASP_SUCCESS;
    for (int s = 0; s < nsweeps && st >= 0; ++s) st = M.sweep(M.b, M.u);
    HIPCK(hipStreamSynchronize(g_ctx.stream));
    if (st < 0) return st;
    HIPCK(hipMemcpy(u, M.u, sizeof(double) * n, hipMemcpyDeviceToHost));
    str_swz_info(M, info);
    return FASP_SUCCESS;
}
int fasp_hip_str_swz_levels(const dSTRmat* A, const int* neigh, int nneigh, const int* order, int* visit, int* level, int cap)
{
    FASP_ENTRY();
    if (!A || nneigh < 0) return ERROR_INPUT_PAR;
    const StrSwzRaw raw(A, neigh, nneigh, order);
    StrSwzPlan P;
    if (str_swz_plan(__func__, A, raw.n(), raw.o(), true, P) < 0) return ERROR_INPUT_PAR;
    for (size_t v = 0; v < P.seq.size() && (int)v < cap; ++v) {
        if (visit) visit[v] = P.seq[v];
        if (level) level[v] = P.lev[v];
    }
    return (int)P.seq.size();
}
int fasp_hip_time_str_swz(const dSTRmat* A, const int* neigh, int nneigh, const int* order, int reps, double* ms_factor, double* ms_sweep, int* info)
{
    FASP_ENTRY();
    if (info) std::fill(info, info + 8, 0);
    if (!A || reps <= 0 || nneigh < 0 || A->ngrid <= 0) return ERROR_INPUT_PAR;
    const StrSwzRaw raw(A, neigh, nneigh, order);
    StrSwzPlan P;
    if (str_swz_plan(__func__, A, raw.n(), raw.o(), true, P) < 0) return ERROR_INPUT_PAR;
    if (ctx_init() < 0) return ERROR_MISC;
    StrSwzDev M(A, std::move(P), nullptr, nullptr);   // (the warm-up factorisation)
    if (!M.ok) return M.st;
    str_swz_info(M, info);
    if (str_swz_refuse_stopped(__func__, M) < 0) return ERROR_INPUT_PAR;
    const size_t n = (size_t)M.P.ngrid * M.P.nc;
    std::vector<double> hb(n);
    for (size_t i = 0; i < n; ++i) hb[i] = std::sin(0.37 * (double)i) + 0.1;
    HIPCK(hipMemcpy(M.b, hb.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    double tf = 0.0, ts = 0.0;
    int st = time_reps(reps, [&] { return M.launch_factor(); }, &tf);
    if (st >= 0) st = M.precond(M.b, M.u);   // warm-up
    if (st >= 0) st = time_reps(reps, [&] { return M.precond(M.b, M.u); }, &ts);
    str_swz_info(M, info);
    if (ms_factor) *ms_factor = tf;
    if (ms_sweep) *ms_sweep = ts;
    return st;
}
