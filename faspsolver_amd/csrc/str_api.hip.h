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
    const int nc = A->nc, nc2 = nc * nc, ngrid = A->ngrid, nband = A->nband, rows = nc * ngrid;
    int* ia = (int*)fasp_mem_calloc((unsigned)rows + 1, sizeof(int));
    auto has_term = [&](int i, int b) { const long long j = (long long)i + A->offsets[b]; return j >= 0 && j < ngrid; };
    long long nnz = 0;
    for (int i = 0; i < ngrid; ++i) {
        int blocks = 1;
        for (int b = 0; b < nband; ++b) blocks += has_term(i, b) ? 1 : 0;
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
            if (b >= 0 && !has_term(i, b)) continue;
            const int     off = b < 0 ? 0 : A->offsets[b], col0 = (i + off) * nc;
            const double* src = b < 0 ? A->diag + (size_t)i * nc2 : A->offdiag[b] + (size_t)(off < 0 ? i + off : i) * nc2;
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
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    str_mxv(M, dx.d, dy.d); str_mxv(M, dx.d, dy.d);
    (void)hipEventRecord(e0, g_ctx.stream);
    for (int i = 0; i < reps; ++i) str_mxv(M, dx.d, dy.d);
    (void)hipEventRecord(e1, g_ctx.stream);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return (double)ms / reps;
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
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.0;
    if (str_ilu_apply(M, M.r, M.z) < 0) return -1.0;   // warm-up
    (void)hipEventRecord(e0, g_ctx.stream);
    for (int i = 0; i < reps; ++i) (void)str_ilu_apply(M, M.r, M.z);
    (void)hipEventRecord(e1, g_ctx.stream);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (seq_err_check() < 0) return -1.0;
    return (double)ms / reps;
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
