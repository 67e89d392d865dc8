// safe_krylov.hip.h -- the Krylov methods with a safety net (KrySPcg.c, KrySPbcgs.c, KrySPminres.c; the GMRES pair is gmres_device,
// modes 2 and 4): the best iterate seen so far is kept and handed back when the iteration breaks down, produces a NaN or ends on a worse
// iterate than an earlier one.  The update kernels carry every vector pass the reference makes between writing the new iterate and
// deciding about the safety net (isnan, the copy to u_best, norminf, norm2, the norm of the update, the residual norm).
// Part of the single translation unit solver.hip (included there, behind krylov.hip.h; not a stand-alone header).

// ---------------------------------------------------------------------------
// kernels.  Elementwise results have the bits of the reference's BLAS-1 sequence (fasp_blas_darray_axpy: y + a x; _axpby: a x + b y;
// no contraction); the sums go through this project's fixed trees (block partials, then k_finalize).
// An iterate is written OUT OF PLACE (u_in -> u_out, which may be the same buffer): see SafeIterate below.
// ---------------------------------------------------------------------------
// block partials of NQ quantities (bit k of MAXMASK: a maximum), partials[k * gridDim.x + blockIdx.x] -- the layout k_finalize reads
template <int NQ, unsigned MAXMASK>
__device__ __forceinline__ void safe_block_partials(const double (&q)[NQ], double* __restrict__ partials)
{
    __shared__ double lds[NQ][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        double v = q[k];
        if ((MAXMASK >> k) & 1u) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
        } else {
            v = subwave_sum<64>(v);
        }
        if (lane == 0) lds[k][wave] = v;
    }
    __syncthreads();
    if (threadIdx.x < NQ) {
        const int k = threadIdx.x;
        const double v = ((MAXMASK >> k) & 1u) ? fmax(fmax(lds[k][0], lds[k][1]), fmax(lds[k][2], lds[k][3]))
                                               : ((lds[k][0] + lds[k][1]) + lds[k][2]) + lds[k][3];
        partials[k * gridDim.x + blockIdx.x] = v;
    }
}

// KrySPcg.c:151-208 (and KrySPminres.c:170-173, :216-270 with p = p1, t = t1):  u_out = u_in + alpha p;  r += (-alpha) t;
// q0 = r.r, q1 = u.u, q2 = p.p, q3 = max|u|, q4 = number of NaN entries of u
__global__ __launch_bounds__(BLOCK) void k_safe_cg_update(int n, double alpha, const double* __restrict__ p,
                                                           const double* __restrict__ t, const double* u_in, double* u_out,
                                                           double* __restrict__ r, double* __restrict__ partials)
{
    double q[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const double ma = -alpha;
    auto one = [&](double pi, double ti, double ui, double ri, double& uo, double& ro) {
        uo = ui + alpha * pi;
        ro = ri + ma * ti;
        q[0] += ro * ro;
        q[1] += uo * uo;
        q[2] += pi * pi;
        q[3] = fmax(q[3], fabs(uo));
        q[4] += (uo != uo) ? 1.0 : 0.0;
    };
    const int n2 = n >> 1;
    const double2* p2 = reinterpret_cast<const double2*>(p);
    const double2* t2 = reinterpret_cast<const double2*>(t);
    const double2* ui2 = reinterpret_cast<const double2*>(u_in);
    double2*       uo2 = reinterpret_cast<double2*>(u_out);
    double2*       r2 = reinterpret_cast<double2*>(r);
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n2; i += gridDim.x * BLOCK) {
        const double2 pv = p2[i], tv = t2[i], uv = ui2[i], rv = r2[i];
        double2 uo, ro;
        one(pv.x, tv.x, uv.x, rv.x, uo.x, ro.x);
        one(pv.y, tv.y, uv.y, rv.y, uo.y, ro.y);
        uo2[i] = uo;
        r2[i] = ro;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double uo, ro;
        one(p[n - 1], t[n - 1], u_in[n - 1], r[n - 1], uo, ro);
        u_out[n - 1] = uo;
        r[n - 1] = ro;
    }
    safe_block_partials<5, 1u << 3>(q, partials);
}

// KrySPbcgs.c:158-159:  s = r + (-alpha) z
__global__ __launch_bounds__(BLOCK) void k_safe_bcgs_s(int n, double alpha, const double* __restrict__ r, const double* __restrict__ z,
                                                        double* __restrict__ s)
{
    const double ma = -alpha;
    const int n2 = n >> 1;
    const double2* r2 = reinterpret_cast<const double2*>(r);
    const double2* z2 = reinterpret_cast<const double2*>(z);
    double2*       s2 = reinterpret_cast<double2*>(s);
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n2; i += gridDim.x * BLOCK) {
        const double2 rv = r2[i], zv = z2[i];
        double2 sv;
        sv.x = rv.x + ma * zv.x;
        sv.y = rv.y + ma * zv.y;
        s2[i] = sv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) s[n - 1] = r[n - 1] + ma * z[n - 1];
}

// KrySPbcgs.c:171-174: q0 = t.t, q1 = s.t in one pass over t
__global__ __launch_bounds__(BLOCK) void k_safe_dot2(int n, const double* __restrict__ t, const double* __restrict__ s,
                                                      double* __restrict__ partials)
{
    double q[2] = {0.0, 0.0};
    const int n2 = n >> 1;
    const double2* t2 = reinterpret_cast<const double2*>(t);
    const double2* s2 = reinterpret_cast<const double2*>(s);
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n2; i += gridDim.x * BLOCK) {
        const double2 tv = t2[i], sv = s2[i];
        q[0] += tv.x * tv.x; q[1] += sv.x * tv.x;
        q[0] += tv.y * tv.y; q[1] += sv.y * tv.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) { q[0] += t[n - 1] * t[n - 1]; q[1] += s[n - 1] * t[n - 1]; }
    safe_block_partials<2, 0u>(q, partials);
}

// KrySPbcgs.c:182-193, :209-210, :220, :238, :257:  sp_out = alpha pp + omega sp_in;  u_out = u_in + sp_out;  s += (-omega) t;  r = s;
// q0 = (r, rho), q1 = sp.sp, q2 = u.u, q3 = r.r, q4 = max|u|, q5 = number of NaN entries of u.
// sp_in may be s itself (no preconditioner: sp is a copy of s) or sp_out (the preconditioner wrote it); u_in may be u_out.
__global__ __launch_bounds__(BLOCK) void k_safe_bcgs_update(int n, double alpha, double omega, const double* __restrict__ pp,
                                                             const double* sp_in, double* sp_out, const double* u_in, double* u_out,
                                                             double* s, const double* __restrict__ t, double* __restrict__ r,
                                                             const double* __restrict__ rho, double* __restrict__ partials)
{
    double q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double mo = -omega;
    auto one = [&](double ppi, double spi, double ui, double si, double ti, double rhoi, double& spo, double& uo, double& so) {
        spo = alpha * ppi + omega * spi;
        uo = ui + spo;
        so = si + mo * ti;
        q[0] += so * rhoi;
        q[1] += spo * spo;
        q[2] += uo * uo;
        q[3] += so * so;
        q[4] = fmax(q[4], fabs(uo));
        q[5] += (uo != uo) ? 1.0 : 0.0;
    };
    const int n2 = n >> 1;
    const double2* pp2 = reinterpret_cast<const double2*>(pp);
    const double2* spi2 = reinterpret_cast<const double2*>(sp_in);
    double2*       spo2 = reinterpret_cast<double2*>(sp_out);
    const double2* ui2 = reinterpret_cast<const double2*>(u_in);
    double2*       uo2 = reinterpret_cast<double2*>(u_out);
    double2*       s2 = reinterpret_cast<double2*>(s);
    const double2* t2 = reinterpret_cast<const double2*>(t);
    double2*       r2 = reinterpret_cast<double2*>(r);
    const double2* rho2 = reinterpret_cast<const double2*>(rho);
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n2; i += gridDim.x * BLOCK) {
        const double2 ppv = pp2[i], spv = spi2[i], uv = ui2[i], sv = s2[i], tv = t2[i], rhov = rho2[i];
        double2 spo, uo, so;
        one(ppv.x, spv.x, uv.x, sv.x, tv.x, rhov.x, spo.x, uo.x, so.x);
        one(ppv.y, spv.y, uv.y, sv.y, tv.y, rhov.y, spo.y, uo.y, so.y);
        spo2[i] = spo;
        uo2[i] = uo;
        s2[i] = so;
        r2[i] = so;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int i = n - 1;
        double spo, uo, so;
        one(pp[i], sp_in[i], u_in[i], s[i], t[i], rho[i], spo, uo, so);
        sp_out[i] = spo;
        u_out[i] = uo;
        s[i] = so;
        r[i] = so;
    }
    safe_block_partials<6, 1u << 4>(q, partials);
}

// KrySPbcgs.c:203-206:  p += (-omega) z;  p = 1.0 r + beta p
__global__ __launch_bounds__(BLOCK) void k_safe_bcgs_p(int n, double omega, double beta, const double* __restrict__ r,
                                                        const double* __restrict__ z, double* __restrict__ p)
{
    const double mo = -omega;
    const int n2 = n >> 1;
    const double2* r2 = reinterpret_cast<const double2*>(r);
    const double2* z2 = reinterpret_cast<const double2*>(z);
    double2*       p2 = reinterpret_cast<double2*>(p);
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n2; i += gridDim.x * BLOCK) {
        const double2 rv = r2[i], zv = z2[i];
        double2 pv = p2[i];
        pv.x = pv.x + mo * zv.x;
        pv.y = pv.y + mo * zv.y;
        pv.x = 1.0 * rv.x + beta * pv.x;
        pv.y = 1.0 * rv.y + beta * pv.y;
        p2[i] = pv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double v = p[n - 1] + mo * z[n - 1];
        p[n - 1] = 1.0 * r[n - 1] + beta * v;
    }
}

// KrySPgmres.c / KrySPvgmres.c, the end of a restart cycle (:296-303):  x_out = x_in + r;  q0 = x.x, q1 = max|x|, q2 = number of NaN entries
__global__ __launch_bounds__(BLOCK) void k_safe_x_update(int n, const double* __restrict__ r, const double* x_in, double* x_out,
                                                          double* __restrict__ partials)
{
    double q[3] = {0.0, 0.0, 0.0};
    auto one = [&](double ri, double xi, double& xo) {
        xo = xi + 1.0 * ri;
        q[0] += xo * xo;
        q[1] = fmax(q[1], fabs(xo));
        q[2] += (xo != xo) ? 1.0 : 0.0;
    };
    const int n2 = n >> 1;
    const double2* r2 = reinterpret_cast<const double2*>(r);
    const double2* xi2 = reinterpret_cast<const double2*>(x_in);
    double2*       xo2 = reinterpret_cast<double2*>(x_out);
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n2; i += gridDim.x * BLOCK) {
        const double2 rv = r2[i], xv = xi2[i];
        double2 xo;
        one(rv.x, xv.x, xo.x);
        one(rv.y, xv.y, xo.y);
        xo2[i] = xo;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double xo;
        one(r[n - 1], x_in[n - 1], xo);
        x_out[n - 1] = xo;
    }
    safe_block_partials<3, 1u << 1>(q, partials);
}

// ---------------------------------------------------------------------------
// The iterate and the best iterate: two device buffers whose roles swap.  When the current iterate is the best one the next update
// writes the other buffer, otherwise it updates in place; "save the best" is a pointer assignment, and the caller's vector (x0) is
// written once, by finish().  A copy is exact, so this changes no bits.  swap == false (fasp_hip_tune("safe_fused", 0)): the iterate
// stays in x0 and save() is the reference's fasp_darray_cp into x1.  x1 starts as zeros, as the reference's calloc leaves u_best.
// ---------------------------------------------------------------------------
struct SafeIterate {
    double *x0, *x1, *cur, *best;
    int  n;
    bool swap;
    SafeIterate(double* caller, double* spare, int n_, bool swap_) : x0(caller), x1(spare), cur(caller), best(spare), n(n_), swap(swap_) {}
    double* out() const { return (swap && cur == best) ? (cur == x0 ? x1 : x0) : cur; }   // where the next update writes
    int save()
    {
        if (swap) { best = cur; return 0; }
        HIPCK(hipMemcpyAsync(best, cur, sizeof(double) * n, hipMemcpyDeviceToDevice, g_ctx.stream));
        return 0;
    }
    int finish(bool restore)   // the caller's vector = the best iterate (restore) or the current one
    {
        const double* src = restore ? best : cur;
        if (src != x0) HIPCK(hipMemcpyAsync(x0, src, sizeof(double) * n, hipMemcpyDeviceToDevice, g_ctx.stream));
        cur = x0;
        return 0;
    }
};

// number of NaN entries of x with the existing kernel (fasp_dvec_isnan, AuxVector.c:39)
static int d_nan_count(int n, const double* x, double& count)
{
    double red[2];
    const int G = vec_grid(n);
    hipLaunchKernelGGL(k_norm1_nan, dim3(G), dim3(BLOCK), 0, g_ctx.stream, n, x, g_ctx.d_partials);
    d_finalize(G, 2, 0u, 0, false);
    if (fetch_red(0, 2, red) < 0) return ERROR_MISC;
    count = red[1];
    return 0;
}

// The update steps, each in its fused form (one launch) or as the reference's sequence over the existing BLAS-1 launches; the scalars
// land in red[] in the order of the fused kernel's partials.
// red = {r.r, u.u, p.p, max|u|, #NaN(u)}
static int safe_cg_update(bool fused, int n, double alpha, const double* p, const double* t, SafeIterate& U, double* r, double* red)
{
    if (fused) {
        const int G = vec_grid(n / 2 + 1);
        double* const o = U.out();
        hipLaunchKernelGGL(k_safe_cg_update, dim3(G), dim3(BLOCK), 0, g_ctx.stream, n, alpha, p, t, (const double*)U.cur, o, r,
                           g_ctx.d_partials);
        U.cur = o;
        d_finalize(G, 5, 1u << 3, 0, false);
        return fetch_red(0, 5, red);
    }
    double two[2];
    d_axpy(n, alpha, p, U.cur);
    d_axpy(n, -alpha, t, r);
    if (d_dot(n, r, r, red) < 0) return ERROR_MISC;
    KCK(d_nan_count(n, U.cur, red[4]));
    if (d_norms(n, U.cur, two) < 0) return ERROR_MISC;
    red[1] = two[0]; red[3] = two[1];
    return d_dot(n, p, p, red + 2);
}
static void safe_bcgs_s(bool fused, int n, double alpha, const double* r, const double* z, double* s)
{
    if (fused) {
        hipLaunchKernelGGL(k_safe_bcgs_s, dim3(vec_grid(n / 2 + 1)), dim3(BLOCK), 0, g_ctx.stream, n, alpha, r, z, s);
        return;
    }
    (void)hipMemcpyAsync(s, r, sizeof(double) * n, hipMemcpyDeviceToDevice, g_ctx.stream);
    d_axpy(n, -alpha, z, s);
}
// red = {t.t, s.t}
static int safe_dot2(bool fused, int n, const double* t, const double* s, double* red)
{
    if (fused) {
        const int G = vec_grid(n / 2 + 1);
        hipLaunchKernelGGL(k_safe_dot2, dim3(G), dim3(BLOCK), 0, g_ctx.stream, n, t, s, g_ctx.d_partials);
        d_finalize(G, 2, 0u, 0, false);
        return fetch_red(0, 2, red);
    }
    if (d_dot(n, t, t, red) < 0) return ERROR_MISC;
    return d_dot(n, s, t, red + 1);
}
// sp: the buffer of the update; sp_in: what it holds now (sp itself, or s when there is no preconditioner: the reference's copy of s)
// red = {(r,rho), sp.sp, u.u, r.r, max|u|, #NaN(u)}
static int safe_bcgs_update(bool fused, int n, double alpha, double omega, const double* pp, const double* sp_in, double* sp,
                            SafeIterate& U, double* s, const double* t, double* r, const double* rho, double* red)
{
    if (fused) {
        const int G = vec_grid(n / 2 + 1);
        double* const o = U.out();
        hipLaunchKernelGGL(k_safe_bcgs_update, dim3(G), dim3(BLOCK), 0, g_ctx.stream, n, alpha, omega, pp, sp_in, sp,
                           (const double*)U.cur, o, s, t, r, rho, g_ctx.d_partials);
        U.cur = o;
        d_finalize(G, 6, 1u << 4, 0, false);
        return fetch_red(0, 6, red);
    }
    double two[2];
    if (sp_in != sp) HIPCK(hipMemcpyAsync(sp, sp_in, sizeof(double) * n, hipMemcpyDeviceToDevice, g_ctx.stream));
    d_axpby(n, alpha, pp, omega, sp);
    d_axpy(n, 1.0, sp, U.cur);
    d_axpy(n, -omega, t, s);
    HIPCK(hipMemcpyAsync(r, s, sizeof(double) * n, hipMemcpyDeviceToDevice, g_ctx.stream));
    if (d_dot(n, r, rho, red) < 0) return ERROR_MISC;
    if (d_dot(n, sp, sp, red + 1) < 0) return ERROR_MISC;
    if (d_norms(n, U.cur, two) < 0) return ERROR_MISC;
    red[2] = two[0]; red[4] = two[1];
    if (d_dot(n, r, r, red + 3) < 0) return ERROR_MISC;
    return d_nan_count(n, U.cur, red[5]);
}
static void safe_bcgs_p(bool fused, int n, double omega, double beta, const double* r, const double* z, double* p)
{
    if (fused) {
        hipLaunchKernelGGL(k_safe_bcgs_p, dim3(vec_grid(n / 2 + 1)), dim3(BLOCK), 0, g_ctx.stream, n, omega, beta, r, z, p);
        return;
    }
    d_axpy(n, -omega, z, p);
    d_axpby(n, 1.0, r, beta, p);
}
// red = {x.x, max|x|, #NaN(x)}  (declared in krylov.hip.h: gmres_device ends its restart cycles with it)
// (gmres_device keeps the two buffers itself; the unfused sequence updates in place: x_in == x_out)
static int safe_x_update(bool fused, int n, const double* r, const double* x_in, double* x_out, double* red)
{
    if (fused) {
        const int G = vec_grid(n / 2 + 1);
        hipLaunchKernelGGL(k_safe_x_update, dim3(G), dim3(BLOCK), 0, g_ctx.stream, n, r, x_in, x_out, g_ctx.d_partials);
        d_finalize(G, 3, 1u << 1, 0, false);
        return fetch_red(0, 3, red);
    }
    if (x_in != x_out) return ERROR_INPUT_PAR;
    d_axpy(n, 1.0, r, x_out);
    if (d_norms(n, x_out, red) < 0) return ERROR_MISC;
    return d_nan_count(n, x_out, red[2]);
}

// ---------------------------------------------------------------------------
// drivers: the host scalar control flow of the reference's safe texts, branch for branch
// ---------------------------------------------------------------------------
// the RESTORE_BESTSOL block the three texts share (KrySPcg.c:325-354, KrySPbcgs.c:384-413, KrySPminres.c:444-472): true residual of
// u_best whenever iter != iter_best -- also at a MaxIt exit -- and the best iterate wins when it is better by more than maxdiff
static int safe_restore(KVecOps& V, const double* b, SafeIterate& U, double* r, double* z, int StopType, int PrtLvl, int iter,
                        int iter_best, double maxdiff, double absres, double normr0, double& relres)
{
    bool restore = false;
    if (iter != iter_best) {
        double absres_best = BIGREAL, t2;
        KCK(V.resid(U.best, b, r));
        switch (StopType) {
            case STOP_REL_RES: case STOP_MOD_REL_RES: KCK(V.nrm2(r, absres_best)); break;
            case STOP_REL_PRECRES: KCK(V.pc(r, z)); KCK(V.dot(z, r, t2)); absres_best = std::sqrt(std::fabs(t2)); break;
        }
        if (absres > absres_best + maxdiff || std::isnan(absres)) {
            if (PrtLvl > PRINT_NONE) std::printf("### WARNING: Discard current iteration. Restore iteration %d!\n", iter_best);
            restore = true;
            relres = absres_best / normr0;
        }
    }
    return U.finish(restore);
}
static int safe_final(KVecOps& V, SafeIterate& U, int PrtLvl, int iter, int MaxIt, double relres, double absres, double normr0, PcgOut* out)
{
    KCK(U.finish(false));   // (an exit that jumps over RESTORE_BESTSOL keeps the current iterate)
    if (PrtLvl > PRINT_NONE) {  // ITS_FINAL, KryUtil.inl:95-105
        if (iter > MaxIt) std::printf("### WARNING: MaxIt = %d reached with relative residual %.10e.\n", MaxIt, relres);
        else if (iter >= 0) std::printf("Number of iterations = %d with relative residual %.10e.\n", iter, relres);
    }
    if (out) { out->relres = relres; out->absres = absres; out->normr0 = normr0; }
    HIPCK(hipStreamSynchronize(V.s));
    return iter > MaxIt ? ERROR_SOLVER_MAXIT : iter;
}

// fasp_solver_dcsr_spcg, KrySPcg.c:60-370 (== fasp_solver_dstr_spcg, :726)
static int spcg_device(KOps& K, const double* b, double* u, double tol, int MaxIt, int StopType, int PrtLvl, PcgOut* out)
{
    KVecOps V(K);
    const int m = V.m;
    const bool fused = g_tune.safe_fused != 0;
    const double maxdiff = tol * STAG_RATIO, sol_inf_tol = SMALLREAL;
    int iter = 0, stag = 1, more_step = 1, iter_best = 0, st;
    double absres0 = BIGREAL, absres = BIGREAL, relres = BIGREAL, normu = BIGREAL, normr0 = BIGREAL, absres_best = BIGREAL;
    double reldiff, factor, alpha, beta, temp1, temp2, red[8];
    KCK(V.ensure(5));
    double *p = V.vec(0), *zbuf = V.vec(1), *r = V.vec(2), *t = V.vec(3), *z = nullptr;
    SafeIterate U(u, V.vec(4), m, fused);
    auto apply_pc = [&]() -> int {  // z = B r: the preconditioner's own output buffer, or r itself
        if (K.pc) return K.pc(r, &z);
        z = r;
        return FASP_SUCCESS;
    };
    auto resnorm = [&](bool have_rr, double rr) -> int {  // :157-175 and its copies
        switch (StopType) {
            case STOP_REL_RES:
                if (!have_rr) KCK(V.dot(r, r, rr));
                absres = std::sqrt(rr); relres = absres / normr0; break;
            case STOP_REL_PRECRES:
                if ((st = apply_pc()) < 0) return st;
                KCK(V.dot(z, r, rr)); absres = std::sqrt(std::fabs(rr)); relres = absres / normr0; break;
            case STOP_MOD_REL_RES:
                if (!have_rr) KCK(V.dot(r, r, rr));
                absres = std::sqrt(rr); relres = absres / normu; break;
        }
        return 0;
    };

    if (PrtLvl > PRINT_NONE) std::printf("\nCalling Safe CG solver (%s) ...\n", K.fmt);
    KCK(V.resid(U.cur, b, r));
    if ((st = apply_pc()) < 0) return st;
    switch (StopType) {
        case STOP_REL_RES:
            KCK(V.nrm2(r, absres0)); normr0 = std::max(SMALLREAL, absres0); relres = absres0 / normr0; break;
        case STOP_REL_PRECRES:
            KCK(V.dot(r, z, temp2)); absres0 = std::sqrt(temp2); normr0 = std::max(SMALLREAL, absres0); relres = absres0 / normr0; break;
        case STOP_MOD_REL_RES:
            KCK(V.nrm2(r, absres0)); KCK(V.nrm2(U.cur, normu)); normu = std::max(SMALLREAL, normu); relres = absres0 / normu; break;
        default:
            std::printf("### ERROR: Unknown stopping type! [%s]\n", "fasp_solver_dcsr_spcg");
            goto FINISHED;
    }
    if (relres < tol) goto FINISHED;
    itinfo(PrtLvl, StopType, iter, relres, absres0, 0.0);
    KCK(V.cp(p, z));
    KCK(V.dot(z, r, temp1));

    while (iter++ < MaxIt) {
        // t = A p and (t, p): on the SpMV where the format has the fused kernel
        {
            if (K.halo(p) < 0) return ERROR_MISC;
            const int gdot = K.mxv_dot ? K.mxv_dot(p, t) : -1;
            if (gdot >= 0) { d_finalize(gdot, 1, 0u, 0, false); if (fetch_red(0, 1, red) < 0) return ERROR_MISC; temp2 = red[0]; }
            else { K.mxv(p, t); KCK(V.dot(t, p, temp2)); }
        }
        if (std::fabs(temp2) > SMALLREAL2) alpha = temp1 / temp2;
        else goto RESTORE_BESTSOL;   // possible breakdown

        // u += alpha p, r -= alpha t, with every norm the checks below read
        if (safe_cg_update(fused, m, alpha, p, t, U, r, red) < 0) return ERROR_MISC;
        if ((st = resnorm(true, red[0])) < 0) return st;
        factor = absres / absres0;
        itinfo(PrtLvl, StopType, iter, relres, absres, factor);

        if (red[4] > 0.0) { absres = BIGREAL; goto RESTORE_BESTSOL; }   // the solution is NaN
        if (absres < absres_best - maxdiff) {   // save the best-so-far solution
            absres_best = absres;
            iter_best = iter;
            KCK(U.save());
        }
        if (red[3] <= sol_inf_tol) {   // Check I
            if (PrtLvl > PRINT_MIN)
                std::printf("### WARNING: Iteration stopped -- solution almost zero! [%s:%d]\n", "fasp_solver_dcsr_spcg", 199);
            iter = ERROR_SOLVER_SOLSTAG;
            break;
        }
        normu = std::sqrt(red[1]);   // Check II, in every iteration
        reldiff = std::fabs(alpha) * std::sqrt(red[2]) / normu;
        if ((stag <= MAX_STAG) & (reldiff < maxdiff)) {
            if (PrtLvl >= PRINT_MORE) {
                std::printf("||u-u'|| = %.10e and the comp. rel. res. = %.10e.\n", reldiff, relres);
                std::printf("### WARNING: Iteration restarted -- stagnation! [%s:%d]\n", "fasp_solver_dcsr_spcg", 213);
            }
            KCK(V.resid(U.cur, b, r));
            if ((st = resnorm(false, 0.0)) < 0) return st;
            if (PrtLvl >= PRINT_MORE) std::printf("### WARNING: The actual relative residual = %.10e!\n", relres);
            if (relres < tol) break;
            if (stag >= MAX_STAG) {
                if (PrtLvl > PRINT_MIN)
                    std::printf("### WARNING: Iteration stopped -- staggnation! [%s:%d]\n", "fasp_solver_dcsr_spcg", 246);
                iter = ERROR_SOLVER_STAG;
                break;
            }
            KCK(V.zero(p));
            ++stag;
        }
        if (relres < tol) {   // Check III: prevent false convergence
            if (PrtLvl >= PRINT_MORE) std::printf("### WARNING: The computed relative residual = %.10e!\n", relres);
            KCK(V.resid(U.cur, b, r));
            if ((st = resnorm(false, 0.0)) < 0) return st;
            if (PrtLvl >= PRINT_MORE) std::printf("### WARNING: The actual relative residual = %.10e!\n", relres);
            if (relres < tol) break;
            if (more_step >= MAX_RESTART) {
                if (PrtLvl > PRINT_MIN)
                    std::printf("### WARNING: The tolerence might be too small! [%s:%d]\n", "fasp_solver_dcsr_spcg", 292);
                iter = ERROR_SOLVER_TOLSMALL;
                break;
            }
            KCK(V.zero(p));
            ++more_step;
        }
        absres0 = absres;
        if (StopType != STOP_REL_PRECRES) { if ((st = apply_pc()) < 0) return st; }
        KCK(V.dot(z, r, temp2));
        beta = temp2 / temp1;
        temp1 = temp2;
        d_axpby(m, 1.0, z, beta, p);   // p = z + beta p
    }

RESTORE_BESTSOL:
    if ((st = safe_restore(V, b, U, r, zbuf, StopType, PrtLvl, iter, iter_best, maxdiff, absres, normr0, relres)) < 0) return st;
FINISHED:
    return safe_final(V, U, PrtLvl, iter, MaxIt, relres, absres, normr0, out);
}

// fasp_solver_dcsr_spbcgs, KrySPbcgs.c:61-430 (== fasp_solver_dbsr_spbcgs, :452, and fasp_solver_dstr_spbcgs, :1234)
static int spbcgs_device(KOps& K, const double* b, double* u, double tol, int MaxIt, int StopType, int PrtLvl, PcgOut* out)
{
    KVecOps V(K);
    const int m = V.m;
    const bool fused = g_tune.safe_fused != 0;
    const double maxdiff = tol * STAG_RATIO, sol_inf_tol = SMALLREAL, TOL_s = tol * 1e-2;
    int iter = 0, stag = 1, more_step = 1, iter_best = 0, st = 0;
    double alpha, beta, omega, temp1, temp2, tempr = 0.0, red[8];
    double absres0 = BIGREAL, absres = BIGREAL, relres = BIGREAL, normu = BIGREAL, normr0 = BIGREAL, absres_best = BIGREAL;
    double reldiff, factor, normd;
    KCK(V.ensure(9));
    double *p = V.vec(0), *z = V.vec(1), *r = V.vec(2), *t = V.vec(3), *rho = V.vec(4), *ppbuf = V.vec(5), *s = V.vec(6), *sp = V.vec(7);
    const double *pp = nullptr, *sp_in = nullptr;
    SafeIterate U(u, V.vec(8), m, fused);
    auto resnorm = [&](bool have_rr, double rr, bool check3) -> int {  // :218-235 and its copies
        switch (StopType) {
            case STOP_REL_RES:
                if (!have_rr) KCK(V.dot(r, r, rr));
                absres = std::sqrt(rr); relres = absres / normr0; break;
            case STOP_REL_PRECRES:
                KCK(V.pc(r, z)); KCK(V.dot(r, z, rr)); absres = std::sqrt(std::fabs(rr));
                relres = (check3 ? tempr : absres) / normr0;   // (:354 divides tempr)
                break;
            case STOP_MOD_REL_RES:
                if (!have_rr) KCK(V.dot(r, r, rr));
                absres = std::sqrt(rr); relres = absres / normu; break;
        }
        return 0;
    };
    auto reinit = [&]() -> int {  // :273-285 == :328-340 (pp is recomputed at the top of the loop)
        KCK(V.resid(U.cur, b, r));
        KCK(V.cp(p, r));
        KCK(V.cp(rho, r));
        return V.dot(r, rho, temp1);
    };

    if (PrtLvl > PRINT_NONE) std::printf("\nCalling Safe BiCGstab solver (%s) ...\n", K.fmt);
    KCK(V.resid(U.cur, b, r));
    KCK(V.nrm2(r, absres0));
    switch (StopType) {
        case STOP_REL_RES: case STOP_REL_PRECRES: normr0 = std::max(SMALLREAL, absres0); relres = absres0 / normr0; break;
        case STOP_MOD_REL_RES: KCK(V.nrm2(U.cur, normu)); normu = std::max(SMALLREAL, normu); relres = absres0 / normu; break;
        default:
            std::printf("### ERROR: Unknown stopping type! [%s]\n", "fasp_solver_dcsr_spbcgs");
            goto FINISHED;
    }
    if (relres < tol) goto FINISHED;
    itinfo(PrtLvl, StopType, iter, relres, absres0, 0.0);
    KCK(V.cp(rho, r));
    KCK(V.dot(r, rho, temp1));
    KCK(V.cp(p, r));

    while (iter++ < MaxIt) {
        // pp = B p (without a preconditioner the reference copies: p is read in its place)
        if (K.pc) { KCK(V.pc(p, ppbuf)); pp = ppbuf; } else pp = p;
        KCK(V.mxv(const_cast<double*>(pp), z));
        KCK(V.dot(z, rho, temp2));
        if (std::fabs(temp2) > SMALLREAL) alpha = temp1 / temp2;
        else {
            std::printf("### WARNING: Divided by zero! [%s:%d]\n", "fasp_solver_dcsr_spbcgs", 154);
            goto FINISHED;
        }
        safe_bcgs_s(fused, m, alpha, r, z, s);
        if (K.pc) { KCK(V.pc(s, sp)); sp_in = sp; } else sp_in = s;
        KCK(V.mxv(const_cast<double*>(sp_in), t));
        if (safe_dot2(fused, m, t, s, red) < 0) return ERROR_MISC;
        tempr = red[0];
        if (std::fabs(tempr) > SMALLREAL) omega = red[1] / tempr;
        else {
            omega = 0.0;
            if (PrtLvl >= PRINT_SOME) std::printf("### WARNING: Divided by zero! [%s:%d]\n", "fasp_solver_dcsr_spbcgs", 178);
        }
        // delu = alpha pp + omega sp, u += delu, r = s - omega t, and every norm the checks below read
        if (safe_bcgs_update(fused, m, alpha, omega, pp, sp_in, sp, U, s, t, r, rho, red) < 0) return ERROR_MISC;
        temp2 = temp1;
        temp1 = red[0];
        if (std::fabs(temp2) > SMALLREAL) beta = (temp1 * alpha) / (temp2 * omega);
        else {
            std::printf("### WARNING: Divided by zero! [%s:%d]\n", "fasp_solver_dcsr_spbcgs", 199);
            goto RESTORE_BESTSOL;
        }
        safe_bcgs_p(fused, m, omega, beta, r, z, p);   // p = r + beta (p - omega z)
        normd = std::sqrt(red[1]);
        normu = std::sqrt(red[2]);
        reldiff = normd / normu;
        if (normd < TOL_s) {
            std::printf("### WARNING: sp is too small! [%s:%d]\n", "fasp_solver_dcsr_spbcgs", 214);
            goto FINISHED;
        }
        if ((st = resnorm(true, red[3], false)) < 0) return st;
        if (red[5] > 0.0) { absres = BIGREAL; goto RESTORE_BESTSOL; }   // the solution is NaN
        if (absres < absres_best - maxdiff) {
            absres_best = absres;
            iter_best = iter;
            KCK(U.save());
        }
        factor = absres / absres0;
        itinfo(PrtLvl, StopType, iter, relres, absres, factor);
        if (red[4] <= sol_inf_tol) {   // Check I
            if (PrtLvl > PRINT_MIN)
                std::printf("### WARNING: Iteration stopped -- solution almost zero! [%s:%d]\n", "fasp_solver_dcsr_spbcgs", 259);
            iter = ERROR_SOLVER_SOLSTAG;
            goto FINISHED;
        }
        if ((stag <= MAX_STAG) && (reldiff < maxdiff)) {   // Check II
            if (PrtLvl >= PRINT_MORE) {
                std::printf("||u-u'|| = %.10e and the comp. rel. res. = %.10e.\n", reldiff, relres);
                std::printf("### WARNING: Iteration restarted -- stagnation! [%s:%d]\n", "fasp_solver_dcsr_spbcgs", 269);
            }
            KCK(reinit());
            if ((st = resnorm(false, 0.0, false)) < 0) return st;
            if (PrtLvl >= PRINT_MORE) std::printf("### WARNING: The actual relative residual = %.10e!\n", relres);
            if (relres < tol) break;
            if (stag >= MAX_STAG) {
                if (PrtLvl > PRINT_MIN)
                    std::printf("### WARNING: Iteration stopped -- staggnation! [%s:%d]\n", "fasp_solver_dcsr_spbcgs", 313);
                iter = ERROR_SOLVER_STAG;
                goto FINISHED;
            }
            ++stag;
        }
        if (relres < tol) {   // Check III
            if (PrtLvl >= PRINT_MORE) std::printf("### WARNING: The computed relative residual = %.10e!\n", relres);
            KCK(reinit());
            if ((st = resnorm(false, 0.0, true)) < 0) return st;
            if (PrtLvl >= PRINT_MORE) std::printf("### WARNING: The actual relative residual = %.10e!\n", relres);
            if (relres < tol) break;
            if (more_step >= MAX_RESTART) {
                if (PrtLvl > PRINT_MIN)
                    std::printf("### WARNING: The tolerence might be too small! [%s:%d]\n", "fasp_solver_dcsr_spbcgs", 368);
                iter = ERROR_SOLVER_TOLSMALL;
                goto FINISHED;
            } else if (PrtLvl > PRINT_NONE)
                std::printf("### WARNING: Iteration restarted -- stagnation! [%s:%d]\n", "fasp_solver_dcsr_spbcgs", 373);
            ++more_step;
        }
        absres0 = absres;
    }

RESTORE_BESTSOL:
    if ((st = safe_restore(V, b, U, r, z, StopType, PrtLvl, iter, iter_best, maxdiff, absres, normr0, relres)) < 0) return st;
FINISHED:
    return safe_final(V, U, PrtLvl, iter, MaxIt, relres, absres, normr0, out);
}

// fasp_solver_dcsr_spminres, KrySPminres.c:60-488 (== fasp_solver_dstr_spminres, :962)
static int spminres_device(KOps& K, const double* b, double* u, double tol, int MaxIt, int StopType, int PrtLvl, PcgOut* out)
{
    KVecOps V(K);
    const int m = V.m;
    const bool fused = g_tune.safe_fused != 0;
    const double maxdiff = tol * STAG_RATIO, sol_inf_tol = SMALLREAL;
    int iter = 0, stag = 1, more_step = 1, iter_best = 0, st = 0;
    double absres0 = BIGREAL, absres = BIGREAL, normr0 = BIGREAL, relres = BIGREAL, absres_best = BIGREAL;
    double normu2 = BIGREAL, normuu, normp, factor, alpha, alpha0, alpha1, temp2, red[8];
    KCK(V.ensure(12));
    double *p0 = V.vec(0), *p1 = V.vec(1), *p2 = V.vec(2), *z0 = V.vec(3), *z1 = V.vec(4), *t0 = V.vec(5),
           *t1 = V.vec(6), *t = V.vec(7), *tp = V.vec(8), *tz = V.vec(9), *r = V.vec(10);
    const MinresVecs W{p0, p1, p2, z0, z1, t0, t1, t, tp, tz, r};
    SafeIterate U(u, V.vec(11), m, fused);
    auto resnorm = [&](bool have_rr, double rr) -> int {  // :219-239 and its copies
        switch (StopType) {
            case STOP_REL_RES:
                if (!have_rr) KCK(V.dot(r, r, rr));
                temp2 = rr; absres = std::sqrt(temp2); relres = absres / normr0; break;
            case STOP_REL_PRECRES:
                KCK(V.pc(r, t)); KCK(V.dot(r, t, temp2)); temp2 = std::fabs(temp2);
                absres = std::sqrt(temp2); relres = absres / normr0; break;
            case STOP_MOD_REL_RES:
                if (!have_rr) KCK(V.dot(r, r, rr));
                temp2 = rr; absres = std::sqrt(temp2); relres = absres / normu2; break;
        }
        return 0;
    };
    auto restart = [&]() -> int {  // :317-352 == :400-435
        KCK(V.zero(p0));
        KCK(V.pc(r, p1));
        KCK(V.mxv(p1, tp));
        KCK(V.pc(tp, tz));
        KCK(V.dot(tz, tp, normp));
        normp = std::sqrt(normp);
        KCK(V.cp(t, p1));
        KCK(V.zero(t0)); KCK(V.zero(z0)); KCK(V.zero(t1)); KCK(V.zero(z1)); KCK(V.zero(p1));
        d_axpy(m, 1 / normp, t, p1);
        d_axpy(m, 1 / normp, tp, t1);
        d_axpy(m, 1 / normp, tz, z1);
        return 0;
    };

    if (PrtLvl > PRINT_NONE) std::printf("\nCalling Safe MinRes solver (%s) ...\n", K.fmt);
    KCK(V.zero(p0));
    KCK(V.resid(U.cur, b, r));
    KCK(V.pc(r, p1));
    switch (StopType) {
        case STOP_REL_RES:
            KCK(V.nrm2(r, absres0)); normr0 = std::max(SMALLREAL, absres0); relres = absres0 / normr0; break;
        case STOP_REL_PRECRES:
            KCK(V.dot(r, p1, temp2)); absres0 = std::sqrt(temp2); normr0 = std::max(SMALLREAL, absres0); relres = absres0 / normr0; break;
        case STOP_MOD_REL_RES:
            KCK(V.nrm2(r, absres0)); KCK(V.nrm2(U.cur, normu2)); normu2 = std::max(SMALLREAL, normu2); relres = absres0 / normu2; break;
        default:
            std::printf("### ERROR: Unknown stopping type! [%s]\n", "fasp_solver_dcsr_spminres");
            goto FINISHED;
    }
    if (relres < tol) goto FINISHED;
    itinfo(PrtLvl, StopType, iter, relres, absres0, 0.0);
    KCK(minres_lanczos_start(V, W));   // :137-161 (the same lines as KryPminres.c)

    while (iter++ < MaxIt) {
        // :166-173: alpha = <r, z1>; u += alpha p1; r -= alpha t1 -- with ||r||^2, ||u||^2, max|u| and the NaN count of :216-262
        KCK(V.dot(r, z1, alpha));
        if (safe_cg_update(fused, m, alpha, p1, t1, U, r, red) < 0) return ERROR_MISC;
        // :175-214: the rest of the Lanczos step (minres_lanczos_step's lines behind its two updates)
        KCK(V.mxv(z1, t));
        KCK(V.dot(z1, t, alpha1));
        KCK(V.mxv(z0, t));
        KCK(V.dot(z1, t, alpha0));
        KCK(V.cp(p2, z1));
        d_axpy(m, -alpha1, p1, p2);
        d_axpy(m, -alpha0, p0, p2);
        KCK(V.mxv(p2, tp));
        KCK(V.pc(tp, tz));
        KCK(V.dot(tz, tp, normp));
        normp = std::sqrt(std::fabs(normp));
        KCK(V.cp(t, p2));
        KCK(V.zero(p2));
        d_axpy(m, 1 / normp, t, p2);
        KCK(V.cp(p0, p1)); KCK(V.cp(p1, p2)); KCK(V.cp(t0, t1)); KCK(V.cp(z0, z1));
        KCK(V.zero(t1)); KCK(V.zero(z1));
        d_axpy(m, 1 / normp, tp, t1);
        d_axpy(m, 1 / normp, tz, z1);

        normu2 = std::sqrt(red[1]);
        if ((st = resnorm(true, red[0])) < 0) return st;
        factor = absres / absres0;
        itinfo(PrtLvl, StopType, iter, relres, absres, factor);
        if (red[4] > 0.0) { absres = BIGREAL; goto RESTORE_BESTSOL; }   // the solution is NaN
        if (absres < absres_best - maxdiff) {
            absres_best = absres;
            iter_best = iter;
            KCK(U.save());
        }
        if (red[3] <= sol_inf_tol) {   // Check I
            if (PrtLvl > PRINT_MIN)
                std::printf("### WARNING: Iteration stopped -- solution almost zero! [%s:%d]\n", "fasp_solver_dcsr_spminres", 263);
            iter = ERROR_SOLVER_SOLSTAG;
            break;
        }
        KCK(V.nrm2(p1, normuu));   // Check II, in every iteration (the NEW p1, as the reference reads it)
        normuu = std::fabs(alpha) * (normuu / normu2);
        if (normuu < maxdiff) {
            if (stag < MAX_STAG && PrtLvl >= PRINT_MORE) {
                std::printf("||u-u'|| = %.10e and the comp. rel. res. = %.10e.\n", normuu, relres);
                std::printf("### WARNING: Iteration restarted -- stagnation! [%s:%d]\n", "fasp_solver_dcsr_spminres", 277);
            }
            KCK(V.resid(U.cur, b, r));
            if ((st = resnorm(false, 0.0)) < 0) return st;
            if (PrtLvl >= PRINT_MORE) std::printf("### WARNING: The actual relative residual = %.10e!\n", relres);
            if (relres < tol) break;
            if (stag >= MAX_STAG) {
                if (PrtLvl > PRINT_MIN)
                    std::printf("### WARNING: Iteration stopped -- staggnation! [%s:%d]\n", "fasp_solver_dcsr_spminres", 313);
                iter = ERROR_SOLVER_STAG;
                break;
            }
            ++stag;
            KCK(restart());
        }
        if (relres < tol) {   // Check III
            if (PrtLvl >= PRINT_MORE) std::printf("### WARNING: The computed relative residual = %.10e!\n", relres);
            KCK(V.resid(U.cur, b, r));
            if ((st = resnorm(false, 0.0)) < 0) return st;
            if (PrtLvl >= PRINT_MORE) std::printf("### WARNING: The actual relative residual = %.10e!\n", relres);
            if (relres < tol) break;
            if (more_step >= MAX_RESTART) {
                if (PrtLvl > PRINT_MIN)
                    std::printf("### WARNING: The tolerence might be too small! [%s:%d]\n", "fasp_solver_dcsr_spminres", 394);
                iter = ERROR_SOLVER_TOLSMALL;
                break;
            }
            ++more_step;
            KCK(restart());
        }
        absres0 = absres;
    }

RESTORE_BESTSOL:
    if ((st = safe_restore(V, b, U, r, t, StopType, PrtLvl, iter, iter_best, maxdiff, absres, normr0, relres)) < 0) return st;
FINISHED:
    return safe_final(V, U, PrtLvl, iter, MaxIt, relres, absres, normr0, out);
}
