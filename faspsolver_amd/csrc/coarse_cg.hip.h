// coarse_cg.hip.h -- coarsest level: safe CG (single-workgroup kernel or batched device-resident iteration).
// Part of the single translation unit solver.hip (included there, in this order; not a stand-alone header).

// ---------------------------------------------------------------------------
// coarsest level: safe-net CG without preconditioner (KrySPcg.c:60, called from
// PreMGUtil.inl:47 with StopType = STOP_REL_RES, maxit = MAX(250, MIN(n*n, 1000))).
// One host synchronisation per iteration: alpha is formed on the device.
// ---------------------------------------------------------------------------
// Coarsest levels that fit one CU's caches are solved by the single-workgroup kernels of
// small_solvers.hip.h (one launch, one synchronisation per solve instead of per iteration).
static bool small_coarse_ok(long long rows, long long stored_values)
{
    static int enabled = -1;
    if (enabled < 0) {
        const char* e = std::getenv("FASP_HIP_SMALL_COARSE");
        enabled = (e && std::atoi(e) == 0) ? 0 : 1;
    }
    return enabled && rows <= 4096 && stored_values <= 131072;
}
static SmallOut* small_out_dev() { return reinterpret_cast<SmallOut*>(g_ctx.d_partials2); }
static int small_out_fetch(SmallOut& o)
{
    HIPCK(hipMemcpyAsync(g_ctx.h_part, g_ctx.d_partials2, sizeof(SmallOut), hipMemcpyDeviceToHost, g_ctx.stream));
    HIPCK(hipStreamSynchronize(g_ctx.stream));
    std::memcpy(&o, g_ctx.h_part, sizeof(SmallOut));
    return 0;
}

// k_spcg_persist (small_solvers.hip.h): deal the rows of the coarsest matrix to the waves of the chip -- whole rows,
// longest first, always to the least loaded wave -- and lay their entries out slot by slot (64 lanes x NE slots per
// wave) for the registers.  Returns false (and remembers it) when the level does not fit the scheme.
static bool g_persist_disabled = false;
static bool build_persist_plan(fasp_hip_amg* h, int level)
{
    auto& P = h->persist;
    if (P.tried) return P.ok;
    P.tried = true;
    const HostCSR& A = h->H.L[(size_t)level].A;
    const int m = A.row;
    const int nblocks = g_ctx.num_cu, nw = (nblocks - 1) * 8;   // 512-thread blocks, block 0 owns no rows
    if (m < 1 || m > 6144 || m != A.col || nw < 8 || A.nnz <= 0) return false;
    std::vector<int> order((size_t)m), slots((size_t)m);
    for (int i = 0; i < m; ++i) { order[(size_t)i] = i; slots[(size_t)i] = (A.ia[i + 1] - A.ia[i] + 63) / 64; }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return slots[(size_t)x] > slots[(size_t)y]; });
    std::vector<int> load((size_t)nw, 0), cnt((size_t)nw, 0), wrow((size_t)nw * 8, -1), wend((size_t)nw * 8, 0);
    // least-loaded wave first: a binary heap of (load, wave)
    std::vector<std::pair<int, int>> heap;
    for (int w = 0; w < nw; ++w) heap.emplace_back(0, w);
    auto cmp = [](const std::pair<int, int>& x, const std::pair<int, int>& y) { return x > y; };
    std::make_heap(heap.begin(), heap.end(), cmp);
    for (int i : order) {
        if (slots[(size_t)i] == 0) continue;   // empty row: t_i = 0 is written by nobody -> not representable here
        std::pop_heap(heap.begin(), heap.end(), cmp);
        std::pair<int, int> top = heap.back();
        const int w = top.second;
        if (cnt[(size_t)w] >= 8) return false;
        load[(size_t)w] += slots[(size_t)i];
        wrow[(size_t)w * 8 + cnt[(size_t)w]] = i;
        wend[(size_t)w * 8 + cnt[(size_t)w]] = load[(size_t)w];
        cnt[(size_t)w]++;
        heap.back() = std::make_pair(load[(size_t)w], w);
        std::push_heap(heap.begin(), heap.end(), cmp);
    }
    for (int i = 0; i < m; ++i) if (slots[(size_t)i] == 0) return false;
    const int maxload = *std::max_element(load.begin(), load.end());
    const int NE = maxload <= 32 ? 32 : maxload <= 48 ? 48 : maxload <= 56 ? 56 : maxload <= 64 ? 64 : 0;   // doubles per lane that stay in the 256 registers of a lane
    if (!NE) return false;
    const size_t tot = (size_t)nw * NE * 64;
    Buf<double> vals(tot);
    Buf<unsigned short> cols(tot);
    std::memset(vals.data(), 0, tot * sizeof(double));
    std::memset(cols.data(), 0, tot * sizeof(unsigned short));
#pragma omp parallel for schedule(dynamic, 16)
    for (int w = 0; w < nw; ++w) {
        int base = 0;
        for (int j = 0; j < cnt[(size_t)w]; ++j) {
            const int row = wrow[(size_t)w * 8 + j];
            const int kb = A.ia[row], len = A.ia[row + 1] - kb;
            for (int e = 0; e < len; ++e) {
                const size_t at = ((size_t)w * NE + base + e / 64) * 64 + (size_t)(e % 64);
                vals[at] = A.val[kb + e];
                cols[at] = (unsigned short)(A.ja[kb + e] * 8);   // byte offset into p's LDS image (m <= 6144: < 65536)
            }
            base = wend[(size_t)w * 8 + j];
        }
    }
    bool ok = hipMalloc(&P.vals, tot * sizeof(double)) == hipSuccess && hipMalloc(&P.cols, tot * sizeof(unsigned short)) == hipSuccess &&
              hipMalloc(&P.wrow, sizeof(int) * (size_t)nw * 8) == hipSuccess && hipMalloc(&P.wend, sizeof(int) * (size_t)nw * 8) == hipSuccess &&
              hipMalloc(&P.t2, sizeof(double) * 4 * (size_t)m) == hipSuccess && hipMalloc(&P.sync, 1024) == hipSuccess;   // t2: [2][m] 16-byte records
    if (ok) ok = hipMemcpy(P.vals, vals.data(), tot * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy(P.cols, cols.data(), tot * sizeof(unsigned short), hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy(P.wrow, wrow.data(), sizeof(int) * (size_t)nw * 8, hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy(P.wend, wend.data(), sizeof(int) * (size_t)nw * 8, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) ok = hipMemset(P.t2, 0, sizeof(double) * 4 * (size_t)m) == hipSuccess;   // epoch 0 is never waited for
    if (!ok) return false;
    P.NE = NE; P.nblocks = nblocks; P.ok = true;
    return true;
}

template <int NE>
static int launch_spcg_persist(const SpcgPersistArgs& pa, size_t lds)
{
    static bool attr = false;
    if (!attr) {
        HIPCK(hipFuncSetAttribute((const void*)k_spcg_persist<NE>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024));
        attr = true;
    }
    // (fasp_hip_tune("spcg_test_hang", 1): one block short -- the others time out, the solve falls back; tests only)
    hipLaunchKernelGGL(k_spcg_persist<NE>, dim3(pa.nblocks - (g_tune.spcg_test_hang ? 1 : 0)), dim3(512), lds, g_ctx.stream, pa);
    return FASP_SUCCESS;
}

static int coarse_spcg(fasp_hip_amg* h, DevLevel& D, double tol, int prtlvl)
{
    const DevCSR& A = D.A;
    const int m = A.row;
    const int nn = (int)((unsigned)m * (unsigned)m);
    const int MaxIt = std::max(250, std::min(nn, 1000));
    if (small_coarse_ok(m, A.nnz)) {
        SpcgArgs a{};
        a.A = SmallCSR{m, A.ia, A.ja, A.val};
        a.b = D.b; a.u = D.x; a.p = h->cp; a.r = h->cr; a.t = h->ct; a.u_best = h->cbest;
        a.tol = tol; a.MaxIt = MaxIt; a.x_zero = D.x_zero ? 1 : 0; a.out = small_out_dev(); a.nnz = A.nnz;
        a.lazy = h->lazy_active ? h->d_lazy : nullptr;
        // everything in LDS when it fits: vectors 5 m doubles, matrix 12 nnz + 4 (m + 1) bytes
        const size_t lds_v = sizeof(double) * 5 * (size_t)m;
        const size_t lds_m = 12 * (size_t)A.nnz + 4 * ((size_t)m + 1);
        static bool attr = false;
        if (!attr) {
            (void)hipFuncSetAttribute((const void*)k_spcg_small<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
            (void)hipFuncSetAttribute((const void*)k_spcg_small<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
            attr = true;
        }
        // at most 128 rows: one wavefront, vectors in registers, the matrix dense in LDS (small_solvers.hip.h, k_spcg_wave)
        int LD = m; while (LD % 32 != 1) ++LD;     // row stride in doubles: conflict-free lane = row reads
        const size_t lds_w = sizeof(double) * (128 * (size_t)LD + 128);
        const bool one_wave = g_tune.small_onewave && m <= 128 && lds_w <= 148 * 1024;
        if (one_wave && g_tune.small_onewave >= 3) {   // the matrix in registers as 16 x 16 blocks, p broadcast inside the multiply-adds (k_spcg_dpp)
            const int NBK = m <= 64 ? 4 : m <= 96 ? 6 : 8, DUP = NBK == 4 ? 4 : 2, RB = NBK / DUP;
            if (!h->reg_img || h->reg_mc != -NBK) {   // the register image, once per hierarchy: group g = tid / 16 carries column block g % NBK and row blocks (g / NBK) RB ..
                const HostCSR& Ah = h->H.L.back().A;
                const int NT = 16 * NBK * DUP;   // threads of k_spcg_dpp
                std::vector<double> img((size_t)RB * 16 * NT, 0.0);
                for (int row = 0; row < m; ++row)
                    for (int k = Ah.ia[row]; k < Ah.ia[row + 1]; ++k) {
                        const int c = Ah.ja[k], cb = c >> 4, j = c & 15, rb = row >> 4, l = row & 15;
                        const int half = rb / RB, kk = rb % RB, g = half * NBK + cb;
                        img[(size_t)(kk * 16 + j) * NT + 16 * g + l] += Ah.val[k];
                    }
                if (h->reg_img) (void)hipFree(h->reg_img);
                HIPCK(hipMalloc((void**)&h->reg_img, sizeof(double) * img.size()));
                HIPCK(hipMemcpy(h->reg_img, img.data(), sizeof(double) * img.size(), hipMemcpyHostToDevice));
                h->reg_mc = -NBK;   // (negative: k_spcg_dpp's layout)
            }
            a.img = h->reg_img;
            const bool ahead = g_tune.small_onewave >= 4;   // the direction goes out before the tests of the iteration (a wavefront more: the first one multiplies nothing)
            h->coarse_kinfo[0] = 1; h->coarse_kinfo[1] = NBK; h->coarse_kinfo[2] = ahead ? 1 : 0;
            if (NBK == 4 && ahead) hipLaunchKernelGGL((k_spcg_dpp<4, 4, true>), dim3(1), dim3(320), 0, g_ctx.stream, a, LD);
            else if (NBK == 4) hipLaunchKernelGGL((k_spcg_dpp<4, 4, false>), dim3(1), dim3(256), 0, g_ctx.stream, a, LD);
            else if (NBK == 6 && ahead) hipLaunchKernelGGL((k_spcg_dpp<6, 2, true>), dim3(1), dim3(256), 0, g_ctx.stream, a, LD);
            else if (NBK == 6) hipLaunchKernelGGL((k_spcg_dpp<6, 2, false>), dim3(1), dim3(192), 0, g_ctx.stream, a, LD);
            else if (ahead) hipLaunchKernelGGL((k_spcg_dpp<8, 2, true>), dim3(1), dim3(320), 0, g_ctx.stream, a, LD);
            else hipLaunchKernelGGL((k_spcg_dpp<8, 2, false>), dim3(1), dim3(256), 0, g_ctx.stream, a, LD);
        }
        else if (one_wave && g_tune.small_onewave >= 2) {   // the matrix in registers (four wavefronts); small_onewave 1: dense in LDS, one wavefront
            const int MC = m <= 64 ? 32 : m <= 96 ? 48 : 64;
            if (!h->reg_img || h->reg_mc != MC) {   // the register image, once per hierarchy: thread t = (row t / 2, half t % 2), entry k = column 4 (k / 2) + 2 (t % 2) + k % 2
                const HostCSR& Ah = h->H.L.back().A;
                std::vector<double> img((size_t)MC * SPCG_REG_NT, 0.0);
                for (int row = 0; row < m; ++row)
                    for (int k = Ah.ia[row]; k < Ah.ia[row + 1]; ++k) {
                        const int c = Ah.ja[k], hh = (c >> 1) & 1, kk = 2 * (c >> 2) + (c & 1);
                        if (kk < MC) img[(size_t)kk * SPCG_REG_NT + 2 * row + hh] += Ah.val[k];
                    }
                if (h->reg_img) (void)hipFree(h->reg_img);
                HIPCK(hipMalloc((void**)&h->reg_img, sizeof(double) * img.size()));
                HIPCK(hipMemcpy(h->reg_img, img.data(), sizeof(double) * img.size(), hipMemcpyHostToDevice));
                h->reg_mc = MC;
            }
            a.img = h->reg_img;
            static bool attr_r = false;
            if (!attr_r) {
                (void)hipFuncSetAttribute((const void*)k_spcg_reg<32>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
                (void)hipFuncSetAttribute((const void*)k_spcg_reg<48>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
                (void)hipFuncSetAttribute((const void*)k_spcg_reg<64>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
                attr_r = true;
            }
            const size_t lds_r = sizeof(double) * (2 * (size_t)MC + 4);
            h->coarse_kinfo[0] = 2; h->coarse_kinfo[1] = MC; h->coarse_kinfo[2] = 0;
            if (m <= 64) hipLaunchKernelGGL(k_spcg_reg<32>, dim3(1), dim3(SPCG_REG_NT), lds_r, g_ctx.stream, a, LD);
            else if (m <= 96) hipLaunchKernelGGL(k_spcg_reg<48>, dim3(1), dim3(SPCG_REG_NT), lds_r, g_ctx.stream, a, LD);
            else hipLaunchKernelGGL(k_spcg_reg<64>, dim3(1), dim3(SPCG_REG_NT), lds_r, g_ctx.stream, a, LD);
        }
        else if (one_wave) {
            static bool attr_w = false;
            if (!attr_w) { (void)hipFuncSetAttribute((const void*)k_spcg_wave, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024); attr_w = true; }
            hipLaunchKernelGGL(k_spcg_wave, dim3(1), dim3(64), lds_w, g_ctx.stream, a, LD);
            h->coarse_kinfo[0] = 3; h->coarse_kinfo[1] = 0; h->coarse_kinfo[2] = 0;
        }
        else if (g_tune.small_lds && lds_v + lds_m <= 148 * 1024) {
            hipLaunchKernelGGL((k_spcg_small<true, true>), dim3(1), dim3(SMALL_BLOCK), lds_v + lds_m, g_ctx.stream, a);
            h->coarse_kinfo[0] = 4; h->coarse_kinfo[1] = 2; h->coarse_kinfo[2] = 0;
        }
        else if (g_tune.small_lds && lds_v <= 148 * 1024) {
            hipLaunchKernelGGL((k_spcg_small<true, false>), dim3(1), dim3(SMALL_BLOCK), lds_v, g_ctx.stream, a);
            h->coarse_kinfo[0] = 4; h->coarse_kinfo[1] = 1; h->coarse_kinfo[2] = 0;
        }
        else {
            hipLaunchKernelGGL((k_spcg_small<false, false>), dim3(1), dim3(SMALL_BLOCK), 0, g_ctx.stream, a);
            h->coarse_kinfo[0] = 4; h->coarse_kinfo[1] = 0; h->coarse_kinfo[2] = 0;
        }
        D.x_zero = false;
        if (a.lazy) return FASP_SUCCESS;   // the verdict is read once per application of the preconditioner (precond_amg)
        SmallOut o;
        if (small_out_fetch(o) < 0) return ERROR_MISC;
        h->coarse_iters += o.iters;
        if (std::getenv("FASP_HIP_DEBUG_COARSE")) std::printf("[coarse small] status %d iters %d relres %.6e\n", o.status, o.iters, o.relres);
        return o.status;
    }
    const double maxdiff = tol * STAG_RATIO;
    int iter = 0, stag = 1, more_step = 1, iter_best = 0;
    double absres0 = BIGREAL, absres = BIGREAL, relres = BIGREAL, normu = BIGREAL, normr0 = BIGREAL;
    double reldiff, factor, alpha = 0.0, beta, temp1, temp2, absres_best = BIGREAL;
    double *p = h->cp, *r = h->cr, *t = h->ct, *u_best = h->cbest, *u = D.x;
    const double* b = D.b;
    double red[8];
    hipStream_t s = g_ctx.stream;
    (void)prtlvl;

    // one launch per iteration (k_spcg_fused) when p fits the LDS of a CU and the level is stored as plain CSR
    // (p in LDS: 8 m bytes of dynamic LDS next to the reduction scratch, within the 64 KB a kernel gets without opting in)
    const bool fused = g_tune.spcg_fused && m <= 8000 && A.val && A.ja && !A.code && !A.pat;
    // one launch per coarse SOLVE with the matrix resident in the register files (k_spcg_persist): needs the chip to
    // itself (every block resident at once) -- not when several validation ranks share a device
    bool persist = fused && g_tune.spcg_persist && !g_persist_disabled && !comm_shares_devices() &&
                   (size_t)m * 24 <= 150 * 1024 && build_persist_plan(h, (int)(&D - &h->L[0]));
    if (!h->spcg_state) HIPCK(hipMalloc(&h->spcg_state, sizeof(SpcgState)));
    if (fused) {  // the start of the solve on the device too: no host round trip before the first batch
        if (!D.x_zero) d_resid(A, u, b, r);
        SpcgInitArgs ia{};
        ia.m = m; ia.x_zero = D.x_zero ? 1 : 0; ia.MaxIt = MaxIt; ia.tol = tol; ia.maxdiff = maxdiff;
        ia.b = b; ia.u = u; ia.r = r; ia.p = p; ia.u_best = u_best; ia.st = h->spcg_state;
        hipLaunchKernelGGL(k_spcg_init, dim3(1), dim3(512), 0, s, ia);
        D.x_zero = false;
        goto ITERATE;
    }

    // u_best starts as zeros (calloc'ed work array, KrySPcg.c:88)
    HIPCK(hipMemsetAsync(u_best, 0, sizeof(double) * m, s));

    // r = b - A u  (u == 0 on entry from the cycle: r = b, no matrix pass)
    if (D.x_zero) {
        HIPCK(hipMemcpyAsync(r, b, sizeof(double) * m, hipMemcpyDeviceToDevice, s));
        HIPCK(hipMemsetAsync(u, 0, sizeof(double) * m, s));
        D.x_zero = false;
    } else {
        d_resid(A, u, b, r);
    }
    if (d_dot(m, r, r, red) < 0) return ERROR_MISC;  // z = r: (r,r) serves both ||r|| and (z,r)
    absres0 = std::sqrt(red[0]);
    normr0  = std::max(SMALLREAL, absres0);
    relres  = absres0 / normr0;
    if (relres < tol) goto FINISHED;
    HIPCK(hipMemcpyAsync(p, r, sizeof(double) * m, hipMemcpyDeviceToDevice, s));
    temp1 = red[0];

ITERATE:
    {
        // Device-resident iteration state; the host queues `batch` iterations (SpMV + step kernel
        // each) without waiting and synchronises once per batch.  When one of the reference's
        // tests fires, k_spcg_step raises `stop`, the launches queued behind it return at once,
        // and the branch is replayed here from the recorded scalars (KrySPcg.c:172-330).
        // the first batch is sized by the previous solve on this level (the count hardly moves from cycle to
        // cycle): normally one synchronisation per solve; 1 + iterations launches, the first one has no step
        int batch = std::max(1, std::min(g_tune.spcg_batch > 0 ? g_tune.spcg_batch : 8, 64));
        const int batch_next = batch;
        if (fused && h->spcg_last_iters > 0) batch = std::max(4, std::min(h->spcg_last_iters + 1, 96));
        SpcgState S{};
        if (!fused) {
            S.temp1 = temp1; S.temp1_prev = temp1; S.absres_best = absres_best; S.normr0 = normr0; S.tol = tol;
            S.maxdiff = maxdiff; S.iter = 0; S.iter_best = 0; S.stag = stag; S.MaxIt = MaxIt; S.stop = SPCG_RUN;
            S.absres = absres; S.relres = relres; S.alpha = 0.0;  // values before the first iteration
            HIPCK(hipMemcpyAsync(h->spcg_state, &S, sizeof(S), hipMemcpyHostToDevice, s));
        }
        double *R[2] = {r, nullptr}, *P[2] = {p, nullptr}, *T[2] = {t, nullptr};
        SpcgBc* bc = nullptr;
        int  cur = 0;        // parity of the buffers that hold r and p
        bool first = true;   // next launch starts a batch sequence: SpMV only
        if (fused) {
            if (!h->spcg_fused_buf) HIPCK(hipMalloc(&h->spcg_fused_buf, sizeof(double) * (3 * (size_t)m + 4)));
            R[1] = h->spcg_fused_buf; P[1] = R[1] + m; T[1] = P[1] + m;
            bc = reinterpret_cast<SpcgBc*>(T[1] + m);
        }
        for (;;) {
            if (persist) {
                auto& PP = h->persist;
                // epochs of this launch: (launch number) << 11 | iteration + 1 (max_steps <= 1002 < 2048); on wrap-around the
                // records are cleared, so an old record can never carry a current epoch
                PP.launches = (PP.launches + 1u) & 0x1fffffu;
                if (PP.launches == 0u) { HIPCK(hipMemsetAsync(PP.t2, 0, sizeof(double) * 4 * (size_t)m, s)); PP.launches = 1u; }
                SpcgPersistArgs pa{};
                pa.epoch0 = PP.launches << 11;
                pa.m = m; pa.max_steps = MaxIt + 2; pa.nblocks = PP.nblocks; pa.st = h->spcg_state;
                pa.r = r; pa.p = p; pa.u = u; pa.u_best = u_best; pa.t2 = PP.t2; pa.sync = PP.sync;
                pa.vals = PP.vals; pa.cols = PP.cols; pa.wrow = PP.wrow; pa.wend = PP.wend;
                HIPCK(hipMemsetAsync(PP.sync, 0, 1024, s));
                // p, r, t in every block; a fourth vector (u, used by block 0) when the CU's 160 KiB allow it
                pa.u_lds = (sizeof(double) * 4 * (size_t)m + 1024 <= 160 * 1024) ? 1 : 0;
                const size_t lds = sizeof(double) * (pa.u_lds ? 4 : 3) * (size_t)m;
                int lst;
                if (PP.NE == 32) lst = launch_spcg_persist<32>(pa, lds);
                else if (PP.NE == 48) lst = launch_spcg_persist<48>(pa, lds);
                else if (PP.NE == 56) lst = launch_spcg_persist<56>(pa, lds);
                else lst = launch_spcg_persist<64>(pa, lds);
                if (lst < 0) return lst;
                h->coarse_kinfo[0] = 6; h->coarse_kinfo[1] = PP.NE; h->coarse_kinfo[2] = pa.u_lds;
            }
            for (int q = 0; q < batch && fused && !persist; ++q) {
                SpcgFusedArgs fa{};
                fa.m = m; fa.first = first ? 1 : 0; fa.in = cur; fa.st = h->spcg_state; fa.bc = bc;
                fa.ia = A.ia; fa.ja = A.ja; fa.ja16 = A.jbase ? nullptr : A.ja16; fa.val = A.val;
                for (int k = 0; k < 2; ++k) { fa.r[k] = R[k]; fa.p[k] = P[k]; fa.t[k] = T[k]; }
                fa.u = u; fa.u_best = u_best;
                // two 512-thread blocks per CU are resident (126 VGPRs): one wave of blocks, block 0 included
                const int cap = g_tune.spcg_grid > 0 ? g_tune.spcg_grid : 2 * g_ctx.num_cu - 1;
                const dim3 grid(1 + std::max(1, std::min((m + 7) / 8, cap)));
                const size_t lds = sizeof(double) * (size_t)m;
                if (m <= 512 * 4) hipLaunchKernelGGL(k_spcg_fused<4>, grid, dim3(512), lds, s, fa);
                else if (m <= 512 * 10) hipLaunchKernelGGL(k_spcg_fused<10>, grid, dim3(512), lds, s, fa);
                else hipLaunchKernelGGL(k_spcg_fused<16>, grid, dim3(512), lds, s, fa);
                h->coarse_kinfo[0] = 5; h->coarse_kinfo[1] = m <= 512 * 4 ? 4 : m <= 512 * 10 ? 10 : 16; h->coarse_kinfo[2] = 0;
                cur ^= 1; first = false;
            }
            for (int q = 0; q < batch && !fused; ++q) {
                CsrArgs a{}; a.x = p; a.y = t; a.dotv = p; a.partials = g_ctx.d_partials; a.stop = &h->spcg_state->stop;
                SpcgStepArgs sa{};
                sa.m = m; sa.st = h->spcg_state; sa.t = t; sa.p = p; sa.u = u; sa.r = r; sa.u_best = u_best;
                sa.ntp = launch_csr<OP_MXV_DOT>(A, a);
                sa.tp_partials = g_ctx.d_partials;
                if (m <= 512 * 4) hipLaunchKernelGGL(k_spcg_step_reg<4>, dim3(1), dim3(512), 0, s, sa);
                else if (m <= 512 * 10) hipLaunchKernelGGL(k_spcg_step_reg<10>, dim3(1), dim3(512), 0, s, sa);
                else hipLaunchKernelGGL(k_spcg_step, dim3(1), dim3(SMALL_BLOCK), 0, s, sa);
                h->coarse_kinfo[0] = 7; h->coarse_kinfo[1] = m <= 512 * 4 ? 4 : m <= 512 * 10 ? 10 : 0; h->coarse_kinfo[2] = 0;
            }
            // The persistent kernel normally ends because the recurrence's residual met the tolerance, and the reference then forms the TRUE
            // residual (Check III, KrySPcg.c:258-275): a second wait of the host per coarse solve.  It is queued here, behind the kernel,
            // into the scratch vector t -- the same kernels on the same u -- and its norm travels with the state: one wait (round 5).
            bool spec_rr = false;
            if (persist && g_tune.spcg_spec) {
                d_resid(A, u, b, t);
                if (d_dot_to(m, t, t, 14, false) < 0) return ERROR_MISC;
                spec_rr = true;
            }
            HIPCK(hipMemcpyAsync(g_ctx.h_part, h->spcg_state, sizeof(SpcgState), hipMemcpyDeviceToHost, s));
            static_assert(sizeof(SpcgState) % 8 == 0 && sizeof(SpcgState) + 24 <= sizeof(double) * 64, "the error word and the speculative norm travel behind the state");
            if (persist) HIPCK(hipMemcpyAsync(reinterpret_cast<char*>(g_ctx.h_part) + sizeof(SpcgState), h->persist.sync, 16, hipMemcpyDeviceToHost, s));
            if (spec_rr) HIPCK(hipMemcpyAsync(reinterpret_cast<char*>(g_ctx.h_part) + sizeof(SpcgState) + 16, g_ctx.d_red + 14, 8, hipMemcpyDeviceToHost, s));
            HIPCK(hipStreamSynchronize(s));
            std::memcpy(&S, g_ctx.h_part, sizeof(S));
            double spec_val = 0.0;
            if (spec_rr) std::memcpy(&spec_val, reinterpret_cast<char*>(g_ctx.h_part) + sizeof(SpcgState) + 16, 8);
            if (persist) {   // a block that gave up waiting raised the error word -- also when block 0 itself never ran
                unsigned ew[4];
                std::memcpy(ew, reinterpret_cast<char*>(g_ctx.h_part) + sizeof(SpcgState), 16);
                if (ew[3] != 0u && S.stop == SPCG_RUN) S.stop = SPCG_HANG;
            }
            iter = S.iter; absres_best = S.absres_best; iter_best = S.iter_best;
            batch = batch_next;
            if (fused) {
                normr0 = S.normr0;
                if (S.stop == SPCG_ZERO_RHS) { relres = S.relres; goto FINISHED; }  // KrySPcg.c:135
            }
#ifdef SPCG_PERSIST_STAMPS
            if (persist) {
                unsigned dbg[64];
                (void)hipMemcpy(dbg, h->persist.sync, sizeof(dbg), hipMemcpyDeviceToHost);
                std::printf("[persist stamps, 10 ns ticks, %d steps] lead:", S.iter);
                for (int q = 0; q < 8; ++q) std::printf(" %u", dbg[32 + q]);
                std::printf(" | block 1:");
                for (int q = 0; q < 8; ++q) std::printf(" %u", dbg[40 + q]);
                std::printf("   (spmv meet(second group of records + verdict) read step(tail) pass1-2 pass3 first-group-of-records(block 1) poll-rounds)\n");
            }
#endif
            if (S.stop == SPCG_HANG) {
                // A block of the persistent kernel was not resident (another process on this GPU, a concurrently resident
                // kernel): a benign condition, not a failed solve.  r, p, u and the scalars are those of the last finished
                // iteration -- this coarse solve goes on through the per-iteration kernels, and so do all later ones.
                std::fprintf(stderr, "### WARNING: fasp_hip: the persistent coarse CG kernel timed out waiting for a block that was not "
                                     "resident (is another process using this GPU?); continuing with the per-iteration kernels\n");
                g_persist_disabled = true;
                persist = false;
                S.stop = SPCG_RUN;
                HIPCK(hipMemcpyAsync(h->spcg_state, &S, sizeof(S), hipMemcpyHostToDevice, s));
                HIPCK(hipStreamSynchronize(s));  // S lives on this stack frame
                cur = 0; first = true;
                continue;
            }
            if (S.stop == SPCG_RUN) continue;
            if (fused && !persist) { cur = S.pad; r = R[cur]; p = P[cur]; first = true; }  // where the last finished step left r and p
            // a test fired in iteration S.iter: finish that iteration as the reference does
            temp2 = S.tp; temp1 = S.temp1_prev;
            red[0] = S.rr; red[1] = S.uu; red[2] = S.pp; red[3] = S.maxu; red[4] = S.nan;
            // (on a breakdown the step kernel leaves absres / relres of the PREVIOUS iteration in the state,
            // which is what the reference's variables hold when it jumps to RESTORE_BESTSOL, KrySPcg.c:176)
            alpha = S.alpha; absres = S.absres; relres = S.relres;
            if (S.stop == SPCG_DIV0) goto RESTORE_BESTSOL;
            factor = absres / absres0; (void)factor; (void)alpha;
            if (S.stop == SPCG_NAN) { absres = BIGREAL; goto RESTORE_BESTSOL; }
            if (S.stop == SPCG_SOLSTAG) { iter = ERROR_SOLVER_SOLSTAG; break; }  // Check I
            if (S.stop == SPCG_MAXIT) { iter = MaxIt + 1; break; }
            normu = std::sqrt(red[1]);
            reldiff = std::fabs(S.alpha) * std::sqrt(red[2]) / normu;
            if ((stag <= MAX_STAG) & (reldiff < maxdiff)) {  // Check II
                spec_rr = false;   // (what follows works on r itself)
                d_resid(A, u, b, r);
                if (d_dot(m, r, r, red) < 0) return ERROR_MISC;
                absres = std::sqrt(red[0]);
                relres = absres / normr0;
                if (relres < tol) break;
                if (stag >= MAX_STAG) { iter = ERROR_SOLVER_STAG; break; }
                HIPCK(hipMemsetAsync(p, 0, sizeof(double) * m, s));
                ++stag;
            }
            if (relres < tol) {  // Check III: true residual
                if (spec_rr && S.stop != SPCG_HANG) red[0] = spec_val;   // formed behind the kernel, in t
                else {
                    spec_rr = false;
                    d_resid(A, u, b, r);
                    if (d_dot(m, r, r, red) < 0) return ERROR_MISC;
                }
                absres = std::sqrt(red[0]);
                relres = absres / normr0;
                if (relres < tol) break;
                if (spec_rr) HIPCK(hipMemcpyAsync(r, t, sizeof(double) * m, hipMemcpyDeviceToDevice, s));   // the solve goes on from the true residual
                if (more_step >= MAX_RESTART) { iter = ERROR_SOLVER_TOLSMALL; break; }
                HIPCK(hipMemsetAsync(p, 0, sizeof(double) * m, s));
                ++more_step;
            }
            // every branch that gets here restarted: p was zeroed, so p = z + beta p = r
            absres0 = absres;
            temp2 = red[0];
            beta = temp2 / temp1;
            temp1 = temp2;
            d_axpby(m, 1.0, r, beta, p);
            S.temp1 = temp1; S.temp1_prev = temp1; S.stag = stag; S.stop = SPCG_RUN;
            HIPCK(hipMemcpyAsync(h->spcg_state, &S, sizeof(S), hipMemcpyHostToDevice, s));
            HIPCK(hipStreamSynchronize(s));  // S lives on this stack frame
        }
    }

RESTORE_BESTSOL:
    if (iter != iter_best) {
        d_resid(A, u_best, b, r);
        if (d_dot(m, r, r, red) < 0) return ERROR_MISC;
        absres_best = std::sqrt(red[0]);
        if (absres > absres_best + maxdiff || std::isnan(absres)) {
            HIPCK(hipMemcpyAsync(u, u_best, sizeof(double) * m, hipMemcpyDeviceToDevice, s));
            relres = absres_best / normr0;
        }
    }
FINISHED:
    if (std::getenv("FASP_HIP_DEBUG_COARSE")) std::printf("[coarse batched] iter %d relres %.6e absres %.6e best %d\n", iter, relres, absres, iter_best);
    if (iter > 0) { h->coarse_iters += iter; h->spcg_last_iters = iter; }
    if (iter > MaxIt) return ERROR_SOLVER_MAXIT;
    return iter;
}

