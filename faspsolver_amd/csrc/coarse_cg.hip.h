// coarse_cg.hip.h -- coarsest level: safe CG (single-workgroup kernel or batched device-resident iteration).
// Part of the single translation unit solver.hip (included there, in this order; not a stand-alone header).

// ---------------------------------------------------------------------------
// coarsest level: safe-net CG without preconditioner (KrySPcg.c:60, called from
// PreMGUtil.inl:47 with StopType = STOP_REL_RES, maxit = MAX(250, MIN(n*n, 1000))).
//
// plan_coarse_spcg decides ONCE which kernel family solves the level and how it is launched (a pure host function:
// fasp_hip_coarse_plan shows it to the CPU); launch_spcg_small / launch_spcg_fused / launch_spcg_step / launch_spcg_persist
// execute that plan; coarse_spcg drives the solve over named steps; mgcycle and coarse_solve read the same plan.
// ---------------------------------------------------------------------------
static int coarse_maxit(int m) { return std::max(250, std::min((int)((unsigned)m * (unsigned)m), 1000)); }

// FASP_HIP_SMALL_COARSE=0 (read once): no single-workgroup coarse solvers (small_solvers.hip.h), scalar and block path
static bool small_coarse_enabled()
{
    static int enabled = -1;
    if (enabled < 0) {
        const char* e = std::getenv("FASP_HIP_SMALL_COARSE");
        enabled = (e && std::atoi(e) == 0) ? 0 : 1;
    }
    return enabled != 0;
}
static SmallOut* small_out_dev() { return reinterpret_cast<SmallOut*>(g_ctx.d_partials2); }
static int small_out_fetch(SmallOut& o)
{
    HIPCK(hipMemcpyAsync(g_ctx.h_part, g_ctx.d_partials2, sizeof(SmallOut), hipMemcpyDeviceToHost, g_ctx.stream));
    HIPCK(hipStreamSynchronize(g_ctx.stream));
    std::memcpy(&o, g_ctx.h_part, sizeof(SmallOut));
    return 0;
}

constexpr int COARSE_LDS_FIT = 148 * 1024;   // dynamic LDS a single-workgroup coarse CG asks for at most
constexpr int COARSE_LDS_OPT = 150 * 1024;   // ... and what its kernels are opted into
constexpr int CU_LDS = 160 * 1024;

// What the plan reads.  ia: the host row pointer of the level (nullptr: the persistent form is refused).
struct CoarseTraits {
    int m = 0; long long nnz = 0; const int* ia = nullptr;
    bool plain_csr = false;      // the device operator is usable as plain CSR (A.val && A.ja && !A.code && !A.pat)
    int  num_cu = 0;
    bool shared_device = false;  // comm_shares_devices(): k_spcg_persist needs the chip to itself
    bool persist_off = false;    // g_persist_disabled, or the level's deal could not be uploaded
    bool small_coarse = true;    // small_coarse_enabled()
};
// (struct CoarsePlan, what the decision returns: hierarchy.hip.h, next to the handle that keeps it)
constexpr int spcg_inst(int family, int p1, int p2 = 0) { return family * 1000 + p1 * 10 + p2; }
static int spcg_inst(const CoarsePlan& p) { return spcg_inst(p.family, p.p1, p.family == 6 ? 0 : p.p2); }

// k_spcg_persist (small_solvers.hip.h): deal the rows of the coarsest matrix to the waves of the chip -- whole rows, longest first, always to
// the least loaded wave, at most 8 rows per wave.  NE = doubles per lane (slots of 64 entries per wave, rounded up to 32 / 48 / 56 / 64: what
// stays in the 256 registers of a lane); 0: the level does not fit the scheme.
struct PersistDeal { int NE = 0, nw = 0; std::vector<int> wrow, wend; };
static PersistDeal deal_persist(int m, long long nnz, const int* ia, int num_cu)
{
    PersistDeal d;
    const int nw = (num_cu - 1) * 8;   // 512-thread blocks, block 0 owns no rows
    if (!ia || m < 1 || m > 6144 || nw < 8 || nnz <= 0) return d;
    std::vector<int> order((size_t)m), slots((size_t)m);
    for (int i = 0; i < m; ++i) { order[(size_t)i] = i; slots[(size_t)i] = (ia[i + 1] - ia[i] + 63) / 64; }
    for (int i = 0; i < m; ++i) if (slots[(size_t)i] == 0) return d;   // empty row: t_i = 0 is written by nobody -> not representable here
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return slots[(size_t)x] > slots[(size_t)y]; });
    std::vector<int> load((size_t)nw, 0), cnt((size_t)nw, 0), wrow((size_t)nw * 8, -1), wend((size_t)nw * 8, 0);
    // least-loaded wave first: a binary heap of (load, wave)
    std::vector<std::pair<int, int>> heap;
    for (int w = 0; w < nw; ++w) heap.emplace_back(0, w);
    auto cmp = [](const std::pair<int, int>& x, const std::pair<int, int>& y) { return x > y; };
    std::make_heap(heap.begin(), heap.end(), cmp);
    for (int i : order) {
        std::pop_heap(heap.begin(), heap.end(), cmp);
        const int w = heap.back().second;
        if (cnt[(size_t)w] >= 8) return d;
        load[(size_t)w] += slots[(size_t)i];
        wrow[(size_t)w * 8 + cnt[(size_t)w]] = i;
        wend[(size_t)w * 8 + cnt[(size_t)w]] = load[(size_t)w];
        cnt[(size_t)w]++;
        heap.back() = std::make_pair(load[(size_t)w], w);
        std::push_heap(heap.begin(), heap.end(), cmp);
    }
    const int maxload = *std::max_element(load.begin(), load.end());
    d.NE = maxload <= 32 ? 32 : maxload <= 48 ? 48 : maxload <= 56 ? 56 : maxload <= 64 ? 64 : 0;
    if (d.NE) { d.nw = nw; d.wrow = std::move(wrow); d.wend = std::move(wend); }
    return d;
}

// The decision.  deal (may be nullptr): receives the persistent kernel's deal when the plan is family 6.
static CoarsePlan plan_coarse_spcg(const CoarseTraits& c, const Tuning& tune, PersistDeal* deal)
{
    CoarsePlan p;
    const int m = c.m;
    p.MaxIt = coarse_maxit(m);
    p.blocks = 1;
    if (c.small_coarse && m <= 4096 && c.nnz <= 131072) {   // the level fits one CU's caches: one launch, one wait per solve
        p.lazy = 1;
        // at most 128 rows: the vectors in registers, the matrix in registers (k_spcg_dpp, k_spcg_reg) or dense in LDS (k_spcg_wave)
        int LD = m; while (LD % 32 != 1) ++LD;
        const size_t lds_w = sizeof(double) * (128 * (size_t)LD + 128);
        if (tune.small_onewave && m <= 128 && lds_w <= (size_t)COARSE_LDS_FIT) {
            p.LD = LD;
            if (tune.small_onewave >= 3) {   // 16 x 16 blocks, p broadcast inside the multiply-adds; >= 4: the direction goes out before the tests of the iteration (a wavefront more)
                const int NBK = m <= 64 ? 4 : m <= 96 ? 6 : 8, DUP = NBK == 4 ? 4 : 2;
                p.family = 1; p.p1 = NBK; p.p2 = tune.small_onewave >= 4 ? 1 : 0;
                p.threads = 16 * NBK * DUP + 64 * p.p2;
            } else if (tune.small_onewave >= 2) {   // four wavefronts, p broadcast from LDS
                const int MC = m <= 64 ? 32 : m <= 96 ? 48 : 64;
                p.family = 2; p.p1 = MC; p.threads = SPCG_REG_NT; p.lds = (int)(sizeof(double) * (2 * (size_t)MC + 4));
            } else {
                p.family = 3; p.threads = 64; p.lds = (int)lds_w;
            }
            return p;
        }
        // everything in LDS when it fits: vectors 5 m doubles, matrix 12 nnz + 4 (m + 1) bytes
        const size_t lds_v = sizeof(double) * 5 * (size_t)m;
        const size_t lds_m = 12 * (size_t)c.nnz + 4 * ((size_t)m + 1);
        p.family = 4; p.threads = SMALL_BLOCK;
        if (tune.small_lds && lds_v + lds_m <= (size_t)COARSE_LDS_FIT) { p.p1 = 2; p.lds = (int)(lds_v + lds_m); }
        else if (tune.small_lds && lds_v <= (size_t)COARSE_LDS_FIT) { p.p1 = 1; p.lds = (int)lds_v; }
        return p;
    }
    p.batch = std::max(1, std::min(tune.spcg_batch > 0 ? tune.spcg_batch : 8, 64));
    const int E = m <= 512 * 4 ? 4 : m <= 512 * 10 ? 10 : 0;   // elements per thread of the 512-thread vector passes (0: beyond them)
    // one launch per iteration (k_spcg_fused) when p fits the LDS of a CU and the level is stored as plain CSR
    // (p in LDS: 8 m bytes of dynamic LDS next to the reduction scratch, within the 64 KB a kernel gets without opting in)
    const bool fused = tune.spcg_fused && m <= 8000 && c.plain_csr;
    if (!fused) {
        p.family = 7; p.p1 = E; p.threads = E ? 512 : SMALL_BLOCK;
        return p;
    }
    p.dev_start = 1;   // no host round trip before the first batch
    p.threads = 512;
    // one launch per coarse SOLVE with the matrix resident in the register files (k_spcg_persist): needs the chip to
    // itself (every block resident at once) -- not when several validation ranks share a device
    if (tune.spcg_persist && !c.persist_off && !c.shared_device && (size_t)m * 24 <= 150 * 1024) {
        PersistDeal d = deal_persist(m, c.nnz, c.ia, c.num_cu);
        if (d.NE) {
            // p, r, t in every block; a fourth vector (u, used by block 0) when the CU's 160 KiB allow it
            p.family = 6; p.p1 = d.NE; p.p2 = (sizeof(double) * 4 * (size_t)m + 1024 <= (size_t)CU_LDS) ? 1 : 0;
            p.blocks = c.num_cu; p.lds = (int)(sizeof(double) * (p.p2 ? 4 : 3) * (size_t)m);
            if (deal) *deal = std::move(d);
            return p;
        }
    }
    // two 512-thread blocks per CU are resident (126 VGPRs): one wave of blocks, block 0 included
    const int cap = tune.spcg_grid > 0 ? tune.spcg_grid : 2 * c.num_cu - 1;
    p.family = 5; p.p1 = E ? E : 16; p.blocks = 1 + std::max(1, std::min((m + 7) / 8, cap)); p.lds = (int)(sizeof(double) * (size_t)m);
    return p;
}

// fasp_hip_tune and the fallback from the persistent kernel bump the generation: the plan kept on a handle is remade
static unsigned g_coarse_gen = 1;
static bool     g_persist_disabled = false;

// the deal on the device, entries laid out slot by slot (64 lanes x NE slots per wave) for the registers; once per hierarchy
static bool upload_persist(fasp_hip_amg* h, const HostCSR& A, const PersistDeal& d)
{
    auto& P = h->persist;
    if (P.NE) return P.NE == d.NE;
    const int m = A.row, nw = d.nw, NE = d.NE;
    const size_t tot = (size_t)nw * NE * 64;
    Buf<double> vals(tot);
    Buf<unsigned short> cols(tot);
    std::memset(vals.data(), 0, tot * sizeof(double));
    std::memset(cols.data(), 0, tot * sizeof(unsigned short));
#pragma omp parallel for schedule(dynamic, 16)
    for (int w = 0; w < nw; ++w) {
        int base = 0;
        for (int j = 0; j < 8 && d.wrow[(size_t)w * 8 + j] >= 0; ++j) {
            const int row = d.wrow[(size_t)w * 8 + j];
            const int kb = A.ia[row], len = A.ia[row + 1] - kb;
            for (int e = 0; e < len; ++e) {
                const size_t at = ((size_t)w * NE + base + e / 64) * 64 + (size_t)(e % 64);
                vals[at] = A.val[kb + e];
                cols[at] = (unsigned short)(A.ja[kb + e] * 8);   // byte offset into p's LDS image (m <= 6144: < 65536)
            }
            base = d.wend[(size_t)w * 8 + j];
        }
    }
    bool ok = hipMalloc(&P.vals, tot * sizeof(double)) == hipSuccess && hipMalloc(&P.cols, tot * sizeof(unsigned short)) == hipSuccess &&
              hipMalloc(&P.wrow, sizeof(int) * (size_t)nw * 8) == hipSuccess && hipMalloc(&P.wend, sizeof(int) * (size_t)nw * 8) == hipSuccess &&
              hipMalloc(&P.t2, sizeof(double) * 4 * (size_t)m) == hipSuccess && hipMalloc(&P.sync, 1024) == hipSuccess;   // t2: [2][m] 16-byte records
    if (ok) ok = hipMemcpy(P.vals, vals.data(), tot * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy(P.cols, cols.data(), tot * sizeof(unsigned short), hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy(P.wrow, d.wrow.data(), sizeof(int) * (size_t)nw * 8, hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy(P.wend, d.wend.data(), sizeof(int) * (size_t)nw * 8, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) ok = hipMemset(P.t2, 0, sizeof(double) * 4 * (size_t)m) == hipSuccess;   // epoch 0 is never waited for
    if (ok) P.NE = NE;
    return ok;
}

// the plan of level D's coarse solve, kept on the handle
static const CoarsePlan& coarse_plan(fasp_hip_amg* h, const DevLevel& D)
{
    if (h->cplan_gen == g_coarse_gen) return h->cplan;
    const DevCSR& A = D.A;
    const size_t level = (size_t)(&D - &h->L[0]);
    const HostCSR* Ah = level < h->H.L.size() ? &h->H.L[level].A : nullptr;
    CoarseTraits c;
    c.m = A.row; c.nnz = A.nnz;
    c.ia = Ah && Ah->row == A.row && Ah->row == Ah->col && Ah->nnz > 0 ? Ah->ia.data() : nullptr;
    c.plain_csr = A.val && A.ja && !A.code && !A.pat;
    c.num_cu = g_ctx.num_cu;
    c.shared_device = comm_shares_devices();
    c.persist_off = g_persist_disabled || h->persist.failed;
    c.small_coarse = small_coarse_enabled();
    PersistDeal deal;
    h->cplan = plan_coarse_spcg(c, g_tune, &deal);
    if (h->cplan.family == 6 && !upload_persist(h, *Ah, deal)) {   // (no device memory for it: refused for good)
        h->persist.failed = c.persist_off = true;
        h->cplan = plan_coarse_spcg(c, g_tune, nullptr);
    }
    h->cplan_gen = g_coarse_gen;
    return h->cplan;
}

// coarse_kinfo[0..2] (fasp_hip_coarse_kernel_info): the plan whose kernels were just queued
static void report_coarse_plan(int* kinfo, int family, int p1, int p2) { kinfo[0] = family; kinfo[1] = p1; kinfo[2] = p2; }

// a kernel is opted into large dynamic LDS on its first launch
template <auto K>
static hipError_t allow_lds(int bytes)
{
    static hipError_t st = hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return st;
}

// ---------------------------------------------------------------------------
// the register images of the coarsest matrix (k_spcg_dpp, k_spcg_reg), cached on the handle by (family, parameter)
// ---------------------------------------------------------------------------
// k_spcg_dpp: group g = tid / 16 carries column block g % NBK and row blocks (g / NBK) RB ..
static std::vector<double> reg_image_dpp(const HostCSR& Ah, int m, int NBK)
{
    const int DUP = NBK == 4 ? 4 : 2, RB = NBK / DUP, NT = 16 * NBK * DUP;   // NT: threads of k_spcg_dpp that multiply
    std::vector<double> img((size_t)RB * 16 * NT, 0.0);
    for (int row = 0; row < m; ++row)
        for (int k = Ah.ia[row]; k < Ah.ia[row + 1]; ++k) {
            const int c = Ah.ja[k], cb = c >> 4, j = c & 15, rb = row >> 4, l = row & 15;
            const int half = rb / RB, kk = rb % RB, g = half * NBK + cb;
            img[(size_t)(kk * 16 + j) * NT + 16 * g + l] += Ah.val[k];
        }
    return img;
}
// k_spcg_reg: thread t = (row t / 2, half t % 2), entry k = column 4 (k / 2) + 2 (t % 2) + k % 2
static std::vector<double> reg_image_reg(const HostCSR& Ah, int m, int MC)
{
    std::vector<double> img((size_t)MC * SPCG_REG_NT, 0.0);
    for (int row = 0; row < m; ++row)
        for (int k = Ah.ia[row]; k < Ah.ia[row + 1]; ++k) {
            const int c = Ah.ja[k], hh = (c >> 1) & 1, kk = 2 * (c >> 2) + (c & 1);
            if (kk < MC) img[(size_t)kk * SPCG_REG_NT + 2 * row + hh] += Ah.val[k];
        }
    return img;
}
static int reg_image(fasp_hip_amg* h, const CoarsePlan& plan, int m)
{
    if (h->reg_img && h->reg_img_family == plan.family && h->reg_img_par == plan.p1) return FASP_SUCCESS;
    const HostCSR& Ah = h->H.L.back().A;
    const std::vector<double> img = plan.family == 1 ? reg_image_dpp(Ah, m, plan.p1) : reg_image_reg(Ah, m, plan.p1);
    if (h->reg_img) (void)hipFree(h->reg_img);
    HIPCK(hipMalloc((void**)&h->reg_img, sizeof(double) * img.size()));
    HIPCK(hipMemcpy(h->reg_img, img.data(), sizeof(double) * img.size(), hipMemcpyHostToDevice));
    h->reg_img_family = plan.family; h->reg_img_par = plan.p1;
    return FASP_SUCCESS;
}

// ---------------------------------------------------------------------------
// the launchers: each executes the plan, one switch over its instantiation
// ---------------------------------------------------------------------------
#define SPCG_LAUNCH(K, ...) hipLaunchKernelGGL(K, dim3(plan.blocks), dim3(plan.threads), (size_t)plan.lds, g_ctx.stream, __VA_ARGS__)
static void launch_spcg_small(const CoarsePlan& plan, const SpcgArgs& a)
{
    switch (spcg_inst(plan)) {
    case spcg_inst(1, 4, 1): SPCG_LAUNCH((k_spcg_dpp<4, 4, true>), a, plan.LD); break;
    case spcg_inst(1, 4, 0): SPCG_LAUNCH((k_spcg_dpp<4, 4, false>), a, plan.LD); break;
    case spcg_inst(1, 6, 1): SPCG_LAUNCH((k_spcg_dpp<6, 2, true>), a, plan.LD); break;
    case spcg_inst(1, 6, 0): SPCG_LAUNCH((k_spcg_dpp<6, 2, false>), a, plan.LD); break;
    case spcg_inst(1, 8, 1): SPCG_LAUNCH((k_spcg_dpp<8, 2, true>), a, plan.LD); break;
    case spcg_inst(1, 8, 0): SPCG_LAUNCH((k_spcg_dpp<8, 2, false>), a, plan.LD); break;
    case spcg_inst(2, 32): (void)allow_lds<k_spcg_reg<32>>(COARSE_LDS_OPT); SPCG_LAUNCH(k_spcg_reg<32>, a, plan.LD); break;
    case spcg_inst(2, 48): (void)allow_lds<k_spcg_reg<48>>(COARSE_LDS_OPT); SPCG_LAUNCH(k_spcg_reg<48>, a, plan.LD); break;
    case spcg_inst(2, 64): (void)allow_lds<k_spcg_reg<64>>(COARSE_LDS_OPT); SPCG_LAUNCH(k_spcg_reg<64>, a, plan.LD); break;
    case spcg_inst(3, 0): (void)allow_lds<k_spcg_wave>(COARSE_LDS_OPT); SPCG_LAUNCH(k_spcg_wave, a, plan.LD); break;
    case spcg_inst(4, 2): (void)allow_lds<k_spcg_small<true, true>>(COARSE_LDS_OPT); SPCG_LAUNCH((k_spcg_small<true, true>), a); break;
    case spcg_inst(4, 1): (void)allow_lds<k_spcg_small<true, false>>(COARSE_LDS_OPT); SPCG_LAUNCH((k_spcg_small<true, false>), a); break;
    default: SPCG_LAUNCH((k_spcg_small<false, false>), a); break;
    }
}
static void launch_spcg_fused(const CoarsePlan& plan, const SpcgFusedArgs& fa)
{
    switch (spcg_inst(plan)) {
    case spcg_inst(5, 4): SPCG_LAUNCH(k_spcg_fused<4>, fa); break;
    case spcg_inst(5, 10): SPCG_LAUNCH(k_spcg_fused<10>, fa); break;
    default: SPCG_LAUNCH(k_spcg_fused<16>, fa); break;
    }
}
static void launch_spcg_step(const CoarsePlan& plan, const SpcgStepArgs& sa)
{
    switch (spcg_inst(plan)) {
    case spcg_inst(7, 4): SPCG_LAUNCH(k_spcg_step_reg<4>, sa); break;
    case spcg_inst(7, 10): SPCG_LAUNCH(k_spcg_step_reg<10>, sa); break;
    default: SPCG_LAUNCH(k_spcg_step, sa); break;
    }
}
#undef SPCG_LAUNCH
template <int NE>
static int launch_spcg_persist(const CoarsePlan& plan, const SpcgPersistArgs& pa)
{
    HIPCK(allow_lds<k_spcg_persist<NE>>(CU_LDS - 1024));
    // (fasp_hip_tune("spcg_test_hang", 1): one block short -- the others time out, the solve falls back; tests only)
    hipLaunchKernelGGL(k_spcg_persist<NE>, dim3(plan.blocks - (g_tune.spcg_test_hang ? 1 : 0)), dim3(plan.threads), (size_t)plan.lds, g_ctx.stream, pa);
    return FASP_SUCCESS;
}
static int launch_spcg_persist(const CoarsePlan& plan, const SpcgPersistArgs& pa)
{
    switch (spcg_inst(plan)) {
    case spcg_inst(6, 32): return launch_spcg_persist<32>(plan, pa);
    case spcg_inst(6, 48): return launch_spcg_persist<48>(plan, pa);
    case spcg_inst(6, 56): return launch_spcg_persist<56>(plan, pa);
    default: return launch_spcg_persist<64>(plan, pa);
    }
}

// ---------------------------------------------------------------------------
// families 1 .. 4: the whole solve in one launch of one workgroup
// ---------------------------------------------------------------------------
static int spcg_one_launch(fasp_hip_amg* h, DevLevel& D, const CoarsePlan& plan, double tol)
{
    const DevCSR& A = D.A;
    SpcgArgs a{};
    a.A = SmallCSR{A.row, A.ia, A.ja, A.val};
    a.b = D.b; a.u = D.x; a.p = h->cp; a.r = h->cr; a.t = h->ct; a.u_best = h->cbest;
    a.tol = tol; a.MaxIt = plan.MaxIt; a.x_zero = D.x_zero ? 1 : 0; a.out = small_out_dev(); a.nnz = A.nnz;
    a.lazy = h->lazy_active ? h->d_lazy : nullptr;
    if (plan.family <= 2) {
        if (reg_image(h, plan, A.row) < 0) return ERROR_MISC;
        a.img = h->reg_img;
    }
    launch_spcg_small(plan, a);
    report_coarse_plan(h->coarse_kinfo, plan.family, plan.p1, plan.p2);
    D.x_zero = false;
    if (a.lazy) return FASP_SUCCESS;   // the verdict is read once per application of the preconditioner (precond_amg)
    SmallOut o;
    if (small_out_fetch(o) < 0) return ERROR_MISC;
    h->coarse_iters += o.iters;
    if (std::getenv("FASP_HIP_DEBUG_COARSE")) std::printf("[coarse small] status %d iters %d relres %.6e\n", o.status, o.iters, o.relres);
    return o.status;
}

// ---------------------------------------------------------------------------
// families 5 .. 7: device-resident iteration state; the host queues iterations without waiting and synchronises once per
// batch.  When one of the reference's tests fires, the step raises `stop`, the launches queued behind it return at once,
// and the branch is replayed on the host from the recorded scalars (spcg_replay).
// ---------------------------------------------------------------------------
struct SpcgRun {   // what the steps of one solve share
    fasp_hip_amg* h; const DevCSR& A; int m; double tol, maxdiff;
    const double* b; double *u, *r, *p, *t, *u_best;
    double *R[2], *P[2], *T[2]; SpcgBc* bc;   // k_spcg_fused: the two parities of r, p, t and the broadcast record
    int  cur;     // parity of the buffers that hold r and p
    bool first;   // next launch starts a batch sequence: SpMV only
    // the reference's variables (KrySPcg.c)
    int iter = 0, stag = 1, more_step = 1, iter_best = 0;
    double absres0 = BIGREAL, absres = BIGREAL, relres = BIGREAL, normr0 = BIGREAL, temp1 = 0.0, absres_best = BIGREAL;
};
enum SpcgNext { SPCG_GO_ON = 0, SPCG_RESTORE = 1, SPCG_FINISHED = 2 };   // iterate / restore the best iterate and finish / finish

// start on the device (k_spcg_init): no host round trip before the first batch
static int spcg_start_device(SpcgRun& q, DevLevel& D, const CoarsePlan& plan)
{
    if (!D.x_zero) d_resid(q.A, q.u, q.b, q.r);
    SpcgInitArgs ia{};
    ia.m = q.m; ia.x_zero = D.x_zero ? 1 : 0; ia.MaxIt = plan.MaxIt; ia.tol = q.tol; ia.maxdiff = q.maxdiff;
    ia.b = q.b; ia.u = q.u; ia.r = q.r; ia.p = q.p; ia.u_best = q.u_best; ia.st = q.h->spcg_state;
    hipLaunchKernelGGL(k_spcg_init, dim3(1), dim3(512), 0, g_ctx.stream, ia);
    D.x_zero = false;
    return SPCG_GO_ON;
}
// start on the host, one wait; S: the state before the first iteration, on its way to the device
static int spcg_start_host(SpcgRun& q, DevLevel& D, const CoarsePlan& plan, SpcgState& S)
{
    hipStream_t s = g_ctx.stream;
    const int m = q.m;
    double red[8];
    // u_best starts as zeros (calloc'ed work array, KrySPcg.c:88)
    HIPCK(hipMemsetAsync(q.u_best, 0, sizeof(double) * m, s));
    // r = b - A u  (u == 0 on entry from the cycle: r = b, no matrix pass)
    if (D.x_zero) {
        HIPCK(hipMemcpyAsync(q.r, q.b, sizeof(double) * m, hipMemcpyDeviceToDevice, s));
        HIPCK(hipMemsetAsync(q.u, 0, sizeof(double) * m, s));
        D.x_zero = false;
    } else {
        d_resid(q.A, q.u, q.b, q.r);
    }
    if (d_dot(m, q.r, q.r, red) < 0) return ERROR_MISC;  // z = r: (r,r) serves both ||r|| and (z,r)
    q.absres0 = std::sqrt(red[0]);
    q.normr0  = std::max(SMALLREAL, q.absres0);
    q.relres  = q.absres0 / q.normr0;
    if (q.relres < q.tol) return SPCG_FINISHED;
    HIPCK(hipMemcpyAsync(q.p, q.r, sizeof(double) * m, hipMemcpyDeviceToDevice, s));
    q.temp1 = red[0];
    S.temp1 = q.temp1; S.temp1_prev = q.temp1; S.absres_best = q.absres_best; S.normr0 = q.normr0; S.tol = q.tol;
    S.maxdiff = q.maxdiff; S.iter = 0; S.iter_best = 0; S.stag = q.stag; S.MaxIt = plan.MaxIt; S.stop = SPCG_RUN;
    S.absres = q.absres; S.relres = q.relres; S.alpha = 0.0;  // values before the first iteration
    HIPCK(hipMemcpyAsync(q.h->spcg_state, &S, sizeof(S), hipMemcpyHostToDevice, s));
    return SPCG_GO_ON;
}

// queue one batch in the plan's form: the persistent kernel (the whole solve), `batch` fused iterations, or `batch` times SpMV + step
static int spcg_queue(SpcgRun& q, const CoarsePlan& plan, int batch)
{
    fasp_hip_amg* h = q.h;
    hipStream_t s = g_ctx.stream;
    const int m = q.m;
    if (plan.family == 6) {
        auto& PP = h->persist;
        // epochs of this launch: (launch number) << 11 | iteration + 1 (max_steps <= 1002 < 2048); on wrap-around the
        // records are cleared, so an old record can never carry a current epoch
        PP.launches = (PP.launches + 1u) & 0x1fffffu;
        if (PP.launches == 0u) { HIPCK(hipMemsetAsync(PP.t2, 0, sizeof(double) * 4 * (size_t)m, s)); PP.launches = 1u; }
        SpcgPersistArgs pa{};
        pa.epoch0 = PP.launches << 11;
        pa.m = m; pa.max_steps = plan.MaxIt + 2; pa.nblocks = plan.blocks; pa.st = h->spcg_state;
        pa.r = q.r; pa.p = q.p; pa.u = q.u; pa.u_best = q.u_best; pa.t2 = PP.t2; pa.sync = PP.sync;
        pa.vals = PP.vals; pa.cols = PP.cols; pa.wrow = PP.wrow; pa.wend = PP.wend;
        HIPCK(hipMemsetAsync(PP.sync, 0, 1024, s));
        pa.u_lds = plan.p2;
        const int lst = launch_spcg_persist(plan, pa);
        if (lst < 0) return lst;
    }
    for (int k = 0; k < batch && plan.family == 5; ++k) {
        SpcgFusedArgs fa{};
        fa.m = m; fa.first = q.first ? 1 : 0; fa.in = q.cur; fa.st = h->spcg_state; fa.bc = q.bc;
        fa.ia = q.A.ia; fa.ja = q.A.ja; fa.ja16 = q.A.jbase ? nullptr : q.A.ja16; fa.val = q.A.val;
        for (int j = 0; j < 2; ++j) { fa.r[j] = q.R[j]; fa.p[j] = q.P[j]; fa.t[j] = q.T[j]; }
        fa.u = q.u; fa.u_best = q.u_best;
        launch_spcg_fused(plan, fa);
        q.cur ^= 1; q.first = false;
    }
    for (int k = 0; k < batch && plan.family == 7; ++k) {
        CsrArgs a{}; a.x = q.p; a.y = q.t; a.dotv = q.p; a.partials = g_ctx.d_partials; a.stop = &h->spcg_state->stop;
        SpcgStepArgs sa{};
        sa.m = m; sa.st = h->spcg_state; sa.t = q.t; sa.p = q.p; sa.u = q.u; sa.r = q.r; sa.u_best = q.u_best;
        sa.ntp = launch_csr<OP_MXV_DOT>(q.A, a);
        sa.tp_partials = g_ctx.d_partials;
        launch_spcg_step(plan, sa);
    }
    report_coarse_plan(h->coarse_kinfo, plan.family, plan.p1, plan.p2);
    return FASP_SUCCESS;
}

// fetch the state: one wait.  Behind the state travel the persistent kernel's error word and the speculative norm.
// The persistent kernel normally ends because the recurrence's residual met the tolerance, and the reference then forms the TRUE
// residual (Check III, KrySPcg.c:258-275): a second wait of the host per coarse solve.  It is queued here, behind the kernel,
// into the scratch vector t -- the same kernels on the same u -- and its norm travels with the state: one wait (round 5).
static int spcg_fetch(SpcgRun& q, const CoarsePlan& plan, SpcgState& S, bool& spec_rr, double& spec_val)
{
    hipStream_t s = g_ctx.stream;
    const bool persist = plan.family == 6;
    char* behind = reinterpret_cast<char*>(g_ctx.h_part) + sizeof(SpcgState);
    static_assert(sizeof(SpcgState) % 8 == 0 && sizeof(SpcgState) + 24 <= sizeof(double) * 64, "the error word and the speculative norm travel behind the state");
    spec_rr = false; spec_val = 0.0;
    if (persist && g_tune.spcg_spec) {
        d_resid(q.A, q.u, q.b, q.t);
        if (d_dot_to(q.m, q.t, q.t, 14, false) < 0) return ERROR_MISC;
        spec_rr = true;
    }
    HIPCK(hipMemcpyAsync(g_ctx.h_part, q.h->spcg_state, sizeof(SpcgState), hipMemcpyDeviceToHost, s));
    if (persist) HIPCK(hipMemcpyAsync(behind, q.h->persist.sync, 16, hipMemcpyDeviceToHost, s));
    if (spec_rr) HIPCK(hipMemcpyAsync(behind + 16, g_ctx.d_red + 14, 8, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    std::memcpy(&S, g_ctx.h_part, sizeof(S));
    if (spec_rr) std::memcpy(&spec_val, behind + 16, 8);
    if (persist) {   // a block that gave up waiting raised the error word -- also when block 0 itself never ran
        unsigned ew[4];
        std::memcpy(ew, behind, 16);
        if (ew[3] != 0u && S.stop == SPCG_RUN) S.stop = SPCG_HANG;
#ifdef SPCG_PERSIST_STAMPS
        unsigned dbg[64];
        (void)hipMemcpy(dbg, q.h->persist.sync, sizeof(dbg), hipMemcpyDeviceToHost);
        std::printf("[persist stamps, 10 ns ticks, %d steps] lead:", S.iter);
        for (int k = 0; k < 8; ++k) std::printf(" %u", dbg[32 + k]);
        std::printf(" | block 1:");
        for (int k = 0; k < 8; ++k) std::printf(" %u", dbg[40 + k]);
        std::printf("   (spmv meet(second group of records + verdict) read step(tail) pass1-2 pass3 first-group-of-records(block 1) poll-rounds)\n");
#endif
    }
    return FASP_SUCCESS;
}

// A test fired in iteration S.iter: finish that iteration as the reference does (KrySPcg.c:172-330).  SPCG_GO_ON: the solve restarted
// from the true residual, S is back on the device.
static int spcg_replay(SpcgRun& q, const CoarsePlan& plan, SpcgState& S, bool spec_rr, double spec_val)
{
    hipStream_t s = g_ctx.stream;
    const int m = q.m;
    double red[8] = {S.rr, S.uu, S.pp, S.maxu, S.nan};
    q.temp1 = S.temp1_prev;
    // (on a breakdown the step kernel leaves absres / relres of the PREVIOUS iteration in the state,
    // which is what the reference's variables hold when it jumps to RESTORE_BESTSOL, KrySPcg.c:176)
    q.absres = S.absres; q.relres = S.relres;
    if (S.stop == SPCG_DIV0) return SPCG_RESTORE;
    if (S.stop == SPCG_NAN) { q.absres = BIGREAL; return SPCG_RESTORE; }
    if (S.stop == SPCG_SOLSTAG) { q.iter = ERROR_SOLVER_SOLSTAG; return SPCG_RESTORE; }  // Check I
    if (S.stop == SPCG_MAXIT) { q.iter = plan.MaxIt + 1; return SPCG_RESTORE; }
    const double normu = std::sqrt(red[1]);
    const double reldiff = std::fabs(S.alpha) * std::sqrt(red[2]) / normu;
    if ((q.stag <= MAX_STAG) & (reldiff < q.maxdiff)) {  // Check II
        spec_rr = false;   // (what follows works on r itself)
        d_resid(q.A, q.u, q.b, q.r);
        if (d_dot(m, q.r, q.r, red) < 0) return ERROR_MISC;
        q.absres = std::sqrt(red[0]);
        q.relres = q.absres / q.normr0;
        if (q.relres < q.tol) return SPCG_RESTORE;
        if (q.stag >= MAX_STAG) { q.iter = ERROR_SOLVER_STAG; return SPCG_RESTORE; }
        HIPCK(hipMemsetAsync(q.p, 0, sizeof(double) * m, s));
        ++q.stag;
    }
    if (q.relres < q.tol) {  // Check III: true residual
        if (spec_rr) red[0] = spec_val;   // formed behind the kernel, in t
        else {
            d_resid(q.A, q.u, q.b, q.r);
            if (d_dot(m, q.r, q.r, red) < 0) return ERROR_MISC;
        }
        q.absres = std::sqrt(red[0]);
        q.relres = q.absres / q.normr0;
        if (q.relres < q.tol) return SPCG_RESTORE;
        if (spec_rr) HIPCK(hipMemcpyAsync(q.r, q.t, sizeof(double) * m, hipMemcpyDeviceToDevice, s));   // the solve goes on from the true residual
        if (q.more_step >= MAX_RESTART) { q.iter = ERROR_SOLVER_TOLSMALL; return SPCG_RESTORE; }
        HIPCK(hipMemsetAsync(q.p, 0, sizeof(double) * m, s));
        ++q.more_step;
    }
    // every branch that gets here restarted: p was zeroed, so p = z + beta p = r
    q.absres0 = q.absres;
    const double temp2 = red[0], beta = temp2 / q.temp1;
    q.temp1 = temp2;
    d_axpby(m, 1.0, q.r, beta, q.p);
    S.temp1 = q.temp1; S.temp1_prev = q.temp1; S.stag = q.stag; S.stop = SPCG_RUN;
    HIPCK(hipMemcpyAsync(q.h->spcg_state, &S, sizeof(S), hipMemcpyHostToDevice, s));
    HIPCK(hipStreamSynchronize(s));  // S lives on the caller's stack frame
    return SPCG_GO_ON;
}

// restore the best iterate (KrySPcg.c, RESTORE_BESTSOL)
static int spcg_restore_best(SpcgRun& q)
{
    if (q.iter == q.iter_best) return FASP_SUCCESS;
    double red[8];
    d_resid(q.A, q.u_best, q.b, q.r);
    if (d_dot(q.m, q.r, q.r, red) < 0) return ERROR_MISC;
    q.absres_best = std::sqrt(red[0]);
    if (q.absres > q.absres_best + q.maxdiff || std::isnan(q.absres)) {
        HIPCK(hipMemcpyAsync(q.u, q.u_best, sizeof(double) * q.m, hipMemcpyDeviceToDevice, g_ctx.stream));
        q.relres = q.absres_best / q.normr0;
    }
    return FASP_SUCCESS;
}

static int coarse_spcg(fasp_hip_amg* h, DevLevel& D, double tol, int prtlvl)
{
    (void)prtlvl;
    const CoarsePlan* plan = &coarse_plan(h, D);
    if (plan->family <= 4) return spcg_one_launch(h, D, *plan, tol);
    const int m = D.A.row;
    SpcgRun q{h, D.A, m, tol, tol * STAG_RATIO, D.b, D.x, h->cr, h->cp, h->ct, h->cbest, {h->cr, nullptr}, {h->cp, nullptr}, {h->ct, nullptr}, nullptr, 0, true};
    if (!h->spcg_state) HIPCK(hipMalloc(&h->spcg_state, sizeof(SpcgState)));
    SpcgState S{};
    int next = plan->dev_start ? spcg_start_device(q, D, *plan) : spcg_start_host(q, D, *plan, S);
    if (next < 0) return next;
    // the first batch is sized by the previous solve on this level (the count hardly moves from cycle to
    // cycle): normally one synchronisation per solve; 1 + iterations launches, the first one has no step
    int batch = plan->batch;
    if (plan->dev_start) {
        if (h->spcg_last_iters > 0) batch = std::max(4, std::min(h->spcg_last_iters + 1, 96));
        if (!h->spcg_fused_buf) HIPCK(hipMalloc(&h->spcg_fused_buf, sizeof(double) * (3 * (size_t)m + 4)));
        q.R[1] = h->spcg_fused_buf; q.P[1] = q.R[1] + m; q.T[1] = q.P[1] + m;
        q.bc = reinterpret_cast<SpcgBc*>(q.T[1] + m);
    }
    while (next == SPCG_GO_ON) {
        bool spec_rr; double spec_val;
        int st = spcg_queue(q, *plan, batch);
        if (st >= 0) st = spcg_fetch(q, *plan, S, spec_rr, spec_val);
        if (st < 0) return st;
        q.iter = S.iter; q.absres_best = S.absres_best; q.iter_best = S.iter_best;
        batch = plan->batch;
        if (plan->dev_start) {
            q.normr0 = S.normr0;
            if (S.stop == SPCG_ZERO_RHS) { q.relres = S.relres; next = SPCG_FINISHED; break; }  // KrySPcg.c:135
        }
        if (S.stop == SPCG_HANG) {
            // A block of the persistent kernel was not resident (another process on this GPU, a concurrently resident
            // kernel): a benign condition, not a failed solve.  r, p, u and the scalars are those of the last finished
            // iteration -- this coarse solve goes on through the per-iteration kernels, and so do all later ones.
            std::fprintf(stderr, "### WARNING: fasp_hip: the persistent coarse CG kernel timed out waiting for a block that was not "
                                 "resident (is another process using this GPU?); continuing with the per-iteration kernels\n");
            g_persist_disabled = true; ++g_coarse_gen;
            plan = &coarse_plan(h, D);   // (k_spcg_fused now)
            S.stop = SPCG_RUN;
            HIPCK(hipMemcpyAsync(h->spcg_state, &S, sizeof(S), hipMemcpyHostToDevice, g_ctx.stream));
            HIPCK(hipStreamSynchronize(g_ctx.stream));  // S lives on this stack frame
            q.cur = 0; q.first = true;
            continue;
        }
        if (S.stop == SPCG_RUN) continue;
        if (plan->family == 5) { q.cur = S.pad; q.r = q.R[q.cur]; q.p = q.P[q.cur]; q.first = true; }  // where the last finished step left r and p
        next = spcg_replay(q, *plan, S, spec_rr, spec_val);
        if (next < 0) return next;
    }
    if (next == SPCG_RESTORE && spcg_restore_best(q) < 0) return ERROR_MISC;
    if (std::getenv("FASP_HIP_DEBUG_COARSE")) std::printf("[coarse batched] iter %d relres %.6e absres %.6e best %d\n", q.iter, q.relres, q.absres, q.iter_best);
    if (q.iter > 0) { h->coarse_iters += q.iter; h->spcg_last_iters = q.iter; }
    if (q.iter > plan->MaxIt) return ERROR_SOLVER_MAXIT;
    return q.iter;
}
