// solver.hip -- device-resident AMG hierarchy, multigrid cycle, coarse-level safe CG,
// preconditioned CG driver and the C-ABI of libfasp_hip.so.
//
// Boundary (include/fasp_hip.h): fasp_solver_dcsr_krylov_amg() keeps the reference's
// signature (base/src/SolCSR.c:476).  Inside it the host builds the hierarchy
// (host_setup.cpp), uploads it once, and the whole Krylov loop runs on the GPU; only
// reduction scalars cross back, through a pinned buffer.
//
// Reference control flow restated here (paths relative to the reference tree):
//   fasp_solver_dcsr_pcg     base/src/KryPcg.c:96-362   (incl. stagnation / false-convergence)
//   fasp_precond_amg         base/src/PreCSR.c:416-435  (tol NOT forwarded: coarse tol 1e-10)
//   fasp_solver_mgcycle      base/src/PreMGCycle.c:48-274
//   fasp_coarse_itsolver     base/src/PreMGUtil.inl:37-58
//   fasp_solver_dcsr_spcg    base/src/KrySPcg.c:60-367  (pc == NULL)
//
// There is NO CPU fallback: without a usable gfx950 device every entry point that
// computes returns ERROR_MISC after printing why.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <omp.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "fasp_comm.h"
#include "fasp_internal.h"
#include "bsr_sweep_plan.h"
#include "krylov_ws.h"
#include "kernels.hip.h"
#include "kernels2.hip.h"
#include "kernels3.hip.h"
#include "kernels4.hip.h"
#include "kernels5.hip.h"
#include "small_solvers.hip.h"
#include "seq_split.hip.h"
#include "seq_chain.hip.h"

namespace fasp_str { struct CsrSwzDev; }   // csr_swz.hip.h; a Schwarz level of the AMG hierarchy owns one (hierarchy.hip.h)

namespace fasp {

#define HIPCK(expr)                                                                        \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            std::fprintf(stderr, "### ERROR: fasp_hip: %s failed: %s [%s:%d]\n", #expr,    \
                         hipGetErrorString(e_), __FILE__, __LINE__);                       \
            return ERROR_MISC;                                                             \
        }                                                                                  \
    } while (0)

// ---------------------------------------------------------------------------
// device context (one per process: one process per GPU)
// ---------------------------------------------------------------------------
struct Ctx {
    bool        ready  = false;
    int         device = -1;
    hipStream_t stream = nullptr;
    hipStream_t comm_stream = nullptr;   // halo exchanges that overlap the interior rows (hierarchy.hip.h, dist_launch)
    hipEvent_t  ev_ready = nullptr, ev_halo = nullptr;
    double*     d_partials = nullptr;  // 8 quantities x MAXGRID
    double*     d_partials2 = nullptr; // second set (consumer kernels that read the first)
    double*     h_part     = nullptr;  // pinned mirror of d_partials2
    double*     d_red      = nullptr;  // reduced scalars (device)
    double*     h_red      = nullptr;  // pinned host mirror
    int         num_cu     = 256;
};
static Ctx g_ctx;
static int g_requested_device = -1;

constexpr int RED_SLOTS = 16;

static int ctx_init()
{
    if (g_ctx.ready) return FASP_SUCCESS;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        std::fprintf(stderr, "### ERROR: fasp_hip: no HIP device available (%s). This library has "
                             "no CPU fallback.\n", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return ERROR_MISC;
    }
    // an explicit fasp_hip_set_device() wins over the environment; FASP_HIP_DEVICE only fills in when nothing was asked for
    int dev = 0;
    if (g_requested_device >= 0) dev = g_requested_device;
    else if (const char* lr = std::getenv("FASP_HIP_DEVICE")) dev = std::atoi(lr);
    if (dev < 0 || dev >= ndev) {
        // several ranks on one device is the validation set-up only (shared-memory transport): it must be asked for
        const char* wrap = std::getenv("FASP_HIP_ALLOW_DEVICE_WRAP");
        if (wrap && std::atoi(wrap) != 0 && dev >= 0) dev = dev % ndev;
        else {
            std::fprintf(stderr, "### ERROR: fasp_hip: device %d requested, %d visible (one process per GPU; "
                                 "FASP_HIP_ALLOW_DEVICE_WRAP=1 shares devices for the shared-memory validation transport)\n", dev, ndev);
            return ERROR_INPUT_PAR;
        }
    }
    HIPCK(hipSetDevice(dev));
    hipDeviceProp_t prop;
    HIPCK(hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        std::fprintf(stderr, "### WARNING: fasp_hip: device %d is %s; kernels are built for gfx950\n",
                     dev, prop.gcnArchName);
    g_ctx.num_cu = prop.multiProcessorCount;
    g_ctx.device = dev;
    HIPCK(hipStreamCreateWithFlags(&g_ctx.stream, hipStreamNonBlocking));
    HIPCK(hipStreamCreateWithFlags(&g_ctx.comm_stream, hipStreamNonBlocking));
    HIPCK(hipEventCreateWithFlags(&g_ctx.ev_ready, hipEventDisableTiming));
    HIPCK(hipEventCreateWithFlags(&g_ctx.ev_halo, hipEventDisableTiming));
    HIPCK(hipMalloc(&g_ctx.d_partials, sizeof(double) * 8 * MAXGRID));
    HIPCK(hipMalloc(&g_ctx.d_partials2, sizeof(double) * (8 * MAXGRID + 8)));
    HIPCK(hipHostMalloc(&g_ctx.h_part, sizeof(double) * (8 * MAXGRID + 8), hipHostMallocDefault));
    HIPCK(hipMalloc(&g_ctx.d_red, sizeof(double) * RED_SLOTS));
    HIPCK(hipHostMalloc(&g_ctx.h_red, sizeof(double) * RED_SLOTS, hipHostMallocDefault));
    g_ctx.ready = true;
    // development knobs from the environment: FASP_HIP_TUNE="key=value,key=value" (the keys of fasp_hip_tune)
    if (const char* tv = std::getenv("FASP_HIP_TUNE")) {
        std::string all(tv);
        size_t p0 = 0;
        while (p0 < all.size()) {
            size_t p1 = all.find(',', p0);
            if (p1 == std::string::npos) p1 = all.size();
            const std::string kv = all.substr(p0, p1 - p0);
            const size_t eq = kv.find('=');
            if (eq != std::string::npos && fasp_hip_tune(kv.substr(0, eq).c_str(), std::atoi(kv.c_str() + eq + 1)) < 0)
                std::fprintf(stderr, "### WARNING: fasp_hip: FASP_HIP_TUNE: unknown key in '%s'\n", kv.c_str());
            p0 = p1 + 1;
        }
    }
    return FASP_SUCCESS;
}

static inline int vec_grid(int n)
{
    long long g = ((long long)n + BLOCK - 1) / BLOCK;
    if (g > MAXGRID) g = MAXGRID;
    if (g < 1) g = 1;
    return (int)g;
}

#include "device_csr.hip.h"

#include "hierarchy.hip.h"

#include "smoothers.hip.h"

#include "coarse_cg.hip.h"

#include "krylov.hip.h"

#include "safe_krylov.hip.h"

#include "cycles.hip.h"

#include "pcg.hip.h"

}  // namespace fasp

#include "bsr.hip.h"
#include "str_common.hip.h"
#include "csr_swz.hip.h"
#include "str.hip.h"
#include "str_ilu.hip.h"
#include "str_sweep.hip.h"
#include "str_swz.hip.h"

// ===========================================================================
// C ABI
// ===========================================================================
// ---------------------------------------------------------------------------
// Threading contract of the boundary (SURVEY section 8b "Threading"; the serial reference, AuxThreads.c:29-57, lets different
// threads solve on DISJOINT data).  The device side of this library is one context per process -- one stream, one set of
// reduction buffers, the fasp_hip_tune switches -- so every computing entry point takes ONE process-wide lock for its whole
// duration: calls from different host threads are SERIALISED, never interleaved.  The lock is recursive (an entry may call
// another one, and a caller's precond / mxv_matfree callback may call back into the library on the same thread).
// Concurrency across GPUs is one PROCESS per GPU, not threads.
// ---------------------------------------------------------------------------
static std::recursive_mutex g_entry_mutex;
#define FASP_ENTRY() std::lock_guard<std::recursive_mutex> fasp_entry_lock_(g_entry_mutex)

extern "C" {

int fasp_hip_set_device(int device)
{
    FASP_ENTRY();
    if (g_ctx.ready && device != g_ctx.device) {
        std::fprintf(stderr, "### ERROR: fasp_hip: device already bound to %d\n", g_ctx.device);
        return ERROR_INPUT_PAR;
    }
    g_requested_device = device;
    return ctx_init();
}

int fasp_hip_device_count(void)
{
    FASP_ENTRY();
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return ERROR_MISC;
    return n;
}

// PCI bus id ("0000:c1:00.0") of the device this process is bound to (binding it to the default one if nothing is yet): how a
// multi-rank run proves that its ranks sit on DIFFERENT devices (bench_dist.py, tests/test_gpu_dist.py).
int fasp_hip_device_identity(char* out, int cap)
{
    FASP_ENTRY();
    if (!out || cap < 16) return ERROR_INPUT_PAR;
    if (ctx_init() < 0) return ERROR_MISC;
    if (hipDeviceGetPCIBusId(out, cap, g_ctx.device) != hipSuccess) return ERROR_MISC;
    return g_ctx.device;
}

int fasp_hip_available(void)
{
    FASP_ENTRY();
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return 0;
    return 1;
}

int fasp_hip_amg_create_host(fasp_hip_amg** out, const dCSRmat* A, AMG_param* amgparam)
{
    FASP_ENTRY();
    if (!out || !A || !amgparam) return ERROR_INPUT_PAR;
    *out = nullptr;
    int st = check_supported(nullptr, amgparam);
    if (st < 0) return st;
    fasp_hip_amg* h = new fasp_hip_amg();
    st = (amgparam->AMG_type == SA_AMG)   ? host_setup_sa(A, amgparam, h->H)  // SolCSR.c:509-521
         : (amgparam->AMG_type == UA_AMG) ? host_setup_ua(A, amgparam, h->H)
                                          : host_setup_rs(A, amgparam, h->H);
    if (st < 0) { delete h; return st; }
    h->param = *amgparam;
    *out = h;
    return FASP_SUCCESS;
}

// ---- one host setup per node (SURVEY.md section 8e "Setup"): the rank that ran it publishes the host hierarchy
// in a POSIX shared-memory segment, the other ranks of the node map it read-only and take their rows from it.
namespace {
struct ShmHierHeader {
    unsigned long long magic;       // 'FASPHIER'
    unsigned long long total_bytes;
    int                nl;
    AMG_param          param;       // as the setup left it
    struct Lvl { int has_coarse; int dims[3][3]; unsigned long long off[3][3]; unsigned long long cf_off; unsigned long long cf_n; } lvl[MAX_AMG_LVL];
};
constexpr unsigned long long HIER_MAGIC = 0x5245494850534146ull;
inline unsigned long long align64(unsigned long long x) { return (x + 63ull) & ~63ull; }
struct ShmMapping { void* base; size_t bytes; };
std::vector<std::pair<fasp_hip_amg*, ShmMapping>> g_attached;  // unmapped when the handle is destroyed
}  // namespace

int fasp_hip_amg_publish(const fasp_hip_amg* h, const char* name)
{
    FASP_ENTRY();
    if (!h || !name || h->H.L.empty() || (int)h->H.L.size() > MAX_AMG_LVL) return ERROR_INPUT_PAR;
    const int nl = (int)h->H.L.size();
    ShmHierHeader hd;
    std::memset(&hd, 0, sizeof(hd));
    hd.magic = HIER_MAGIC; hd.nl = nl; hd.param = h->param;
    unsigned long long off = align64(sizeof(ShmHierHeader));
    for (int l = 0; l < nl; ++l) {
        const HostLevel& L = h->H.L[l];
        hd.lvl[l].has_coarse = L.has_coarse ? 1 : 0;
        const HostCSR* M[3] = {&L.A, &L.P, &L.R};
        for (int w = 0; w < 3; ++w) {
            if (w > 0 && !L.has_coarse) continue;
            hd.lvl[l].dims[w][0] = M[w]->row; hd.lvl[l].dims[w][1] = M[w]->col; hd.lvl[l].dims[w][2] = M[w]->nnz;
            hd.lvl[l].off[w][0] = off; off = align64(off + 4ull * ((unsigned long long)M[w]->row + 1));
            hd.lvl[l].off[w][1] = off; off = align64(off + 4ull * (unsigned long long)M[w]->nnz);
            hd.lvl[l].off[w][2] = off; off = align64(off + 8ull * (unsigned long long)M[w]->nnz);
        }
        hd.lvl[l].cf_n = L.cfmark.n;
        hd.lvl[l].cf_off = off; off = align64(off + 4ull * L.cfmark.n);
    }
    hd.total_bytes = off;
    const std::string nm = std::string("/") + name;
    shm_unlink(nm.c_str());
    const int fd = shm_open(nm.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
    if (fd < 0 || ftruncate(fd, (off_t)off) != 0) { std::perror("fasp_hip_amg_publish"); if (fd >= 0) close(fd); return ERROR_MISC; }
    char* base = (char*)mmap(nullptr, (size_t)off, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (base == MAP_FAILED) { std::perror("fasp_hip_amg_publish mmap"); return ERROR_ALLOC_MEM; }
    for (int l = 0; l < nl; ++l) {
        const HostLevel& L = h->H.L[l];
        const HostCSR* M[3] = {&L.A, &L.P, &L.R};
        for (int w = 0; w < 3; ++w) {
            if (w > 0 && !L.has_coarse) continue;
            std::memcpy(base + hd.lvl[l].off[w][0], M[w]->ia.data(), 4 * ((size_t)M[w]->row + 1));
            std::memcpy(base + hd.lvl[l].off[w][1], M[w]->ja.data(), 4 * (size_t)M[w]->nnz);
            std::memcpy(base + hd.lvl[l].off[w][2], M[w]->val.data(), 8 * (size_t)M[w]->nnz);
        }
        if (L.cfmark.n) std::memcpy(base + hd.lvl[l].cf_off, L.cfmark.data(), 4 * L.cfmark.n);
    }
    std::memcpy(base, &hd, sizeof(hd));  // header last: a reader that sees the magic sees everything
    munmap(base, (size_t)off);
    return FASP_SUCCESS;
}

int fasp_hip_amg_unpublish(const char* name)
{
    FASP_ENTRY();
    if (!name) return ERROR_INPUT_PAR;
    shm_unlink((std::string("/") + name).c_str());
    return FASP_SUCCESS;
}

int fasp_hip_amg_attach(fasp_hip_amg** out, const char* name)
{
    FASP_ENTRY();
    if (!out || !name) return ERROR_INPUT_PAR;
    *out = nullptr;
    const std::string nm = std::string("/") + name;
    const int fd = shm_open(nm.c_str(), O_RDONLY, 0600);
    if (fd < 0) { std::fprintf(stderr, "### ERROR: fasp_hip_amg_attach: no segment %s\n", nm.c_str()); return ERROR_OPEN_FILE; }
    struct stat sb;
    if (fstat(fd, &sb) != 0 || (size_t)sb.st_size < sizeof(ShmHierHeader)) { close(fd); return ERROR_WRONG_FILE; }
    char* base = (char*)mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_SHARED, fd, 0);
    close(fd);
    if (base == MAP_FAILED) return ERROR_ALLOC_MEM;
    const ShmHierHeader* hd = reinterpret_cast<const ShmHierHeader*>(base);
    if (hd->magic != HIER_MAGIC || hd->total_bytes > (unsigned long long)sb.st_size || hd->nl <= 0 || hd->nl > MAX_AMG_LVL) {
        munmap(base, (size_t)sb.st_size);
        return ERROR_WRONG_FILE;
    }
    fasp_hip_amg* h = new fasp_hip_amg();
    h->param = hd->param;
    h->param.amli_coef = nullptr;  // a pointer of the publishing process; formed again on first use
    h->H.L.resize((size_t)hd->nl);
    for (int l = 0; l < hd->nl; ++l) {
        HostLevel& L = h->H.L[(size_t)l];
        L.has_coarse = hd->lvl[l].has_coarse != 0;
        HostCSR* M[3] = {&L.A, &L.P, &L.R};
        for (int w = 0; w < 3; ++w) {
            if (w > 0 && !L.has_coarse) continue;
            M[w]->row = hd->lvl[l].dims[w][0]; M[w]->col = hd->lvl[l].dims[w][1]; M[w]->nnz = hd->lvl[l].dims[w][2];
            M[w]->ia.view(reinterpret_cast<int*>(base + hd->lvl[l].off[w][0]), (size_t)M[w]->row + 1);
            M[w]->ja.view(reinterpret_cast<int*>(base + hd->lvl[l].off[w][1]), (size_t)M[w]->nnz);
            M[w]->val.view(reinterpret_cast<double*>(base + hd->lvl[l].off[w][2]), (size_t)M[w]->nnz);
        }
        if (hd->lvl[l].cf_n) L.cfmark.view(reinterpret_cast<int*>(base + hd->lvl[l].cf_off), (size_t)hd->lvl[l].cf_n);
    }
    g_attached.push_back({h, ShmMapping{base, (size_t)sb.st_size}});
    *out = h;
    return FASP_SUCCESS;
}

int fasp_hip_amg_upload(fasp_hip_amg* h)
{
    FASP_ENTRY();
    if (!h) return ERROR_INPUT_PAR;
    if (!h->L.empty()) return FASP_SUCCESS;
    int st = ctx_init();
    if (st < 0) return st;
    try { return upload_hierarchy(h); }
    catch (const std::bad_alloc&) { std::printf("### ERROR: fasp_hip: host allocation failed during the upload\n"); return ERROR_ALLOC_MEM; }
}

namespace {
// Overlapped upload (single rank, classical setup): a second thread sends level l to the device -- matrix coding,
// re-sorting and all -- while the host setup builds level l + 1.  256^3: the 3.5-4 s of coding + upload disappear
// behind the 10 s of host setup.
struct AheadUpload {
    fasp_hip_amg*           h = nullptr;
    std::mutex              mu;
    std::condition_variable cv;
    std::vector<int>        ready;
    bool                    done = false;
    int                     status = FASP_SUCCESS;
    int                     coarsest = -1;   // set (under mu) in front of the last level's turn: that one is not smoothed
    std::thread             th;
    static void on_matrix(int level, void* ctx)   // (on the setup thread)
    {
        AheadUpload* self = static_cast<AheadUpload*>(ctx);
        sched_jobs_start_level(self->h, level, true);
    }
    static void on_ready(int level, void* ctx)
    {
        AheadUpload* self = static_cast<AheadUpload*>(ctx);
        { std::lock_guard<std::mutex> lk(self->mu); self->ready.push_back(level); }
        self->cv.notify_one();
    }
    void run()
    {
        (void)hipSetDevice(g_ctx.device);
        HostThreads team;
        double t_first = -1.0;
        for (;;) {
            int l = -1, last = -1;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !ready.empty() || done; });
                if (ready.empty()) return;
                l = ready.front(); ready.erase(ready.begin());
                last = coarsest;
            }
            if (t_first < 0) t_first = wall_seconds();
            const double t0 = wall_seconds();
            if (status >= 0) {
                int st;
                try { st = upload_level(h, l, nullptr); }
                catch (const std::bad_alloc&) { st = ERROR_ALLOC_MEM; }   // (a host buffer of the coding passes: never out of this thread)
                if (st < 0) status = st;
                // sequential smoothers: this level's sweep schedules, on host threads of their own beside the rest of the setup (smoothers.hip.h)
                if (st >= 0 && l != last) sched_jobs_start_level(h, l);
            }
            if (std::getenv("FASP_HIP_SETUP_TIMING"))
                std::printf("  [upload ahead] level %d: %.3f s (started %.3f s after the first)\n", l, wall_seconds() - t0, t0 - t_first);
        }
    }
};
}  // namespace

int fasp_hip_amg_create(fasp_hip_amg** out, const dCSRmat* A, AMG_param* amgparam)
{
    FASP_ENTRY();
    if (!out || !A || !amgparam) return ERROR_INPUT_PAR;
    *out = nullptr;
    int st = check_supported(nullptr, amgparam);
    if (st < 0) return st;
    if ((st = ctx_init()) < 0) return st;  // fail before the (long) host setup when there is no GPU
    if (amgparam->SWZ_levels > 0 && comm_size() > 1) {   // a sweep couples all rows of a level
        std::printf("### ERROR: fasp_hip: Schwarz smoothing (SWZ_levels > 0) has no multi-GPU path\n");
        return ERROR_INPUT_PAR;
    }
    fasp_hip_amg* h = nullptr;
    static const bool timing = std::getenv("FASP_HIP_SETUP_TIMING") != nullptr;
    double tp = wall_seconds();
    auto lap = [&](const char* what) {
        if (!timing) return;
        const double now = wall_seconds();
        std::printf("  [create] %-28s %8.3f s\n", what, now - tp);
        tp = now;
    };
    static const bool ahead_on = !(std::getenv("FASP_HIP_UPLOAD_AHEAD") && std::atoi(std::getenv("FASP_HIP_UPLOAD_AHEAD")) == 0);
    const bool ahead = ahead_on && comm_size() == 1 && amgparam->AMG_type != SA_AMG && amgparam->AMG_type != UA_AMG &&
                       A->nnz >= 1000000;   // worth a thread from a few hundred thousand rows on
    if (ahead) {
        h = new fasp_hip_amg();
        h->param = *amgparam;                    // (compress_enabled() etc. read globals only)
        h->L.resize(MAX_AMG_LVL + 1);            // no reallocation while the second thread fills levels
        AheadUpload up;
        up.h = h;
        up.th = std::thread([&up] { up.run(); });
        g_on_level_ready = &AheadUpload::on_ready; g_on_level_matrix = &AheadUpload::on_matrix; g_on_level_ready_ctx = &up;
        st = host_setup_rs(A, amgparam, h->H);
        g_on_level_ready = nullptr; g_on_level_matrix = nullptr; g_on_level_ready_ctx = nullptr;
        lap("host setup");
        if (st >= 0) {   // the coarsest level
            { std::lock_guard<std::mutex> lk(up.mu); up.coarsest = (int)h->H.L.size() - 1; }
            AheadUpload::on_ready((int)h->H.L.size() - 1, &up);
        }
        { std::lock_guard<std::mutex> lk(up.mu); up.done = true; }
        up.cv.notify_one();
        up.th.join();
        lap("wait for the level uploads");
        if (st >= 0) st = up.status;
        // Schedules started early (sweeps in natural order start the moment a level's matrix is final) for the level that turned out to be
        // the coarsest -- it is solved, not smoothed -- are given back now instead of holding device memory until the hierarchy goes.
        {
            const int last = (int)h->H.L.size() - 1;
            std::lock_guard<std::mutex> lk(h->sched_mu);
            for (auto& J : h->sched_jobs)
                if (J && J->level >= last) {
                    if (J->th.joinable()) J->th.join();
                    if (J->uploaded) J->S.release();
                    J.reset();
                }
        }
        if (st < 0) { h->L.resize(h->H.L.size()); fasp_hip_amg_destroy(h); return st; }
        h->param = *amgparam;
    } else {
        st = fasp_hip_amg_create_host(&h, A, amgparam);
        if (st < 0) return st;
        lap("host setup");
    }
    try { st = upload_hierarchy(h); }
    catch (const std::bad_alloc&) { std::printf("### ERROR: fasp_hip: host allocation failed during the upload\n"); st = ERROR_ALLOC_MEM; }
    lap("upload_hierarchy");
    if (st < 0) { fasp_hip_amg_destroy(h); return st; }
    *out = h;
    return FASP_SUCCESS;
}

void fasp_hip_amg_destroy(fasp_hip_amg* h)
{
    FASP_ENTRY();
    if (h) sched_jobs_join(h);
    if (!h) return;
    if (g_ctx.ready) (void)hipStreamSynchronize(g_ctx.stream);
    for (auto& D : h->L) free_level(D);
    double* v[] = {h->b, h->u, h->p, h->t, h->r, h->cp, h->cr, h->ct, h->cbest};
    for (double* q : v)
        if (q) (void)hipFree(q);
    if (h->d_lazy) (void)hipFree(h->d_lazy);
    if (h->reg_img) (void)hipFree(h->reg_img);
    if (h->h_lazy) (void)hipHostFree(h->h_lazy);
    for (auto& e : h->ev) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    if (h->spcg_state) (void)hipFree(h->spcg_state);
    if (h->spcg_fused_buf) (void)hipFree(h->spcg_fused_buf);
    {
        auto& P = h->persist;
        void* q[] = {P.vals, P.cols, P.wrow, P.wend, P.t2, P.sync};
        for (void* x : q) if (x) (void)hipFree(x);
    }
    ShmMapping map{nullptr, 0};
    for (size_t q = 0; q < g_attached.size(); ++q)
        if (g_attached[q].first == h) { map = g_attached[q].second; g_attached.erase(g_attached.begin() + (long)q); break; }
    delete h;                                     // views release nothing
    if (map.base) munmap(map.base, map.bytes);    // ... and the mapping goes after them
}

// Host-only check of the lossless matrix coding (no GPU needed): codes A the way upload_csr would,
// decodes it again and compares with A bit for bit.  *kind_out = 5 (row patterns), 4 (byte
// dictionary) or 0 (stays plain CSR).  Returns 0 when the round trip is exact.
int fasp_hip_coding_selftest(const dCSRmat* A, int* kind_out)
{
    FASP_ENTRY();
    if (!A || !kind_out) return ERROR_INPUT_PAR;
    HostCSR M;
    M.row = A->row; M.col = A->col; M.nnz = A->nnz;
    M.ia.alloc((size_t)A->row + 1); M.ja.alloc((size_t)std::max(A->nnz, 1)); M.val.alloc((size_t)std::max(A->nnz, 1));
    std::memcpy(M.ia.data(), A->IA, sizeof(int) * ((size_t)A->row + 1));
    std::memcpy(M.ja.data(), A->JA, sizeof(int) * (size_t)A->nnz);
    std::memcpy(M.val.data(), A->val, sizeof(double) * (size_t)A->nnz);
    const bool square = M.row == M.col;
    *kind_out = 0;
    if (!(M.nnz >= 4096 && (double)M.nnz <= 48.0 * M.row)) return FASP_SUCCESS;
    auto bits = [](double v) { unsigned long long b; std::memcpy(&b, &v, 8); return b; };
    {
        Buf<unsigned short> pat; Buf<int> rb;
        std::vector<int> pstart, plen, poff; std::vector<double> pval;
        if (build_rowpat(M, pat, pstart, plen, poff, pval, rb)) {
            *kind_out = 5;
            for (int r = 0; r < M.row; ++r) {
                const int id = pat[r], base = square ? r : rb[r];
                if (plen[id] != M.ia[r + 1] - M.ia[r]) return ERROR_MISC;
                for (int j = 0; j < plen[id]; ++j) {
                    const int k = M.ia[r] + j;
                    if (base + poff[pstart[id] + j] != M.ja[k] || bits(pval[pstart[id] + j]) != bits(M.val[k])) return ERROR_MISC;
                }
                for (int j = plen[id]; j < (plen[id] + 7) / 8 * 8; ++j)  // padding: offset 0, value +0.0
                    if (poff[pstart[id] + j] != 0 || bits(pval[pstart[id] + j]) != 0ull) return ERROR_MISC;
            }
            return FASP_SUCCESS;
        }
    }
    {
        std::vector<int> doff; std::vector<double> dval;
        Buf<unsigned char> code; Buf<int> rb;
        if (build_dict8(M, doff, dval, code, rb)) {
            *kind_out = 4;
            for (int r = 0; r < M.row; ++r) {
                const int base = square ? r : rb[r];
                for (int k = M.ia[r]; k < M.ia[r + 1]; ++k)
                    if (base + doff[code[k]] != M.ja[k] || bits(dval[code[k]]) != bits(M.val[k])) return ERROR_MISC;
            }
        }
    }
    return FASP_SUCCESS;
}

int fasp_hip_amg_num_levels(const fasp_hip_amg* h) { return h ? (int)h->H.L.size() : ERROR_INPUT_PAR; }

// which kernel family serves operator `which` (0 A, 1 P, 2 R) of a level, and how many bytes of
// matrix data one pass of it reads (row pointers / indices / values, or their coded form)
int fasp_hip_amg_kernel_info(const fasp_hip_amg* h, int level, int which, int* kind, double* matrix_bytes)
{
    FASP_ENTRY();
    if (!h || level < 0 || level >= (int)h->L.size() || which < 0 || which > 2) return ERROR_INPUT_PAR;
    const DevLevel& D = h->L[level];
    const DevCSR& M = which == 0 ? D.A : which == 1 ? D.P : D.R;
    if (!M.ia) return ERROR_INPUT_PAR;
    double bytes = 0.0;
    const int k = kernel_family(M, &bytes);   // (device_csr.hip.h: plan_csr, the plan launch_csr executes)
    if (kind) *kind = k;
    if (matrix_bytes) *matrix_bytes = bytes;
    return FASP_SUCCESS;
}

int fasp_hip_coarse_kernel_info(const fasp_hip_amg* h, int* info)
{
    FASP_ENTRY();
    if (!h || !info) return ERROR_INPUT_PAR;
    for (int i = 0; i < 6; ++i) info[i] = h->coarse_kinfo[i];
    info[6] = g_ctx.num_cu; info[7] = 0;
    return FASP_SUCCESS;
}

int fasp_hip_bsr_coarse_kernel_info(const fasp_hip_amg_bsr* h, int* info)
{
    FASP_ENTRY();
    if (!h || !info) return ERROR_INPUT_PAR;
    for (int i = 0; i < 6; ++i) info[i] = h->coarse_kinfo[i];
    info[6] = g_ctx.num_cu; info[7] = 0;
    return FASP_SUCCESS;
}

int fasp_hip_amg_get_matrix(const fasp_hip_amg* h, int level, int which, dCSRmat* view)
{
    FASP_ENTRY();
    if (!h || !view || level < 0 || level >= (int)h->H.L.size()) return ERROR_INPUT_PAR;
    const HostLevel& L = h->H.L[level];
    if (which != 0 && !L.has_coarse) return ERROR_INPUT_PAR;
    *view = which == 0 ? L.A.view() : which == 1 ? L.P.view() : L.R.view();
    return FASP_SUCCESS;
}

int fasp_hip_amg_get_cfmark(const fasp_hip_amg* h, int level, ivector* view)
{
    FASP_ENTRY();
    if (!h || !view || level < 0 || level >= (int)h->H.L.size() || !h->H.L[level].has_coarse)
        return ERROR_INPUT_PAR;
    view->row = h->H.L[level].A.row;
    view->val = const_cast<int*>(h->H.L[level].cfmark.data());
    return FASP_SUCCESS;
}

int fasp_hip_set_rhs(fasp_hip_amg* h, const dvector* b)
{
    FASP_ENTRY();
    if (!h || !b || h->L.empty()) return ERROR_INPUT_PAR;
    const DevLevel& D0 = h->L[0];
    if (b->row != D0.nglobal) return ERROR_MAT_SIZE;  // host vectors are global; a rank uploads its rows
    HIPCK(hipMemcpyAsync(h->b, b->val + D0.row0, sizeof(double) * D0.nloc, hipMemcpyHostToDevice, g_ctx.stream));
    HIPCK(hipStreamSynchronize(g_ctx.stream));
    return FASP_SUCCESS;
}

int fasp_hip_set_guess(fasp_hip_amg* h, const dvector* x)
{
    FASP_ENTRY();
    if (!h || h->L.empty()) return ERROR_INPUT_PAR;
    const DevLevel& D0 = h->L[0];
    if (x) {
        if (x->row != D0.nglobal) return ERROR_MAT_SIZE;
        HIPCK(hipMemcpyAsync(h->u, x->val + D0.row0, sizeof(double) * D0.nloc, hipMemcpyHostToDevice, g_ctx.stream));
    } else {
        HIPCK(hipMemsetAsync(h->u, 0, sizeof(double) * D0.nvec, g_ctx.stream));
    }
    HIPCK(hipStreamSynchronize(g_ctx.stream));
    return FASP_SUCCESS;
}

int fasp_hip_get_solution(fasp_hip_amg* h, dvector* x)
{
    FASP_ENTRY();
    if (!h || !x || h->L.empty()) return ERROR_INPUT_PAR;
    const DevLevel& D0 = h->L[0];
    if (x->row != D0.nglobal) return ERROR_MAT_SIZE;  // a rank fills the rows it owns
    HIPCK(hipMemcpyAsync(x->val + D0.row0, h->u, sizeof(double) * D0.nloc, hipMemcpyDeviceToHost, g_ctx.stream));
    HIPCK(hipStreamSynchronize(g_ctx.stream));
    return FASP_SUCCESS;
}

int fasp_hip_device_synchronize(void)
{
    FASP_ENTRY();
    if (!g_ctx.ready) return FASP_SUCCESS;
    HIPCK(hipStreamSynchronize(g_ctx.stream));
    return FASP_SUCCESS;
}

int fasp_hip_solve_resident(fasp_hip_amg* h, const ITS_param* itparam, double* hist, int hist_cap,
                            fasp_hip_stats* stats)
{
    FASP_ENTRY();
    if (!h || !itparam) return ERROR_INPUT_PAR;
    if (h->L.empty()) return ERROR_INPUT_PAR;  // hierarchy not uploaded
    int st = check_supported(itparam, &h->param);
    if (st < 0) return st;
    its_check(itparam->tol, itparam->maxit);

    h->ev_used = 0;
    h->use_fmg = itparam->precond_type == PREC_FMG;   // SolCSR.c:537-538
    const long long ci0 = h->coarse_iters, vc0 = h->vcycles;
    Hist   H{hist, hist_cap, 0};
    PcgOut po{BIGREAL, BIGREAL, BIGREAL};
    const double t0 = wall_seconds();
    // SolCSR.c:530-551: the AMG preconditioner is always installed on this path;
    // SolCSR.c:84-130: dispatch on itsolver_type (restart is narrowed to SHORT, :62); check_supported let only known types pass
    {
        KOps K = csr_ops(h, 0, true);
        const KParams P{itparam->tol, itparam->abstol, itparam->maxit, (short)itparam->restart, itparam->stop_type, itparam->print_level};
        st = krylov_run(K, (KMethod)itparam->itsolver_type, K_OFFER_ALL, false, P, h->b, h->u, h->p, h->t, h->r, &H, &po);
    }
    HIPCK(hipStreamSynchronize(g_ctx.stream));
    if (seq_err_check() < 0) return ERROR_MISC;   // a broken cluster of the sequential smoothers (smoothers.hip.h)
    const double t_solve = wall_seconds() - t0;

    if (stats) {
        stats->iters = st; stats->nhist = H.n; stats->relres = po.relres; stats->absres = po.absres;
        stats->normr0 = po.normr0; stats->solve_seconds = t_solve; stats->upload_seconds = 0.0;
        double ms = 0.0;
        for (int i = 0; i < h->ev_used; ++i) {
            float e = 0.f;
            if (hipEventElapsedTime(&e, h->ev[i].a, h->ev[i].b) == hipSuccess) ms += e;
        }
        stats->spmv_launches = h->ev_used;
        stats->spmv_ms = h->ev_used ? ms / h->ev_used : 0.0;
        stats->coarse_iters = h->coarse_iters - ci0;
        stats->vcycles = h->vcycles - vc0;
    }
    print_itsolver_time(itparam->print_level, st, t_solve);
    return st;
}

int fasp_hip_solve(fasp_hip_amg* h, const dvector* b, dvector* x, const ITS_param* itparam, double* hist,
                   int hist_cap, fasp_hip_stats* stats)
{
    FASP_ENTRY();
    if (!h || !b || !x || !itparam) return ERROR_INPUT_PAR;
    double t0 = wall_seconds();
    int st = fasp_hip_set_rhs(h, b);
    if (st < 0) return st;
    if ((st = fasp_hip_set_guess(h, x)) < 0) return st;
    double t_up = wall_seconds() - t0;
    st = fasp_hip_solve_resident(h, itparam, hist, hist_cap, stats);
    t0 = wall_seconds();
    const int st2 = fasp_hip_get_solution(h, x);
    if (st2 < 0) return st2;
    t_up += wall_seconds() - t0;
    if (stats) stats->upload_seconds = t_up;
    return st;
}

// AMG as a stand-alone solver on a resident hierarchy (PreMGSolve.c:49); param == NULL: the
// parameters the hierarchy was built with
int fasp_hip_amg_solve(fasp_hip_amg* h, const dvector* b, dvector* x, const AMG_param* param, double* hist,
                       int hist_cap, fasp_hip_stats* stats)
{
    FASP_ENTRY();
    if (!h || !b || !x || h->L.empty()) return ERROR_INPUT_PAR;
    const AMG_param& p = param ? *param : h->param;
    int st = check_supported(nullptr, &p);
    if (st < 0) return st;
    double t0 = wall_seconds();
    if ((st = fasp_hip_set_rhs(h, b)) < 0) return st;
    if ((st = fasp_hip_set_guess(h, x)) < 0) return st;
    double t_up = wall_seconds() - t0;
    h->ev_used = 0;
    const long long ci0 = h->coarse_iters, vc0 = h->vcycles;
    Hist   H{hist, hist_cap, 0};
    PcgOut po{BIGREAL, BIGREAL, BIGREAL};
    t0 = wall_seconds();
    st = amg_solve_device(h, p, H, po);
    const double t_solve = wall_seconds() - t0;
    t0 = wall_seconds();
    const int st2 = fasp_hip_get_solution(h, x);
    if (st2 < 0) return st2;
    t_up += wall_seconds() - t0;
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->iters = st; stats->nhist = H.n; stats->relres = po.relres; stats->absres = po.absres;
        stats->normr0 = po.normr0; stats->solve_seconds = t_solve; stats->upload_seconds = t_up;
        stats->coarse_iters = h->coarse_iters - ci0;
        stats->vcycles = h->vcycles - vc0;
    }
    if (p.print_level > PRINT_NONE) std::printf("AMG solve costs %.4f seconds.\n", t_solve);
    return st;
}

// SolAMG.c:49.  A failed setup returns its error code (the reference would fall back to an
// unpreconditioned CPU GMRES there; this library has no CPU solve path).
int fasp_solver_amg(dCSRmat* A, dvector* b, dvector* x, AMG_param* param)
{
    FASP_ENTRY();
    if (!A || !b || !x || !param) return ERROR_INPUT_PAR;
    const double t0 = wall_seconds();
    int st = check_supported(nullptr, param);
    if (st < 0) return st;
    fasp_hip_amg* h = nullptr;
    g_oneshot_upload = std::getenv("FASP_HIP_ONESHOT_CODING") == nullptr;
    st = fasp_hip_amg_create(&h, A, param);
    g_oneshot_upload = false;
    if (st < 0) return st;
    st = fasp_hip_amg_solve(h, b, x, param, nullptr, 0, nullptr);
    if (param->print_level > PRINT_NONE) std::printf("AMG totally costs %.4f seconds.\n", wall_seconds() - t0);
    fasp_hip_amg_destroy(h);
    return st;
}

// SolFAMG.c:41 -> fasp_famg_solve (PreMGSolve.c:300): ONE full-multigrid cycle as the solver; x is the
// initial guess of the finest level and receives the result.  void in the reference; the status is an extension.
int fasp_solver_famg(const dCSRmat* A, const dvector* b, dvector* x, AMG_param* param)
{
    FASP_ENTRY();
    if (!A || !b || !x || !param) return ERROR_INPUT_PAR;
    const double t0 = wall_seconds();
    int st = check_supported(nullptr, param);
    if (st < 0) return st;
    fasp_hip_amg* h = nullptr;
    g_oneshot_upload = std::getenv("FASP_HIP_ONESHOT_CODING") == nullptr;
    st = fasp_hip_amg_create(&h, A, param);
    g_oneshot_upload = false;
    if (st < 0) return st;
    if ((st = fasp_hip_set_rhs(h, b)) >= 0 && (st = fasp_hip_set_guess(h, x)) >= 0) {
        DevLevel& D0 = h->L[0];
        const int m = D0.A.row;
        double red[2];
        D0.b = h->b;
        (void)hipMemcpyAsync(D0.x, h->u, sizeof(double) * m, hipMemcpyDeviceToDevice, g_ctx.stream);
        D0.x_zero = false;
        st = d_dot(m, h->b, h->b, red, false) < 0 ? ERROR_MISC : FASP_SUCCESS;
        const double sumb = std::sqrt(red[0]);
        if (st >= 0 && sumb <= SMALLREAL) (void)hipMemsetAsync(D0.x, 0, sizeof(double) * m, g_ctx.stream);
        if (st >= 0) st = fmg_cycle(h, *param);
        if (st >= 0) {
            d_resid(D0.A, D0.x, D0.b, D0.w);
            if (d_dot(m, D0.w, D0.w, red, false) < 0) st = ERROR_MISC;
            else if (param->print_level > PRINT_NONE)
                std::printf("FMG finishes with relative residual %e.\n", std::sqrt(red[0]) / std::max(SMALLREAL, sumb));
            (void)hipMemcpyAsync(h->u, D0.x, sizeof(double) * m, hipMemcpyDeviceToDevice, g_ctx.stream);
            const int st2 = fasp_hip_get_solution(h, x);
            if (st2 < 0) st = st2;
        }
    }
    if (param->print_level > PRINT_NONE) std::printf("FAMG totally costs %.4f seconds.\n", wall_seconds() - t0);
    fasp_hip_amg_destroy(h);
    return st;
}

int fasp_hip_precond_amg(fasp_hip_amg* h, const double* r, double* z)
{
    FASP_ENTRY();
    if (!h || !r || !z || h->L.empty()) return ERROR_INPUT_PAR;
    const int m = h->L[0].nloc;
    r += h->L[0].row0; z += h->L[0].row0;  // global host vectors, own rows
    HIPCK(hipMemcpyAsync(h->r, r, sizeof(double) * m, hipMemcpyHostToDevice, g_ctx.stream));
    double* dz = nullptr;
    const int st = precond_amg(h, h->r, &dz);
    if (st < 0) return st;
    HIPCK(hipMemcpyAsync(z, dz, sizeof(double) * m, hipMemcpyDeviceToHost, g_ctx.stream));
    HIPCK(hipStreamSynchronize(g_ctx.stream));
    return seq_err_check();
}

// ---- row-partition inspection (host only; used by the CPU-side distributed tests) ----
int fasp_hip_dist_plan(fasp_hip_amg* h, int rank, int nranks, int min_rows)
{
    FASP_ENTRY();
    if (!h) return ERROR_INPUT_PAR;
    return build_dist_plan(h->H, rank, nranks, min_rows, h->dist);
}

int fasp_hip_dist_level_info(const fasp_hip_amg* h, int level, int* info)
{
    FASP_ENTRY();
    if (!h || !info || level < 0 || level >= (int)h->dist.L.size()) return ERROR_INPUT_PAR;
    const DistLevel& D = h->dist.L[level];
    info[0] = D.replicated; info[1] = D.nglobal; info[2] = D.row0; info[3] = D.nloc;
    info[4] = (int)D.ghosts.size(); info[5] = (int)D.send_idx.size();
    info[6] = h->dist.first_replicated; info[7] = h->dist.nranks;
    return FASP_SUCCESS;
}

int fasp_hip_dist_get_matrix(const fasp_hip_amg* h, int level, int which, dCSRmat* view)
{
    FASP_ENTRY();
    if (!h || !view || level < 0 || level >= (int)h->dist.L.size()) return ERROR_INPUT_PAR;
    const DistLevel& D = h->dist.L[level];
    if (D.replicated) return fasp_hip_amg_get_matrix(h, level, which, view);
    const HostCSR& M = which == 0 ? D.A : which == 1 ? D.P : D.R;
    if (!M.ia.data()) return ERROR_INPUT_PAR;
    *view = M.view();
    return FASP_SUCCESS;
}

int fasp_hip_dist_get_list(const fasp_hip_amg* h, int level, int which, ivector* view)
{
    FASP_ENTRY();
    if (!h || !view || level < 0 || level >= (int)h->dist.L.size()) return ERROR_INPUT_PAR;
    const DistLevel& D = h->dist.L[level];
    if (which >= 5 && which <= 7) {   // interior window [lo, hi) of the local A (5), P (6), R (7); hi < 0: none
        const int* w = which == 5 ? D.winA : which == 6 ? D.winP : D.winR;
        view->row = 2;
        view->val = const_cast<int*>(w);
        return FASP_SUCCESS;
    }
    const std::vector<int>* v = which == 0 ? &D.ghosts : which == 1 ? &D.recv_off : which == 2 ? &D.send_off
                              : which == 3 ? &D.send_idx : which == 4 ? &D.start : nullptr;
    if (!v) return ERROR_INPUT_PAR;
    view->row = (int)v->size();
    view->val = const_cast<int*>(v->data());
    return FASP_SUCCESS;
}

// SolCSR.c:476 -- the drop-in entry point
int fasp_solver_dcsr_krylov_amg(dCSRmat* A, dvector* b, dvector* x, ITS_param* itparam, AMG_param* amgparam)
{
    FASP_ENTRY();
    if (!A || !b || !x || !itparam || !amgparam) return ERROR_INPUT_PAR;
    const double t0 = wall_seconds();
    int st = check_supported(itparam, amgparam);
    if (st < 0) return st;
    fasp_hip_amg* h = nullptr;
    g_oneshot_upload = std::getenv("FASP_HIP_ONESHOT_CODING") == nullptr;  // (set the variable to keep the coding)
    st = fasp_hip_amg_create(&h, A, amgparam);
    g_oneshot_upload = false;
    if (st < 0) return st;
    st = fasp_hip_solve(h, b, x, itparam, nullptr, 0, nullptr);
    if (itparam->print_level >= PRINT_MIN)
        std::printf("AMG_Krylov method totally costs %.4f seconds.\n", wall_seconds() - t0);
    fasp_hip_amg_destroy(h);
    return st;
}

// ---------------------------------------------------------------------------
// BSR path: resident hierarchy + the drop-in of SolBSR.c:349
// ---------------------------------------------------------------------------
void fasp_hip_bsr_amg_destroy(fasp_hip_amg_bsr* h)
{
    FASP_ENTRY();
    if (!h) return;
    if (g_ctx.ready) (void)hipStreamSynchronize(g_ctx.stream);
    for (auto& Lv : h->L) {
        double* v[] = {Lv.dinv, Lv.b, Lv.x, Lv.x2, Lv.w};
        for (double* q : v) if (q) (void)hipFree(q);
        for (auto& sc : Lv.sched) sc.release();
        if (Lv.d_send_idx) (void)hipFree(Lv.d_send_idx);
        if (Lv.d_sendbuf) (void)hipFree(Lv.d_sendbuf);
        ilu_dev_destroy(Lv.ilu);
        bsr_level_sweeps_destroy(Lv);
    }
    double* v[] = {h->b, h->u, h->p, h->t, h->r};
    for (double* q : v) if (q) (void)hipFree(q);
    if (h->small_ws) (void)hipFree(h->small_ws);
    delete h;
}

// host part only (no GPU needed): the hierarchy can be inspected, not solved with
int fasp_hip_bsr_amg_create_host(fasp_hip_amg_bsr** out, const dBSRmat* A, AMG_param* amgparam)
{
    FASP_ENTRY();
    if (!out || !A || !amgparam) return ERROR_INPUT_PAR;
    *out = nullptr;
    int st = check_supported_bsr(nullptr, amgparam, A->nb);
    if (st < 0) return st;
    fasp_hip_amg_bsr* h = new fasp_hip_amg_bsr();
    st = host_setup_ua_bsr(A, amgparam, h->H);
    if (st < 0) { delete h; return st; }
    h->param = *amgparam;
    *out = h;
    return FASP_SUCCESS;
}

int fasp_hip_bsr_amg_create(fasp_hip_amg_bsr** out, const dBSRmat* A, AMG_param* amgparam)
{
    FASP_ENTRY();
    if (!out || !A || !amgparam) return ERROR_INPUT_PAR;
    *out = nullptr;
    int st = check_supported_bsr(nullptr, amgparam, A->nb);
    if (st < 0) return st;
    if ((st = ctx_init()) < 0) return st;
    if (amgparam->ILU_levels > 0 && comm_size() > 1) {   // a triangular solve couples all rows of a level
        std::printf("### ERROR: fasp_hip: ILU smoothing (ILU_levels > 0) has no multi-GPU path\n");
        return ERROR_INPUT_PAR;
    }
    fasp_hip_amg_bsr* h = nullptr;
    if ((st = fasp_hip_bsr_amg_create_host(&h, A, amgparam)) < 0) return st;
    const int nl = (int)h->H.L.size();
    h->L.resize(nl);
    // one process per GPU: block rows partitioned over the ranks (dist_plan.cpp, build_dist_plan_bsr); levels below
    // FASP_HIP_DIST_MIN_ROWS block rows -- and always the coarsest one -- are kept whole on every rank.  Block Gauss-Seidel /
    // SOR sweeps couple all rows: such hierarchies stay whole.
    std::vector<DistLocalBSR> local;
    if (comm_size() > 1) {
        int min_rows = 200000;
        if (const char* e = std::getenv("FASP_HIP_DIST_MIN_ROWS")) min_rows = std::atoi(e);
        if (h->param.smoother != SMOOTHER_JACOBI) min_rows = 2147483647;
        min_rows = std::max(min_rows, h->H.L[(size_t)nl - 1].A.ROW + 1);
        HostThreads team;
        if ((st = build_dist_plan_bsr(h->H, comm_rank(), comm_size(), min_rows, h->dist, local)) < 0) { fasp_hip_bsr_amg_destroy(h); return st; }
        h->distributed = !h->dist.L[0].replicated;
    }
    for (int l = 0; l < nl; ++l) {
        const HostLevelBSR& HL = h->H.L[l];
        BsrLevel& Lv = h->L[l];
        const int nb = HL.A.nb, nb2 = nb * nb;
        const DistLevel* DL = (comm_size() > 1 && !h->dist.L[(size_t)l].replicated) ? &h->dist.L[(size_t)l] : nullptr;
        Lv.replicated = DL == nullptr;
        Lv.nglobal = HL.A.ROW;
        Lv.row0 = DL ? DL->row0 : 0; Lv.nloc = DL ? DL->nloc : HL.A.ROW; Lv.nghost = DL ? (int)DL->ghosts.size() : 0;
        const dBSRmat vA = DL ? local[(size_t)l].A.view() : HL.A.view();
        Lv.A.reset(new TmpBSR(&vA));
        bool ok = Lv.A->ok;
        Lv.n = Lv.nloc * nb;
        Lv.nv = (Lv.nloc + Lv.nghost) * nb;
        if (HL.has_coarse) {
            const dBSRmat vP = DL ? local[(size_t)l].P.view() : HL.P.view(), vR = DL ? local[(size_t)l].R.view() : HL.R.view();
            Lv.P.reset(new TmpBSR(&vP));
            Lv.R.reset(new TmpBSR(&vR));
            ok = ok && Lv.P->ok && Lv.R->ok;
            const size_t nd = (size_t)Lv.nloc * nb2;
            if (hipMalloc(&Lv.dinv, sizeof(double) * std::max<size_t>(nd, 1)) != hipSuccess) ok = false;
            else (void)hipMemcpy(Lv.dinv, HL.diaginv.data() + (size_t)Lv.row0 * nb2, sizeof(double) * nd, hipMemcpyHostToDevice);
        }
        if (ok && HL.LU && !DL) {   // the level's factor, resident with the hierarchy (not through the host-pointer registry)
            int ist;
            Lv.ilu = ilu_upload(&HL.LU->d, nb, &ist);
            if (!Lv.ilu) { fasp_hip_bsr_amg_destroy(h); return ist < 0 ? ist : ERROR_ALLOC_MEM; }
        }
        if (ok && DL) {   // halo lists, expanded from blocks to scalars
            const int P = comm_size();
            Lv.send_off.assign((size_t)P + 1, 0); Lv.recv_off.assign((size_t)P + 1, 0);
            for (int q = 0; q <= P; ++q) { Lv.send_off[(size_t)q] = DL->send_off[(size_t)q] * nb; Lv.recv_off[(size_t)q] = DL->recv_off[(size_t)q] * nb; }
            std::vector<int> sidx(DL->send_idx.size() * (size_t)nb);
            for (size_t i = 0; i < DL->send_idx.size(); ++i)
                for (int c = 0; c < nb; ++c) sidx[i * nb + c] = DL->send_idx[i] * nb + c;
            if (hipMalloc(&Lv.d_send_idx, sizeof(int) * std::max<size_t>(sidx.size(), 1)) != hipSuccess ||
                hipMalloc(&Lv.d_sendbuf, sizeof(double) * std::max<size_t>(sidx.size(), 1)) != hipSuccess) ok = false;
            else if (!sidx.empty()) (void)hipMemcpy(Lv.d_send_idx, sidx.data(), sizeof(int) * sidx.size(), hipMemcpyHostToDevice);
        }
        if (!ok || dalloc(&Lv.b, Lv.nv) < 0 || dalloc(&Lv.x, Lv.nv) < 0 || dalloc(&Lv.x2, Lv.nv) < 0 ||
            dalloc(&Lv.w, Lv.nv) < 0) {
            fasp_hip_bsr_amg_destroy(h);
            return ERROR_ALLOC_MEM;
        }
    }
    const size_t n0 = (size_t)h->L[0].nv;
    if (dalloc(&h->b, n0) < 0 || dalloc(&h->u, n0) < 0 || dalloc(&h->p, n0) < 0 || dalloc(&h->t, n0) < 0 ||
        dalloc(&h->r, n0) < 0) {
        fasp_hip_bsr_amg_destroy(h);
        return ERROR_ALLOC_MEM;
    }
    HIPCK(hipStreamSynchronize(g_ctx.stream));
    *out = h;
    return FASP_SUCCESS;
}

// block rows of level 0 this rank owns: info[0] = 1 if the level is whole on every rank, [1] first owned block row,
// [2] owned block rows, [3] ghost blocks, [4] first level kept whole, [5] block size
int fasp_hip_bsr_dist_info(const fasp_hip_amg_bsr* h, int* info)
{
    FASP_ENTRY();
    if (!h || !info || h->L.empty()) return ERROR_INPUT_PAR;
    const BsrLevel& L0 = h->L[0];
    int first_rep = 0;
    while (first_rep < (int)h->L.size() && !h->L[(size_t)first_rep].replicated) ++first_rep;
    info[0] = L0.replicated ? 1 : 0; info[1] = L0.row0; info[2] = L0.nloc; info[3] = L0.nghost; info[4] = first_rep; info[5] = L0.A->nb;
    return FASP_SUCCESS;
}

int fasp_hip_bsr_amg_num_levels(const fasp_hip_amg_bsr* h) { return h ? (int)h->H.L.size() : ERROR_INPUT_PAR; }

int fasp_hip_bsr_amg_get_matrix(const fasp_hip_amg_bsr* h, int level, int which, dBSRmat* view)
{
    FASP_ENTRY();
    if (!h || !view || level < 0 || level >= (int)h->H.L.size()) return ERROR_INPUT_PAR;
    const HostLevelBSR& L = h->H.L[level];
    if (which != 0 && !L.has_coarse) return ERROR_INPUT_PAR;
    *view = which == 0 ? L.A.view() : which == 1 ? L.P.view() : L.R.view();
    return FASP_SUCCESS;
}

const double* fasp_hip_bsr_amg_get_diaginv(const fasp_hip_amg_bsr* h, int level)
{
    FASP_ENTRY();
    if (!h || level < 0 || level >= (int)h->H.L.size() || !h->H.L[level].has_coarse) return nullptr;
    return h->H.L[level].diaginv.data();
}

int fasp_hip_bsr_solve(fasp_hip_amg_bsr* h, const dvector* b, dvector* x, const ITS_param* itparam, double* hist,
                       int hist_cap, fasp_hip_stats* stats)
{
    FASP_ENTRY();
    if (!h || !b || !x || !itparam || h->L.empty()) return ERROR_INPUT_PAR;
    const int n = h->L[0].n;                                    // owned scalar rows
    const int nglob = h->L[0].nglobal * h->H.L[0].A.nb;          // b and x are the GLOBAL vectors: a rank reads / fills its rows
    const size_t off0 = (size_t)h->L[0].row0 * h->H.L[0].A.nb;
    if (b->row != nglob || x->row != nglob) return ERROR_MAT_SIZE;
    int st = check_supported_bsr(itparam, &h->param, h->H.L[0].A.nb);
    if (st < 0) return st;
    its_check(itparam->tol, itparam->maxit);
    hipStream_t s = g_ctx.stream;
    double t0 = wall_seconds();
    HIPCK(hipMemcpyAsync(h->b, b->val + off0, sizeof(double) * n, hipMemcpyHostToDevice, s));
    HIPCK(hipMemcpyAsync(h->u, x->val + off0, sizeof(double) * n, hipMemcpyHostToDevice, s));
    HIPCK(hipStreamSynchronize(s));
    double t_up = wall_seconds() - t0;

    const long long ci0 = h->coarse_iters, vc0 = h->vcycles;
    Hist   H{hist, hist_cap, 0};
    PcgOut po{BIGREAL, BIGREAL, BIGREAL};
    t0 = wall_seconds();
    KOps K = bsr_ops(h, 0, 0);
    const KParams P{itparam->tol, itparam->abstol, itparam->maxit, (short)itparam->restart, itparam->stop_type, itparam->print_level};
    st = krylov_run(K, (KMethod)itparam->itsolver_type, K_OFFER_BSR, false, P, h->b, h->u, h->p, h->t, h->r, &H, &po);   // fasp_solver_dbsr_itsolver, SolBSR.c:55-150
    HIPCK(hipStreamSynchronize(s));
    const double t_solve = wall_seconds() - t0;
    t0 = wall_seconds();
    HIPCK(hipMemcpy(x->val + off0, h->u, sizeof(double) * n, hipMemcpyDeviceToHost));
    t_up += wall_seconds() - t0;
    if (h->L[0].ilu && st >= 0 && seq_err_check() < 0) st = ERROR_MISC;   // a single-launch ILU solve of the cycle that timed out
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->iters = st; stats->nhist = H.n; stats->relres = po.relres; stats->absres = po.absres;
        stats->normr0 = po.normr0; stats->solve_seconds = t_solve; stats->upload_seconds = t_up;
        stats->coarse_iters = h->coarse_iters - ci0;
        stats->vcycles = h->vcycles - vc0;
    }
    print_itsolver_time(itparam->print_level, st, t_solve);
    return st;
}

// SolBSR.c:349: UA-AMG setup on the host, hierarchy uploaded, Krylov loop on the device
int fasp_solver_dbsr_krylov_amg(dBSRmat* A, dvector* b, dvector* x, ITS_param* itparam, AMG_param* amgparam)
{
    FASP_ENTRY();
    if (!A || !b || !x || !itparam || !amgparam) return ERROR_INPUT_PAR;
    const double t0 = wall_seconds();
    int st = check_supported_bsr(itparam, amgparam, A->nb);
    if (st < 0) return st;
    fasp_hip_amg_bsr* h = nullptr;
    st = fasp_hip_bsr_amg_create(&h, A, amgparam);
    if (st < 0) return st;
    st = fasp_hip_bsr_solve(h, b, x, itparam, nullptr, 0, nullptr);
    if (itparam->print_level >= PRINT_MIN)
        std::printf("AMG_Krylov method totally costs %.4f seconds.\n", wall_seconds() - t0);
    fasp_hip_bsr_amg_destroy(h);
    return st;
}

// ---------------------------------------------------------------------------
// kernel-level operators with host pointers (reference names, device kernels)
// ---------------------------------------------------------------------------
namespace {
struct TmpCSR {
    DevCSR D;
    bool   ok = false;
    explicit TmpCSR(const dCSRmat* A)
    {
        if (ctx_init() < 0) return;
        D.row = A->row; D.col = A->col; D.nnz = A->nnz;
        if (hipMalloc(&D.ia, sizeof(int) * ((size_t)A->row + 1)) != hipSuccess) return;
        if (hipMalloc(&D.ja, sizeof(int) * std::max(A->nnz, 1)) != hipSuccess) return;
        if (hipMalloc(&D.val, sizeof(double) * std::max(A->nnz, 1)) != hipSuccess) return;
        (void)hipMemcpy(D.ia, A->IA, sizeof(int) * ((size_t)A->row + 1), hipMemcpyHostToDevice);
        (void)hipMemcpy(D.ja, A->JA, sizeof(int) * (size_t)A->nnz, hipMemcpyHostToDevice);
        (void)hipMemcpy(D.val, A->val, sizeof(double) * (size_t)A->nnz, hipMemcpyHostToDevice);
        pick_kernel(D);
        ok = true;
    }
    ~TmpCSR() { D.release(); }
};
struct TmpVec {
    double* d = nullptr;
    size_t  n;
    TmpVec(const double* h, size_t n_) : n(n_)
    {
        if (hipMalloc(&d, sizeof(double) * std::max<size_t>(n, 1)) != hipSuccess) { d = nullptr; return; }
        if (h) (void)hipMemcpy(d, h, sizeof(double) * n, hipMemcpyHostToDevice);
    }
    void get(double* h) { (void)hipStreamSynchronize(g_ctx.stream); (void)hipMemcpy(h, d, sizeof(double) * n, hipMemcpyDeviceToHost); }
    ~TmpVec() { if (d) (void)hipFree(d); }
};
[[noreturn]] void die_no_device(const char* fn)
{
    std::fprintf(stderr, "### ERROR: %s: no usable HIP device and no CPU fallback in libfasp_hip\n", fn);
    std::exit(ERROR_MISC);
}
}  // namespace

// ---------------------------------------------------------------------------
// plug-in level of the reference: the Krylov methods with a caller
// supplied `precond` (fasp.h:1095), and the AMG preconditioner as such a plug-in
// ---------------------------------------------------------------------------
// PreCSR.c:416 signature: z = B r, host vectors; data is the fasp_hip_amg* of fasp_hip_precond_setup
void fasp_hip_precond_fct(double* r, double* z, void* data)
{
    FASP_ENTRY();
    fasp_hip_amg* h = static_cast<fasp_hip_amg*>(data);
    if (fasp_hip_precond_amg(h, r, z) < 0) {
        std::fprintf(stderr, "### ERROR: fasp_hip_precond_fct: device preconditioner failed\n");
        std::exit(ERROR_MISC);
    }
}

// PreCSR.c:46 for PREC_AMG: hierarchy built and uploaded once, handed out as a `precond`
precond* fasp_hip_precond_setup(dCSRmat* A, AMG_param* amgparam)
{
    FASP_ENTRY();
    fasp_hip_amg* h = nullptr;
    if (fasp_hip_amg_create(&h, A, amgparam) < 0) return nullptr;
    precond* pc = static_cast<precond*>(std::calloc(1, sizeof(precond)));
    pc->data = h;
    pc->fct = fasp_hip_precond_fct;
    return pc;
}

#include "precond_api.hip.h"
#include "ilu.hip.h"
#include "bsr_sweep.hip.h"
#include "rap.hip.h"

void fasp_hip_precond_free(precond* pc)
{
    FASP_ENTRY();
    if (!pc) return;
    if (pc->fct == fasp_hip_precond_fct) fasp_hip_amg_destroy(static_cast<fasp_hip_amg*>(pc->data));
    std::free(pc);
}

namespace {
bool same_host_matrix(const HostCSR& M, const dCSRmat* A)
{
    return M.row == A->row && M.col == A->col && M.nnz == A->nnz &&
           std::memcmp(M.ia.data(), A->IA, sizeof(int) * ((size_t)A->row + 1)) == 0 &&
           std::memcmp(M.ja.data(), A->JA, sizeof(int) * (size_t)A->nnz) == 0 &&
           std::memcmp(M.val.data(), A->val, sizeof(double) * (size_t)A->nnz) == 0;
}

// ---------------------------------------------------------------------------
// The plug-in driver: every Krylov entry point with a caller's `precond` -- CSR (SolCSR.c), BSR (SolBSR.c) and
// structured (SolSTR.c) and matrix-free (SolMatFree.c) -- is this one function.  What the families do differently is a KFamily.
// ---------------------------------------------------------------------------
struct PcState;
// Each field mirrors what the family's own function did before the three were merged; none of them is a choice made here.
struct KFamily {
    const char* fmt;             // K.fmt, the "(%s)" of the solvers' first line: "CSR" / "BSR" / "STR" / "MatFree", as today
    bool ctx_first;              // ctx_init() before the argument checks, failure -> die_no_device (BSR: after them, via TmpBSR)
    bool bad_bsr_dies;           // a BSR operator that cannot be uploaded -> die_bsr (matrix-free: ERROR_ALLOC_MEM), as today
    bool refuse_multi_rank;      // comm_size() > 1 -> ERROR_INPUT_PAR; the BSR family has never checked
    bool refuse_empty;           // b->row <= 0 -> ERROR_INPUT_PAR; only the matrix-free family checks, as today
    int  (*find_amg)(precond*, int n, PcState&);   // which `precond`s are a device AMG handle; < 0: one of another size
    bool borrow_resident;        // same_host_matrix: solve on the handle's resident level-0 operator (CSR only, as today)
    bool fused_mxv_dot;          // K.mxv_dot for a CSR operator (CSR only; the matrix-free texts never ask for it)
    bool (*bind_diag)(precond*, int n, int nb, PcState&, KOps&, int* st);   // (block-)diagonal preconditioner on the device (STR: its ILU factors too); none: host-staged
    IluDev* (*ilu_lookup)(precond*, int n, std::unique_ptr<IluDev, void (*)(IluDev*)>&, int* which, int* st);
    bool handle_ilu_checked;     // seq_err_check() also when the handle's level 0 smooths with ILU (BSR handles only, as today)
    bool mf_texts;               // the reference's older texts (pcg_mf_device, gmres_mf_device, minres_mf_device), as today
    unsigned offered;            // methods of the family
};

// what a bound preconditioner keeps alive for the length of the solve
struct PcState {
    fasp_hip_amg*     h = nullptr;    // recognised device AMG handle, scalar ...
    fasp_hip_amg_bsr* hb = nullptr;   // ... or block
    IluDev*           ilu = nullptr;
    std::unique_ptr<IluDev, void (*)(IluDev*)> ilu_tmp{nullptr, ilu_dev_destroy};
    std::unique_ptr<StrIluDev> strilu;   // structured ILU factor, uploaded for this solve
    std::unique_ptr<StrSwzDev> strswz;   // structured block Gauss-Seidel: the caller's factors, uploaded for this solve
    std::unique_ptr<TmpVec> ddiag, dz;   // device diagonal; output of the diagonal and of a foreign preconditioner
    std::vector<double> hr, hz;          // host staging of a foreign preconditioner
    double* out(int n) { if (!dz) dz.reset(new TmpVec(nullptr, (size_t)n)); return dz->d; }
};

int find_amg_csr(precond* pc, int n, PcState& S)   // fasp_hip_precond_fct or a reference-style fasp_precond_amg object
{
    S.h = (pc && pc->fct == fasp_hip_precond_fct) ? static_cast<fasp_hip_amg*>(pc->data) : amg_handle_of_precond(pc);
    return (S.h && (S.h->L.empty() || S.h->L[0].A.row != n)) ? ERROR_INPUT_PAR : FASP_SUCCESS;
}
int find_amg_matfree(precond* pc, int n, PcState& S)   // fasp_hip_precond_fct only
{
    S.h = (pc && pc->fct == fasp_hip_precond_fct) ? static_cast<fasp_hip_amg*>(pc->data) : nullptr;
    return (S.h && (S.h->L.empty() || S.h->L[0].A.row != n)) ? ERROR_INPUT_PAR : FASP_SUCCESS;
}
int find_amg_bsr(precond* pc, int n, PcState& S)
{
    S.hb = (pc && pc->fct == fasp_hip_bsr_precond_fct) ? static_cast<fasp_hip_amg_bsr*>(pc->data) : nullptr;
    return (S.hb && (S.hb->L.empty() || S.hb->L[0].n != n)) ? ERROR_INPUT_PAR : FASP_SUCCESS;
}
// the reference's diagonal preconditioner (PreCSR.c:172): recognised by its function pointer, applied on the device
bool bind_diag_csr(precond* pc, int n, int, PcState& S, KOps& K, int* st)
{
    if (!(pc && pc->fct == fasp_precond_diag && pc->data && static_cast<dvector*>(pc->data)->row == n)) return false;
    S.ddiag.reset(new TmpVec(static_cast<dvector*>(pc->data)->val, (size_t)n));
    const double* dd = S.ddiag->d;
    double* zz = S.out(n);
    if (!dd || !zz) { *st = ERROR_ALLOC_MEM; return true; }
    K.pc = [dd, zz, n](double* in, double** out) {
        hipLaunchKernelGGL(k_diag_precond, dim3(vec_grid(n)), dim3(BLOCK), 0, g_ctx.stream, n, dd, (const double*)in, zz);
        *out = zz;
        return 0;
    };
    return true;
}
// the reference's Schwarz preconditioner (PreCSR.c:371): recognised by its address.  The blocks of its SWZ_data are made resident at the
// first use (uploaded and factored on the device) and stay so until fasp_swz_data_free; per application z = 0 and the sweeps of SWZ_type,
// no host traffic.  Data the sweeps refuse ends the solve (ERROR_INPUT_PAR); data for another matrix size leaves it a foreign host function.
bool bind_swz_csr(precond* pc, int n, int, PcState&, KOps& K, int* st)
{
    if (!(pc && pc->data && pc->fct == fasp_precond_swz)) return false;
    const SWZ_data* d = static_cast<const SWZ_data*>(pc->data);
    if (d->A.row != n) return false;
    CsrSwzDev* M = csr_swz_device_of("fasp_precond_swz", d, st);
    if (!M) return true;
    if (csr_swz_refuse_stopped("fasp_precond_swz", *M) < 0) { *st = ERROR_INPUT_PAR; return true; }
    const int type = d->SWZ_type;
    K.pc = [M, type](double* in, double** out) { *out = M->x; return M->precond(type, in, M->x); };
    return true;
}
// the CSR family's device preconditioners besides its ILU and AMG: Schwarz and the diagonal
bool bind_pc_csr(precond* pc, int n, int nb, PcState& S, KOps& K, int* st)
{
    return bind_swz_csr(pc, n, nb, S, K, st) || bind_diag_csr(pc, n, nb, S, K, st);
}
// block-diagonal preconditioner of the reference (PreBSR.c:49): z_i = Dinv_i r_i on the device
bool bind_diag_bsr(precond* pc, int n, int nb, PcState& S, KOps& K, int* st)
{
    if (!(pc && pc->fct == fasp_precond_dbsr_diag && pc->data && static_cast<precond_diag_bsr*>(pc->data)->diag.row == n * nb)) return false;
    S.ddiag.reset(new TmpVec(static_cast<precond_diag_bsr*>(pc->data)->diag.val, (size_t)n * nb));
    const double* dd = S.ddiag->d;
    double* zz = S.out(n);
    if (!dd || !zz) { *st = ERROR_ALLOC_MEM; return true; }
    K.pc = [dd, zz, n, nb](double* in, double** out) {
        hipLaunchKernelGGL(k_bsr_dinv_apply, dim3(vec_grid(n)), dim3(BLOCK), 0, g_ctx.stream, n, nb, dd, (const double*)in, zz);
        *out = zz;
        return 0;
    };
    return true;
}
// block-diagonal preconditioner of a structured matrix (PreSTR.c:44): z_i = Dinv_i r_i on the device
bool bind_diag_str(precond* pc, int n, int nc, PcState& S, KOps& K, int* st)
{
    if (!(pc && pc->fct == fasp_precond_dstr_diag && pc->data)) return false;
    const precond_diag_str* d = static_cast<const precond_diag_str*>(pc->data);
    if (d->nc != nc || d->diag.row != n * nc || !d->diag.val) return false;
    S.ddiag.reset(new TmpVec(d->diag.val, (size_t)n * nc));
    const double* dd = S.ddiag->d;
    double* zz = S.out(n);
    if (!dd || !zz) { *st = ERROR_ALLOC_MEM; return true; }
    K.pc = [dd, zz, n, nc](double* in, double** out) {
        hipLaunchKernelGGL(k_str_dinv_apply, dim3(vec_grid(n)), dim3(BLOCK), 0, g_ctx.stream, n, nc, dd, (const double*)in, zz);
        *out = zz;
        return 0;
    };
    return true;
}
// the reference's structured ILU preconditioners (PreSTR.c:71 / :349): recognised by their address; a factor of the operator's ngrid
// and nc that passes str_ilu_describe is uploaded once and both triangular solves run on the device (str_ilu.hip.h).  Anything
// else about such a `precond` (another size, a coefficient between points that are no geometric neighbours) leaves it a foreign
// host function: staged, correct and slow.
bool bind_ilu_str(precond* pc, int n, int nc, PcState& S, KOps& K, int* st)
{
    if (!(pc && pc->data && (pc->fct == fasp_precond_dstr_ilu0 || pc->fct == fasp_precond_dstr_ilu1))) return false;
    const dSTRmat* LU = static_cast<const dSTRmat*>(pc->data);
    StrIluDesc D;
    if (!str_ilu_describe(LU, pc->fct == fasp_precond_dstr_ilu1 ? 1 : 0, D, nullptr) || D.nc != nc || D.ngrid * D.nc != n) return false;
    S.strilu.reset(new StrIluDev(LU, D));
    if (!S.strilu->ok) { *st = ERROR_ALLOC_MEM; return true; }
    StrIluDev* M = S.strilu.get();
    K.pc = [M](double* in, double** out) { *out = M->z; return str_ilu_apply(*M, in, M->z); };
    return true;
}
// the reference's block Gauss-Seidel preconditioner (PreSTR.c:1715): recognised by its address.  Factors that live on the device already
// (fasp_solver_dstr_krylov_blockgs) are found through the address of the data; a caller's host factors are checked, repacked and uploaded once
// per solve.  Per application: z = 0 and one sweep, no host traffic.  Data the sweep refuses ends the solve (ERROR_INPUT_PAR), as the
// direct call would leave z untouched; data for another matrix size leaves it a foreign host function.
bool bind_blockgs_str(precond* pc, int n, int nc, PcState& S, KOps& K, int* st)
{
    if (!(pc && pc->data && pc->fct == fasp_precond_dstr_blockgs)) return false;
    const precond_data_str* d = static_cast<const precond_data_str*>(pc->data);
    if (!d->A_str || d->A_str->nc != nc || (long long)d->A_str->ngrid * nc != n) return false;
    StrSwzDev* M = str_swz_resident(pc->data);
    if (!M) {
        StrSwzPlan P;
        if (str_swz_plan("fasp_precond_dstr_blockgs", d->A_str, d->neigh, d->order, true, P) < 0 ||
            str_swz_check_factors("fasp_precond_dstr_blockgs", P, d->diaginv, d->pivot) < 0) { *st = ERROR_INPUT_PAR; return true; }
        S.strswz.reset(new StrSwzDev(d->A_str, std::move(P), d->diaginv, d->pivot));
        if (!S.strswz->ok) { *st = S.strswz->st; return true; }
        M = S.strswz.get();
    }
    K.pc = [M](double* in, double** out) { *out = M->u; return M->precond(in, M->u); };
    return true;
}
// the structured family's device preconditioners: its ILU factors (a format of their own: no IluDev) and the block diagonal
bool bind_pc_str(precond* pc, int n, int nc, PcState& S, KOps& K, int* st)
{
    return bind_ilu_str(pc, n, nc, S, K, st) || bind_blockgs_str(pc, n, nc, S, K, st) || bind_diag_str(pc, n, nc, S, K, st);
}
// the structured family knows no device AMG handle and no MSR factor (its ILU is bound by bind_ilu_str)
int find_amg_none(precond*, int, PcState&) { return FASP_SUCCESS; }
IluDev* ilu_lookup_none(precond*, int, std::unique_ptr<IluDev, void (*)(IluDev*)>&, int* which, int* st) { *which = -1; *st = FASP_SUCCESS; return nullptr; }
constexpr unsigned K_OFFER_STR = kbit(K_CG) | kbit(K_BiCGstab) | kbit(K_GMRES) | kbit(K_VGMRES) | kbit(K_MinRes);

//                              fmt        ctx_first bad_bsr_dies refuse_multi_rank refuse_empty find_amg          borrow_resident fused_mxv_dot bind_diag      ilu_lookup          handle_ilu_checked mf_texts offered
const KFamily FAMILY_CSR     = {"CSR",     true,     false,       true,             false,       find_amg_csr,     true,           true,         bind_pc_csr,   ilu_of_precond,     false,             false,   K_OFFER_ALL | K_OFFER_SAFE_CSR};
const KFamily FAMILY_BSR     = {"BSR",     false,    true,        false,            false,       find_amg_bsr,     false,          false,        bind_diag_bsr, ilu_of_precond_bsr, true,              false,   K_OFFER_BSR | K_OFFER_SAFE_BSR};
const KFamily FAMILY_STR     = {"STR",     true,     false,       true,             false,       find_amg_none,    false,          false,        bind_pc_str,   ilu_lookup_none,    false,             false,   K_OFFER_STR | K_OFFER_SAFE_STR};
const KFamily FAMILY_MATFREE = {"MatFree", true,     false,       true,             true,        find_amg_matfree, false,          false,        nullptr,       ilu_of_precond,     false,             true,    K_OFFER_MATFREE};

// K.pc for the caller's `precond`: a device AMG handle (S.h / S.hb, found by F.find_amg), a device ILU, a device (block-)
// diagonal, else a foreign host function, staged through host memory.  pc == NULL: K.pc stays empty (identity).
int bind_precond(const KFamily& F, precond* pc, int n, int nb, PcState& S, KOps& K)
{
    int ilu_which_ = -1, st = FASP_SUCCESS;
    if (S.h) { fasp_hip_amg* h = S.h; K.pc = [h](double* in, double** out) { return precond_amg(h, in, out); }; return st; }  // stays in HBM
    if (S.hb) { fasp_hip_amg_bsr* h = S.hb; K.pc = [h](double* in, double** out) { return precond_amg_bsr(h, in, out); }; return st; }
    S.ilu = F.ilu_lookup(pc, n, S.ilu_tmp, &ilu_which_, &st);
    if (st < 0) return st;
    if (S.ilu) {
        // the reference's (block) ILU preconditioner: recognised by its function pointer, both triangular solves on the device
        IluDev* ilu = S.ilu;
        K.pc = [ilu, ilu_which_](double* in, double** out) { *out = ilu->z; return ilu_apply(ilu, ilu_which_, in, ilu->z); };
        return st;
    }
    if (F.bind_diag && F.bind_diag(pc, n, nb, S, K, &st)) return st;
    if (pc && pc->fct) {
        // foreign preconditioner: a host function; the residual is staged through host memory
        S.hr.resize((size_t)n); S.hz.resize((size_t)n);
        double *hr = S.hr.data(), *hz = S.hz.data(), *zz = S.out(n);
        if (!zz) return ERROR_ALLOC_MEM;
        K.pc = [hr, hz, zz, n, pc](double* in, double** out) {
            HIPCK(hipMemcpyAsync(hr, in, sizeof(double) * n, hipMemcpyDeviceToHost, g_ctx.stream));
            HIPCK(hipStreamSynchronize(g_ctx.stream));
            pc->fct(hr, hz, pc->data);
            HIPCK(hipMemcpyAsync(zz, hz, sizeof(double) * n, hipMemcpyHostToDevice, g_ctx.stream));
            *out = zz;
            return 0;
        };
    }
    return st;
}

// where the operator comes from: a host dCSRmat, a host dBSRmat, a host dSTRmat, or an mxv_matfree -- which is one of the three when
// fasp_solver_matfree_init installed it (recognised by its function pointer), else a host callback
struct KOperator {
    enum Kind { CSR, BSR, STR, HOST } kind;
    const void* A;
    const mxv_matfree* mf = nullptr;
    bool valid = true;
    KOperator(const dCSRmat* M) : kind(CSR), A(M) {}
    KOperator(const dBSRmat* M) : kind(BSR), A(M) {}
    KOperator(const dSTRmat* M) : kind(STR), A(M) {}
    KOperator(const mxv_matfree* m) : kind(HOST), A(nullptr), mf(m), valid(m && m->fct)
    {
        if (valid && m->fct == fasp_hip_mxv_csr) { kind = CSR; A = m->data; }
        if (valid && m->fct == fasp_hip_mxv_bsr) { kind = BSR; A = m->data; }
        if (valid && m->fct == fasp_hip_mxv_str) { kind = STR; A = m->data; }
    }
};

double g_plugin_run_seconds = 0.0;   // fasp_hip_plugin_solve_seconds
int krylov_plugin(const char* fn, const KFamily& F, KMethod method, KOperator op, dvector* b, dvector* u, precond* pc,
                  const KParams& P)
{
    if (F.ctx_first && ctx_init() < 0) die_no_device(fn);
    const dCSRmat* Ac = op.kind == KOperator::CSR ? static_cast<const dCSRmat*>(op.A) : nullptr;
    const dBSRmat* Ab = op.kind == KOperator::BSR ? static_cast<const dBSRmat*>(op.A) : nullptr;
    const dSTRmat* As = op.kind == KOperator::STR ? static_cast<const dSTRmat*>(op.A) : nullptr;
    if (!op.valid || !b || !u || (op.kind != KOperator::HOST && !op.A)) return ERROR_INPUT_PAR;
    const int n = b->row;
    if (u->row != n || (F.refuse_empty && n <= 0)) return ERROR_INPUT_PAR;
    if (Ac && (Ac->row != Ac->col || Ac->row != n)) return ERROR_INPUT_PAR;
    if (Ab && (Ab->ROW != Ab->COL || Ab->ROW * Ab->nb != n)) return ERROR_INPUT_PAR;
    if (As && (str_plan(As, nullptr) < 0 || As->ngrid * As->nc != n)) return ERROR_INPUT_PAR;
    if (F.refuse_multi_rank && comm_size() > 1) return ERROR_INPUT_PAR;  // plug-in level: one GPU
    PcState S;
    int st = F.find_amg(pc, n, S);
    if (st < 0) return st;

    // the operator: uploaded, or the handle's resident copy of it
    KrylovWs ws;
    KOps K;
    K.n = n; K.nvec = (size_t)n; K.fmt = F.fmt; K.dist = false; K.ws = &ws;
    K.halo = [](double*) { return 0; };
    std::unique_ptr<TmpCSR> csr;
    std::unique_ptr<TmpBSR> bsr;
    std::unique_ptr<TmpSTR> str;
    std::unique_ptr<TmpVec> dy;
    std::vector<double> hx, hy;
    if (Ac) {
        const DevCSR* dA = nullptr;
        if (F.borrow_resident && S.h && same_host_matrix(S.h->H.L[0].A, Ac)) dA = &S.h->L[0].A;  // the resident level-0 operator is A itself
        else {
            csr.reset(new TmpCSR(Ac));
            if (!csr->ok) return ERROR_ALLOC_MEM;
            dA = &csr->D;
        }
        K.mxv = [dA](const double* x, double* y) { d_mxv(*dA, x, y); };
        K.resid = [dA](const double* x, const double* bb, double* r) { d_resid(*dA, x, bb, r); };
        if (F.fused_mxv_dot)
            K.mxv_dot = [dA](const double* x, double* y) {
                CsrArgs a{}; a.x = x; a.y = y; a.dotv = x; a.partials = g_ctx.d_partials;
                return launch_csr<OP_MXV_DOT>(*dA, a);
            };
    } else if (Ab) {
        bsr.reset(new TmpBSR(Ab));
        if (!bsr->ok) { if (F.bad_bsr_dies) die_bsr(fn); return ERROR_ALLOC_MEM; }
        const TmpBSR* Mp = bsr.get();
        K.mxv = [Mp](const double* x, double* y) { bsr_mxv(*Mp, x, y); };
        K.resid = [Mp](const double* x, const double* bb, double* r) { bsr_resid(*Mp, x, bb, r); };
    } else if (As) {
        str.reset(new TmpSTR(As));
        if (!str->ok) return ERROR_ALLOC_MEM;
        const TmpSTR* Mp = str.get();
        K.mxv = [Mp](const double* x, double* y) { str_mxv(*Mp, x, y); };
        K.resid = [Mp](const double* x, const double* bb, double* r) { str_resid(*Mp, x, bb, r); };
    } else {   // a host callback: its vectors are staged through host memory once per application
        hx.resize((size_t)n); hy.resize((size_t)n);
        dy.reset(new TmpVec(nullptr, (size_t)n));
        if (!dy->d) return ERROR_ALLOC_MEM;
        const mxv_matfree* mf = op.mf;
        double *px = hx.data(), *py = hy.data(), *yy = dy->d;
        auto host_mxv = [px, py, n, mf](const double* x, double* y) {
            (void)hipMemcpyAsync(px, x, sizeof(double) * n, hipMemcpyDeviceToHost, g_ctx.stream);
            (void)hipStreamSynchronize(g_ctx.stream);
            mf->fct(mf->data, px, py);
            (void)hipMemcpyAsync(y, py, sizeof(double) * n, hipMemcpyHostToDevice, g_ctx.stream);
            (void)hipStreamSynchronize(g_ctx.stream);  // hy is reused by the next application
        };
        K.mxv = host_mxv;
        K.resid = [host_mxv, yy, n](const double* x, const double* bb, double* r) {  // r = 1.0 b + (-1.0) A x
            host_mxv(x, yy);
            (void)hipMemcpyAsync(r, yy, sizeof(double) * n, hipMemcpyDeviceToDevice, g_ctx.stream);
            d_axpby(n, 1.0, bb, -1.0, r);
        };
    }

    TmpVec db(b->val, (size_t)n), du(u->val, (size_t)n);
    if (!db.d || !du.d) return ERROR_ALLOC_MEM;
    std::unique_ptr<TmpVec> cgv[3];   // p, t, r: only pcg_device takes scratch vectors from its caller
    if (method == K_CG && !F.mf_texts)
        for (auto& v : cgv) { v.reset(new TmpVec(nullptr, (size_t)n)); if (!v->d) return ERROR_ALLOC_MEM; }
    double* const sp = cgv[0] ? cgv[0]->d : nullptr, *const stv = cgv[1] ? cgv[1]->d : nullptr, *const sr = cgv[2] ? cgv[2]->d : nullptr;
    if ((st = bind_precond(F, pc, n, Ab ? Ab->nb : As ? As->nc : 1, S, K)) < 0) return st;
    Hist   H{nullptr, 0, 0};
    PcgOut po{BIGREAL, BIGREAL, BIGREAL};
    const double t_run = wall_seconds();
    st = krylov_run(K, method, F.offered, F.mf_texts, P, db.d, du.d, sp, stv, sr, &H, &po);   // (every driver ends with a stream synchronise)
    g_plugin_run_seconds = wall_seconds() - t_run;
    du.get(u->val);
    // a single-launch ILU solve (of the preconditioner, or of a block handle's cycle) that timed out
    if ((S.ilu || (S.strilu && S.strilu->used_pipe) || (F.handle_ilu_checked && S.hb && S.hb->L[0].ilu)) && st >= 0 && seq_err_check() < 0) st = ERROR_MISC;
    return st;
}
}  // namespace

// KryPcg.c:96
int fasp_solver_dcsr_pcg(dCSRmat* A, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                         const int MaxIt, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_CSR, K_CG, A, b, u, pc, {tol, abstol, MaxIt, 0, StopType, PrtLvl});
}
// KryPgmres.c:66
int fasp_solver_dcsr_pgmres(dCSRmat* A, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                            const int MaxIt, const short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_CSR, K_GMRES, A, b, x, pc, {tol, abstol, MaxIt, restart, StopType, PrtLvl});
}
// KryPvgmres.c:66
int fasp_solver_dcsr_pvgmres(dCSRmat* A, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                             const int MaxIt, const short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_CSR, K_VGMRES, A, b, x, pc, {tol, abstol, MaxIt, restart, StopType, PrtLvl});
}
// KryPbcgs.c:62
int fasp_solver_dcsr_pbcgs(dCSRmat* A, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                           const int MaxIt, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_CSR, K_BiCGstab, A, b, u, pc, {tol, abstol, MaxIt, 0, StopType, PrtLvl});
}
// KryPminres.c:61
int fasp_solver_dcsr_pminres(dCSRmat* A, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                             const int MaxIt, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_CSR, K_MinRes, A, b, u, pc, {tol, abstol, MaxIt, 0, StopType, PrtLvl});
}
// KryPgcg.c:60
int fasp_solver_dcsr_pgcg(dCSRmat* A, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                          const int MaxIt, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_CSR, K_GCG, A, b, u, pc, {tol, abstol, MaxIt, 0, StopType, PrtLvl});
}
// KryPgcr.c:55
int fasp_solver_dcsr_pgcr(dCSRmat* A, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                          const int MaxIt, const short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_CSR, K_GCR, A, b, x, pc, {tol, abstol, MaxIt, restart, StopType, PrtLvl});
}
// KryPvfgmres.c:67
int fasp_solver_dcsr_pvfgmres(dCSRmat* A, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                              const int MaxIt, const short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_CSR, K_VFGMRES, A, b, x, pc, {tol, abstol, MaxIt, restart, StopType, PrtLvl});
}

// ---- the same plug-in level for block matrices ---------------------------------
// z = B r with the resident block hierarchy (PreBSR.c:1149 signature); data = fasp_hip_amg_bsr*
void fasp_hip_bsr_precond_fct(double* r, double* z, void* data)
{
    FASP_ENTRY();
    fasp_hip_amg_bsr* h = static_cast<fasp_hip_amg_bsr*>(data);
    if (!h || h->L.empty() || ctx_init() < 0) die_bsr(__func__);
    const int n = h->L[0].n;
    TmpVec dr(r, (size_t)n);
    double* dz = nullptr;
    if (!dr.d || precond_amg_bsr(h, dr.d, &dz) < 0) die_bsr(__func__);
    (void)hipStreamSynchronize(g_ctx.stream);
    if (h->L[0].ilu && seq_err_check() < 0) die_bsr(__func__);   // a single-launch ILU solve of the cycle that timed out
    (void)hipMemcpy(z, dz, sizeof(double) * n, hipMemcpyDeviceToHost);
}

precond* fasp_hip_bsr_precond_setup(dBSRmat* A, AMG_param* amgparam)
{
    FASP_ENTRY();
    fasp_hip_amg_bsr* h = nullptr;
    if (fasp_hip_bsr_amg_create(&h, A, amgparam) < 0) return nullptr;
    precond* pc = static_cast<precond*>(std::calloc(1, sizeof(precond)));
    pc->data = h;
    pc->fct = fasp_hip_bsr_precond_fct;
    return pc;
}

void fasp_hip_bsr_precond_free(precond* pc)
{
    FASP_ENTRY();
    if (!pc) return;
    if (pc->fct == fasp_hip_bsr_precond_fct) fasp_hip_bsr_amg_destroy(static_cast<fasp_hip_amg_bsr*>(pc->data));
    std::free(pc);
}

// KryPcg.c:386, KryPbcgs.c:400, KryPgmres.c:357, KryPvgmres.c:416, KryPvfgmres.c:386
int fasp_solver_dbsr_pcg(dBSRmat* A, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                         const int MaxIt, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_BSR, K_CG, A, b, u, pc, {tol, abstol, MaxIt, 0, StopType, PrtLvl});
}
int fasp_solver_dbsr_pbcgs(dBSRmat* A, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                           const int MaxIt, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_BSR, K_BiCGstab, A, b, u, pc, {tol, abstol, MaxIt, 0, StopType, PrtLvl});
}
int fasp_solver_dbsr_pgmres(dBSRmat* A, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                            const int MaxIt, const short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_BSR, K_GMRES, A, b, x, pc, {tol, abstol, MaxIt, restart, StopType, PrtLvl});
}
int fasp_solver_dbsr_pvgmres(dBSRmat* A, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                             const int MaxIt, const short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_BSR, K_VGMRES, A, b, x, pc, {tol, abstol, MaxIt, restart, StopType, PrtLvl});
}
int fasp_solver_dbsr_pvfgmres(dBSRmat* A, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                              const int MaxIt, const short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_BSR, K_VFGMRES, A, b, x, pc, {tol, abstol, MaxIt, restart, StopType, PrtLvl});
}

// ---------------------------------------------------------------------------
// The other solver-level entry points of SolCSR.c / SolBSR.c: dispatch on itsolver_type with a caller's
// preconditioner, no preconditioner, or the (block-)diagonal one.
// ---------------------------------------------------------------------------
void fasp_precond_diag(double* r, double* z, void* data)  // PreCSR.c:172 (host arrays)
{
    FASP_ENTRY();
    const dvector* diag = static_cast<const dvector*>(data);
    std::memcpy(z, r, sizeof(double) * (size_t)diag->row);
    for (int i = 0; i < diag->row; ++i)
        if (std::fabs(diag->val[i]) > SMALLREAL) z[i] /= diag->val[i];
}
void fasp_precond_dbsr_diag(double* r, double* z, void* data)  // PreBSR.c:49 (host arrays): z_i = Dinv_i r_i
{
    FASP_ENTRY();
    const precond_diag_bsr* d = static_cast<const precond_diag_bsr*>(data);
    const int nb = d->nb, nb2 = nb * nb, m = d->diag.row / nb2;
    for (int i = 0; i < m; ++i)
        for (int rr = 0; rr < nb; ++rr) {
            const double* D = d->diag.val + (size_t)i * nb2 + rr * nb;
            double s = D[0] * r[(size_t)i * nb];
            for (int c = 1; c < nb; ++c) s = s + D[c] * r[(size_t)i * nb + c];
            z[(size_t)i * nb + rr] = s;
        }
}

// SolCSR.c:56
int fasp_solver_dcsr_itsolver(dCSRmat* A, dvector* b, dvector* x, precond* pc, ITS_param* itparam)
{
    FASP_ENTRY();
    if (!itparam) return ERROR_INPUT_PAR;
    const short prtlvl = itparam->print_level, stop_type = itparam->stop_type, restart = (short)itparam->restart;
    const int MaxIt = itparam->maxit;
    const double tol = itparam->tol, abstol = itparam->abstol, t0 = wall_seconds();
    int iter;
    its_check(tol, MaxIt);
    switch (itparam->itsolver_type) {
        case SOLVER_CG: iter = fasp_solver_dcsr_pcg(A, b, x, pc, tol, abstol, MaxIt, stop_type, prtlvl); break;
        case SOLVER_BiCGstab: iter = fasp_solver_dcsr_pbcgs(A, b, x, pc, tol, abstol, MaxIt, stop_type, prtlvl); break;
        case SOLVER_MinRes: iter = fasp_solver_dcsr_pminres(A, b, x, pc, tol, abstol, MaxIt, stop_type, prtlvl); break;
        case SOLVER_GMRES: iter = fasp_solver_dcsr_pgmres(A, b, x, pc, tol, abstol, MaxIt, restart, stop_type, prtlvl); break;
        case SOLVER_VGMRES: iter = fasp_solver_dcsr_pvgmres(A, b, x, pc, tol, abstol, MaxIt, restart, stop_type, prtlvl); break;
        case SOLVER_VFGMRES: iter = fasp_solver_dcsr_pvfgmres(A, b, x, pc, tol, abstol, MaxIt, restart, stop_type, prtlvl); break;
        case SOLVER_GCG: iter = fasp_solver_dcsr_pgcg(A, b, x, pc, tol, abstol, MaxIt, stop_type, prtlvl); break;
        case SOLVER_GCR: iter = fasp_solver_dcsr_pgcr(A, b, x, pc, tol, abstol, MaxIt, restart, stop_type, prtlvl); break;
        default:
            std::printf("### ERROR: Unknown iterative solver type %d! [%s]\n", itparam->itsolver_type, __func__);
            return ERROR_SOLVER_TYPE;
    }
    print_itsolver_time(prtlvl, iter, wall_seconds() - t0);
    return iter;
}
// SolCSR.c:245
int fasp_solver_dcsr_krylov(dCSRmat* A, dvector* b, dvector* x, ITS_param* itparam)
{
    FASP_ENTRY();
    if (!itparam) return ERROR_INPUT_PAR;
    const double t0 = wall_seconds();
    const int status = fasp_solver_dcsr_itsolver(A, b, x, nullptr, itparam);
    if (itparam->print_level >= PRINT_MIN) std::printf("Krylov method totally costs %.4f seconds.\n", wall_seconds() - t0);
    return status;
}
// SolCSR.c:333: diagonal preconditioner from fasp_dcsr_getdiag(0, A, ..) -- the FIRST diagonal hit of each row
int fasp_solver_dcsr_krylov_diag(dCSRmat* A, dvector* b, dvector* x, ITS_param* itparam)
{
    FASP_ENTRY();
    if (!A || !itparam || !A->IA || !A->JA || !A->val) return ERROR_INPUT_PAR;
    const double t0 = wall_seconds();
    const int n = std::min(A->row, A->col);
    std::vector<double> dv((size_t)std::max(n, 1), 0.0);
    for (int i = 0; i < n; ++i)
        for (int k = A->IA[i]; k < A->IA[i + 1]; ++k)
            if (A->JA[k] == i) { dv[(size_t)i] = A->val[k]; break; }
    dvector diag{n, dv.data()};
    precond pc{&diag, fasp_precond_diag};
    const int status = fasp_solver_dcsr_itsolver(A, b, x, &pc, itparam);
    if (itparam->print_level >= PRINT_MIN) std::printf("Diag_Krylov method totally costs %.4f seconds.\n", wall_seconds() - t0);
    return status;
}
// SolBSR.c:64
int fasp_solver_dbsr_itsolver(dBSRmat* A, dvector* b, dvector* x, precond* pc, ITS_param* itparam)
{
    FASP_ENTRY();
    if (!itparam) return ERROR_INPUT_PAR;
    const short prtlvl = itparam->print_level, stop_type = itparam->stop_type, restart = (short)itparam->restart;
    const int MaxIt = itparam->maxit;
    const double tol = itparam->tol, abstol = itparam->abstol, t0 = wall_seconds();
    int iter;
    its_check(tol, MaxIt);
    switch (itparam->itsolver_type) {
        case SOLVER_CG: iter = fasp_solver_dbsr_pcg(A, b, x, pc, tol, abstol, MaxIt, stop_type, prtlvl); break;
        case SOLVER_BiCGstab: iter = fasp_solver_dbsr_pbcgs(A, b, x, pc, tol, abstol, MaxIt, stop_type, prtlvl); break;
        case SOLVER_GMRES: iter = fasp_solver_dbsr_pgmres(A, b, x, pc, tol, abstol, MaxIt, restart, stop_type, prtlvl); break;
        case SOLVER_VGMRES: iter = fasp_solver_dbsr_pvgmres(A, b, x, pc, tol, abstol, MaxIt, restart, stop_type, prtlvl); break;
        case SOLVER_VFGMRES: iter = fasp_solver_dbsr_pvfgmres(A, b, x, pc, tol, abstol, MaxIt, restart, stop_type, prtlvl); break;
        default:
            std::printf("### ERROR: Unknown iterative solver type %d! [%s]\n", itparam->itsolver_type, __func__);
            return ERROR_SOLVER_TYPE;
    }
    print_itsolver_time(prtlvl, iter, wall_seconds() - t0);
    return iter;
}
// SolBSR.c:145
int fasp_solver_dbsr_krylov(dBSRmat* A, dvector* b, dvector* x, ITS_param* itparam)
{
    FASP_ENTRY();
    if (!itparam) return ERROR_INPUT_PAR;
    const double t0 = wall_seconds();
    const int status = fasp_solver_dbsr_itsolver(A, b, x, nullptr, itparam);
    if (itparam->print_level >= PRINT_MIN) std::printf("Krylov method totally costs %.4f seconds.\n", wall_seconds() - t0);
    return status;
}
// SolBSR.c:186: block-diagonal preconditioner, inverse blocks by fasp_smat_inv
int fasp_solver_dbsr_krylov_diag(dBSRmat* A, dvector* b, dvector* x, ITS_param* itparam)
{
    FASP_ENTRY();
    if (!A || !itparam || !A->IA || !A->JA || !A->val) return ERROR_INPUT_PAR;
    if (A->nb < 1 || A->nb > 7) {
        std::printf("### ERROR: fasp_hip: block-diagonal preconditioner needs 1 <= nb <= 7, got %d\n", A->nb);
        return ERROR_INPUT_PAR;
    }
    const double t0 = wall_seconds();
    const int nb2 = A->nb * A->nb;
    std::vector<double> dv((size_t)std::max(A->ROW, 1) * nb2, 0.0);
    const int st = bsr_diaginv(A, dv.data());
    if (st < 0) return st;
    precond_diag_bsr diag;
    diag.nb = A->nb; diag.diag.row = A->ROW * nb2; diag.diag.val = dv.data();
    precond pc{&diag, fasp_precond_dbsr_diag};
    const int status = fasp_solver_dbsr_itsolver(A, b, x, &pc, itparam);
    if (itparam->print_level > PRINT_NONE) std::printf("Diag_Krylov method totally costs %.4f seconds.\n", wall_seconds() - t0);
    return status;
}

#include "str_api.hip.h"
#include "csr_swz_api.hip.h"

// ---------------------------------------------------------------------------
// The Krylov methods with a safety net (KrySPcg.c, KrySPbcgs.c, KrySPminres.c, KrySPgmres.c, KrySPvgmres.c) and their dispatchers
// (SolCSR.c:163 / :295): the plug-in driver with the drivers of safe_krylov.hip.h.  The reference's prototypes have no abstol.
// Without a usable device these entries print why and return ERROR_MISC with x untouched; several ranks are refused (one GPU).
// ---------------------------------------------------------------------------
namespace {
int safe_plugin(const char* fn, const KFamily& F, KMethod method, KOperator op, const dvector* b, dvector* u, precond* pc,
                const KParams& P)
{
    if (ctx_init() < 0) {
        std::printf("### ERROR: %s: no usable HIP device and no CPU fallback in libfasp_hip\n", fn);
        return ERROR_MISC;
    }
    if (comm_size() > 1) {
        std::printf("### ERROR: %s: the safe-net solvers run on one GPU, this job has %d ranks\n", fn, comm_size());
        return ERROR_INPUT_PAR;
    }
    return krylov_plugin(fn, F, method, op, const_cast<dvector*>(b), u, pc, P);
}
}  // namespace
// KrySPcg.c:60
int fasp_solver_dcsr_spcg(const dCSRmat* A, const dvector* b, dvector* u, precond* pc, const double tol, const int MaxIt,
                          const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return safe_plugin(__func__, FAMILY_CSR, K_SPCG, A, b, u, pc, {tol, 0.0, MaxIt, 0, StopType, PrtLvl});
}
// KrySPbcgs.c:61
int fasp_solver_dcsr_spbcgs(const dCSRmat* A, const dvector* b, dvector* u, precond* pc, const double tol, const int MaxIt,
                            const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return safe_plugin(__func__, FAMILY_CSR, K_SPBiCGstab, A, b, u, pc, {tol, 0.0, MaxIt, 0, StopType, PrtLvl});
}
// KrySPminres.c:60
int fasp_solver_dcsr_spminres(const dCSRmat* A, const dvector* b, dvector* u, precond* pc, const double tol, const int MaxIt,
                              const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return safe_plugin(__func__, FAMILY_CSR, K_SPMinRes, A, b, u, pc, {tol, 0.0, MaxIt, 0, StopType, PrtLvl});
}
// KrySPgmres.c:66
int fasp_solver_dcsr_spgmres(const dCSRmat* A, const dvector* b, dvector* x, precond* pc, const double tol, const int MaxIt,
                             short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return safe_plugin(__func__, FAMILY_CSR, K_SPGMRES, A, b, x, pc, {tol, 0.0, MaxIt, restart, StopType, PrtLvl});
}
// KrySPvgmres.c:68
int fasp_solver_dcsr_spvgmres(const dCSRmat* A, const dvector* b, dvector* x, precond* pc, const double tol, const int MaxIt,
                              short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return safe_plugin(__func__, FAMILY_CSR, K_SPVGMRES, A, b, x, pc, {tol, 0.0, MaxIt, restart, StopType, PrtLvl});
}
// KrySPbcgs.c:452, KrySPgmres.c:409, KrySPvgmres.c:449
int fasp_solver_dbsr_spbcgs(const dBSRmat* A, const dvector* b, dvector* u, precond* pc, const double tol, const int MaxIt,
                            const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return safe_plugin(__func__, FAMILY_BSR, K_SPBiCGstab, A, b, u, pc, {tol, 0.0, MaxIt, 0, StopType, PrtLvl});
}
int fasp_solver_dbsr_spgmres(const dBSRmat* A, const dvector* b, dvector* x, precond* pc, const double tol, const int MaxIt,
                             short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return safe_plugin(__func__, FAMILY_BSR, K_SPGMRES, A, b, x, pc, {tol, 0.0, MaxIt, restart, StopType, PrtLvl});
}
int fasp_solver_dbsr_spvgmres(const dBSRmat* A, const dvector* b, dvector* x, precond* pc, const double tol, const int MaxIt,
                              short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return safe_plugin(__func__, FAMILY_BSR, K_SPVGMRES, A, b, x, pc, {tol, 0.0, MaxIt, restart, StopType, PrtLvl});
}
// KrySPcg.c:726, KrySPbcgs.c:1234, KrySPminres.c:962, KrySPgmres.c:1095, KrySPvgmres.c:1210
int fasp_solver_dstr_spcg(const dSTRmat* A, const dvector* b, dvector* u, precond* pc, const double tol, const int MaxIt,
                          const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return safe_plugin(__func__, FAMILY_STR, K_SPCG, A, b, u, pc, {tol, 0.0, MaxIt, 0, StopType, PrtLvl});
}
int fasp_solver_dstr_spbcgs(const dSTRmat* A, const dvector* b, dvector* u, precond* pc, const double tol, const int MaxIt,
                            const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return safe_plugin(__func__, FAMILY_STR, K_SPBiCGstab, A, b, u, pc, {tol, 0.0, MaxIt, 0, StopType, PrtLvl});
}
int fasp_solver_dstr_spminres(const dSTRmat* A, const dvector* b, dvector* u, precond* pc, const double tol, const int MaxIt,
                              const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return safe_plugin(__func__, FAMILY_STR, K_SPMinRes, A, b, u, pc, {tol, 0.0, MaxIt, 0, StopType, PrtLvl});
}
int fasp_solver_dstr_spgmres(const dSTRmat* A, const dvector* b, dvector* x, precond* pc, const double tol, const int MaxIt,
                             short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return safe_plugin(__func__, FAMILY_STR, K_SPGMRES, A, b, x, pc, {tol, 0.0, MaxIt, restart, StopType, PrtLvl});
}
int fasp_solver_dstr_spvgmres(const dSTRmat* A, const dvector* b, dvector* x, precond* pc, const double tol, const int MaxIt,
                              short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return safe_plugin(__func__, FAMILY_STR, K_SPVGMRES, A, b, x, pc, {tol, 0.0, MaxIt, restart, StopType, PrtLvl});
}
// SolCSR.c:163: an itsolver_type without a safe text is refused before any work, as there
int fasp_solver_dcsr_itsolver_s(dCSRmat* A, dvector* b, dvector* x, precond* pc, ITS_param* itparam)
{
    FASP_ENTRY();
    if (!itparam) return ERROR_INPUT_PAR;
    const short prtlvl = itparam->print_level, stop_type = itparam->stop_type, restart = (short)itparam->restart;
    const int MaxIt = itparam->maxit;
    const double tol = itparam->tol, t0 = wall_seconds();
    int iter;
    its_check(tol, MaxIt);
    switch (itparam->itsolver_type) {
        case SOLVER_CG: iter = fasp_solver_dcsr_spcg(A, b, x, pc, tol, MaxIt, stop_type, prtlvl); break;
        case SOLVER_BiCGstab: iter = fasp_solver_dcsr_spbcgs(A, b, x, pc, tol, MaxIt, stop_type, prtlvl); break;
        case SOLVER_MinRes: iter = fasp_solver_dcsr_spminres(A, b, x, pc, tol, MaxIt, stop_type, prtlvl); break;
        case SOLVER_GMRES: iter = fasp_solver_dcsr_spgmres(A, b, x, pc, tol, MaxIt, restart, stop_type, prtlvl); break;
        case SOLVER_VGMRES: iter = fasp_solver_dcsr_spvgmres(A, b, x, pc, tol, MaxIt, restart, stop_type, prtlvl); break;
        default:
            std::printf("### ERROR: Unknown iterative solver type %d! [%s]\n", itparam->itsolver_type, __func__);
            return ERROR_SOLVER_TYPE;
    }
    print_itsolver_time(prtlvl, iter, wall_seconds() - t0);
    return iter;
}
// SolCSR.c:295
int fasp_solver_dcsr_krylov_s(dCSRmat* A, dvector* b, dvector* x, ITS_param* itparam)
{
    FASP_ENTRY();
    if (!itparam) return ERROR_INPUT_PAR;
    const double t0 = wall_seconds();
    const int status = fasp_solver_dcsr_itsolver_s(A, b, x, nullptr, itparam);
    if (itparam->print_level >= PRINT_MIN) std::printf("Krylov method totally costs %.4f seconds.\n", wall_seconds() - t0);
    return status;
}

// ---------------------------------------------------------------------------
// Matrix-free interface of the reference (fasp.h:1109 mxv_matfree, SolMatFree.c): Krylov methods
// that see the operator only as y = A x.  An operator installed by fasp_solver_matfree_init
// (MAT_CSR / MAT_BSR / MAT_STR) is recognised by its function pointer: the matrix is uploaded once and the
// whole iteration stays in HBM.  Any other mf->fct is a host callback: its vectors are staged
// through host memory once per application (as for foreign preconditioners).
// ---------------------------------------------------------------------------
void fasp_hip_mxv_csr(const void* A, const double* x, double* y)  // SolMatFree.c: fasp_blas_mxv_csr
{
    FASP_ENTRY();
    fasp_blas_dcsr_mxv(static_cast<const dCSRmat*>(A), x, y);
}
void fasp_hip_mxv_bsr(const void* A, const double* x, double* y)  // SolMatFree.c: fasp_blas_mxv_bsr
{
    FASP_ENTRY();
    fasp_blas_dbsr_mxv(static_cast<const dBSRmat*>(A), x, y);
}
void fasp_hip_mxv_str(const void* A, const double* x, double* y)  // SolMatFree.c: fasp_blas_mxv_str
{
    FASP_ENTRY();
    fasp_blas_dstr_mxv(static_cast<const dSTRmat*>(A), x, y);
}

// SolMatFree.c:201
void fasp_solver_matfree_init(int matrix_format, mxv_matfree* mf, void* A)
{
    FASP_ENTRY();
    switch (matrix_format) {
        case MAT_CSR: mf->fct = fasp_hip_mxv_csr; break;
        case MAT_BSR: mf->fct = fasp_hip_mxv_bsr; break;
        case MAT_STR: mf->fct = fasp_hip_mxv_str; break;
        default:  // the reference also knows BLC / CSRL: formats this library does not have
            std::printf("### ERROR: Unknown matrix format %d!\n", matrix_format);
            std::exit(ERROR_DATA_STRUCTURE);
    }
    mf->data = A;
}

// KryPcg.c:1260, KryPbcgs.c:1349, KryPgcg.c:213, KryPgmres.c:1309, KryPvgmres.c:1468, KryPvfgmres.c:1026
int fasp_solver_pcg(mxv_matfree* mf, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                    const int MaxIt, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_MATFREE, K_CG, mf, b, u, pc, {tol, abstol, MaxIt, 0, StopType, PrtLvl});
}
int fasp_solver_pbcgs(mxv_matfree* mf, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                      const int MaxIt, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_MATFREE, K_BiCGstab, mf, b, u, pc, {tol, abstol, MaxIt, 0, StopType, PrtLvl});
}
int fasp_solver_pgcg(mxv_matfree* mf, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                     const int MaxIt, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_MATFREE, K_GCG, mf, b, u, pc, {tol, abstol, MaxIt, 0, StopType, PrtLvl});
}
int fasp_solver_pgmres(mxv_matfree* mf, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                       const int MaxIt, const short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_MATFREE, K_GMRES, mf, b, x, pc, {tol, abstol, MaxIt, restart, StopType, PrtLvl});
}
int fasp_solver_pvgmres(mxv_matfree* mf, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                        const int MaxIt, short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_MATFREE, K_VGMRES, mf, b, x, pc, {tol, abstol, MaxIt, restart, StopType, PrtLvl});
}
int fasp_solver_pvfgmres(mxv_matfree* mf, dvector* b, dvector* x, precond* pc, const double tol, const double abstol,
                         const int MaxIt, const short restart, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_MATFREE, K_VFGMRES, mf, b, x, pc, {tol, abstol, MaxIt, restart, StopType, PrtLvl});
}
// KryPminres.c:1283: the reference's older MinRes text for mxv_matfree (minres_mf_device, krylov.hip.h)
int fasp_solver_pminres(mxv_matfree* mf, dvector* b, dvector* u, precond* pc, const double tol, const double abstol,
                        const int MaxIt, const short StopType, const short PrtLvl)
{
    FASP_ENTRY();
    return krylov_plugin(__func__, FAMILY_MATFREE, K_MinRes, mf, b, u, pc, {tol, abstol, MaxIt, 0, StopType, PrtLvl});
}

// SolMatFree.c:58: dispatch on itsolver_type
int fasp_solver_itsolver(mxv_matfree* mf, dvector* b, dvector* x, precond* pc, ITS_param* itparam)
{
    FASP_ENTRY();
    if (!itparam) return ERROR_INPUT_PAR;
    const short prtlvl = itparam->print_level, stop_type = itparam->stop_type;
    const int restart = itparam->restart, MaxIt = itparam->maxit;
    const double tol = itparam->tol, abstol = itparam->abstol;
    const double t0 = wall_seconds();
    int iter = ERROR_SOLVER_TYPE;
    its_check(tol, MaxIt);
    switch (itparam->itsolver_type) {
        case SOLVER_CG: iter = fasp_solver_pcg(mf, b, x, pc, tol, abstol, MaxIt, stop_type, prtlvl); break;
        case SOLVER_BiCGstab: iter = fasp_solver_pbcgs(mf, b, x, pc, tol, abstol, MaxIt, stop_type, prtlvl); break;
        case SOLVER_MinRes: iter = fasp_solver_pminres(mf, b, x, pc, tol, abstol, MaxIt, stop_type, prtlvl); break;
        case SOLVER_GMRES: iter = fasp_solver_pgmres(mf, b, x, pc, tol, abstol, MaxIt, (short)restart, stop_type, prtlvl); break;
        case SOLVER_VGMRES: iter = fasp_solver_pvgmres(mf, b, x, pc, tol, abstol, MaxIt, (short)restart, stop_type, prtlvl); break;
        case SOLVER_VFGMRES: iter = fasp_solver_pvfgmres(mf, b, x, pc, tol, abstol, MaxIt, (short)restart, stop_type, prtlvl); break;
        case SOLVER_GCG: iter = fasp_solver_pgcg(mf, b, x, pc, tol, abstol, MaxIt, stop_type, prtlvl); break;
        default:
            std::printf("### ERROR: Unknown iterative solver type %d! [%s]\n", itparam->itsolver_type, __func__);
            return ERROR_SOLVER_TYPE;
    }
    print_itsolver_time(prtlvl, iter, wall_seconds() - t0);
    return iter;
}

// SolMatFree.c:157: Krylov method without preconditioner
int fasp_solver_krylov(mxv_matfree* mf, dvector* b, dvector* x, ITS_param* itparam)
{
    FASP_ENTRY();
    if (!itparam) return ERROR_INPUT_PAR;
    const double t0 = wall_seconds();
    const int status = fasp_solver_itsolver(mf, b, x, nullptr, itparam);
    if (itparam->print_level >= PRINT_MIN) std::printf("Krylov method totally costs %.4f seconds.\n", wall_seconds() - t0);
    return status;
}

void fasp_blas_dcsr_mxv(const dCSRmat* A, const double* x, double* y)
{
    FASP_ENTRY();
    TmpCSR M(A);
    if (!M.ok) die_no_device(__func__);
    TmpVec dx(x, A->col), dy(nullptr, A->row);
    d_mxv(M.D, dx.d, dy.d);
    dy.get(y);
}

void fasp_blas_dcsr_aAxpy(const double alpha, const dCSRmat* A, const double* x, double* y)
{
    FASP_ENTRY();
    TmpCSR M(A);
    if (!M.ok) die_no_device(__func__);
    TmpVec dx(x, A->col), dy(y, A->row);
    d_aAxpy(alpha, M.D, dx.d, dy.d);
    dy.get(y);
}

double fasp_blas_darray_dotprod(const int n, const double* x, const double* y)
{
    FASP_ENTRY();
    if (ctx_init() < 0) die_no_device(__func__);
    TmpVec dx(x, n), dy(y, n);
    double out = 0.0;
    (void)d_dot(n, dx.d, dy.d, &out);
    return out;
}

double fasp_blas_darray_norm2(const int n, const double* x)
{
    FASP_ENTRY();
    if (ctx_init() < 0) die_no_device(__func__);
    TmpVec dx(x, n);
    double out[2] = {0, 0};
    (void)d_norms(n, dx.d, out);
    return std::sqrt(out[0]);
}

double fasp_blas_darray_norminf(const int n, const double* x)
{
    FASP_ENTRY();
    if (ctx_init() < 0) die_no_device(__func__);
    TmpVec dx(x, n);
    double out[2] = {0, 0};
    (void)d_norms(n, dx.d, out);
    return out[1];
}

void fasp_blas_darray_axpy(const int n, const double a, const double* x, double* y)
{
    FASP_ENTRY();
    if (ctx_init() < 0) die_no_device(__func__);
    TmpVec dx(x, n), dy(y, n);
    d_axpy(n, a, dx.d, dy.d);
    dy.get(y);
}

void fasp_blas_darray_axpby(const int n, const double a, const double* x, const double b, double* y)
{
    FASP_ENTRY();
    if (ctx_init() < 0) die_no_device(__func__);
    TmpVec dx(x, n), dy(y, n);
    d_axpby(n, a, dx.d, b, dy.d);
    dy.get(y);
}

// ---- the remaining names of SURVEY.md section 8 rows a10-a12 as stand-alone entries over the solve's own kernels ----
// alpha = y' A x (BlaSpmvCSR.c:839): the fused SpMV + dot epilogue the coarse-scaling step of the cycle uses
double fasp_blas_dcsr_vmv(const dCSRmat* A, const double* x, const double* y)
{
    FASP_ENTRY();
    TmpCSR M(A);
    if (!M.ok) die_no_device(__func__);
    TmpVec dx(x, A->col), dy(y, A->row), dt(nullptr, A->row);
    CsrArgs a{}; a.x = dx.d; a.y = dt.d; a.dotv = dy.d; a.partials = g_ctx.d_partials;
    const int G = launch_csr<OP_MXV_DOT>(M.D, a);
    d_finalize(G, 1, 0u, 0, false);
    double out = 0.0;
    (void)fetch_red(0, 1, &out);
    return out;
}
namespace {
// the matrix of the *_agg kernels: the caller's pattern with unit entries (the reference never reads val there, and
// 1.0 * x = x exactly, so the general kernels ARE the aggregation kernels: same sums, same order)
struct TmpUnitCSR {
    dCSRmat view;
    std::vector<double> ones;
    explicit TmpUnitCSR(const dCSRmat* A) : view(*A), ones((size_t)std::max(A->nnz, 1), 1.0) { view.val = ones.data(); }
};
}  // namespace
void fasp_blas_dcsr_mxv_agg(const dCSRmat* A, const double* x, double* y)  // BlaSpmvCSR.c:438
{
    FASP_ENTRY();
    TmpUnitCSR U(A);
    fasp_blas_dcsr_mxv(&U.view, x, y);
}
void fasp_blas_dcsr_aAxpy_agg(const double alpha, const dCSRmat* A, const double* x, double* y)  // BlaSpmvCSR.c:727
{
    FASP_ENTRY();
    TmpUnitCSR U(A);
    fasp_blas_dcsr_aAxpy(alpha, &U.view, x, y);
}
void fasp_blas_darray_ax(const int n, const double a, double* x)  // BlaArray.c:43
{
    FASP_ENTRY();
    if (a == 1.0) return;
    if (ctx_init() < 0) die_no_device(__func__);
    TmpVec dx(x, n);
    hipLaunchKernelGGL(k_scale, dim3(vec_grid(n)), dim3(BLOCK), 0, g_ctx.stream, n, a, dx.d);
    dx.get(x);
}
void fasp_blas_darray_axpyz(const int n, const double a, const double* x, const double* y, double* z)  // BlaArray.c:403
{
    FASP_ENTRY();
    if (ctx_init() < 0) die_no_device(__func__);
    TmpVec dx(x, n), dy(y, n), dz(nullptr, n);
    hipLaunchKernelGGL(k_axpyz, dim3(vec_grid(n)), dim3(BLOCK), 0, g_ctx.stream, n, a, dx.d, dy.d, dz.d);
    dz.get(z);
}
namespace {
int norm1_nan(const char* fn, int n, const double* x, double out[2])
{
    if (ctx_init() < 0) die_no_device(fn);
    TmpVec dx(x, n);
    const int G = vec_grid(n);
    hipLaunchKernelGGL(k_norm1_nan, dim3(G), dim3(BLOCK), 0, g_ctx.stream, n, dx.d, g_ctx.d_partials);
    d_finalize(G, 2, 0u, 0, false);
    return fetch_red(0, 2, out);
}
}  // namespace
double fasp_blas_darray_norm1(const int n, const double* x)  // BlaArray.c:663
{
    FASP_ENTRY();
    double out[2] = {0, 0};
    (void)norm1_nan(__func__, n, x, out);
    return out[0];
}
short fasp_dvec_isnan(const dvector* u)  // AuxVector.c:39
{
    FASP_ENTRY();
    double out[2] = {0, 0};
    (void)norm1_nan(__func__, u->row, u->val, out);
    return out[1] > 0.0 ? 1 : 0;
}
void fasp_darray_cp(const int n, const double* x, double* y)  // AuxArray.c:210: through HBM (upload, device copy, download)
{
    FASP_ENTRY();
    if (ctx_init() < 0) die_no_device(__func__);
    TmpVec dx(x, n), dy(nullptr, n);
    (void)hipMemcpyAsync(dy.d, dx.d, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, g_ctx.stream);
    dy.get(y);
}
void fasp_darray_set(const int n, double* x, const double val)  // AuxArray.c:41
{
    FASP_ENTRY();
    if (ctx_init() < 0) die_no_device(__func__);
    TmpVec dx(nullptr, n);
    hipLaunchKernelGGL(k_set, dim3(vec_grid(n)), dim3(BLOCK), 0, g_ctx.stream, n, val, dx.d);
    dx.get(x);
}

void fasp_blas_dbsr_mxv(const dBSRmat* A, const double* x, double* y)
{
    FASP_ENTRY();
    TmpBSR M(A);
    if (!M.ok) die_bsr(__func__);
    TmpVec dx(x, (size_t)A->COL * A->nb), dy(nullptr, (size_t)A->ROW * A->nb);
    BsrArgs a{}; a.x = dx.d; a.y = dy.d;
    launch_bsr<0>(M, a);
    dy.get(y);
}

void fasp_blas_dbsr_aAxpy(const double alpha, const dBSRmat* A, const double* x, double* y)
{
    FASP_ENTRY();
    if (alpha == 0.0) return;  // BlaSpmvBSR.c:548
    TmpBSR M(A);
    if (!M.ok) die_bsr(__func__);
    TmpVec dx(x, (size_t)A->COL * A->nb), dy(y, (size_t)A->ROW * A->nb);
    BsrArgs a{}; a.x = dx.d; a.y = dy.d; a.alpha = alpha;
    launch_bsr<1>(M, a);
    dy.get(y);
}

// BlaSparseBSR.c:543 (host): diagonal blocks inverted as fasp_smat_inv does (BlaSmallMatInv.c:603): closed forms for
// nb = 2, 3, 4, Gauss-Jordan with full pivoting for 5..7; nb == 1: reciprocals
dvector fasp_dbsr_getdiaginv(const dBSRmat* A)
{
    FASP_ENTRY();
    dvector out{0, nullptr};
    if (!A || A->nb < 1 || A->nb > 7) {
        std::fprintf(stderr, "### ERROR: fasp_dbsr_getdiaginv: block size %d not supported (1..7)\n", A ? A->nb : -1);
        return out;
    }
    out.row = A->ROW * A->nb * A->nb;
    out.val = (double*)std::calloc((size_t)std::max(out.row, 1), sizeof(double));
    (void)bsr_diaginv(A, out.val);
    return out;
}

void fasp_smoother_dbsr_jacobi1(dBSRmat* A, dvector* b, dvector* u, double* diaginv)
{
    FASP_ENTRY();
    TmpBSR M(A);
    if (!M.ok) die_bsr(__func__);
    const size_t n = (size_t)A->ROW * A->nb;
    TmpVec du(u->val, n), dun(nullptr, n), db(b->val, n), dd(diaginv, (size_t)A->ROW * A->nb * A->nb);
    BsrArgs a{}; a.x = du.d; a.y = dun.d; a.b = db.d; a.dinv = dd.d;
    launch_bsr<2>(M, a);
    dun.get(u->val);
}

// test entry: one block Gauss-Seidel / SOR sweep of a host matrix through the schedule and the launches of the cycle's sweeps
int fasp_hip_bsr_sweep(const dBSRmat* A, const double* b, double* u, const double* diaginv, int descend, int sor, double w,
                       int* nlevels)
{
    FASP_ENTRY();
    if (!A || !b || !u || !diaginv || !nlevels || !A->IA || (A->NNZ > 0 && (!A->JA || !A->val))) return ERROR_INPUT_PAR;
    if (A->nb < 1 || A->nb > 7 || A->storage_manner != 0 || A->ROW != A->COL || A->ROW < 0 || A->NNZ < 0) return ERROR_INPUT_PAR;
    TmpBSR M(A);
    if (!M.ok) return ERROR_MISC;   // no device (or no memory on it)
    const size_t n = (size_t)A->ROW * A->nb;
    TmpVec du(u, n), db(b, n), dd(diaginv, n * A->nb);
    if (!du.d || !db.d || !dd.d) return ERROR_MISC;
    DevLevel::Sched S;
    int st = bsr_seq_schedule(A->ROW, A->COL, A->NNZ, A->IA, A->JA, descend != 0, S);
    if (st >= 0) st = bsr_seq_launch(M, S, db.d, dd.d, du.d, sor != 0, w);
    if (st >= 0) { *nlevels = (int)S.ptr.size() - 1; du.get(u); }
    else (void)hipStreamSynchronize(g_ctx.stream);
    S.release();
    return st;
}

double fasp_hip_time_bsr_mxv(const dBSRmat* A, int reps)
{
    FASP_ENTRY();
    TmpBSR M(A);
    if (!M.ok || reps <= 0) return -1.0;
    TmpVec dx(nullptr, (size_t)A->COL * A->nb), dy(nullptr, (size_t)A->ROW * A->nb);
    (void)hipMemsetAsync(dx.d, 0, sizeof(double) * dx.n, g_ctx.stream);
    BsrArgs a{}; a.x = dx.d; a.y = dy.d;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    launch_bsr<0>(M, a); launch_bsr<0>(M, a);
    (void)hipEventRecord(e0, g_ctx.stream);
    for (int i = 0; i < reps; ++i) launch_bsr<0>(M, a);
    (void)hipEventRecord(e1, g_ctx.stream);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return (double)ms / reps;
}

// ItrSmootherCSR.c:98 -- rows i_1..i_n (either direction) of the square system
void fasp_smoother_dcsr_jacobi(dvector* u, const int i_1, const int i_n, const int s, dCSRmat* A, dvector* b,
                               int L, const double w)
{
    FASP_ENTRY();
    (void)s;
    TmpCSR M(A);
    if (!M.ok) die_no_device(__func__);
    const int n = A->row;
    const int lo = std::min(i_1, i_n), hi = std::max(i_1, i_n);
    if (lo != 0 || hi != n - 1) {
        std::fprintf(stderr, "### ERROR: fasp_smoother_dcsr_jacobi (device): only full sweeps 0..n-1 supported\n");
        std::exit(ERROR_INPUT_PAR);
    }
    std::vector<double> d(n, 0.0);
    bool dup = false;
    for (int i = 0; i < n; ++i) {
        int hits = 0;
        for (int k = A->IA[i]; k < A->IA[i + 1]; ++k)
            if (A->JA[k] == i) { d[i] = A->val[k]; ++hits; }
        dup = dup || hits > 1;
    }
    M.D.dup_diag = dup;   // (a diagonal stored twice: the kernels that take the diagonal's product out of a full row sum do not apply)
    TmpVec du(u->val, n), du2(nullptr, n), db(b->val, n), dd(d.data(), n);
    double *x = du.d, *xo = du2.d;
    while (L--) {
        CsrArgs a{};
        a.x = x; a.y = xo; a.b = db.d; a.diag = dd.d; a.omega = w;
        launch_csr<OP_JACOBI>(M.D, a);
        std::swap(x, xo);
    }
    (void)hipStreamSynchronize(g_ctx.stream);
    (void)hipMemcpy(u->val, x, sizeof(double) * n, hipMemcpyDeviceToHost);
}

#ifdef FLOW_TIMING
extern "C" int fasp_hip_flow_times(unsigned long long* out, int n)   // (development build only: tools/perf_gs_one.py)
{
    FASP_ENTRY();
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(fasp::g_flow_times), sizeof(unsigned long long) * (size_t)std::min(n, 8192)) == hipSuccess ? 0 : -1;
}
#endif

// development knob: override kernel selection / launch geometry at run time
static int g_time_cold = 0;   // fasp_hip_tune("time_cold"): fasp_hip_time_kernel times every launch on its own behind a flush of the Infinity Cache
int fasp_hip_tune(const char* key, int value)
{
    FASP_ENTRY();
    if (!key) return ERROR_INPUT_PAR;
    ++g_coarse_gen;   // the coarse plans kept on the handles are remade (coarse_cg.hip.h)
    if (!std::strcmp(key, "maxgrid")) g_tune.maxgrid = value;
    else if (!std::strcmp(key, "xcd")) g_tune.xcd = value;
    else if (!std::strcmp(key, "gen2")) g_tune.gen2 = value;
    else if (!std::strcmp(key, "ws2_bpc")) g_tune.ws2_bpc = value;
    else if (!std::strcmp(key, "nt")) g_tune.nt = value;
    else if (!std::strcmp(key, "kind")) g_tune.kind = value;
    else if (!std::strcmp(key, "compress")) g_tune.compress = value;
    else if (!std::strcmp(key, "rpl")) g_tune.rpl = value;
    else if (!std::strcmp(key, "lds_tab")) g_tune.lds_tab = value;
    else if (!std::strcmp(key, "xcd_pat")) g_tune.xcd_pat = value;
    else if (!std::strcmp(key, "spcg_batch")) g_tune.spcg_batch = value;
    else if (!std::strcmp(key, "spcg_fused")) g_tune.spcg_fused = value;
    else if (!std::strcmp(key, "spcg_persist")) { g_tune.spcg_persist = value; if (value) g_persist_disabled = false; }
    else if (!std::strcmp(key, "spcg_test_hang")) g_tune.spcg_test_hang = value;
    else if (!std::strcmp(key, "spcg_grid")) g_tune.spcg_grid = value;
    else if (!std::strcmp(key, "small_lds")) g_tune.small_lds = value;
    else if (!std::strcmp(key, "small_onewave")) g_tune.small_onewave = value;
    else if (!std::strcmp(key, "ja16")) g_tune.ja16 = value;
    else if (!std::strcmp(key, "device_sort")) g_device_sort = value;
    else if (!std::strcmp(key, "halo_overlap")) g_halo_overlap = value;
    else if (!std::strcmp(key, "coarse_mode")) g_coarse_mode = value;            // replicated levels: 0 redundant work, 1 split rows + all-gather, -1 (default) split over peer windows only
    else if (!std::strcmp(key, "coarse_split_min")) g_coarse_split_min = value;
    else if (!std::strcmp(key, "split_rows")) g_tune.split_rows = value;
    else if (!std::strcmp(key, "gs_multicolor")) g_tune.gs_multicolor = value;
    else if (!std::strcmp(key, "seq_flow")) { g_tune.seq_flow = value; if (value) g_flow_disabled = false; }
    else if (!std::strcmp(key, "ilu_smooth_fused")) g_tune.ilu_smooth_fused = value;   // ILU step of the block cycle: 1 (default) the U solve writes x = x + z itself, 0 a separate axpy pass -- same bits
    else if (!std::strcmp(key, "swz_run")) g_tune.swz_run = value;   // Schwarz sweeps: stretches of narrow dependency levels in one launch of one workgroup (k_csr_swz_run): -1 (default) inside the AMG cycles on the levels whose schedule is nearly serial (csr_swz.hip.h, SWZ_RUN_MEAN), 0 never, 1 on every Schwarz level of a cycle and in the stand-alone entries -- same bits
    else if (!std::strcmp(key, "swz_run_width")) g_tune.swz_run_width = value;   // blocks a level of such a stretch has at most (16); read at launch
    else if (!std::strcmp(key, "ilu_form")) g_tune.ilu_form = value;   // ILU triangular solves: -1 (default) by the schedule's depth, 0 one launch per level, 1 one launch
    else if (!std::strcmp(key, "bsr_sweep_form")) g_tune.bsr_sweep_form = value;   // block GS / SOR sweeps over the slab plan (bsr_sweep.hip.h): -1 (default) by the plan's depth, 0 one launch per level, 1 one launch -- same bits
    else if (!std::strcmp(key, "bsr_cycle_sweep")) g_tune.bsr_cycle_sweep = value;   // GS / SGS / SOR / SSOR sweeps of the block AMG cycle and the GS sweeps behind its ILU step: 0 (default) k_bsr_seq_level per dependency level, 1 the slab plan and kernels of bsr_sweep.hip.h -- same bits
    else if (!std::strcmp(key, "str_ilu_form")) g_tune.str_ilu_form = value;   // structured ILU solves (str_ilu_plan): -1 (default) by the plan, 0 one launch per level, 1 planes pipelined over workgroups (3-D)
    else if (!std::strcmp(key, "str_ilu_wgs")) g_tune.str_ilu_wgs = value;     // workgroups of the pipelined form at most (0, default: twice the compute units)
    else if (!std::strcmp(key, "str_sweep_form")) g_tune.str_sweep_form = value;   // structured GS / SOR sweeps (str_sweep_plan): -1 (default) by the plan, 0 one launch per level, 1 planes pipelined over workgroups (3-D), 2 the ordered form (level list)
    else if (!std::strcmp(key, "str_sweep_wgs")) g_tune.str_sweep_wgs = value;     // workgroups of the pipelined sweep at most (0, default: twice the compute units)
    else if (!std::strcmp(key, "seq_strip_kb")) g_tune.seq_strip_kb = value;  // KB of lower entries per strip of the dataflow solve (0, default: 256 / 512 / 1024 by level shape, seq_sched.cpp)
    else if (!std::strcmp(key, "seq_jobs")) g_tune.seq_jobs = value;
    else if (!std::strcmp(key, "local_square")) g_tune.local_square = value;   // a rank's rows of a partitioned level are coded like a square operator (read at upload)
    else if (!std::strcmp(key, "seq_grid")) g_tune.seq_grid = value;     // workgroups of the dataflow solve at most (0: twice the strips the chain front is in at a time + 2, seq_sched.cpp; < 0: as many as are resident)
    else if (!std::strcmp(key, "seq_chain")) g_tune.seq_chain = value;   // chain form of the triangular solve (seq_chain.hip.h): 0 never, 1 on chain-bound sweeps, 2 wherever it applies; read when a schedule is built
    else if (!std::strcmp(key, "seq_chain_n1")) g_tune.seq_chain_n1 = value;       // blocks of 64 rows in tier 1 (0: two)
    else if (!std::strcmp(key, "seq_chain_grid")) g_tune.seq_chain_grid = value;   // tier-2 workgroups of the chain launch (0: default)
    else if (!std::strcmp(key, "seq_test_hang")) g_tune.seq_test_hang = value;     // tests: the next chain launches go without their tier-2 workgroups -- every waiter runs into its bounded poll (2 s)
    else if (!std::strcmp(key, "seq_rest_lanes")) g_tune.seq_rest_lanes = value;   // lanes per row of the rest pass (0: from the mean row length); read at launch
    else if (!std::strcmp(key, "seq_chain_ref")) g_tune.seq_chain_ref = value;     // 1: the plain one-wavefront form (k_tri_chain_ref: A/B, fallback)
    else if (!std::strcmp(key, "seq_spine")) g_tune.seq_spine = value;   // 0 never, 1 where the schedule chooses it, 2 wherever a row has two lanes (seq_sched.h); read when a schedule is built
    else if (!std::strcmp(key, "seq_partition")) g_seq_partition = value;
    else if (!std::strcmp(key, "fuse_zr")) g_tune.fuse_zr = value;
    else if (!std::strcmp(key, "fuse_presmooth")) g_tune.fuse_presmooth = value;
    else if (!std::strcmp(key, "seq_lanes")) g_tune.seq_lanes = value;
    else if (!std::strcmp(key, "lazy_coarse")) g_tune.lazy_coarse = value;
    else if (!std::strcmp(key, "xtile")) g_tune.xtile = value;
    else if (!std::strcmp(key, "rp5_max")) g_tune.rp5_max = value;
    else if (!std::strcmp(key, "rp_bpc")) g_tune.rp_bpc = value;
    else if (!std::strcmp(key, "rp_stream")) g_tune.rp_stream = value;
    else if (!std::strcmp(key, "renumber")) g_tune.renumber = value;             // brick renumbering of the uncoded mid levels at upload (order-independent smoothers only; hierarchy.hip.h): 1 on (default), 2 also levels behind a coded one (whose transfer operators keep their coding and take a numbering bridge), 0 off; read when a hierarchy is uploaded
    else if (!std::strcmp(key, "renumber_chunk")) g_tune.renumber_chunk = value; // rows per chunk inside which the balls grow (reorder.cpp)
    else if (!std::strcmp(key, "time_cold")) g_time_cold = value;
    else if (!std::strcmp(key, "estream")) g_tune.estream = value;   // long-row operators: the entry-parallel stream kernel where it measured faster (1, default: mean rows below 256 entries), wherever its tables exist (2), never (0: the row kernel); read at launch
    else if (!std::strcmp(key, "rgroup")) g_tune.rgroup = value;     // long-row square operators: the row-group form and k_csr_rgroup never (0: no copy is built), where it measured faster (1, default; not under estream 0), wherever the copy exists (2); read at upload (0 or not) and at launch
    else if (!std::strcmp(key, "rgroup_rows")) g_tune.rgroup_rows = value;     // ... rows per group: 8 (default) or 16; read at upload
    else if (!std::strcmp(key, "rgroup_waves")) g_tune.rgroup_waves = value;   // ... waves per group: 2, 4 or 8 (default: by the mean row length, 2 below 256 entries, 8 from 1 000 on); read at launch
    else if (!std::strcmp(key, "sell")) g_tune.sell = value;         // value-indexed sliced-ELL form where an operator has it (1, default) or its plain-CSR kernels (0), the other codings untouched; read at launch
    else if (!std::strcmp(key, "es_dbg")) g_tune.es_dbg = value;     // (FASP_LAB_DEBUG builds: parts of the stream kernel switched off -- timings only)
    else if (!std::strcmp(key, "pcg_dev_beta")) g_tune.pcg_dev_beta = value;   // top-level PCG: (z, r), beta and alpha stay on the device, one host wait per iteration (1, default) or two (0)
    else if (!std::strcmp(key, "seq_chain_touch")) g_tune.seq_chain_touch = value;   // chain form: blocks by which a workgroup of its own on the chain's XCD touches the band planes ahead (8; 0: the importer wave does, four ahead)
    else if (!std::strcmp(key, "seq_chain_touch_t1")) g_tune.seq_chain_touch_t1 = value;   // ... and tier 1's entries of those blocks (1, default)
    else if (!std::strcmp(key, "seq_zero_skip")) g_tune.seq_zero_skip = value;   // sequential sweeps: the parallel pass of a sweep that starts from the zero vector reads b only (1, default) or every entry (0)
    else if (!std::strcmp(key, "safe_fused")) g_tune.safe_fused = value;       // safe-net Krylov solvers: the fused update kernels and the swapping iterate buffers (1, default) or the reference's pass-by-pass sequence over the existing BLAS-1 launches with a real copy to u_best (0: A/B, second implementation) -- same elementwise bits
    else if (!std::strcmp(key, "pcg_fold")) g_tune.pcg_fold = value;           // one rank: (t,p) and (z,r) are summed from their partials by the kernels that divide by them (1, default) or by a k_finalize launch each (0)
    else if (!std::strcmp(key, "spcg_spec")) g_tune.spcg_spec = value;         // persistent coarse CG: the true residual of Check III queued behind the kernel, one host wait per coarse solve (1, default) or two (0)
    else if (!std::strcmp(key, "ev_every")) g_tune.ev_every = value;           // the level-0 t = A p launch inside a solve is bracketed by an event pair every n-th iteration (4; 1: every one)
    else if (!std::strcmp(key, "rp_xcd")) g_tune.rp_xcd = value;
    else if (!std::strcmp(key, "rp_strip")) g_tune.rp_strip = value;   // coded operators of a 3-D grid: an XCD sweeps a strip of every plane (1: the square ones, 2: the transfer operators too, default) or a slab of planes (0)
    else if (!std::strcmp(key, "host_parallel_min")) g_parallel_min_nnz = value;
    else if (!std::strcmp(key, "rap_form")) g_rap_form = value;           // Galerkin product on the device (rap.hip.h): -1 (default) by the mean work per row, 0 one lane per coarse row, 1 one wavefront per coarse row -- same bytes
    else if (!std::strcmp(key, "rap_arena_kb")) g_rap_arena_kb = value;   // ... KiB of its table arena: rows go in batches that fit (a batch of one row always does)
    else if (!std::strcmp(key, "device_rap")) g_device_rap = value;       // the AMG setups form their Galerkin products on the device (1) or on the host (0, default) -- same bytes; read by every product
    else if (!std::strcmp(key, "lanes")) g_tune.lanes = value;
    else if (!std::strcmp(key, "wrows")) g_tune.wrows = value;
    else if (!std::strcmp(key, "wcap")) g_tune.wcap = value;
    else return ERROR_INPUT_PAR;
    return FASP_SUCCESS;
}

// measurement entry: wall seconds the last plug-in Krylov solve of this process spent in its driver (operator upload, preconditioner
// binding and the copy of x back to the host excluded)
double fasp_hip_plugin_solve_seconds(void)
{
    FASP_ENTRY();
    return g_plugin_run_seconds;
}

// test entry: update step `which` of the safe-net solvers (safe_krylov.hip.h) in its fused form and as the reference's sequence over the
// existing BLAS-1 launches, on the same inputs (fasp_hip_dev.h has the inputs and the layout of out)
int fasp_hip_safe_update_selftest(int which, int n, int seed, double* out)
{
    FASP_ENTRY();
    if (!out || n < 1 || which < 0 || which > 5 || seed < 0) return ERROR_INPUT_PAR;
    if (ctx_init() < 0) return ERROR_MISC;
    constexpr int NV = 7;   // vectors 0 .. 6: the inputs, by the step's own list
    const double alpha = 0.37, omega = -0.61, beta = 1.29;
    const bool nans = seed >= 1000;
    auto value = [seed](int k, int i) {   // splitmix64 of (i, seed, k) -> [-1, 1)
        unsigned long long z = ((unsigned long long)i + 1ull) * 0x9E3779B97F4A7C15ull + (unsigned long long)seed * 0xBF58476D1CE4E5B9ull +
                               (unsigned long long)k * 0x94D049BB133111EBull;
        z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
        return (double)(z >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
    };
    std::vector<double> h((size_t)n), g0((size_t)n), g1((size_t)n);
    TmpVec* v[2][NV + 1] = {};   // two sets (fused, sequence); vector NV: the second iterate buffer
    std::vector<std::unique_ptr<TmpVec>> own;
    for (int set = 0; set < 2; ++set)
        for (int k = 0; k <= NV; ++k) {
            for (int i = 0; i < n; ++i) h[(size_t)i] = k == NV ? 0.0 : value(k, i);
            if (k == 0 && nans) h[0] = h[(size_t)(n / 2)] = h[(size_t)n - 1] = std::nan("");   // vector 0 is the iterate
            own.emplace_back(new TmpVec(h.data(), (size_t)n));
            if (!own.back()->d) return ERROR_ALLOC_MEM;
            v[set][k] = own.back().get();
        }
    double red[2][8] = {};
    int nq = 0, nout = 0, outs[4] = {0, 0, 0, 0};   // the step's output vectors
    int st = 0;
    for (int set = 0; set < 2 && st >= 0; ++set) {
        const bool fused = set == 0;
        auto D = [&](int k) { return v[set][k]->d; };
        // the fused form writes the iterate OUT OF PLACE here (vector NV), the sequence in place (vector 0): both are compared
        SafeIterate U(D(0), D(NV), n, fused);
        if (fused) U.best = U.cur;
        switch (which) {
            case 0:   // u = 0, p = 1, t = 2, r = 3
                st = safe_cg_update(fused, n, alpha, D(1), D(2), U, D(3), red[set]); nq = 5; nout = 2; outs[0] = 0; outs[1] = 3; break;
            case 1:   // r = 1, z = 2 -> s = 3
                safe_bcgs_s(fused, n, alpha, D(1), D(2), D(3)); nq = 0; nout = 1; outs[0] = 3; break;
            case 2:   // u = 0, pp = 1, sp = 2, s = 3, t = 4, rho = 5 -> r = 6
                st = safe_bcgs_update(fused, n, alpha, omega, D(1), D(2), D(2), U, D(3), D(4), D(6), D(5), red[set]);
                nq = 6; nout = 4; outs[0] = 0; outs[1] = 2; outs[2] = 3; outs[3] = 6; break;
            case 3:   // r = 1, z = 2, p = 3
                safe_bcgs_p(fused, n, omega, beta, D(1), D(2), D(3)); nq = 0; nout = 1; outs[0] = 3; break;
            case 4:   // t = 1, s = 2
                st = safe_dot2(fused, n, D(1), D(2), red[set]); nq = 2; nout = 0; break;
            default: {   // x = 0, r = 1
                double* const xo = fused ? D(NV) : D(0);
                st = safe_x_update(fused, n, D(1), D(0), xo, red[set]); U.cur = xo; nq = 3; nout = 1; outs[0] = 0; break;
            }
        }
        if (fused && U.cur != D(0)) std::swap(v[set][0], v[set][NV]);   // vector 0 of the set: where the iterate is now
    }
    if (st < 0) return st;
    HIPCK(hipStreamSynchronize(g_ctx.stream));
    long long mismatches = 0;
    for (int o = 0; o < nout; ++o) {
        v[0][outs[o]]->get(g0.data());
        v[1][outs[o]]->get(g1.data());
        for (int i = 0; i < n; ++i) mismatches += std::memcmp(&g0[(size_t)i], &g1[(size_t)i], sizeof(double)) != 0;
    }
    out[0] = (double)mismatches;
    out[1] = (double)nq;
    for (int k = 0; k < 8; ++k) { out[2 + k] = red[0][k]; out[10 + k] = red[1][k]; }
    return FASP_SUCCESS;
}

// test entry: ONE launch of a BLAS-1 kernel (kernels.hip.h; k_pack of hierarchy.hip.h) on the caller's inputs, with the grid rule and the
// context buffers of its production call site, followed by k_finalize where the solvers follow it with one (fasp_hip_dev.h has the
// kernels, the variants and the layout of every argument).  No reference and no input generator live here.
int fasp_hip_blas1_op(int kernel, int variant, int n, const int* ipar, const double* scal, const double* const* vin, double* const* vout,
                      const double* part_in, int npart, const int* idx, double* red, double* part_out, int* grid, double* pub)
{
    FASP_ENTRY();
    enum { CG_UPDATE, AXPBY_BETA, MGS_STEP, FINALIZE, DOT, NORMS, NORM1_NAN, AXPY, AXPBY, AXPYZ, AXPY_SELF, SCALE, SET, POLY_SCALE,
           POLY_START, POLY_STEP, JACOBI_ZERO, L1_ZERO, DIAG_PRECOND, BSR_DINV_APPLY, PACK, NKERNEL };
    constexpr int NSLOT = 6;
    static const int nvec[NKERNEL] = {6, 2, 3, 0, 2, 1, 1, 2, 2, 3, 1, 1, 1, 3, 4, 6, 3, 3, 3, 3, 2};
    static const int maxvar[NKERNEL] = {31, 1, 3, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (kernel < 0 || kernel >= NKERNEL || variant < 0 || variant > maxvar[kernel] || n < 1 || n > (1 << 30) || !ipar || !scal || !vin ||
        !vout || !red || !part_out || !grid || !pub || npart < 0)
        return ERROR_INPUT_PAR;
    for (int k = 0; k < nvec[kernel]; ++k)
        if (!vin[k]) return ERROR_INPUT_PAR;
    const bool folded = (kernel == CG_UPDATE || kernel == AXPBY_BETA || kernel == MGS_STEP) && (variant & 1);
    if (kernel == CG_UPDATE && (variant & 8) && (variant & 16)) return ERROR_INPUT_PAR;   // one diagonal source
    if (folded ? (npart < 1 || npart > MAXGRID || !part_in) : (kernel != FINALIZE && npart != 0)) return ERROR_INPUT_PAR;
    int nq = 0;
    unsigned maxmask = 0u;
    size_t len[NSLOT] = {(size_t)n, (size_t)n, (size_t)n, (size_t)n, (size_t)n, (size_t)n};
    if (kernel == FINALIZE) {   // n = G partials of each of ipar[0] quantities
        nq = ipar[0]; maxmask = (unsigned)ipar[1];
        if (nq < 1 || nq > 8 || n > MAXGRID || npart != nq * n || !part_in) return ERROR_INPUT_PAR;
    } else if (kernel == BSR_DINV_APPLY) {
        const int nb = ipar[0];
        if (nb < 1 || n % nb != 0 || (long long)n * nb > (1ll << 30)) return ERROR_INPUT_PAR;
        len[0] = (size_t)n * nb;
    } else if (kernel == PACK) {   // n = nsend, ipar[0] = length of v
        const int nv = ipar[0];
        if (nv < 1 || !idx) return ERROR_INPUT_PAR;
        for (int i = 0; i < n; ++i)
            if (idx[i] < 0 || idx[i] >= nv) return ERROR_INPUT_PAR;
        len[0] = (size_t)nv;
    }
    if (ctx_init() < 0) return ERROR_MISC;
    hipStream_t s = g_ctx.stream;
    std::unique_ptr<TmpVec> v[NSLOT];
    double* d[NSLOT] = {};
    for (int k = 0; k < nvec[kernel]; ++k) {
        v[k].reset(new TmpVec(vin[k], len[k]));
        if (!(d[k] = v[k]->d)) return ERROR_ALLOC_MEM;
    }
    TmpVec hh(nullptr, 4);   // the Hessenberg column of a GMRES workspace (k_mgs_step)
    int* d_idx = nullptr;
    struct IdxGuard { int*& p; ~IdxGuard() { if (p) (void)hipFree(p); } } idx_guard{d_idx};
    if (!hh.d) return ERROR_ALLOC_MEM;
    if (kernel == PACK) {
        HIPCK(hipMalloc(&d_idx, sizeof(int) * (size_t)n));
        HIPCK(hipMemcpy(d_idx, idx, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    }
    // every scalar slot starts as NaN (all bits set): a slot the kernel should have written, and did not, shows
    HIPCK(hipMemset(g_ctx.d_red, 0xff, sizeof(double) * RED_SLOTS));
    HIPCK(hipMemset(hh.d, 0xff, sizeof(double) * 4));
    auto put = [&](double* dst, const double* src, size_t cnt) { return hipMemcpy(dst, src, sizeof(double) * cnt, hipMemcpyHostToDevice); };
    if (npart > 0) HIPCK(put(g_ctx.d_partials, part_in, (size_t)npart));
    constexpr int ZR_SLOT = 12;   // pcg.hip.h: (z, r) of this and of the previous iteration
    const double* partials = g_ctx.d_partials;   // where the kernel left its partials
    const double* pub_dev = nullptr;
    double* red_dev = g_ctx.d_red;
    int G = 0;
    auto cd = [](double* p) { return (const double*)p; };
    switch (kernel) {
        case CG_UPDATE: {   // vectors p, t, u, r, zx, zdiag; scal temp1, (t,p), zomega, zdiag_value
            const bool t1dev = variant & 2, full = variant & 4, zarr = variant & 8, zval = variant & 16;
            G = vec_grid(n);
            if (!folded) HIPCK(put(g_ctx.d_red + 8, scal + 1, 1));
            if (t1dev) HIPCK(put(g_ctx.d_red + ZR_SLOT, scal + 0, 1));
            double* const upd = folded ? g_ctx.d_partials2 : g_ctx.d_partials;
            hipLaunchKernelGGL(k_cg_update, dim3(G), dim3(BLOCK), 0, s, n, t1dev ? std::nan("") : scal[0], cd(g_ctx.d_red + 8),
                               folded ? cd(g_ctx.d_partials) : (const double*)nullptr, folded ? npart : 0, cd(d[0]), cd(d[1]), d[2], d[3], upd,
                               full ? 1 : 0, folded ? g_ctx.d_red + 8 : (double*)nullptr, (zarr || zval) ? d[4] : (double*)nullptr,
                               zarr ? cd(d[5]) : (const double*)nullptr, scal[2], t1dev ? cd(g_ctx.d_red + ZR_SLOT) : (const double*)nullptr,
                               scal[3]);
            nq = full ? 5 : 1; maxmask = full ? 0x8u : 0u; partials = upd; pub_dev = g_ctx.d_red + 8;
        } break;
        case AXPBY_BETA:   // vectors x, y; scal num, den
            G = vec_grid(n / 2 + 1);
            if (!folded) HIPCK(put(g_ctx.d_red + ZR_SLOT + 1, scal + 0, 1));
            HIPCK(put(g_ctx.d_red + ZR_SLOT, scal + 1, 1));
            hipLaunchKernelGGL(k_axpby_beta, dim3(G), dim3(BLOCK), 0, s, n, cd(d[0]), cd(g_ctx.d_red + ZR_SLOT + 1), cd(g_ctx.d_red + ZR_SLOT),
                               d[1], cd(g_ctx.d_partials), folded ? npart : 0, g_ctx.d_red + ZR_SLOT + 1);
            pub_dev = g_ctx.d_red + ZR_SLOT + 1;
            break;
        case MGS_STEP: {   // vectors pj, pi, pnext; scal h
            double* const pnext = (variant & 2) ? d[2] : nullptr;
            G = vec_grid(n);
            if (folded) {
                double* const mine = g_ctx.d_partials2 + 4 * MAXGRID;
                hipLaunchKernelGGL(k_mgs_step, dim3(G), dim3(BLOCK), 0, s, n, (const double*)nullptr, cd(d[0]), d[1], cd(pnext), mine,
                                   cd(g_ctx.d_partials), npart, hh.d);
                partials = mine;
            } else {
                HIPCK(put(hh.d, scal + 0, 1));
                hipLaunchKernelGGL(k_mgs_step, dim3(G), dim3(BLOCK), 0, s, n, cd(hh.d), cd(d[0]), d[1], cd(pnext), g_ctx.d_partials);
            }
            nq = 1; red_dev = hh.d + 1; pub_dev = hh.d;
        } break;
        case FINALIZE: G = n; break;
        case DOT: G = vec_grid(n); hipLaunchKernelGGL(k_dot, dim3(G), dim3(BLOCK), 0, s, n, cd(d[0]), cd(d[1]), g_ctx.d_partials); nq = 1; break;
        case NORMS: G = vec_grid(n); hipLaunchKernelGGL(k_norms, dim3(G), dim3(BLOCK), 0, s, n, cd(d[0]), g_ctx.d_partials); nq = 2; maxmask = 0x2u; break;
        case NORM1_NAN: G = vec_grid(n); hipLaunchKernelGGL(k_norm1_nan, dim3(G), dim3(BLOCK), 0, s, n, cd(d[0]), g_ctx.d_partials); nq = 2; break;
        case AXPY: G = vec_grid(n / 2 + 1); hipLaunchKernelGGL(k_axpy, dim3(G), dim3(BLOCK), 0, s, n, scal[0], cd(d[0]), d[1]); break;
        case AXPBY: G = vec_grid(n / 2 + 1); hipLaunchKernelGGL(k_axpby, dim3(G), dim3(BLOCK), 0, s, n, scal[0], cd(d[0]), scal[1], d[1]); break;
        case AXPYZ:   // vectors x, y, z; variant 1: z is x, 2: z is y
            G = vec_grid(n);
            hipLaunchKernelGGL(k_axpyz, dim3(G), dim3(BLOCK), 0, s, n, scal[0], cd(d[0]), cd(d[1]), d[variant == 1 ? 0 : variant == 2 ? 1 : 2]);
            break;
        case AXPY_SELF: G = vec_grid(n); hipLaunchKernelGGL(k_axpy_self, dim3(G), dim3(BLOCK), 0, s, n, scal[0], d[0]); break;
        case SCALE: G = vec_grid(n); hipLaunchKernelGGL(k_scale, dim3(G), dim3(BLOCK), 0, s, n, scal[0], d[0]); break;
        case SET: G = vec_grid(n); hipLaunchKernelGGL(k_set, dim3(G), dim3(BLOCK), 0, s, n, scal[0], d[0]); break;
        case POLY_SCALE: G = vec_grid(n); hipLaunchKernelGGL(k_poly_scale, dim3(G), dim3(BLOCK), 0, s, n, cd(d[0]), cd(d[1]), d[2]); break;
        case POLY_START:   // vectors dinv, rbar, v0, v1; scal k1, k2, k3
            G = vec_grid(n);
            hipLaunchKernelGGL(k_poly_start, dim3(G), dim3(BLOCK), 0, s, n, scal[0], scal[1], scal[2], cd(d[0]), cd(d[1]), d[2], d[3]);
            break;
        case POLY_STEP:   // vectors dinv, r, rbar, v0, v1, vnew; scal k4, k5
            G = vec_grid(n);
            hipLaunchKernelGGL(k_poly_step, dim3(G), dim3(BLOCK), 0, s, n, scal[0], scal[1], cd(d[0]), cd(d[1]), d[2], d[3], d[4], d[5]);
            break;
        case JACOBI_ZERO: G = vec_grid(n); hipLaunchKernelGGL(k_jacobi_zero, dim3(G), dim3(BLOCK), 0, s, n, scal[0], cd(d[0]), cd(d[1]), d[2]); break;
        case L1_ZERO: G = vec_grid(n); hipLaunchKernelGGL(k_l1_zero, dim3(G), dim3(BLOCK), 0, s, n, cd(d[0]), cd(d[1]), d[2]); break;
        case DIAG_PRECOND: G = vec_grid(n); hipLaunchKernelGGL(k_diag_precond, dim3(G), dim3(BLOCK), 0, s, n, cd(d[0]), cd(d[1]), d[2]); break;
        case BSR_DINV_APPLY: G = vec_grid(n); hipLaunchKernelGGL(k_bsr_dinv_apply, dim3(G), dim3(BLOCK), 0, s, n, ipar[0], cd(d[0]), cd(d[1]), d[2]); break;
        default: G = vec_grid(n); hipLaunchKernelGGL(k_pack, dim3(G), dim3(BLOCK), 0, s, n, (const int*)d_idx, cd(d[0]), d[1]); break;
    }
    if (nq > 0) hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, s, partials, G, nq, maxmask, red_dev);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(s));
    for (int k = 0; k < nvec[kernel]; ++k)
        if (vout[k]) HIPCK(hipMemcpy(vout[k], d[k], sizeof(double) * len[k], hipMemcpyDeviceToHost));
    if (nq > 0) {
        HIPCK(hipMemcpy(red, red_dev, sizeof(double) * nq, hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(part_out, partials, sizeof(double) * (size_t)nq * G, hipMemcpyDeviceToHost));
    }
    if (pub_dev) HIPCK(hipMemcpy(pub, pub_dev, sizeof(double), hipMemcpyDeviceToHost));
    grid[0] = G; grid[1] = nq;
    return FASP_SUCCESS;
}

// CPU test entry: the sliced-ELL coding of A as upload_csr would build it (device_csr.hip.h, build_sell), decoded again and walked on the host
int fasp_hip_sell_selftest(const dCSRmat* A, int cap_percent, int* info, double* bytes, int* ia_out, int* ja_out, double* val_out, const double* x, double* y)
{
    if (!A || !info || A->row < 0 || A->nnz < 0) return ERROR_INPUT_PAR;
    HostCSR M;
    M.row = A->row; M.col = A->col; M.nnz = A->nnz;
    M.ia.view(A->IA, (size_t)A->row + 1); M.ja.view(A->JA, (size_t)std::max(A->nnz, 1)); M.val.view(A->val, (size_t)std::max(A->nnz, 1));
    SellHost S;
    int why = 0;
    const bool ok = build_sell(M, S, cap_percent > 0 ? cap_percent : SELL_CAP_PERCENT, &why);
    info[0] = ok ? 1 : 0; info[1] = why; info[2] = S.nv; info[3] = S.vbits; info[4] = S.obits; info[5] = S.nslice;
    info[6] = ok ? (int)std::min<long long>(S.slots / 64, 0x7fffffff) : 0; info[7] = SELL_MAXV;
    if (bytes) *bytes = ok ? S.bytes(M.row) : 0.0;
    if (!ok) return FASP_SUCCESS;
    if (ia_out && ja_out && val_out) sell_decode_host(S, M.row, ia_out, ja_out, val_out);
    if (x && y) sell_mxv_host(S, M.row, x, y);
    return FASP_SUCCESS;
}

// CPU test entry: plan_csr (device_csr.hip.h) for an operator with these traits (fasp_hip_dev.h has the layout).  No device: the plan
// dereferences nothing, so a pointer that is "set" points at a dummy.
int fasp_hip_csr_plan(const int* traits, int op, int windowed, int want_partials, int* plan, double* bytes)
{
    FASP_ENTRY();
    if (!traits || !plan || op < OP_MXV || op > OP_MXV_DOT) return ERROR_INPUT_PAR;
    static double dummy[1];
    const int* t = traits;
    auto flag = [&](int i) -> void* { return t[i] ? dummy : nullptr; };
    DevCSR M;
    M.row = t[0]; M.col = t[1]; M.nnz = t[2]; M.kind = t[3]; M.lanes = t[4]; M.wrows = t[5]; M.wcap = t[6]; M.nxrows = t[7]; M.plane = t[8];
    M.npat = t[9]; M.npent = t[10]; M.sell_nv = t[11]; M.sell_nslice = t[12]; M.sell_slots = t[13]; M.ntcols = t[14]; M.es_W = t[15]; M.es_nc = t[16];
    M.code = (unsigned char*)flag(17); M.pat = (unsigned short*)flag(18); M.rowbase = (int*)flag(19); M.dpos = (int*)flag(20); M.dup_diag = t[21] != 0;
    M.ja16 = (unsigned short*)flag(22); M.jbase = (int*)flag(23); M.lja16 = (unsigned short*)flag(24); M.sell_code = (unsigned*)flag(25);
    M.es_tab = (int*)flag(26); M.es_ja16 = (unsigned short*)flag(27);
    const CsrPlan p = plan_csr(M, op, windowed || g_tune.split_rows > 0, want_partials != 0);
    const int out[11] = {(int)p.kernel, p.family, p.tile_rows, p.bpc, p.xcd_map, p.tpp, p.nt, p.ja16, p.jbase, p.fused_zr, kernel_family(M, nullptr)};
    std::copy(out, out + 11, plan);
    if (bytes) *bytes = p.bytes;
    return FASP_SUCCESS;
}

// CPU test entries: plan_coarse_spcg (coarse_cg.hip.h) and plan_coarse_bsr (bsr.hip.h) under the tune keys in force (fasp_hip_dev.h has the layouts)
int fasp_hip_coarse_plan(int m, int nnz, const int* ia, int plain_csr, int num_cu, int* plan_out)
{
    FASP_ENTRY();
    if (m < 1 || nnz < 0 || !plan_out) return ERROR_INPUT_PAR;
    CoarseTraits c;
    c.m = m; c.nnz = nnz; c.ia = ia; c.plain_csr = plain_csr != 0; c.num_cu = num_cu;
    c.shared_device = comm_shares_devices(); c.persist_off = g_persist_disabled; c.small_coarse = small_coarse_enabled();
    const CoarsePlan p = plan_coarse_spcg(c, g_tune, nullptr);
    const int out[11] = {p.family, p.p1, p.p2, p.threads, p.blocks, p.lds, p.LD, p.MaxIt, p.lazy, p.dev_start, p.batch};
    std::copy(out, out + 11, plan_out);
    return FASP_SUCCESS;
}

int fasp_hip_bsr_coarse_plan(int nb, int ROW, int NNZ, int* plan_out)
{
    FASP_ENTRY();
    if (nb < 1 || ROW < 1 || NNZ < 0 || (long long)ROW * nb > 0x7fffffff || !plan_out) return ERROR_INPUT_PAR;
    const BsrCoarsePlan p = plan_coarse_bsr(nb, ROW, NNZ, small_coarse_enabled(), g_tune);
    const int out[6] = {p.family, p.LV, p.cache2, p.lds, p.threads, p.blocks};
    std::copy(out, out + 6, plan_out);
    return FASP_SUCCESS;
}

// ... with the traits of the row-group copy behind the 28 (fasp_hip_dev.h): rg_code set, rows per group, groups, 32-bit words of code
int fasp_hip_csr_plan2(const int* traits, int op, int windowed, int want_partials, int* plan, double* bytes)
{
    FASP_ENTRY();
    if (!traits || !plan || op < OP_MXV || op > OP_MXV_DOT) return ERROR_INPUT_PAR;
    static double dummy[1];
    const int* t = traits;
    auto flag = [&](int i) -> void* { return t[i] ? dummy : nullptr; };
    DevCSR M;
    M.row = t[0]; M.col = t[1]; M.nnz = t[2]; M.kind = t[3]; M.lanes = t[4]; M.wrows = t[5]; M.wcap = t[6]; M.nxrows = t[7]; M.plane = t[8];
    M.npat = t[9]; M.npent = t[10]; M.sell_nv = t[11]; M.sell_nslice = t[12]; M.sell_slots = t[13]; M.ntcols = t[14]; M.es_W = t[15]; M.es_nc = t[16];
    M.code = (unsigned char*)flag(17); M.pat = (unsigned short*)flag(18); M.rowbase = (int*)flag(19); M.dpos = (int*)flag(20); M.dup_diag = t[21] != 0;
    M.ja16 = (unsigned short*)flag(22); M.jbase = (int*)flag(23); M.lja16 = (unsigned short*)flag(24); M.sell_code = (unsigned*)flag(25);
    M.es_tab = (int*)flag(26); M.es_ja16 = (unsigned short*)flag(27);
    M.rg_code = (unsigned*)flag(28); M.rg_R = t[29]; M.rg_ng = t[30]; M.rg_words = t[31];
    const CsrPlan p = plan_csr(M, op, windowed || g_tune.split_rows > 0, want_partials != 0);
    const int out[11] = {(int)p.kernel, p.family, p.tile_rows, p.bpc, p.xcd_map, p.tpp, p.nt, p.ja16, p.jbase, p.fused_zr, kernel_family(M, nullptr)};
    std::copy(out, out + 11, plan);
    if (bytes) *bytes = p.bytes;
    return FASP_SUCCESS;
}

// CPU test entry: the row-group coding of A as an upload would build it (device_csr.hip.h, build_rgroup), decoded again and walked on the host
int fasp_hip_rgroup_selftest(const dCSRmat* A, int rows_per_group, int waves, double min_reuse, int* info, double* bytes, int* ia_out, int* ja_out, double* val_out, const double* x, double* y)
{
    if (!A || !info || A->row < 0 || A->nnz < 0 || (rows_per_group != 8 && rows_per_group != 16) || (waves != 2 && waves != 4 && waves != 8)) return ERROR_INPUT_PAR;
    HostCSR M;
    M.row = A->row; M.col = A->col; M.nnz = A->nnz;
    M.ia.view(A->IA, (size_t)A->row + 1); M.ja.view(A->JA, (size_t)std::max(A->nnz, 1)); M.val.view(A->val, (size_t)std::max(A->nnz, 1));
    RGroupHost G;
    int why = 0;
    const bool ok = build_rgroup(M, rows_per_group, min_reuse > 0.0 ? min_reuse : RG_MIN_REUSE, G, &why);
    unsigned long long hsh = 1469598103934665603ull;   // FNV-1a over table, code and values
    auto eat = [&](const void* p, size_t n) { const unsigned char* q = (const unsigned char*)p; for (size_t i = 0; i < n; ++i) { hsh ^= q[i]; hsh *= 1099511628211ull; } };
    if (ok) { eat(G.meta.data(), 4 * G.meta.size()); eat(G.code.data(), 4 * (size_t)(((G.words + 3) & ~3ll) + 4)); eat(G.val.data(), 8 * ((size_t)M.nnz + 2)); }
    info[0] = ok ? 1 : 0; info[1] = why; info[2] = G.R; info[3] = G.ng; info[4] = (int)G.chunks; info[5] = (int)G.ucols; info[6] = (int)G.words;
    info[7] = (int)(hsh & 0x7fffffffu); info[8] = (int)((hsh >> 32) & 0x7fffffffu); info[9] = RG_MIN_ROW;
    if (bytes) *bytes = ok ? rgroup_bytes(M.nnz, G.words, G.ng) : 0.0;
    if (!ok) return FASP_SUCCESS;
    if (ia_out && ja_out && val_out) rgroup_decode_host(G, M.row, ia_out, ja_out, val_out);
    if (x && y) rgroup_mxv_host(G, M.row, waves, x, y);
    return FASP_SUCCESS;
}

// CPU test entry: the tables of k_csr_estream for a matrix with these row pointers, walked on the host (device_csr.hip.h)
int fasp_hip_estream_selftest(const int* ia, int nrow, int nnz, int per_wave, int wmax, int* info)
{
    if (!ia || nrow < 1 || nnz < 1 || per_wave < 8 || wmax < 32) return ERROR_INPUT_PAR;
    return estream_selftest_host(ia, nrow, nnz, per_wave, wmax, info);
}

// Measured device ceilings beside the roofline: a 16-byte-per-lane read, copy and triad over buffers of
// `bytes` each (use >= 512 MiB: beyond the 256 MiB Infinity Cache).  out[0..2] = GB/s of read, copy (read + write
// counted), triad (two reads + one write counted).  Returns 0 or a negative error code.
int fasp_hip_measure_ceilings(double* out, size_t bytes, int reps)
{
    FASP_ENTRY();
    if (!out || bytes < (1u << 20) || reps <= 0) return ERROR_INPUT_PAR;
    if (ctx_init() != FASP_SUCCESS) return ERROR_MISC;
    f64x2_t *p = nullptr, *q = nullptr, *r = nullptr;
    HIPCK(hipMalloc(&p, bytes)); HIPCK(hipMalloc(&q, bytes)); HIPCK(hipMalloc(&r, bytes));
    HIPCK(hipMemsetAsync(p, 0, bytes, g_ctx.stream)); HIPCK(hipMemsetAsync(q, 0, bytes, g_ctx.stream));
    HIPCK(hipMemsetAsync(r, 0, bytes, g_ctx.stream));
    const size_t n16 = bytes / 16;
    hipEvent_t e0, e1;
    HIPCK(hipEventCreate(&e0)); HIPCK(hipEventCreate(&e1));
    const int grid = 4 * g_ctx.num_cu;
    for (int which = 0; which < 3; ++which) {
        auto run = [&]() {
            if (which == 0) hipLaunchKernelGGL(k_read16, dim3(grid), dim3(BLOCK), 0, g_ctx.stream, n16, p, (double*)q);
            else if (which == 1) hipLaunchKernelGGL(k_copy16, dim3(grid), dim3(BLOCK), 0, g_ctx.stream, n16, p, q);
            else hipLaunchKernelGGL(k_triad16, dim3(grid), dim3(BLOCK), 0, g_ctx.stream, n16, 0.5, p, q, r);
        };
        run(); run();
        HIPCK(hipEventRecord(e0, g_ctx.stream));
        for (int i = 0; i < reps; ++i) run();
        HIPCK(hipEventRecord(e1, g_ctx.stream));
        HIPCK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCK(hipEventElapsedTime(&ms, e0, e1));
        out[which] = (double)(which + 1) * (double)bytes * reps / ((double)ms * 1e-3) / 1e9;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(p); (void)hipFree(q); (void)hipFree(r);
    return FASP_SUCCESS;
}

// timed micro-benchmark of one kernel class on a resident level
double fasp_hip_time_kernel(fasp_hip_amg* h, int kind, int level, int reps)
{
    FASP_ENTRY();
    if (!h || level < 0 || level >= (int)h->L.size() || reps <= 0) return -1.0;
    DevLevel& D = h->L[level];
    const int n = D.A.row;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.0;
    double* x = D.xa; double* y = D.xb; double* w = D.w;
    auto run = [&]() {
        switch (kind) {
            case 0: d_mxv(D.A, x, y); break;
            case 1: d_aAxpy(-1.0, D.A, x, y); break;
            case 2: { CsrArgs a{}; a.x = x; a.y = y; a.b = w; a.diag = D.diag; a.omega = 0.6667; launch_csr<OP_JACOBI>(D.A, a); } break;
            case 3: hipLaunchKernelGGL(k_dot, dim3(vec_grid(n)), dim3(BLOCK), 0, g_ctx.stream, n, x, y, g_ctx.d_partials); break;
            case 4: d_axpy(n, 0.5, x, y); break;
            case 5: { CsrArgs a{}; a.x = x; a.y = y; a.dotv = x; a.partials = g_ctx.d_partials; launch_csr<OP_MXV_DOT>(D.A, a); } break;
            case 6: if (D.R.ia) d_mxv(D.R, w, h->L[level + 1].xa); break;
            case 7: if (D.P.ia) d_aAxpy(1.0, D.P, h->L[level + 1].xa, y); break;
            case 8:   // the plain stream bound of a level: its values (and as many bytes again for every 4 of index data) read 16 bytes per lane
                if (D.A.val) hipLaunchKernelGGL(k_read16, dim3(2048), dim3(BLOCK), 0, g_ctx.stream, (size_t)D.A.nnz / 2, (const f64x2_t*)D.A.val, y);
                break;
            case 10: case 11: case 12: case 13: (void)seq_sweep(h, level, kind - 10, 1, 1.0); break;   // GS sweep: ascending, descending, C rows, F rows
            default: break;
        }
    };
    (void)hipMemsetAsync(x, 0, sizeof(double) * n, g_ctx.stream);
    (void)hipMemsetAsync(y, 0, sizeof(double) * n, g_ctx.stream);
    (void)hipMemsetAsync(w, 0, sizeof(double) * n, g_ctx.stream);
    double* const keep_b = D.b; double* const keep_x = D.x;
    if (kind >= 10) { D.b = w; D.x = x; }   // the sweeps work on the level's own vectors: scratch ones while timing
    if (g_time_cold) {
        // as a solve meets the kernel: one event pair per launch, 512 MB of other data READ in between (1) -- nothing of the operator or the
        // vectors waits in the Infinity Cache; back to back, a level of up to 256 MB is served from there -- or WRITTEN in between (2): the
        // launch also pays for the write-back of what its predecessors left there
        double* big = nullptr;
        const size_t bigb = (size_t)512 << 20;
        if (hipMalloc(&big, bigb + 4096) != hipSuccess) return -1.0;
        (void)hipMemsetAsync(big, 0, bigb, g_ctx.stream);
        double tot = 0.0;
        for (int i = 0; i < reps + 1; ++i) {
            if (g_time_cold >= 2) (void)hipMemsetAsync(big, 0, bigb, g_ctx.stream);
            else hipLaunchKernelGGL(k_read16, dim3(1024), dim3(BLOCK), 0, g_ctx.stream, bigb / 16, (const f64x2_t*)big, big + bigb / 8);
            (void)hipEventRecord(e0, g_ctx.stream);
            run();
            (void)hipEventRecord(e1, g_ctx.stream);
            (void)hipEventSynchronize(e1);
            float ms1 = 0.f;
            (void)hipEventElapsedTime(&ms1, e0, e1);
            if (i >= 1) tot += ms1;
        }
        (void)hipFree(big);
        D.b = keep_b; D.x = keep_x;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        return tot / reps;
    }
    run(); run();
    (void)hipEventRecord(e0, g_ctx.stream);
    for (int i = 0; i < reps; ++i) run();
    (void)hipEventRecord(e1, g_ctx.stream);
    (void)hipEventSynchronize(e1);
    D.b = keep_b; D.x = keep_x;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return (double)ms / reps;
}


// Test entry: one row operation of launch_csr on an operator of a resident level, with the vectors given and returned on the host.
// which: 0 A, 1 P, 2 R.  op: the RowOp codes (0 y = M x, 1 y = b - M x, 2 y += M x, 3 y -= M x, 4 y += scalar M x, 5 Jacobi sweep with weight
// scalar (A only), 6 L1-diagonal sweep (A only), 7 y = M x with (y, b)), or 8: y = M x with the first Jacobi sweep of the level the result is
// the right-hand side of written along, y2_i = scalar y_i / b_i.  x: M.col values (ops 5, 6: the iterate); b, y, y2: M.row values.
// red (may be NULL): ops 7 and 5 -- the finished sum of the fused partials, (y, b) or (x_new, b); NaN when the kernel did not produce them.
static int row_op_host(DevLevel& D, int which, int op, const double* x, const double* b, double* y, double* y2, double scalar, double* red)
{
    if (which < 0 || which > 2 || op < 0 || op > 8 || !x || !y) return ERROR_INPUT_PAR;
    const DevCSR& M = which == 0 ? D.A : which == 1 ? D.P : D.R;
    if (!M.ia || ((op == 5 || op == 6) && which != 0) || ((op == 1 || op >= 5) && !b) || (op == 8 && !y2)) return ERROR_INPUT_PAR;
    const size_t nr = (size_t)std::max(M.row, 1), nc = (size_t)std::max(M.col, 1);
    double *dx = nullptr, *db = nullptr, *dy = nullptr, *dy2 = nullptr;
    int st = FASP_SUCCESS;
    auto run = [&]() -> int {
        HIPCK(hipMalloc(&dx, 8 * nc)); HIPCK(hipMalloc(&db, 8 * nr)); HIPCK(hipMalloc(&dy, 8 * nr)); HIPCK(hipMalloc(&dy2, 8 * nr));
        HIPCK(hipMemcpy(dx, x, 8 * (size_t)M.col, hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(dy, y, 8 * (size_t)M.row, hipMemcpyHostToDevice));
        if (b) HIPCK(hipMemcpy(db, b, 8 * (size_t)M.row, hipMemcpyHostToDevice));
        CsrArgs a{};
        a.x = dx; a.y = dy; a.b = db;
        int G = 0;
        bool have_red = false;
        switch (op) {
            case 0: G = launch_csr<OP_MXV>(M, a); break;
            case 1: G = launch_csr<OP_RESID>(M, a); break;
            case 2: G = launch_csr<OP_ADD>(M, a); break;
            case 3: G = launch_csr<OP_SUB>(M, a); break;
            case 4: a.alpha = scalar; G = launch_csr<OP_AXPY>(M, a); break;
            case 5:
                a.diag = D.diag; a.omega = scalar;
                if (red) a.partials = g_ctx.d_partials;
                G = launch_csr<OP_JACOBI>(M, a);
                have_red = red && plan_csr(M, OP_JACOBI, false, true).fused_zr;
                break;
            case 6: a.diag = D.l1; a.omega = scalar; G = launch_csr<OP_L1DIAG>(M, a); break;
            case 7: a.b = nullptr; a.dotv = db; a.partials = g_ctx.d_partials; G = launch_csr<OP_MXV_DOT>(M, a); have_red = red != nullptr; break;
            default: a.b = nullptr; a.zx = dy2; a.zdiag = db; a.zomega = scalar; G = launch_csr<OP_MXV>(M, a); break;
        }
        if (red) *red = std::nan("");
        if (have_red) {
            d_finalize(G, 1, 0u, 0, false);
            if (fetch_red(0, 1, red) < 0) return ERROR_MISC;
        }
        HIPCK(hipStreamSynchronize(g_ctx.stream));
        HIPCK(hipMemcpy(y, dy, 8 * (size_t)M.row, hipMemcpyDeviceToHost));
        if (op == 8) HIPCK(hipMemcpy(y2, dy2, 8 * (size_t)M.row, hipMemcpyDeviceToHost));
        return FASP_SUCCESS;
    };
    st = run();
    (void)hipFree(dx); (void)hipFree(db); (void)hipFree(dy); (void)hipFree(dy2);
    return st;
}

int fasp_hip_level_op(fasp_hip_amg* h, int level, int which, int op, const double* x, const double* b, double* y, double* y2, double scalar, double* red)
{
    FASP_ENTRY();
    if (!h || level < 0 || level >= (int)h->L.size()) return ERROR_INPUT_PAR;
    return row_op_host(h->L[level], which, op, x, b, y, y2, scalar, red);
}
// Development / test entry: one smoothing step of a resident level through smooth() (smoothers.hip.h), the way a cycle takes it before
// (post 0) or after (1) the coarse correction, vectors given and returned on the host.  zero_start 1: the step starts from the lazily zero
// iterate (x_zero), x is not read.  The level's right-hand side pointer and lazy flags are put back; its iterate is overwritten.
int fasp_hip_level_smooth(fasp_hip_amg* h, int level, int post, int smoother, int order, int nsweeps, double relax, int ndeg, int zero_start,
                          const double* b, double* x)
{
    FASP_ENTRY();
    if (!h || !b || !x || level < 0 || level >= (int)h->L.size() || h->distributed || (post != 0 && post != 1) ||
        (zero_start != 0 && zero_start != 1) || nsweeps < 0 || ndeg < 0) return ERROR_INPUT_PAR;
    DevLevel& D = h->L[level];
    if (!D.replicated || D.swz || !D.x || !D.xo) return ERROR_INPUT_PAR;
    const size_t n = (size_t)D.A.row;
    double* const b0 = D.b;
    const bool xz0 = D.x_zero, ps0 = D.presmoothed;
    double* db = nullptr;
    HIPCK(hipMalloc(&db, sizeof(double) * std::max<size_t>((size_t)D.nvec, 1)));
    auto run = [&]() -> int {
        HIPCK(hipMemcpyAsync(db, b, sizeof(double) * n, hipMemcpyHostToDevice, g_ctx.stream));
        if (!zero_start) HIPCK(hipMemcpyAsync(D.x, x, sizeof(double) * n, hipMemcpyHostToDevice, g_ctx.stream));
        D.b = db; D.x_zero = zero_start != 0; D.presmoothed = false;
        const int st = smooth(h, level, post != 0, smoother, order, nsweeps, relax, ndeg);
        if (st < 0) return st;
        materialise_zero(D);
        HIPCK(hipStreamSynchronize(g_ctx.stream));
        if (seq_err_check() < 0) return ERROR_MISC;
        HIPCK(hipMemcpy(x, D.x, sizeof(double) * n, hipMemcpyDeviceToHost));
        return FASP_SUCCESS;
    };
    const int st = run();
    (void)hipStreamSynchronize(g_ctx.stream);
    D.b = b0; D.x_zero = xz0; D.presmoothed = ps0;
    (void)hipFree(db);
    return st;
}
// ... and of a matrix given on the host, uploaded the way a level's A is (coding, kernel selection, diagonal tables).  A rectangular matrix is
// uploaded the way a transfer operator is: no diagonal tables, so ops 5 and 6 return ERROR_INPUT_PAR.  *kind_out: the family code of
// fasp_hip_amg_kernel_info (kernel_family, device_csr.hip.h: the plan of y = M x on the whole operator).
int fasp_hip_matrix_op(const dCSRmat* A, int op, const double* x, const double* b, double* y, double* y2, double scalar, double* red, int* kind_out)
{
    FASP_ENTRY();
    if (!A || ctx_init() < 0) return ERROR_INPUT_PAR;
    HostCSR M;
    M.row = A->row; M.col = A->col; M.nnz = A->nnz;
    M.ia.view(A->IA, (size_t)A->row + 1); M.ja.view(A->JA, (size_t)std::max(A->nnz, 1)); M.val.view(A->val, (size_t)std::max(A->nnz, 1));
    DevLevel D;
    int st;
    {
        HostThreads team;
        st = upload_csr(M, D.A);
        if (st >= 0) st = upload_rgroup(M, D.A);
        if (st >= 0 && M.row == M.col) st = upload_diag(M, D);
    }
    if (st >= 0 && (op == 5 || op == 6) && !D.diag) st = ERROR_INPUT_PAR;
    if (st >= 0) st = row_op_host(D, 0, op, x, b, y, y2, scalar, red);
    if (kind_out) *kind_out = kernel_family(D.A, nullptr);   // under the tune keys of this call: the family of y = M x on the whole operator
    free_level(D);
    return st;
}

// Test entry: the traits plan_csr reads (fasp_hip_csr_plan's layout, fasp_hip_dev.h) of the device copy fasp_hip_matrix_op makes of A -- the same
// upload_csr, and upload_diag for a square matrix -- so that a test can ask fasp_hip_csr_plan for the kernel of every operation on that very copy.
int fasp_hip_matrix_traits(const dCSRmat* A, int* traits)
{
    FASP_ENTRY();
    if (!A || !traits || ctx_init() < 0) return ERROR_INPUT_PAR;
    HostCSR M;
    M.row = A->row; M.col = A->col; M.nnz = A->nnz;
    M.ia.view(A->IA, (size_t)A->row + 1); M.ja.view(A->JA, (size_t)std::max(A->nnz, 1)); M.val.view(A->val, (size_t)std::max(A->nnz, 1));
    DevLevel D;
    int st;
    {
        HostThreads team;
        st = upload_csr(M, D.A);
        if (st >= 0) st = upload_rgroup(M, D.A);
        if (st >= 0 && M.row == M.col) st = upload_diag(M, D);
    }
    if (st >= 0) {
        const DevCSR& d = D.A;
        const int out[28] = {d.row, d.col, d.nnz, d.kind, d.lanes, d.wrows, d.wcap, d.nxrows, d.plane, d.npat, d.npent, d.sell_nv, d.sell_nslice,
                             (int)d.sell_slots, (int)d.ntcols, d.es_W, d.es_nc, d.code != nullptr, d.pat != nullptr, d.rowbase != nullptr, d.dpos != nullptr,
                             d.dup_diag, d.ja16 != nullptr, d.jbase != nullptr, d.lja16 != nullptr, d.sell_code != nullptr, d.es_tab != nullptr, d.es_ja16 != nullptr};
        std::copy(out, out + 28, traits);
    }
    free_level(D);
    return st < 0 ? st : FASP_SUCCESS;
}

// ... and the 32 traits of fasp_hip_csr_plan2's layout (the row-group copy behind the 28), under the tune keys in force at the call
int fasp_hip_matrix_traits2(const dCSRmat* A, int* traits)
{
    FASP_ENTRY();
    if (!A || !traits || ctx_init() < 0) return ERROR_INPUT_PAR;
    HostCSR M;
    M.row = A->row; M.col = A->col; M.nnz = A->nnz;
    M.ia.view(A->IA, (size_t)A->row + 1); M.ja.view(A->JA, (size_t)std::max(A->nnz, 1)); M.val.view(A->val, (size_t)std::max(A->nnz, 1));
    DevLevel D;
    int st;
    {
        HostThreads team;
        st = upload_csr(M, D.A);
        if (st >= 0) st = upload_rgroup(M, D.A);
        if (st >= 0 && M.row == M.col) st = upload_diag(M, D);
    }
    if (st >= 0) {
        const DevCSR& d = D.A;
        const int out[32] = {d.row, d.col, d.nnz, d.kind, d.lanes, d.wrows, d.wcap, d.nxrows, d.plane, d.npat, d.npent, d.sell_nv, d.sell_nslice,
                             (int)d.sell_slots, (int)d.ntcols, d.es_W, d.es_nc, d.code != nullptr, d.pat != nullptr, d.rowbase != nullptr, d.dpos != nullptr,
                             d.dup_diag, d.ja16 != nullptr, d.jbase != nullptr, d.lja16 != nullptr, d.sell_code != nullptr, d.es_tab != nullptr, d.es_ja16 != nullptr,
                             d.rg_code != nullptr, d.rg_R, d.rg_ng, (int)d.rg_words};
        std::copy(out, out + 32, traits);
    }
    free_level(D);
    return st < 0 ? st : FASP_SUCCESS;
}

// Development / test entry: one operator through the resident upload path (lossless coding, kernel selection as for a
// hierarchy level) timed with HIP events on the launch stream.  op: 0 y = A x, 1 y -= A x, 2 Jacobi sweep, 5 y = A x
// fused with (y, x).  Returns milliseconds per launch (< 0: error); *kind_out = the family (codes of fasp_hip_amg_kernel_info) of
// the plan of the operation that was timed.
double fasp_hip_time_matrix(const dCSRmat* A, int op, int reps, int* kind_out)
{
    FASP_ENTRY();
    if (!A || reps <= 0 || ctx_init() < 0) return -1.0;
    HostCSR M;
    M.row = A->row; M.col = A->col; M.nnz = A->nnz;
    M.row_aligned = A->col > A->row && std::getenv("FASP_HIP_TIME_ROW_ALIGNED") != nullptr;   // (tools/perf_local_op.py: a rank's rows of a partitioned level)
    M.ia.view(A->IA, (size_t)A->row + 1); M.ja.view(A->JA, (size_t)std::max(A->nnz, 1)); M.val.view(A->val, (size_t)std::max(A->nnz, 1));
    DevCSR D;
    {
        HostThreads team;
        if (upload_csr(M, D) < 0 || upload_rgroup(M, D) < 0) { D.release(); return -1.0; }
    }
    const int n = A->row, nc = A->col;
    double *x = nullptr, *y = nullptr, *w = nullptr, *dg = nullptr;
    if (hipMalloc(&x, 8 * (size_t)std::max(nc, n)) != hipSuccess || hipMalloc(&y, 8 * (size_t)n) != hipSuccess ||
        hipMalloc(&w, 8 * (size_t)n) != hipSuccess || hipMalloc(&dg, 8 * (size_t)n) != hipSuccess) { D.release(); return -1.0; }
    (void)hipMemsetAsync(x, 0, 8 * (size_t)std::max(nc, n), g_ctx.stream);
    (void)hipMemsetAsync(y, 0, 8 * (size_t)n, g_ctx.stream);
    (void)hipMemsetAsync(w, 0, 8 * (size_t)n, g_ctx.stream);
    hipLaunchKernelGGL(k_set, dim3(vec_grid(n)), dim3(BLOCK), 0, g_ctx.stream, n, 1.0, dg);
    const int row_op = op == 0 ? OP_MXV : op == 1 ? OP_SUB : op == 2 ? OP_JACOBI : OP_MXV_DOT;
    auto run = [&]() {
        switch (row_op) {
            case OP_MXV: d_mxv(D, x, y); break;
            case OP_SUB: d_aAxpy(-1.0, D, x, y); break;
            case OP_JACOBI: { CsrArgs a{}; a.x = x; a.y = y; a.b = w; a.diag = dg; a.omega = 0.6667; launch_csr<OP_JACOBI>(D, a); } break;
            default: { CsrArgs a{}; a.x = x; a.y = y; a.dotv = x; a.partials = g_ctx.d_partials; launch_csr<OP_MXV_DOT>(D, a); } break;
        }
    };
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    run(); run();
    (void)hipEventRecord(e0, g_ctx.stream);
    for (int i = 0; i < reps; ++i) run();
    (void)hipEventRecord(e1, g_ctx.stream);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (kind_out) *kind_out = plan_csr(D, row_op, g_tune.split_rows > 0, false).family;
    (void)hipFree(x); (void)hipFree(y); (void)hipFree(w); (void)hipFree(dg);
    D.release();
    return (double)ms / reps;
}

}  // extern "C"
