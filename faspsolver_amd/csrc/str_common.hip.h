// str_common.hip.h -- what the structured (dSTRmat) parts share: the device band store, the grid rule, the level schedulers, the dispatch on
// the block width.  Part of the single translation unit solver.hip (included there before str.hip.h; not a stand-alone header).
// Host code but for the device-memory owner; every decision below is stated here and nowhere else.

namespace fasp_str {

// device allocations that live as long as their owner
struct DevPool {
    std::vector<void*> owned;
    DevPool() = default;
    DevPool(const DevPool&) = delete;
    DevPool& operator=(const DevPool&) = delete;
    ~DevPool() { for (void* p : owned) (void)hipFree(p); }
    template <class T> bool get(T** dst, size_t count)
    {
        void* p = nullptr;
        if (hipMalloc(&p, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) { (void)hipGetLastError(); return false; }
        owned.push_back(p);
        *dst = static_cast<T*>(p);
        return true;
    }
};

// f(std::integral_constant<int, NC>{}) for the block width nc = 1 .. 7: the one dispatch of a launch on NC
template <class F>
static int str_for_nc(int nc, F&& f)
{
    switch (nc) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        default: return ERROR_INPUT_PAR;
    }
}

// The coefficient block (nc x nc, row-major) of grid row i in band `slot` of a dSTRmat: slot < 0 the diagonal, otherwise offdiag[slot], where
// a lower band is stored by column.  nullptr where the term does not exist by the reference's index rule, 0 <= i + offset < ngrid.
static const double* str_block(const dSTRmat* A, int slot, int i)
{
    const size_t nc2 = (size_t)A->nc * A->nc;
    if (slot < 0) return A->diag + (size_t)i * nc2;
    const long long off = A->offsets[slot], j = i + off;
    if (j < 0 || j >= A->ngrid) return nullptr;
    return A->offdiag[slot] + (size_t)(off < 0 ? j : i) * nc2;
}
static bool str_block_is_zero(const double* c, int nc2)
{
    for (int e = 0; e < nc2; ++e)
        if (!(c[e] == 0.0)) return false;   // (a NaN is not a zero)
    return true;
}

// The device band store, index-free: band k is `stride` doubles long (ngrid nc^2 rounded up to 8 doubles, so that every band starts on a
// 64-byte boundary), the block of grid point i sits at i nc^2 whatever the offset, the slots without a term hold zeros.
struct StrBands {
    double* val = nullptr;
    size_t  stride = 0;
    int     nb = 0;
    std::vector<int> off;   // the offset of every band (0: the diagonal)
    double* band(int k) const { return val + (size_t)k * stride; }
    // picks: the bands to hold, as str_block names them; each must have a term (|offset| < ngrid, or ngrid == 0).  The memory is pool's.
    bool init(DevPool& pool, const dSTRmat* A, const std::vector<int>& picks)
    {
        const size_t nc2 = (size_t)A->nc * A->nc;
        nb = (int)picks.size();
        stride = ((size_t)A->ngrid * nc2 + 7) / 8 * 8;
        off.resize(picks.size());
        if (!pool.get(&val, stride * picks.size())) return false;
        if (nb && hipMemset(val, 0, sizeof(double) * stride * picks.size()) != hipSuccess) return false;
        for (int k = 0; k < nb; ++k) {
            const int    o = picks[(size_t)k] < 0 ? 0 : A->offsets[picks[(size_t)k]], lo = o < 0 ? -o : 0;   // lo: the first row with a term
            const size_t len = (size_t)A->ngrid - (size_t)std::abs(o);
            off[(size_t)k] = o;
            if (len && hipMemcpy(band(k) + (size_t)lo * nc2, str_block(A, picks[(size_t)k], lo), sizeof(double) * len * nc2, hipMemcpyHostToDevice) != hipSuccess) return false;
        }
        return true;
    }
};

// The grid rule: grid point i = x + gx (y + gy z).  A 2-D grid (one of nx, ny, nz is 1) has lines of nline points and no planes
// (nplane = ngrid, gz = 1); a 3-D grid has lines of nx and planes of nxy.
struct StrGrid {
    int nline = 0, nplane = 0, gx = 0, gy = 0, gz = 0;
    // which direction an offset of the set {+-1, +-nline, +-nplane} steps in (a plane step only where there are planes); false: none
    bool classify(int off, int& dx, int& dy, int& dz) const
    {
        const int m = std::abs(off), sg = off < 0 ? -1 : 1;
        dx = dy = dz = 0;
        if (m == 1) dx = sg;
        else if (m == nline) dy = sg;
        else if (m == nplane && gz > 1) dz = sg;
        else return false;
        return true;
    }
    bool holds(int x, int y, int z) const { return (unsigned)x < (unsigned)gx && (unsigned)y < (unsigned)gy && (unsigned)z < (unsigned)gz; }
};
// why: the reason when the sizes of A describe no such grid (an empty one among them).  The guards run in this order so that nothing
// divides by zero: nline < 2 comes before % nline, nplane < nline (which refuses nxy <= 0) before % nplane.
static bool str_grid(const dSTRmat* A, StrGrid& G, const char** why)
{
    const int ngrid = A->ngrid;
    if (A->nx == 1) { G.nline = A->ny; G.nplane = ngrid; }
    else if (A->ny == 1 || A->nz == 1) { G.nline = A->nx; G.nplane = ngrid; }
    else { G.nline = A->nx; G.nplane = A->nxy; }
    if (G.nline < 2 || G.nline >= ngrid || ngrid % G.nline || G.nplane < G.nline || G.nplane % G.nline || ngrid % G.nplane) { *why = "degenerate grid"; return false; }
    G.gx = G.nline; G.gy = G.nplane / G.nline; G.gz = ngrid / G.nplane;
    return true;
}
// The scan behind "grid-like": every coefficient of band `slot` that the reference would use (the index rule) between two points that are
// not geometric neighbours in the direction (dx, dy, dz) must be exactly 0.0, and where they are, i + offset must be that neighbour (it is for
// every direction classify() names; the ILU's come from its own table).  reaches false: the term reaches no geometric neighbour at all -- a
// plane term of an ILU factor on a 2-D grid; the sweeps never have one, classify() names no plane step there -- so the whole band must be 0.0.
static bool str_offgrid_coefficients_are_zero(const dSTRmat* A, const StrGrid& G, int slot, int dx, int dy, int dz, bool reaches, const char** why)
{
    const int nc2 = A->nc * A->nc, off = A->offsets[slot];
    for (int i = 0; i < A->ngrid; ++i) {
        const double* c = str_block(A, slot, i);
        if (!c) continue;
        const int x = i % G.gx, y = (i / G.gx) % G.gy, z = i / (G.gx * G.gy);
        if (reaches && G.holds(x + dx, y + dy, z + dz)) {
            if (i + off != (x + dx) + G.gx * ((y + dy) + G.gy * (z + dz))) { *why = "offsets do not match the grid"; return false; }
        } else if (!str_block_is_zero(c, nc2)) { *why = "a non-zero (or NaN) coefficient between grid points that are not geometric neighbours"; return false; }
    }
    return true;
}

// The anti-diagonal levels x + wy y + wz z of a grid: level l holds the planes zlo[l] .. zlo[l] + npts[l] / gy - 1, enumerated with gy
// points per plane (a kernel drops the (y, z) whose x leaves the grid).
static void str_diag_levels(int gx, int gy, int gz, int wy, int wz, std::vector<int>& zlo, std::vector<int>& npts)
{
    const int inplane = (gx - 1) + wy * (gy - 1), nlev = inplane + wz * (gz - 1) + 1;
    zlo.resize((size_t)nlev); npts.resize((size_t)nlev);
    for (int l = 0; l < nlev; ++l) {
        const int lo = l > inplane ? (l - inplane + wz - 1) / wz : 0, hi = std::min(gz - 1, l / wz);
        zlo[(size_t)l] = lo; npts[(size_t)l] = (hi - lo + 1) * gy;
    }
}

// The dependency levels of a sequence of visits: level(v) = 1 + the largest level among the earlier visits that wrote a point v reads or
// writes, or that read a point v writes (-1: none).  writes(v, f) / reads(v, f) call f(p) for every point p that visit v writes / reads
// besides; each is called twice per visit.  One pass with two arrays per point.  Returns the number of levels.
template <class W, class R>
static int str_visit_levels(int ngrid, size_t nvisits, W&& writes, R&& reads, std::vector<int>& lev)
{
    std::vector<int> lw((size_t)std::max(ngrid, 1), -1), mr((size_t)std::max(ngrid, 1), -1);   // level of the last writer, of the highest reader
    lev.resize(nvisits);
    int nlev = 0;
    for (size_t v = 0; v < nvisits; ++v) {
        int L = -1;
        writes(v, [&](int p) { L = std::max(L, std::max(lw[(size_t)p], mr[(size_t)p])); });
        reads(v, [&](int p) { L = std::max(L, lw[(size_t)p]); });
        lev[v] = ++L;
        writes(v, [&](int p) { lw[(size_t)p] = L; });
        reads(v, [&](int p) { mr[(size_t)p] = std::max(mr[(size_t)p], L); });
        nlev = std::max(nlev, L + 1);
    }
    return nlev;
}

// The visits sorted stably by level: list, and the slice of every level in it (lvl_first, nlev + 1 entries).  widest (may be NULL): the
// longest slice.
static void str_bucket_by_level(const std::vector<int>& seq, const std::vector<int>& lev, int nlev, std::vector<int>& lvl_first, std::vector<int>& list,
                                int* widest)
{
    lvl_first.assign((size_t)nlev + 1, 0);
    for (size_t v = 0; v < seq.size(); ++v) ++lvl_first[(size_t)lev[v] + 1];
    for (int l = 0; l < nlev; ++l) {
        if (widest) *widest = std::max(*widest, lvl_first[(size_t)l + 1]);
        lvl_first[(size_t)l + 1] += lvl_first[(size_t)l];
    }
    std::vector<int> at(lvl_first.begin(), lvl_first.end() - 1);
    list.assign(seq.size(), 0);
    for (size_t v = 0; v < seq.size(); ++v) list[(size_t)at[(size_t)lev[v]]++] = seq[v];
}

// the 16 words of a pipelined form: [0] ticket, [1] error word, [6..7] the host-mapped error word's address (flow_give_up)
static bool str_sync_words(unsigned* dev)
{
    unsigned sync0[16] = {};
    const unsigned long long herr_addr = (unsigned long long)seq_err_device_word();
    std::memcpy(sync0 + 6, &herr_addr, 8);
    return hipMemcpy(dev, sync0, sizeof(sync0), hipMemcpyHostToDevice) == hipSuccess;
}

// body() `reps` times (while its status is >= 0) between two events on the stream; *ms: milliseconds per repetition.  Returns the last
// status, ERROR_MISC without events.
template <class F>
static int time_reps(int reps, F&& body, double* ms)
{
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess) return ERROR_MISC;
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return ERROR_MISC; }
    int st = FASP_SUCCESS;
    (void)hipEventRecord(e0, g_ctx.stream);
    for (int i = 0; i < reps && st >= 0; ++i) st = body();
    (void)hipEventRecord(e1, g_ctx.stream);
    (void)hipEventSynchronize(e1);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    *ms = (double)t / reps;
    return st;
}
}  // namespace fasp_str
