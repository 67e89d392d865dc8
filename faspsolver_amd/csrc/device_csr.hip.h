// device_csr.hip.h -- device matrices: CSR in HBM, lossless coding at upload, kernel selection and launch, BLAS-1 wrappers.
// Part of the single translation unit solver.hip (included there, in this order; not a stand-alone header).

// ---------------------------------------------------------------------------
// device matrices
// ---------------------------------------------------------------------------
struct DevCSR {
    int     row = 0, col = 0, nnz = 0;
    int*    ia  = nullptr;
    int*    ja  = nullptr;
    double* val = nullptr;
    int*    dpos = nullptr;  // storage index of the last diagonal entry per row (-1: none); A matrices only
    bool    dup_diag = false;  // some row stores its diagonal more than once
    bool    sorted = false;    // device copy has every row sorted by column (long-row operators)
    int     lanes = 8;       // vector kernel: lanes cooperating on one row
    int     kind = 0;        // 0 vector, 1 block-level stream, 2 wave-level stream
    int     tile_rows = 256; // block stream kernel: rows per block tile
    int     wrows = 64, wcap = 512;  // wave stream kernel: rows per wave tile, LDS products per wave
    // dictionary coding (k_csr_dict8): present when the matrix has <= 256 distinct (offset, value) pairs
    unsigned char* code = nullptr;
    int*    rowbase = nullptr;  // nullptr: column offsets are relative to the row index
    int*    doff = nullptr;
    double* dval = nullptr;
    // row-pattern coding (k_csr_rowpat): present when the matrix has <= 65536 distinct rows
    unsigned short* pat = nullptr;
    int*    pstart = nullptr;
    int*    plen = nullptr;
    int*    poff = nullptr;
    double* pval = nullptr;
    int     npat = 0, npent = 0;
    unsigned short* ja16 = nullptr;  // JA as 16-bit values (long-row operators with <= 65536 columns, or whose rows each span less than 65536 columns: then relative to jbase)
    int*            jbase = nullptr; // ja16 is relative to the row's smallest column (operators with more than 65536 columns); nullptr: absolute
    int     nxrows = -1;             // k_csr_rowpat4 / 5: rows outside their wave's uniform pattern(s); -1: the pair sweep does not apply
    int     plane = 0;               // square row-pattern-coded operators: the largest column offset of a pattern (the rows of a z-plane of a 3-D grid)
    // local operator of a row-partitioned level: the rows [win_lo, win_hi) read no ghost column (multiples of WIN_ALIGN
    // or the row count; win_hi < 0: no such window worth a split launch) -- they run while the halo is in flight
    int     win_lo = 0, win_hi = -1;
    // k_csr_xtile: distinct columns per 64-row wave tile + 16-bit positions per entry (nullptr: not built)
    unsigned short* lja16 = nullptr;
    int*    tptr = nullptr;
    int*    tcols = nullptr;
    long long ntcols = 0;            // entries of tcols
    // numbering bridge (hierarchy.hip.h, brick renumbering behind a CODED level): the operator itself keeps the natural numbering on both
    // sides -- its row patterns stay what they are -- and the side that lives on the renumbered level is permuted on the fly:
    // bridge_dir 1 (restriction): the product goes to bscratch, y[k] = bscratch[bridge[k]]; 2 (prolongation): bscratch[bridge[k]] = x[k], then the
    // product reads bscratch.  bridge = the level's order (new -> natural), owned by the level; bscratch owned here.
    const int* bridge = nullptr;
    double*    bscratch = nullptr;
    int        bridge_dir = 0;
    // k_csr_estream (kernels3.hip.h): the entry-parallel decomposition of a long-row operator with 16-bit columns (build_estream)
    int*       es_tab = nullptr;    // one allocation: wc[W + 1], centry[nc + 1], crow[nc + 1], hw0[W], np[W], cbase[nc] (relative columns only)
    unsigned short* es_ja16 = nullptr;   // 16-bit columns relative to the chunk's smallest column (operators with > 65536 columns)
    double*    es_part = nullptr;   // 2 W doubles + W counters behind them
    int        es_W = 0, es_nc = 0;
    // k_csr_sell (kernels4.hip.h): value-indexed sliced-ELL form of a mid-length-row operator with few distinct values (build_sell)
    unsigned*      sell_code = nullptr;   // one 32-bit word per slot
    int*           sell_meta = nullptr;   // one allocation: sptr[nslice + 1], sbase[nslice]
    unsigned char* sell_rlen = nullptr;
    double*        sell_tab = nullptr;
    int            sell_nv = 0, sell_obits = 0, sell_nslice = 0;
    long long      sell_slots = 0;
    // k_csr_rgroup (kernels5.hip.h): groups of rg_R consecutive rows over the union of their columns (build_rgroup); beside the plain copy
    unsigned*      rg_code = nullptr;   // per group: chunk value offsets, then one word per union column
    double*        rg_val = nullptr;    // the values in the walk's order
    int*           rg_meta = nullptr;   // per group {word offset, value offset, smallest column, chunks} + a closing entry
    int            rg_R = 0, rg_ng = 0;
    long long      rg_words = 0;
    void    release()
    {
        if (rg_code) (void)hipFree(rg_code);
        if (rg_val) (void)hipFree(rg_val);
        if (rg_meta) (void)hipFree(rg_meta);
        rg_code = nullptr; rg_val = nullptr; rg_meta = nullptr; rg_R = rg_ng = 0; rg_words = 0;
        if (sell_code) (void)hipFree(sell_code);
        if (sell_meta) (void)hipFree(sell_meta);
        if (sell_rlen) (void)hipFree(sell_rlen);
        if (sell_tab) (void)hipFree(sell_tab);
        sell_code = nullptr; sell_meta = nullptr; sell_rlen = nullptr; sell_tab = nullptr; sell_nv = sell_obits = sell_nslice = 0; sell_slots = 0;
        if (es_tab) (void)hipFree(es_tab);
        if (es_part) (void)hipFree(es_part);
        if (es_ja16) (void)hipFree(es_ja16);
        es_tab = nullptr; es_part = nullptr; es_ja16 = nullptr; es_W = es_nc = 0;
        if (bscratch) (void)hipFree(bscratch);
        bscratch = nullptr; bridge = nullptr; bridge_dir = 0;
        if (lja16) (void)hipFree(lja16);
        if (tptr) (void)hipFree(tptr);
        if (tcols) (void)hipFree(tcols);
        lja16 = nullptr; tptr = nullptr; tcols = nullptr;
        nxrows = -1;
        if (ja16) (void)hipFree(ja16);
        ja16 = nullptr;
        if (jbase) (void)hipFree(jbase);
        jbase = nullptr;
        if (ia) (void)hipFree(ia);
        if (ja) (void)hipFree(ja);
        if (val) (void)hipFree(val);
        if (dpos) (void)hipFree(dpos);
        if (code) (void)hipFree(code);
        if (rowbase) (void)hipFree(rowbase);
        if (doff) (void)hipFree(doff);
        if (dval) (void)hipFree(dval);
        if (pat) (void)hipFree(pat);
        if (pstart) (void)hipFree(pstart);
        if (plen) (void)hipFree(plen);
        if (poff) (void)hipFree(poff);
        if (pval) (void)hipFree(pval);
        pat = nullptr; pstart = plen = poff = nullptr; pval = nullptr;
        ia = ja = dpos = rowbase = doff = nullptr; val = dval = nullptr; code = nullptr;
    }
};

// Kernel family per matrix, from its mean row length (measured on MI355X, P7(256)
// hierarchy, profiles/r01_kernel_sweep.md):
//   <= 48 nnz/row : wave-level stream kernel, 64 rows / 512 products per wave
//   longer rows   : sub-wavefront-per-row vector kernel with ~avg/4 lanes per row
static void pick_kernel(DevCSR& M)
{
    const double avg = M.row > 0 ? (double)M.nnz / M.row : 1.0;
    static const double stream_max = std::getenv("FASP_HIP_STREAM_MAX") ? std::atof(std::getenv("FASP_HIP_STREAM_MAX")) : 48.0;
    M.kind = avg <= stream_max ? 2 : 0;  // (kind 3, one workgroup per row, measured slower than L = 64: profiles/)
    // lanes per row of the sub-wavefront kernel, measured on the levels of P7(256) (profiles/r02_lanes_per_row.txt):
    // 16 lanes up to ~300 entries per row, 32 up to ~1000, 64 beyond -- and never so few that rows x lanes leaves
    // the 2048 x 256 threads of the persistent grid unfilled (the last levels: few, very long rows)
    M.lanes = avg < 300.0 ? 16 : avg < 1000.0 ? 32 : 64;
    while (M.lanes < 64 && (double)M.row * M.lanes < 0.75 * MAXGRID * BLOCK) M.lanes *= 2;
    if (avg < 48.0) M.lanes = avg < 3.0 ? 2 : avg < 6.0 ? 4 : avg < 24.0 ? 8 : 16;  // short rows on the sub-wavefront kernel
    // Small transfer operators (fewer 256-row tiles than the chip has block slots): the stream kernel's
    // long per-tile chain is pure latency there; the sub-wavefront kernel spreads the rows over 8-32x
    // more blocks (level-3 restriction of P7(256): 25 -> 10 us).  Square operators keep the stream
    // kernel (its row sums follow the reference's order).
    static const int small_rows = std::getenv("FASP_HIP_SMALL_XFER_ROWS") ? std::atoi(std::getenv("FASP_HIP_SMALL_XFER_ROWS")) : 256 * 1024;
    if (M.kind == 2 && M.row != M.col && M.row < small_rows) M.kind = 0;
    int R = 256;
    while (R < STREAM_MAXR && R * 2 * avg <= 3072.0) R <<= 1;
    M.tile_rows = R;
    M.wrows = 64;
    M.wcap  = 512;
}

// Lossless dictionary coding of a matrix with <= 256 distinct (column - base, value) pairs
// (kernels.hip.h, k_csr_dict8).  base = row index for square matrices, first stored column of
// the row otherwise.  Returns false (nothing allocated) when the matrix has more pairs.
// One-shot callers (fasp_solver_dcsr_krylov_amg / fasp_solver_amg: one solve per setup) skip the
// hashing / re-sorting of the device copies: at 256^3 it costs 3.7 s of host time and saves 0.04 s per solve.
// Resident handles (fasp_hip_amg_create + many fasp_hip_solve) keep it.
static bool g_oneshot_upload = false;
static bool compress_enabled()
{
    if (g_oneshot_upload) return false;
    static int en = -1;
    if (en < 0) { const char* e = std::getenv("FASP_HIP_COMPRESS"); en = (e && std::atoi(e) == 0) ? 0 : 1; }
    return en != 0;
}
struct PairKey { int off; unsigned long long bits; };
static inline unsigned pair_hash(int off, unsigned long long bits)
{
    unsigned long long h = bits * 0x9E3779B97F4A7C15ull + (unsigned long long)(unsigned)off * 0xC2B2AE3D27D4EB4Full;
    return (unsigned)(h >> 40);
}
static bool build_dict8(const HostCSR& M, std::vector<int>& doff, std::vector<double>& dval,
                        Buf<unsigned char>& code, Buf<int>& rowbase)
{
    const bool square = M.row == M.col;
    const int n = M.row;
    if (n <= 0 || M.nnz <= 0) return false;
    constexpr int SLOTS = 1024;
    struct Table {
        int      cnt = 0;
        int      slot_id[SLOTS];
        PairKey  keys[257];
        Table() { for (int& s : slot_id) s = -1; }
        // returns the id of the pair, inserting it; -1 when the table is full
        int find_or_add(int off, unsigned long long bits, bool add)
        {
            unsigned h = pair_hash(off, bits) & (SLOTS - 1);
            for (;;) {
                const int id = slot_id[h];
                if (id < 0) {
                    if (!add || cnt >= 257) return -1;
                    keys[cnt] = PairKey{off, bits};
                    slot_id[h] = cnt;
                    return cnt++;
                }
                if (keys[id].off == off && keys[id].bits == bits) return id;
                h = (h + 1) & (SLOTS - 1);
            }
        }
    };
    auto base_of = [&](int r) { return square ? r : (M.ia[r] < M.ia[r + 1] ? M.ja[M.ia[r]] : 0); };
    auto bits_of = [](double v) { unsigned long long b; std::memcpy(&b, &v, 8); return b; };
    // pass 1: distinct pairs (every thread scans its share, bails out beyond 256)
    const int nt = omp_get_max_threads();
    std::vector<Table> local((size_t)nt);
    bool fail = false;
#pragma omp parallel num_threads(nt)
    {
        Table& T = local[(size_t)omp_get_thread_num()];
#pragma omp for schedule(static)
        for (int r = 0; r < n; ++r) {
            if (fail || T.cnt > 256) continue;
            const int base = base_of(r);
            for (int k = M.ia[r]; k < M.ia[r + 1]; ++k)
                if (T.find_or_add(M.ja[k] - base, bits_of(M.val[k]), true) < 0 || T.cnt > 256) { fail = true; break; }
        }
    }
    if (fail) return false;
    std::vector<PairKey> all;
    for (const Table& T : local) all.insert(all.end(), T.keys, T.keys + T.cnt);
    std::sort(all.begin(), all.end(), [](const PairKey& x, const PairKey& y) {
        return x.off != y.off ? x.off < y.off : x.bits < y.bits; });
    all.erase(std::unique(all.begin(), all.end(), [](const PairKey& x, const PairKey& y) {
        return x.off == y.off && x.bits == y.bits; }), all.end());
    if (all.size() > 256) return false;
    doff.assign(256, 0); dval.assign(256, 0.0);
    Table G;
    for (size_t i = 0; i < all.size(); ++i) {
        G.find_or_add(all[i].off, all[i].bits, true);  // ids in sorted order: deterministic
        doff[i] = all[i].off;
        std::memcpy(&dval[i], &all[i].bits, 8);
    }
    // pass 2: codes
    code.alloc((size_t)M.nnz);
    if (!square) rowbase.alloc((size_t)n);
#pragma omp parallel
    {
        Table T = G;
#pragma omp for schedule(static)
        for (int r = 0; r < n; ++r) {
            const int base = base_of(r);
            if (!square) rowbase[r] = base;
            for (int k = M.ia[r]; k < M.ia[r + 1]; ++k)
                code[k] = (unsigned char)T.find_or_add(M.ja[k] - base, bits_of(M.val[k]), false);
        }
    }
    return true;
}

// Row-pattern coding (kernels.hip.h, k_csr_rowpat): every row is replaced by the id of its
// (column - base, value) list when the matrix has at most 65 536 distinct lists with at most
// 1 M entries in total.  Lossless; ids are numbered by first occurrence, so the coding is
// deterministic.  Returns false when the matrix does not qualify (or on a hash collision).
static bool build_rowpat(const HostCSR& M, Buf<unsigned short>& pat, std::vector<int>& pstart, std::vector<int>& plen,
                         std::vector<int>& poff, std::vector<double>& pval, Buf<int>& rowbase)
{
    // column offsets relative to the row index: square operators, and a rank's rows of a partitioned level (the ghost columns of
    // a boundary plane are numbered like the plane: the same offset in every row of it)
    const bool square = M.row == M.col || M.row_aligned;
    const int n = M.row;
    if (n <= 0 || M.nnz <= 0) return false;
    if ((long long)M.col >= (1ll << 28)) return false;   // the coded kernels form byte offsets of x in 32 bits
    constexpr int MAXPAT = 65535, MAXENT = 1 << 20;   // (id 0xffff is the pad of the pair kernels)
    auto base_of = [&](int r) { return square ? r : (M.ia[r] < M.ia[r + 1] ? M.ja[M.ia[r]] : 0); };
    auto bits_of = [](double v) { unsigned long long b; std::memcpy(&b, &v, 8); return b; };
    auto row_hash = [&](int r) {
        unsigned long long h = 0x9FB21C651E98DF25ull * (unsigned long long)(M.ia[r + 1] - M.ia[r] + 1);
        const int base = base_of(r);
        for (int k = M.ia[r]; k < M.ia[r + 1]; ++k) {
            h ^= (unsigned long long)(unsigned)(M.ja[k] - base) * 0x9E3779B97F4A7C15ull + bits_of(M.val[k]) * 0xC2B2AE3D27D4EB4Full;
            h = (h << 23 | h >> 41) * 0xD6E8FEB86659FD93ull;
        }
        return h ? h : 1ull;
    };
    auto same_row = [&](int r, int q) {  // identical (offset, value) lists
        const int len = M.ia[r + 1] - M.ia[r];
        if (len != M.ia[q + 1] - M.ia[q]) return false;
        const int br = base_of(r), bq = base_of(q);
        for (int j = 0; j < len; ++j) {
            if (M.ja[M.ia[r] + j] - br != M.ja[M.ia[q] + j] - bq) return false;
            if (bits_of(M.val[M.ia[r] + j]) != bits_of(M.val[M.ia[q] + j])) return false;
        }
        return true;
    };
    // pass 1: hash of every row; per-thread sets of (hash -> first row), bounded
    Buf<unsigned long long> rh((size_t)n);
    // worth it only when rows really repeat (>= 8 rows per pattern, below): the sets are sized for that bound, and a
    // small operator is hashed by a small team (a 3 MB set per thread of a 32-thread team costs more than the hashing)
    const int maxpat = std::min<long long>(MAXPAT, n / 8);
    if (maxpat < 1) return false;
    const int nt = std::max(1, std::min(omp_get_max_threads(), n / 32768));
    int slots_pow = 1024;
    while (slots_pow < 4 * (maxpat + 1)) slots_pow *= 2;   // open addressing, <= 25 % load
    const int SLOTS = slots_pow;
    struct Set {
        std::vector<unsigned long long> key;
        std::vector<int> first;
        int cnt = 0, SLOTS;
        explicit Set(int slots) : key((size_t)slots, 0ull), first((size_t)slots, -1), SLOTS(slots) {}
        bool add(unsigned long long h, int r)
        {
            unsigned s = (unsigned)(h >> 20) & (SLOTS - 1);
            for (;;) {
                if (key[s] == 0ull) { key[s] = h; first[s] = r; ++cnt; return true; }
                if (key[s] == h) { if (r < first[s]) first[s] = r; return true; }
                s = (s + 1) & (SLOTS - 1);
            }
        }
        int find(unsigned long long h) const
        {
            unsigned s = (unsigned)(h >> 20) & (SLOTS - 1);
            for (;;) {
                if (key[s] == 0ull) return -1;
                if (key[s] == h) return first[s];
                s = (s + 1) & (SLOTS - 1);
            }
        }
    };
    std::vector<Set*> local((size_t)nt, nullptr);
    bool fail = false;
#pragma omp parallel num_threads(nt)
    {
        Set* S = new Set(SLOTS);
        local[(size_t)omp_get_thread_num()] = S;
#pragma omp for schedule(static)
        for (int r = 0; r < n; ++r) {
            const unsigned long long h = row_hash(r);
            rh[r] = h;
            if (fail) continue;
            S->add(h, r);
            if (S->cnt > maxpat) fail = true;
        }
    }
    Set* Gs = nullptr;
    std::vector<std::pair<int, unsigned long long>> reps;  // (first row, hash)
    if (!fail) {
        Gs = new Set(SLOTS);
        for (Set* S : local)
            if (S)
                for (int s = 0; s < SLOTS && !fail; ++s)
                    if (S->key[s]) { Gs->add(S->key[s], S->first[s]); if (Gs->cnt > maxpat) fail = true; }
    }
    for (Set* S : local) delete S;
    if (fail) { delete Gs; return false; }
    for (int s = 0; s < SLOTS; ++s)
        if (Gs->key[s]) reps.emplace_back(Gs->first[s], Gs->key[s]);
    std::sort(reps.begin(), reps.end());
    long long tot = 0;
    for (auto& q : reps) tot += (M.ia[q.first + 1] - M.ia[q.first] + 7) / 8 * 8;
    // worth it only when rows really repeat: >= 8 rows per pattern and a table << the matrix
    if (tot > MAXENT || (long long)reps.size() * 8 > n || tot * 4 > M.nnz) { delete Gs; return false; }
    // pattern table; the set now maps hash -> pattern id
    pstart.assign(reps.size(), 0); plen.assign(reps.size(), 0);
    poff.clear(); pval.clear();
    for (size_t i = 0; i < reps.size(); ++i) {  // lists padded to multiples of 8 entries with (offset 0, value 0)
        const int r = reps[i].first, base = base_of(r);
        pstart[i] = (int)poff.size();
        plen[i] = M.ia[r + 1] - M.ia[r];
        for (int k = M.ia[r]; k < M.ia[r + 1]; ++k) { poff.push_back(M.ja[k] - base); pval.push_back(M.val[k]); }
        while (poff.size() % 8) { poff.push_back(0); pval.push_back(0.0); }
    }
    for (int s = 0; s < SLOTS; ++s) Gs->first[s] = -1;
    {
        Set& S = *Gs;
        for (size_t i = 0; i < reps.size(); ++i) {
            unsigned s = (unsigned)(reps[i].second >> 20) & (SLOTS - 1);
            while (S.key[s] != reps[i].second) s = (s + 1) & (SLOTS - 1);
            S.first[s] = (int)i;
        }
    }
    pat.alloc((size_t)n);
    if (!square) rowbase.alloc((size_t)n);
    bool collision = false;
#pragma omp parallel for schedule(static) num_threads(nt)
    for (int r = 0; r < n; ++r) {
        const int id = Gs->find(rh[r]);
        if (id < 0 || !same_row(r, reps[(size_t)id].first)) { collision = true; continue; }
        pat[r] = (unsigned short)id;
        if (!square) rowbase[r] = base_of(r);
    }
    delete Gs;
    return !collision;
}

// The "plane" of a square pattern-coded operator: the row distance P (a multiple of 8 tiles of the pair sweep) for which the
// column offsets of the patterns are closest to multiples of P -- the rows of a z-plane of a 3-D grid numbered x-fastest, or of
// whatever the coarse numbering has made of it.  With it an XCD can sweep ONE STRIP (P / 8 rows) of every plane: a row's z-neighbours
// are in the same strip of the neighbouring planes, its x / y neighbours in the same strip except at the strip's edges
// (kernels.hip.h, tile_of, xcd_map == -2).  Cost of a candidate = mean over the pattern entries of min(|o mod+- P|, P / 8) / (P / 8):
// the share of rows whose neighbour lies in another XCD's strip.  0: no candidate below 0.2.
static int grid_plane_of(const std::vector<int>& poff, int nrow)
{
    constexpr int UNIT = 8 * 2 * BLOCK;   // eight tiles of 2 * BLOCK rows
    std::vector<int> cand;
    for (int o : poff) {
        const long long m = std::llabs((long long)o);
        const long long c = (m + UNIT / 2) / UNIT * UNIT;
        if (c >= UNIT && c <= nrow / 4 && std::find(cand.begin(), cand.end(), (int)c) == cand.end() && cand.size() < 64) cand.push_back((int)c);
    }
    int best = 0;
    double best_cost = 0.2;
    for (int P : cand) {
        double cost = 0.0;
        for (int o : poff) {
            long long r = (long long)o % P;
            if (r > P / 2) r -= P;
            if (r < -P / 2) r += P;
            cost += (double)std::min<long long>(std::llabs(r), P / 8) / (P / 8);
        }
        cost /= std::max<size_t>(poff.size(), 1);
        if (cost < best_cost || (cost == best_cost && P > best)) { best_cost = cost; best = P; }
    }
    return best;
}

// 16-bit copy of the column indices (in the order of the device copy) for the operators the
// sub-wavefront kernel serves: their time is the (JA, val) stream, 12 -> 10 bytes per entry.
// (Round 5: operators with MORE than 65536 columns whose every row spans less than 65536 of them -- levels 3 and 4 of P7(256): 257 139 and
// 80 619 rows, spans of a few grid planes -- store their indices relative to the row's smallest column, 4 bytes per row more.)
static bool rows_span_16bit(const int* ia, const int* ja, int row)
{
    int bad = 0;
#pragma omp parallel for schedule(static) reduction(+ : bad)
    for (int i = 0; i < row; ++i) {
        if (ia[i + 1] <= ia[i]) continue;
        int lo = ja[ia[i]], hi = lo;
        for (int k = ia[i] + 1; k < ia[i + 1]; ++k) { lo = std::min(lo, ja[k]); hi = std::max(hi, ja[k]); }
        if (hi - lo >= 65536) ++bad;
    }
    return bad == 0;
}
static int upload_ja16(DevCSR& D, const int* ia_host, const int* ja_dev_order)
{
    static const bool on = !(std::getenv("FASP_HIP_JA16") && std::atoi(std::getenv("FASP_HIP_JA16")) == 0);
    if (!on || D.kind != 0 || D.nnz < 4096) return FASP_SUCCESS;
    const bool relative = D.col > 65536;
    if (relative && !rows_span_16bit(ia_host, ja_dev_order, D.row)) return FASP_SUCCESS;
    Buf<unsigned short> j16((size_t)D.nnz);
    Buf<int> base(relative ? (size_t)D.row : 0);
#pragma omp parallel for schedule(static)
    for (int i = 0; i < D.row; ++i) {
        int lo = 0;
        if (relative) {
            lo = ia_host[i + 1] > ia_host[i] ? ja_dev_order[ia_host[i]] : 0;
            for (int k = ia_host[i]; k < ia_host[i + 1]; ++k) lo = std::min(lo, ja_dev_order[k]);
            base[(size_t)i] = lo;
        }
        for (int k = ia_host[i]; k < ia_host[i + 1]; ++k) j16[k] = (unsigned short)(ja_dev_order[k] - lo);
    }
    HIPCK(hipMalloc(&D.ja16, sizeof(unsigned short) * ((size_t)D.nnz + 8)));
    HIPCK(hipMemset(D.ja16 + D.nnz, 0, sizeof(unsigned short) * 8));   // (k_csr_estream reads whole 16-byte pieces: the slack must hold valid columns)
    HIPCK(hipMemcpy(D.ja16, j16.data(), sizeof(unsigned short) * (size_t)D.nnz, hipMemcpyHostToDevice));
    if (relative) {
        HIPCK(hipMalloc(&D.jbase, sizeof(int) * (size_t)D.row));
        HIPCK(hipMemcpy(D.jbase, base.data(), sizeof(int) * (size_t)D.row, hipMemcpyHostToDevice));
    }
    return FASP_SUCCESS;
}

static int g_device_sort = 1;   // fasp_hip_tune("device_sort", 0): per-row sort of the device copies on the host (A/B tests)
// Stable sort of every row's entries by column ON THE DEVICE: one workgroup per row, bitonic network in LDS over the
// keys (column << 32 | position in the row) -- keys are distinct, so the result is THE stable order, the same the host
// std::stable_sort of the fallback below produces.  P7(256): levels 2-9 carry 15-19 M entries each in rows of 64-3100;
// sorting them on the host cost 0.2-0.5 s per level (2.9 s of the 4.4 s upload), here < 5 ms.
constexpr int SORT_BLK = 256, SORT_MAXLEN = 16384;   // 16384 keys = 128 KB of LDS
__global__ __launch_bounds__(SORT_BLK) void k_sort_rows(int nrow, const int* __restrict__ ia, const int* __restrict__ ja_in,
                                                        const double* __restrict__ val_in, int* __restrict__ ja_out,
                                                        double* __restrict__ val_out, unsigned short* __restrict__ ja16, int* __restrict__ jbase)
{
    extern __shared__ unsigned long long sort_keys[];
    const int tid = threadIdx.x;
    for (int r = blockIdx.x; r < nrow; r += gridDim.x) {
        const int kb = ia[r], len = ia[r + 1] - kb;
        int P = 1;
        while (P < len) P <<= 1;
        for (int i = tid; i < P; i += SORT_BLK)
            sort_keys[i] = i < len ? ((unsigned long long)(unsigned)ja_in[kb + i] << 32) | (unsigned)i : ~0ull;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < P / 2; t += SORT_BLK) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                    const unsigned long long a = sort_keys[i], b = sort_keys[l];
                    if ((a > b) == ((i & k) == 0)) { sort_keys[i] = b; sort_keys[l] = a; }
                }
                __syncthreads();
            }
        const int base = (jbase && len > 0) ? (int)(sort_keys[0] >> 32) : 0;   // (sorted: the row's smallest column)
        if (jbase && tid == 0) jbase[r] = base;
        for (int i = tid; i < len; i += SORT_BLK) {
            const unsigned long long key = sort_keys[i];
            const int col = (int)(key >> 32);
            ja_out[kb + i] = col;
            val_out[kb + i] = val_in[kb + (int)(unsigned)key];
            if (ja16) ja16[kb + i] = (unsigned short)(col - base);
        }
        __syncthreads();
    }
}

static int upload_sorted_on_device(const HostCSR& H, DevCSR& D, int maxlen)
{
    static const bool ja16_on = !(std::getenv("FASP_HIP_JA16") && std::atoi(std::getenv("FASP_HIP_JA16")) == 0);
    int* tj = nullptr; double* tv = nullptr;
    HIPCK(hipMalloc(&tj, sizeof(int) * (size_t)H.nnz));
    if (hipMalloc(&tv, sizeof(double) * (size_t)H.nnz) != hipSuccess) { (void)hipFree(tj); return ERROR_ALLOC_MEM; }
    int st = FASP_SUCCESS;
    if (hipMemcpyAsync(tj, H.ja.data(), sizeof(int) * (size_t)H.nnz, hipMemcpyHostToDevice, g_ctx.stream) != hipSuccess ||
        hipMemcpyAsync(tv, H.val.data(), sizeof(double) * (size_t)H.nnz, hipMemcpyHostToDevice, g_ctx.stream) != hipSuccess) st = ERROR_ALLOC_MEM;
    const bool relative = D.col > 65536;
    const bool want16 = ja16_on && D.kind == 0 && D.nnz >= 4096 && (!relative || rows_span_16bit(H.ia.data(), H.ja.data(), H.row));   // as upload_ja16
    if (st >= 0 && want16 && hipMalloc(&D.ja16, sizeof(unsigned short) * ((size_t)D.nnz + 8)) != hipSuccess) st = ERROR_ALLOC_MEM;
    if (st >= 0 && want16 && hipMemsetAsync(D.ja16 + D.nnz, 0, sizeof(unsigned short) * 8, g_ctx.stream) != hipSuccess) st = ERROR_MISC;   // (the slack k_csr_estream's last 16-byte piece reads)
    if (st >= 0 && want16 && relative && hipMalloc(&D.jbase, sizeof(int) * (size_t)std::max(D.row, 1)) != hipSuccess) st = ERROR_ALLOC_MEM;
    if (st >= 0) {
        int P = 64;
        while (P < maxlen) P <<= 1;
        const size_t lds = sizeof(unsigned long long) * (size_t)P;
        if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(k_sort_rows), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) st = ERROR_MISC;
        if (st >= 0) {
            const int grid = std::min(H.row, 256 * 64);
            hipLaunchKernelGGL(k_sort_rows, dim3(grid), dim3(SORT_BLK), lds, g_ctx.stream, H.row, D.ia, tj, tv, D.ja, D.val, D.ja16, D.jbase);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(g_ctx.stream) != hipSuccess) st = ERROR_MISC;
        }
    }
    (void)hipFree(tj); (void)hipFree(tv);
    if (st >= 0) D.sorted = true;
    return st;
}

// k_csr_xtile's structures (kernels2.hip.h): per wave tile of 64 rows the sorted list of the distinct columns of its
// entries, per entry the position of its column in that list.  Refused (nothing built) when a tile has more than
// XT_XCAP distinct columns or the lists would not pay for themselves.
static int build_xtile(const HostCSR& H, DevCSR& D)
{
    static const bool on = !(std::getenv("FASP_HIP_XTILE") && std::atoi(std::getenv("FASP_HIP_XTILE")) == 0);
    if (!on || H.row < 4096 || H.nnz < 16 * H.row) return FASP_SUCCESS;   // short rows: k_csr_lstream's territory
    const int ntile = (H.row + 63) / 64;
    double min_share = 2.5;
    if (const char* e = std::getenv("FASP_HIP_XTILE_MIN_SHARE")) min_share = std::atof(e);
    {   // a sample of the tiles first (every 61st): most operators are decided here, for a percent of the work
        long long ent = 0, dist = 0, nfat = 0, nsamp = 0;
        std::vector<int> cols;
        for (int t = 0; t < ntile; t += 61) {
            const int k0 = H.ia[t * 64], k1 = H.ia[std::min(H.row, t * 64 + 64)];
            cols.assign(H.ja.data() + k0, H.ja.data() + k1);
            std::sort(cols.begin(), cols.end());
            cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
            ent += k1 - k0; dist += (long long)cols.size();
            ++nsamp;
            if ((int)cols.size() > XT_XCAP) ++nfat;
        }
        const bool fat = nfat * 20 > nsamp;   // more than 5 % of the tiles beyond the LDS list
        if (fat || (double)dist * min_share > 1.1 * (double)ent) {
            if (std::getenv("FASP_HIP_SETUP_TIMING"))
                std::printf("        [xtile %d x %d, %d nnz] sample: %.1f entries per distinct column%s: not built\n", H.row, H.col, H.nnz,
                            (double)ent / std::max<long long>(dist, 1), fat ? ", a tile beyond the LDS list" : "");
            return FASP_SUCCESS;
        }
    }
    std::vector<int> cnt((size_t)ntile + 1, 0);
    Buf<unsigned short> l16((size_t)H.nnz);
    std::vector<std::vector<int>> lists((size_t)ntile);
    long long nfat_all = 0;
#pragma omp parallel
    {
        std::vector<int> cols;
#pragma omp for schedule(dynamic, 64) reduction(+ : nfat_all)
        for (int t = 0; t < ntile; ++t) {
            const int k0 = H.ia[t * 64], k1 = H.ia[std::min(H.row, t * 64 + 64)];
            cols.assign(H.ja.data() + k0, H.ja.data() + k1);
            std::sort(cols.begin(), cols.end());
            cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
            if ((int)cols.size() > XT_XCAP) {   // no list: the kernel gathers this tile's operands from global memory
                for (int k = k0; k < k1; ++k) l16[k] = 0;
                ++nfat_all;
                continue;
            }
            for (int k = k0; k < k1; ++k)
                l16[k] = (unsigned short)(std::lower_bound(cols.begin(), cols.end(), H.ja[k]) - cols.begin());
            cnt[(size_t)t + 1] = (int)cols.size();
            lists[(size_t)t] = cols;
        }
    }
    static const bool timing = std::getenv("FASP_HIP_SETUP_TIMING") != nullptr;
    if (nfat_all * 20 > ntile) {
        if (timing) std::printf("        [xtile %d x %d, %d nnz] %lld of %d tiles have more than %d distinct columns: not built\n", H.row, H.col, H.nnz, nfat_all, ntile, XT_XCAP);
        return FASP_SUCCESS;
    }
    int fattest = 0;
    for (int t = 0; t < ntile; ++t) { fattest = std::max(fattest, cnt[(size_t)t + 1]); cnt[(size_t)t + 1] += cnt[(size_t)t]; }
    const long long total = cnt[(size_t)ntile];
    if (timing) std::printf("        [xtile %d x %d, %d nnz] %lld distinct columns in %d tiles (%.1f entries per distinct column, fattest listed tile %d, %lld tiles without a list)\n",
                            H.row, H.col, H.nnz, total, ntile, (double)H.nnz / std::max<long long>(total, 1), fattest, nfat_all);
    // worth it when the rows of a tile share their columns: >= 2.5 entries per distinct column (then 10 + 4 / 2.5 = 11.6
    // bytes per entry against 12, and 2.5 x fewer gathers).  AMG coarse levels in C-point order share little (P7(256):
    // 1.5 on level 1, > 1024 distinct columns per tile on level 2): they keep k_csr_wstream2 until their rows are
    // re-ordered in bricks.  FASP_HIP_XTILE_MIN_SHARE overrides (tests).
    if ((double)total * min_share > (double)H.nnz) return FASP_SUCCESS;
    std::vector<int> flat((size_t)std::max<long long>(total, 1));
#pragma omp parallel for schedule(static)
    for (int t = 0; t < ntile; ++t) std::copy(lists[(size_t)t].begin(), lists[(size_t)t].end(), flat.begin() + cnt[(size_t)t]);
    HIPCK(hipMalloc(&D.lja16, sizeof(unsigned short) * ((size_t)H.nnz + 8)));
    HIPCK(hipMalloc(&D.tptr, sizeof(int) * ((size_t)ntile + 1)));
    HIPCK(hipMalloc(&D.tcols, sizeof(int) * flat.size()));
    HIPCK(hipMemcpy(D.lja16, l16.data(), sizeof(unsigned short) * (size_t)H.nnz, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(D.tptr, cnt.data(), sizeof(int) * ((size_t)ntile + 1), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(D.tcols, flat.data(), sizeof(int) * flat.size(), hipMemcpyHostToDevice));
    D.ntcols = total;
    return FASP_SUCCESS;
}

// k_csr_estream's tables (kernels3.hip.h): the entries of a long-row operator cut into W equal wave ranges and those into chunks of at
// most ES_CAP entries, with the row every chunk starts in, and for the rows that a wave boundary cuts who counts their parts.  Built
// from the row pointers alone (the device copy's rows are sorted, its pointers are the host's).  W depends on the operator only --
// not on the device -- so the association of every row sum is a property of the matrix.
struct EsTables { int W = 0, nc = 0; std::vector<int> wc, centry, crow, hw0, np; };
static void build_estream_host(const int* ia, int nrow, int nnz, int per_wave, int wmax, EsTables& T)
{
    int W = (int)std::min<long long>(wmax, ((long long)nnz + per_wave - 1) / per_wave);
    W = std::max(32, (W + 31) / 32 * 32);   // 8 XCDs x 4 waves per workgroup
    std::vector<int> ebeg((size_t)W + 1);
    for (int w = 0; w <= W; ++w) ebeg[(size_t)w] = (int)(((long long)nnz * w / W) & ~7ll);
    ebeg[(size_t)W] = nnz;
    T.W = W;
    T.wc.assign((size_t)W + 1, 0); T.hw0.assign((size_t)W, 0); T.np.assign((size_t)W, 0);
    T.centry.clear();
    T.centry.reserve((size_t)nnz / ES_CAP + (size_t)W + 2);
    for (int w = 0; w < W; ++w) {
        T.wc[(size_t)w] = (int)T.centry.size();
        const int len = ebeg[(size_t)w + 1] - ebeg[(size_t)w];
        if (len <= 0) continue;
        const int nch = (len + ES_CAP - 1) / ES_CAP;
        const int size = ((len + nch - 1) / nch + 7) & ~7;
        for (int j = 0; j < nch && ebeg[(size_t)w] + j * size < ebeg[(size_t)w + 1]; ++j) T.centry.push_back(ebeg[(size_t)w] + j * size);
    }
    T.wc[(size_t)W] = (int)T.centry.size();
    T.centry.push_back(nnz);
    const int nc = T.nc = (int)T.centry.size() - 1;
    T.crow.resize((size_t)nc + 1);
    auto row_of = [&](int e) {   // the row entry e lies in (e < nnz): the last r with ia[r] <= e
        return (int)(std::upper_bound(ia, ia + nrow + 1, e) - ia) - 1;
    };
#pragma omp parallel for schedule(static)
    for (int c = 0; c <= nc; ++c) T.crow[(size_t)c] = c == 0 ? 0 : c == nc ? nrow - 1 : std::min(nrow - 1, row_of(T.centry[(size_t)c]));
    auto wave_of = [&](int e) { return (int)(std::upper_bound(ebeg.begin(), ebeg.end(), e) - ebeg.begin()) - 1; };
    for (int w = 0; w < W; ++w) {
        const int e0 = ebeg[(size_t)w], e1 = ebeg[(size_t)w + 1];
        if (e1 <= e0) continue;
        const int rh = e0 == 0 ? 0 : row_of(e0);
        if (ia[rh] < e0) T.hw0[(size_t)w] = wave_of(ia[rh]);
        if (e1 < nnz) {
            const int rt = row_of(e1);
            if (ia[rt] < e1 && ia[rt] >= e0) T.np[(size_t)w] = wave_of(ia[rt + 1] - 1) - w + 1;
        }
    }
}

static int build_estream(const int* ia, int nrow, int nnz, DevCSR& D)
{
    static const bool on = !(std::getenv("FASP_HIP_ESTREAM") && std::atoi(std::getenv("FASP_HIP_ESTREAM")) == 0);
    if (!on || !D.ja16 || D.kind != 0 || nnz < 65536 || nrow < 1 || (double)nnz < 48.0 * nrow) return FASP_SUCCESS;   // (long rows: the small transfer operators that run on the row kernel have rows of 3-10 entries)
    static const int per_wave = std::getenv("FASP_HIP_ESTREAM_PER_WAVE") ? std::atoi(std::getenv("FASP_HIP_ESTREAM_PER_WAVE")) : 3072;
    static const int wmax = std::getenv("FASP_HIP_ESTREAM_WMAX") ? std::atoi(std::getenv("FASP_HIP_ESTREAM_WMAX")) : 5120;   // (five workgroups of four waves per CU: what every instantiation keeps resident at once)
    EsTables T;
    build_estream_host(ia, nrow, nnz, per_wave, wmax, T);
    const int W = T.W, nc = T.nc;
    const bool relative = D.jbase != nullptr;
    const size_t nt = (size_t)W + 1 + 2 * ((size_t)nc + 1) + 2 * (size_t)W + (relative ? (size_t)nc + 1 : 0);
    std::vector<int> tab(nt);
    size_t o = 0;
    std::copy(T.wc.begin(), T.wc.end(), tab.begin() + o); o += T.wc.size();
    std::copy(T.centry.begin(), T.centry.end(), tab.begin() + o); o += T.centry.size();
    std::copy(T.crow.begin(), T.crow.end(), tab.begin() + o); o += T.crow.size();
    std::copy(T.hw0.begin(), T.hw0.end(), tab.begin() + o); o += T.hw0.size();
    std::copy(T.np.begin(), T.np.end(), tab.begin() + o);
    HIPCK(hipMalloc(&D.es_tab, sizeof(int) * nt));
    HIPCK(hipMemcpy(D.es_tab, tab.data(), sizeof(int) * nt, hipMemcpyHostToDevice));
    HIPCK(hipMalloc(&D.es_part, sizeof(double) * 2 * (size_t)W + sizeof(unsigned) * (size_t)W));
    HIPCK(hipMemset(D.es_part, 0, sizeof(double) * 2 * (size_t)W + sizeof(unsigned) * (size_t)W));
    D.es_W = W; D.es_nc = nc;
    if (relative) {
        // more than 65536 columns: the row-relative 16-bit columns of the row kernel need every entry's ROW; the stream works on chunks,
        // so it gets columns relative to the smallest column of the CHUNK (built on the device from the sorted 32-bit copy) -- when
        // every chunk spans less than 65536 columns; otherwise the operator keeps the row kernel
        int* cbase = D.es_tab + (size_t)W + 1 + 2 * ((size_t)nc + 1) + 2 * (size_t)W;
        int* flag = cbase + nc;
        const int* centry = D.es_tab + (size_t)W + 1;
        HIPCK(hipMemsetAsync(flag, 0, sizeof(int), g_ctx.stream));
        const int grid = std::max(1, std::min(MAXGRID, (nc + 3) / 4));
        hipLaunchKernelGGL(k_es_chunk_base, dim3(grid), dim3(BLOCK), 0, g_ctx.stream, nc, centry, (const int*)D.ja, cbase, flag);
        int hflag = 0;
        HIPCK(hipMemcpyAsync(&hflag, flag, sizeof(int), hipMemcpyDeviceToHost, g_ctx.stream));
        HIPCK(hipStreamSynchronize(g_ctx.stream));
        if (hflag) {   // a chunk too wide for 16 bits
            (void)hipFree(D.es_tab); (void)hipFree(D.es_part);
            D.es_tab = nullptr; D.es_part = nullptr; D.es_W = D.es_nc = 0;
            return FASP_SUCCESS;
        }
        HIPCK(hipMalloc(&D.es_ja16, sizeof(unsigned short) * ((size_t)nnz + 8)));
        HIPCK(hipMemsetAsync(D.es_ja16 + nnz, 0, sizeof(unsigned short) * 8, g_ctx.stream));
        hipLaunchKernelGGL(k_es_chunk_cols, dim3(grid), dim3(BLOCK), 0, g_ctx.stream, nc, centry, (const int*)D.ja, (const int*)cbase, D.es_ja16);
        HIPCK(hipStreamSynchronize(g_ctx.stream));
    }
    return FASP_SUCCESS;
}

// Host walk of k_csr_estream's control flow over the tables (CPU tests; no device): every entry is covered by exactly one chunk, every
// row is finished exactly once -- inside one wave, or by parts whose count is what its first wave's table says -- and the sum of the
// parts in wave order is the row's sum.  Returns 0, or the negative number of the first check that failed.
static int estream_selftest_host(const int* ia, int nrow, int nnz, int per_wave, int wmax, int* info)
{
    EsTables T;
    build_estream_host(ia, nrow, nnz, per_wave, wmax, T);
    if (info) { info[0] = T.W; info[1] = T.nc; }
    std::vector<int> done((size_t)nrow, 0), parts((size_t)T.W, 0);
    std::vector<long long> covered((size_t)nrow, 0);   // entries of the row seen by chunks
    long long cut_rows = 0;
    for (int c = 0; c < T.nc; ++c) {
        if (T.centry[(size_t)c + 1] <= T.centry[(size_t)c] || T.centry[(size_t)c + 1] - T.centry[(size_t)c] > ES_CAP) return -1;
        if ((T.centry[(size_t)c] & 7) != 0) return -2;
        if (T.crow[(size_t)c] > T.crow[(size_t)c + 1]) return -3;
    }
    if (T.centry[0] != 0 || T.centry[(size_t)T.nc] != nnz) return -4;
    for (int w = 0; w < T.W; ++w) {
        const int c0 = T.wc[(size_t)w], cend = T.wc[(size_t)w + 1];
        if (c0 >= cend) continue;
        const int e0w = T.centry[(size_t)c0], e1w = T.centry[(size_t)cend];
        int pend_r = -1, pend_kb = 0;
        for (int c = c0; c < cend; ++c) {
            const int lo = T.centry[(size_t)c], hi = T.centry[(size_t)c + 1], rf = T.crow[(size_t)c], rl = T.crow[(size_t)c + 1];
            for (int r = rf; r <= rl; ++r) {
                const int kb = ia[r], ke = ia[r + 1];
                covered[(size_t)r] += std::max(0, std::min(ke, hi) - std::max(kb, lo));
                if (ke <= hi) {
                    if (kb >= e0w) { if (done[(size_t)r]++) return -5; }
                    else {
                        const int w0 = T.hw0[(size_t)w];
                        if (w0 < 0 || w0 >= w || T.np[(size_t)w0] < 2 || w0 + T.np[(size_t)w0] - 1 != w) return -6;   // this is the row's LAST part
                        if (++parts[(size_t)w0] == T.np[(size_t)w0]) { if (done[(size_t)r]++) return -7; ++cut_rows; }
                    }
                } else if (c + 1 == cend) { pend_r = r; pend_kb = kb; }
            }
        }
        if (pend_r >= 0 && pend_kb < e1w) {
            const int w0 = pend_kb >= e0w ? w : T.hw0[(size_t)w];
            if (w0 < 0 || w0 > w || T.np[(size_t)w0] < 2 || w0 + T.np[(size_t)w0] - 1 <= w) return -8;   // a first or a middle part: the last one comes later
            if (++parts[(size_t)w0] == T.np[(size_t)w0]) return -9;   // (walking the waves in order, the last part is a finished row above)
        }
    }
    for (int r = 0; r < nrow; ++r) {
        if (done[(size_t)r] != 1) return -10;
        if (covered[(size_t)r] != (long long)ia[r + 1] - ia[r]) return -11;
    }
    for (int w = 0; w < T.W; ++w)
        if (parts[(size_t)w] != T.np[(size_t)w]) return -12;
    if (info) info[2] = (int)cut_rows;
    return 0;
}

// Value-indexed sliced-ELL coding (kernels4.hip.h, k_csr_sell) of an operator in the row-length range of k_csr_wstream2 /
// k_csr_xtile.  Slices of 64 consecutive rows in the operator's own numbering; per slice its smallest column and its longest
// row; per row its length; per entry one 32-bit word = index into the table of the distinct values (compared by bit pattern;
// ordered by frequency, ties by bit pattern: deterministic) << obits | column - the slice's smallest column.  A row's entries
// keep their storage order and are padded at the end, to the slice's longest row, with the word 0.  Lossless.
// Qualifies only if (why_not, when it does not): 1 the operator is outside the size / mean-row-length range; 2 a row has
// more than 255 entries; 3 slots > cap_percent / 100 x entries; 4 more than SELL_MAXV distinct values; 5 index and offset
// do not fit 32 bits together.
struct SellHost {
    int nslice = 0, nv = 0, vbits = 0, obits = 0;
    long long slots = 0;
    std::vector<int> sptr, sbase;
    std::vector<unsigned char> rlen;
    std::vector<double> tab;
    Buf<unsigned> code;
    double bytes(int nrow) const { return 4.0 * (double)slots + (double)nrow + 4.0 * (2.0 * nslice + 1.0) + 8.0 * nv; }
};
constexpr int SELL_CAP_PERCENT = 125;
static bool build_sell(const HostCSR& M, SellHost& S, int cap_percent, int* why_not)
{
    int dummy = 0;
    int& why = why_not ? *why_not : dummy;
    why = 1;
    const int n = M.row;
    if (n <= 0 || M.nnz < 4096 || (double)M.nnz > 48.0 * n || (double)M.nnz <= 7.6 * n) return false;   // (shorter rows: k_csr_lstream)
    if ((long long)M.col >= (1ll << 28)) return false;
    const int ns = (n + 63) / 64;
    // row lengths, slice widths
    S.rlen.assign((size_t)n, 0);
    S.sptr.assign((size_t)ns + 1, 0);
    int toolong = 0;
#pragma omp parallel for schedule(static) reduction(+ : toolong)
    for (int s = 0; s < ns; ++s) {
        int W = 0;
        for (int r = s * 64; r < std::min(n, s * 64 + 64); ++r) {
            const int len = M.ia[r + 1] - M.ia[r];
            if (len > 255) { ++toolong; continue; }
            S.rlen[(size_t)r] = (unsigned char)len;
            W = std::max(W, len);
        }
        S.sptr[(size_t)s + 1] = W;
    }
    if (toolong) { why = 2; return false; }
    long long wsum = 0;
    for (int s = 0; s < ns; ++s) wsum += S.sptr[(size_t)s + 1];
    S.nslice = ns;
    S.slots = 64ll * wsum;
    if (S.slots * 100 > (long long)cap_percent * M.nnz || wsum >= (1ll << 30)) { why = 3; return false; }
    for (int s = 0; s < ns; ++s) S.sptr[(size_t)s + 1] += S.sptr[(size_t)s];
    // distinct values: per-thread sets with counts (a thread gives up beyond the cap), merged
    constexpr int VSLOTS = 32768;
    struct VSet {
        std::vector<unsigned long long> key;
        std::vector<long long> cnt;   // 0: empty slot
        std::vector<int> id;          // index in the table (set once the order is known)
        int n = 0;
        VSet() : key((size_t)VSLOTS, 0ull), cnt((size_t)VSLOTS, 0), id((size_t)VSLOTS, -1) {}
        static unsigned slot_of(unsigned long long b) { return (unsigned)((b * 0x9E3779B97F4A7C15ull) >> 49); }
        bool add(unsigned long long b, long long c)
        {
            unsigned s = slot_of(b);
            for (;;) {
                if (cnt[s] == 0) {
                    if (n >= SELL_MAXV) return false;
                    key[s] = b; cnt[s] = c; ++n;
                    return true;
                }
                if (key[s] == b) { cnt[s] += c; return true; }
                s = (s + 1) & (VSLOTS - 1);
            }
        }
        int slot(unsigned long long b) const   // -1: not in the set
        {
            unsigned s = slot_of(b);
            for (;;) {
                if (cnt[s] == 0) return -1;
                if (key[s] == b) return (int)s;
                s = (s + 1) & (VSLOTS - 1);
            }
        }
    };
    auto bits_of = [](double v) { unsigned long long b; std::memcpy(&b, &v, 8); return b; };
    const int nt = std::max(1, std::min(omp_get_max_threads(), n / 4096 + 1));
    std::vector<VSet*> local((size_t)nt, nullptr);
    bool fail = false;
#pragma omp parallel num_threads(nt)
    {
        VSet* T = new VSet();
        local[(size_t)omp_get_thread_num()] = T;
#pragma omp for schedule(static)
        for (int r = 0; r < n; ++r) {
            if (fail) continue;
            for (int k = M.ia[r]; k < M.ia[r + 1]; ++k)
                if (!T->add(bits_of(M.val[k]), 1)) { fail = true; break; }
        }
    }
    VSet Gs;
    for (VSet* T : local) {
        if (T && !fail)
            for (int s = 0; s < VSLOTS && !fail; ++s)
                if (T->cnt[(size_t)s] && !Gs.add(T->key[(size_t)s], T->cnt[(size_t)s])) fail = true;
        delete T;
    }
    if (fail) { why = 4; return false; }
    std::vector<std::pair<long long, unsigned long long>> order;   // (-count, bits)
    for (int s = 0; s < VSLOTS; ++s)
        if (Gs.cnt[(size_t)s]) order.emplace_back(-Gs.cnt[(size_t)s], Gs.key[(size_t)s]);
    std::sort(order.begin(), order.end());
    S.nv = (int)order.size();
    S.tab.resize(order.size());
    for (size_t i = 0; i < order.size(); ++i) std::memcpy(&S.tab[i], &order[i].second, 8);
    for (size_t i = 0; i < order.size(); ++i) Gs.id[(size_t)Gs.slot(order[i].second)] = (int)i;
    S.vbits = 0;
    while ((1ll << S.vbits) < S.nv) ++S.vbits;
    // slice bases, widest offset
    S.sbase.assign((size_t)ns, 0);
    int maxoff = 0;
#pragma omp parallel for schedule(static) reduction(max : maxoff)
    for (int s = 0; s < ns; ++s) {
        const int k0 = M.ia[s * 64], k1 = M.ia[std::min(n, s * 64 + 64)];
        if (k1 <= k0) continue;
        int lo = M.ja[k0], hi = lo;
        for (int k = k0 + 1; k < k1; ++k) { lo = std::min(lo, M.ja[k]); hi = std::max(hi, M.ja[k]); }
        S.sbase[(size_t)s] = lo;
        maxoff = std::max(maxoff, hi - lo);
    }
    S.obits = 1;
    while ((1ll << S.obits) <= maxoff) ++S.obits;
    if (S.vbits + S.obits > 32) { why = 5; return false; }
    // the words
    S.code.alloc((size_t)std::max<long long>(S.slots, 1));
    bool lost = false;
#pragma omp parallel for schedule(static)
    for (int s = 0; s < ns; ++s) {
        const int W = S.sptr[(size_t)s + 1] - S.sptr[(size_t)s], base = S.sbase[(size_t)s];
        unsigned* cs = S.code.data() + (size_t)S.sptr[(size_t)s] * 64;
        for (int l = 0; l < 64; ++l) {
            const int r = s * 64 + l;
            const int kb = r < n ? M.ia[r] : 0, len = r < n ? M.ia[r + 1] - kb : 0;
            for (int k = 0; k < len; ++k) {
                const int sl = Gs.slot(bits_of(M.val[kb + k]));
                if (sl < 0) { lost = true; continue; }
                const int id = Gs.id[(size_t)sl];
                cs[(size_t)k * 64 + l] = ((unsigned)id << S.obits) | (unsigned)(M.ja[kb + k] - base);
            }
            for (int k = len; k < W; ++k) cs[(size_t)k * 64 + l] = 0u;
        }
    }
    if (lost) { why = 4; return false; }
    why = 0;
    return true;
}

// y = A x over the coded form, walked the way k_csr_sell walks it: slice by slice, a lane per row, step k of all rows of the slice before
// step k + 1, every row summed left to right from 0.0
static void sell_mxv_host(const SellHost& S, int nrow, const double* x, double* y)
{
    const unsigned omask = (1u << S.obits) - 1u;
    for (int s = 0; s < S.nslice; ++s) {
        const int W = S.sptr[(size_t)s + 1] - S.sptr[(size_t)s], base = S.sbase[(size_t)s];
        const unsigned* cs = S.code.data() + (size_t)S.sptr[(size_t)s] * 64;
        double acc[64];
        for (int l = 0; l < 64; ++l) acc[l] = 0.0;
        for (int k = 0; k < W; ++k)
            for (int l = 0; l < 64; ++l) {
                const int r = s * 64 + l;
                if (r >= nrow || k >= (int)S.rlen[(size_t)r]) continue;
                const unsigned c = cs[(size_t)k * 64 + l];
                acc[l] = acc[l] + S.tab[c >> S.obits] * x[base + (int)(c & omask)];
            }
        for (int l = 0; l < 64 && s * 64 + l < nrow; ++l) y[s * 64 + l] = acc[l];
    }
}
// the coded form back to CSR (ia: nrow + 1; ja, val: as many entries as the row lengths add up to)
static void sell_decode_host(const SellHost& S, int nrow, int* ia, int* ja, double* val)
{
    const unsigned omask = (1u << S.obits) - 1u;
    ia[0] = 0;
    for (int r = 0; r < nrow; ++r) ia[r + 1] = ia[r] + (int)S.rlen[(size_t)r];
    for (int r = 0; r < nrow; ++r) {
        const int s = r >> 6, l = r & 63, base = S.sbase[(size_t)s];
        const unsigned* cs = S.code.data() + (size_t)S.sptr[(size_t)s] * 64;
        for (int k = 0; k < (int)S.rlen[(size_t)r]; ++k) {
            const unsigned c = cs[(size_t)k * 64 + l];
            ja[ia[r] + k] = base + (int)(c & omask);
            val[ia[r] + k] = S.tab[c >> S.obits];
        }
    }
}

// Row-group coding (kernels5.hip.h, k_csr_rgroup) of a long-row square operator in the numbering its device copy uses: groups of R
// consecutive rows walked over the sorted union of their columns.  code = per group {nch + 1 value offsets of its chunks of 64 union
// columns, relative to the group's first value; one word per union column: column - the group's smallest column | row mask << (32 - R)},
// padded at the very end to a multiple of four words with the word 0; val = the values without fill, chunk by chunk, inside a chunk row
// by row in union order (+ two zeros at the end: the last 16-byte piece); meta = per group {word offset, value offset, smallest column,
// chunks} + one closing {words, values, 0, 0}.  A row's entries come back sorted by column (the order of the sorted device copy).  Lossless.
// Refused (why_not): 1 the operator is not square; 2 mean row shorter than RG_MIN_ROW entries; 3 a group's columns span more than 65 535;
// 4 a row holds the same column twice; 5 entries / union columns (the mean reuse of a gather) below min_reuse.
constexpr int    RG_MIN_ROW   = 128;
constexpr int    RG_ROWS      = 8;     // rows per group unless fasp_hip_tune("rgroup_rows", 16) asks for 16 (measured: profiles/rgroup.txt)
constexpr double RG_W4_MIN_ROW = 256.0, RG_W8_MIN_ROW = 1000.0;   // waves per group: 2 below a mean row of 256 entries, 4 below 1 000, else 8, unless fasp_hip_tune("rgroup_waves", 2 | 4 | 8)
constexpr double RG_MIN_REUSE = 3.0;   // below it the form would also read more bytes than the 10 per entry of the 16-bit-column copy
struct RGroupHost {
    int R = 0, ng = 0;
    long long words = 0, chunks = 0, ucols = 0;   // 32-bit words of code (without the end padding), chunks, union columns
    std::vector<int> meta;
    Buf<unsigned>    code;
    Buf<double>      val;
};
static double rgroup_bytes(long long nnz, long long words, int ng) { return 8.0 * (double)nnz + 4.0 * (double)words + 16.0 * (ng + 1.0); }
static bool build_rgroup(const HostCSR& M, int R, double min_reuse, RGroupHost& G, int* why_not)
{
    int dummy = 0;
    int& why = why_not ? *why_not : dummy;
    G = RGroupHost();
    G.R = R;
    if (M.row != M.col) { why = 1; return false; }
    if (M.row <= 0 || M.nnz <= 0 || (double)M.nnz < (double)RG_MIN_ROW * M.row) { why = 2; return false; }
    const int n = M.row, ng = (n + R - 1) / R, sh = 32 - R;
    std::vector<std::vector<unsigned>> gcode((size_t)ng);   // per group: chunk offsets + words
    std::vector<int> gbase((size_t)ng, 0), gnch((size_t)ng, 0);
    G.val.alloc((size_t)M.nnz + 2);
    G.val[(size_t)M.nnz] = 0.0; G.val[(size_t)M.nnz + 1] = 0.0;
    int bad = 0;   // the smallest refusal code met (0: none)
#pragma omp parallel
    {
        std::vector<unsigned> mask((size_t)65536, 0u);   // per column offset: rows of the group that hold it
        std::vector<int>      pos((size_t)65536, 0);     // ... its place in the union
        std::vector<unsigned short> touched;
        std::vector<int> slot;                           // per (union column, row): the value's place in the group
        int mybad = 0;
#pragma omp for schedule(dynamic, 16)
        for (int g = 0; g < ng; ++g) {
            const int r0 = g * R, r1 = std::min(n, r0 + R), k0 = M.ia[r0], k1 = M.ia[r1];
            std::vector<unsigned>& out = gcode[(size_t)g];
            if (k1 <= k0) { out.assign(1, 0u); continue; }
            int lo = M.ja[k0], hi = lo;
            for (int k = k0 + 1; k < k1; ++k) { lo = std::min(lo, M.ja[k]); hi = std::max(hi, M.ja[k]); }
            if (hi - lo > 65535) { mybad = mybad ? std::min(mybad, 3) : 3; continue; }
            gbase[(size_t)g] = lo;
            touched.clear();
            bool dup = false;
            for (int r = r0; r < r1; ++r)
                for (int k = M.ia[r]; k < M.ia[r + 1]; ++k) {
                    const int off = M.ja[k] - lo;
                    const unsigned bit = 1u << (r - r0);
                    if (!mask[(size_t)off]) touched.push_back((unsigned short)off);
                    if (mask[(size_t)off] & bit) dup = true;
                    mask[(size_t)off] |= bit;
                }
            if (dup) {
                mybad = mybad ? std::min(mybad, 4) : 4;
                for (unsigned short t : touched) mask[t] = 0u;
                continue;
            }
            std::sort(touched.begin(), touched.end());
            const int nu = (int)touched.size(), nch = (nu + 63) / 64;
            out.resize((size_t)nch + 1 + nu);
            gnch[(size_t)g] = nch;
            slot.assign((size_t)nu * R, -1);
            int next = 0;
            for (int c = 0; c < nch; ++c) {
                out[(size_t)c] = (unsigned)next;
                const int u1 = std::min(nu, 64 * c + 64);
                for (int r = 0; r < R; ++r)
                    for (int u = 64 * c; u < u1; ++u)
                        if (mask[touched[(size_t)u]] >> r & 1u) slot[(size_t)u * R + r] = next++;
            }
            out[(size_t)nch] = (unsigned)next;   // == k1 - k0
            for (int u = 0; u < nu; ++u) {
                pos[touched[(size_t)u]] = u;
                out[(size_t)nch + 1 + u] = (unsigned)touched[(size_t)u] | (mask[touched[(size_t)u]] << sh);
            }
            for (int r = r0; r < r1; ++r)
                for (int k = M.ia[r]; k < M.ia[r + 1]; ++k)
                    G.val[(size_t)k0 + (size_t)slot[(size_t)pos[(size_t)(M.ja[k] - lo)] * R + (r - r0)]] = M.val[k];
            for (unsigned short t : touched) mask[t] = 0u;
        }
#pragma omp critical
        if (mybad) bad = bad ? std::min(bad, mybad) : mybad;
    }
    if (bad) { why = bad; return false; }
    G.ng = ng;
    G.meta.assign(4 * ((size_t)ng + 1), 0);
    long long w = 0;
    for (int g = 0; g < ng; ++g) {
        const std::vector<unsigned>& c = gcode[(size_t)g];
        const int r0 = g * R;
        const int nch = gnch[(size_t)g];
        G.meta[4 * (size_t)g] = (int)w; G.meta[4 * (size_t)g + 1] = M.ia[r0]; G.meta[4 * (size_t)g + 2] = gbase[(size_t)g]; G.meta[4 * (size_t)g + 3] = nch;
        w += (long long)c.size();
        G.chunks += nch;
        G.ucols += (long long)c.size() - (nch + 1);
    }
    if (w >= (1ll << 31) - 8) { why = 2; return false; }
    G.meta[4 * (size_t)ng] = (int)w; G.meta[4 * (size_t)ng + 1] = M.nnz;
    G.words = w;
    if ((double)M.nnz < min_reuse * (double)G.ucols) { why = 5; return false; }
    G.code.alloc((size_t)((w + 3) & ~3ll) + 4);
    for (long long i = w; i < ((w + 3) & ~3ll) + 4; ++i) G.code[(size_t)i] = 0u;
#pragma omp parallel for schedule(static)
    for (int g = 0; g < ng; ++g) std::copy(gcode[(size_t)g].begin(), gcode[(size_t)g].end(), G.code.data() + G.meta[4 * (size_t)g]);
    why = 0;
    return true;
}
// y = A x over the coded form in k_csr_rgroup's order with NW waves per group: per wave its share of the chunks, per lane (union column) and
// row a sum in chunk order; per lane the waves' parts in wave order; the 64 lanes by es_group_sum's tree (row_shr 1, 2, 4, 8 inside rows
// of 16 lanes, then lane 15 of row 0 / 2 into rows 1 / 3, then lane 31 into rows 2 and 3: the total ends in lane 63)
static void rgroup_mxv_host(const RGroupHost& G, int nrow, int NW, const double* x, double* y)
{
    const int R = G.R, sh = 32 - R;
    for (int g = 0; g < G.ng; ++g) {
        const int woff = G.meta[4 * (size_t)g], voff = G.meta[4 * (size_t)g + 1], cbase = G.meta[4 * (size_t)g + 2], nch = G.meta[4 * (size_t)g + 3];
        const int len = G.meta[4 * (size_t)g + 4] - woff - (nch + 1);
        const unsigned* coff = G.code.data() + woff;
        const unsigned* wd = coff + nch + 1;
        double sum[16][64];
        for (int w = 0; w < NW; ++w) {
            double acc[16][64];
            for (int r = 0; r < R; ++r)
                for (int l = 0; l < 64; ++l) acc[r][l] = 0.0;
            for (int c = nch * w / NW; c < nch * (w + 1) / NW; ++c) {
                int at = voff + (int)coff[c];
                for (int r = 0; r < R; ++r)
                    for (int l = 0; l < 64 && 64 * c + l < len; ++l) {
                        const unsigned word = wd[64 * c + l];
                        if (!((word >> (sh + r)) & 1u)) continue;
                        const double p = G.val[(size_t)at++] * x[cbase + (int)(word & 0xffffu)];
                        acc[r][l] = acc[r][l] + p;
                    }
            }
            for (int r = 0; r < R; ++r)
                for (int l = 0; l < 64; ++l) sum[r][l] = w == 0 ? acc[r][l] : sum[r][l] + acc[r][l];
        }
        for (int r = 0; r < R && g * R + r < nrow; ++r) {
            double* v = sum[r];
            double t[64];
            for (int s = 1; s <= 8; s <<= 1) {
                for (int l = 0; l < 64; ++l) t[l] = v[l] + ((l & 15) >= s ? v[l - s] : 0.0);
                for (int l = 0; l < 64; ++l) v[l] = t[l];
            }
            for (int l = 0; l < 64; ++l) t[l] = v[l] + (((l >> 4) & 1) ? v[(l & ~15) - 1] : 0.0);
            for (int l = 0; l < 64; ++l) v[l] = t[l];
            for (int l = 0; l < 64; ++l) t[l] = v[l] + (l >= 32 ? v[31] : 0.0);
            y[g * R + r] = t[63];
        }
    }
}
// the coded form back to CSR, every row sorted by column (ia: nrow + 1; ja, val: nnz)
static void rgroup_decode_host(const RGroupHost& G, int nrow, int* ia, int* ja, double* val)
{
    const int R = G.R, sh = 32 - R;
    int k = 0;
    ia[0] = 0;
    for (int g = 0; g < G.ng; ++g) {
        const int woff = G.meta[4 * (size_t)g], voff = G.meta[4 * (size_t)g + 1], cbase = G.meta[4 * (size_t)g + 2], nch = G.meta[4 * (size_t)g + 3];
        const int len = G.meta[4 * (size_t)g + 4] - woff - (nch + 1);
        const unsigned* coff = G.code.data() + woff;
        const unsigned* wd = coff + nch + 1;
        for (int r = 0; r < R && g * R + r < nrow; ++r) {
            for (int c = 0; c < nch; ++c) {
                int at = voff + (int)coff[c];   // row r's values of the chunk lie behind those of the rows 0 .. r - 1
                const int u1 = std::min(len, 64 * c + 64);
                for (int q = 0; q < r; ++q)
                    for (int u = 64 * c; u < u1; ++u) at += (int)((wd[u] >> (sh + q)) & 1u);
                for (int u = 64 * c; u < u1; ++u)
                    if ((wd[u] >> (sh + r)) & 1u) { ja[k] = cbase + (int)(wd[u] & 0xffffu); val[k] = G.val[(size_t)at++]; ++k; }
            }
            ia[g * R + r + 1] = k;
        }
    }
}

static int upload_sell(const HostCSR& H, DevCSR& D)
{
    static const bool on = !(std::getenv("FASP_HIP_SELL") && std::atoi(std::getenv("FASP_HIP_SELL")) == 0);
    if (!on) return FASP_SUCCESS;
    static const bool timing = std::getenv("FASP_HIP_SETUP_TIMING") != nullptr;
    const double t0 = wall_seconds();
    SellHost S;
    int why = 0;
    const bool ok = build_sell(H, S, SELL_CAP_PERCENT, &why);
    if (timing) std::printf("        [sell %d x %d, %d nnz] %s (%d) %d values, %d + %d bits, %.3f slots per entry, %.3f s\n", H.row, H.col, H.nnz,
                            ok ? "coded" : "not coded", why, S.nv, S.vbits, S.obits, (double)S.slots / std::max(H.nnz, 1), wall_seconds() - t0);
    if (!ok) return FASP_SUCCESS;
    const size_t ns = (size_t)S.nslice;
    std::vector<int> meta(2 * ns + 1);
    std::copy(S.sptr.begin(), S.sptr.end(), meta.begin());
    std::copy(S.sbase.begin(), S.sbase.end(), meta.begin() + (long)ns + 1);
    HIPCK(hipMalloc(&D.sell_code, sizeof(unsigned) * (size_t)std::max<long long>(S.slots, 1)));
    HIPCK(hipMalloc(&D.sell_meta, sizeof(int) * meta.size()));
    HIPCK(hipMalloc(&D.sell_rlen, (size_t)H.row));
    HIPCK(hipMalloc(&D.sell_tab, sizeof(double) * (size_t)S.nv));
    HIPCK(hipMemcpy(D.sell_code, S.code.data(), sizeof(unsigned) * (size_t)S.slots, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(D.sell_meta, meta.data(), sizeof(int) * meta.size(), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(D.sell_rlen, S.rlen.data(), (size_t)H.row, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(D.sell_tab, S.tab.data(), sizeof(double) * (size_t)S.nv, hipMemcpyHostToDevice));
    D.sell_nv = S.nv; D.sell_obits = S.obits; D.sell_nslice = S.nslice; D.sell_slots = S.slots;
    return FASP_SUCCESS;
}

static int upload_csr(const HostCSR& H, DevCSR& D)
{
    D.row = H.row; D.col = H.col; D.nnz = H.nnz;
    HIPCK(hipMalloc(&D.ia, sizeof(int) * ((size_t)H.row + 1)));
    HIPCK(hipMalloc(&D.ja, sizeof(int) * std::max<size_t>(H.nnz, 1)));
    HIPCK(hipMalloc(&D.val, sizeof(double) * (std::max<size_t>(H.nnz, 1) + 2)));   // (+ 16 bytes: k_csr_estream's last 16-byte piece)
    HIPCK(hipMemsetAsync(D.val + std::max<size_t>(H.nnz, 1), 0, sizeof(double) * 2, g_ctx.stream));
    HIPCK(hipMemcpyAsync(D.ia, H.ia.data(), sizeof(int) * ((size_t)H.row + 1), hipMemcpyHostToDevice, g_ctx.stream));
    pick_kernel(D);
    auto upload_plain = [&]() -> int {
        HIPCK(hipMemcpyAsync(D.ja, H.ja.data(), sizeof(int) * (size_t)H.nnz, hipMemcpyHostToDevice, g_ctx.stream));
        HIPCK(hipMemcpyAsync(D.val, H.val.data(), sizeof(double) * (size_t)H.nnz, hipMemcpyHostToDevice, g_ctx.stream));
        return 0;
    };
    // (long rows keep the sub-wavefront kernel: the coded kernels are one-lane-per-row designs)
    if (compress_enabled() && H.nnz >= 4096 && (double)H.nnz <= 48.0 * H.row) {
        Buf<unsigned short> pat; Buf<int> prb;
        std::vector<int> pstart, plen, poff; std::vector<double> pval;
        static const bool rowpat_on = !(std::getenv("FASP_HIP_ROWPAT") && std::atoi(std::getenv("FASP_HIP_ROWPAT")) == 0);
        if (rowpat_on && build_rowpat(H, pat, pstart, plen, poff, pval, prb)) {
            D.npat = (int)pstart.size(); D.npent = (int)poff.size();
            HIPCK(hipMalloc(&D.pat, sizeof(unsigned short) * ((size_t)H.row + 2)));  // + pad: the pair kernels load two ids at once
            HIPCK(hipMalloc(&D.pstart, sizeof(int) * pstart.size()));
            HIPCK(hipMalloc(&D.plen, sizeof(int) * plen.size()));
            HIPCK(hipMemcpy(D.plen, plen.data(), sizeof(int) * plen.size(), hipMemcpyHostToDevice));
            HIPCK(hipMalloc(&D.poff, sizeof(int) * std::max<size_t>(poff.size(), 1)));
            HIPCK(hipMalloc(&D.pval, sizeof(double) * std::max<size_t>(pval.size(), 1)));
            HIPCK(hipMemset(D.pat + H.row, 0xff, sizeof(unsigned short) * 2));   // pad = 0xffff: never a pattern id (MAXPAT 65535)
            HIPCK(hipMemcpy(D.pat, pat.data(), sizeof(unsigned short) * (size_t)H.row, hipMemcpyHostToDevice));
            HIPCK(hipMemcpy(D.pstart, pstart.data(), sizeof(int) * pstart.size(), hipMemcpyHostToDevice));
            HIPCK(hipMemcpy(D.poff, poff.data(), sizeof(int) * poff.size(), hipMemcpyHostToDevice));
            HIPCK(hipMemcpy(D.pval, pval.data(), sizeof(double) * pval.size(), hipMemcpyHostToDevice));
            if (prb.n) {
                HIPCK(hipMalloc(&D.rowbase, sizeof(int) * ((size_t)H.row + 2)));   // + pad: the pair kernel loads two bases at once
                HIPCK(hipMemcpy(D.rowbase, prb.data(), sizeof(int) * (size_t)H.row, hipMemcpyHostToDevice));
                // k_csr_rowpat5 (kernels2.hip.h): the sweep computes the row pairs whose two patterns are those of the pair
                // (128 w + 64, 128 w + 65) of their wave tile w; every other row goes on this list.
                const int nr = H.row, npair = (nr + 1) / 2;
                long long nx = 0;
#pragma omp parallel for schedule(static) reduction(+ : nx)
                for (int w0 = 0; w0 < nr; w0 += 128) {
                    const int    pm = std::min((w0 + 64) / 2, npair - 1);
                    const unsigned domA = pat[(size_t)2 * pm], domB = (2 * pm + 1 < nr) ? pat[(size_t)2 * pm + 1] : 0xffffu;   // (the device copy is padded with 0xffff)
                    for (int r = w0; r < std::min(w0 + 128, nr); r += 2) {
                        const bool vb = r + 1 < nr;
                        if (!(vb && pat[r] == domA && pat[r + 1] == domB)) nx += vb ? 2 : 1;
                    }
                }
                if (nx * 4 <= nr) D.nxrows = (int)nx;   // worth it when most rows are swept (the others go through the wave's queue)
            } else {
                D.plane = grid_plane_of(poff, H.row);
                if (std::getenv("FASP_HIP_SETUP_TIMING")) std::printf("        [upload_csr %d x %d, %d nnz] %d row patterns; grid plane for the XCD strips: %d rows\n", H.row, H.col, H.nnz, (int)pstart.size(), D.plane);
                // k_csr_rowpat4 (kernels2.hip.h): the sweep computes the row pairs (2i, 2i+1) whose two rows have the
                // pattern of row 128 w + 64 of their wave tile w; every other row goes on this list.
                const int nr = H.row, npair = (nr + 1) / 2;
                long long nx = 0;
#pragma omp parallel for schedule(static) reduction(+ : nx)
                for (int w0 = 0; w0 < nr; w0 += 128) {
                    const unsigned dom = pat[(size_t)2 * std::min((w0 + 64) / 2, npair - 1)];
                    for (int r = w0; r < std::min(w0 + 128, nr); r += 2) {
                        const bool vb = r + 1 < nr;
                        if (!(vb && pat[r] == dom && pat[r + 1] == dom)) nx += vb ? 2 : 1;
                    }
                }
                if (nx * 4 <= nr) D.nxrows = (int)nx;  // worth it when most rows are swept
            }
            D.kind = 2;  // plain-CSR twin of a coded operator: the stream kernel (same row-sum order; used by the A/B tests)
            return upload_plain() < 0 ? ERROR_ALLOC_MEM : FASP_SUCCESS;
        }
        std::vector<int> doff; std::vector<double> dval;
        Buf<unsigned char> code; Buf<int> rowbase;
        if (build_dict8(H, doff, dval, code, rowbase)) {
            HIPCK(hipMalloc(&D.code, (size_t)H.nnz + 256));  // + slack: spans are fetched in 16-byte units
            HIPCK(hipMalloc(&D.doff, sizeof(int) * 256));
            HIPCK(hipMalloc(&D.dval, sizeof(double) * 256));
            HIPCK(hipMemcpy(D.code, code.data(), (size_t)H.nnz, hipMemcpyHostToDevice));
            HIPCK(hipMemcpy(D.doff, doff.data(), sizeof(int) * 256, hipMemcpyHostToDevice));
            HIPCK(hipMemcpy(D.dval, dval.data(), sizeof(double) * 256, hipMemcpyHostToDevice));
            if (rowbase.n) {
                HIPCK(hipMalloc(&D.rowbase, sizeof(int) * (size_t)H.row));
                HIPCK(hipMemcpy(D.rowbase, rowbase.data(), sizeof(int) * (size_t)H.row, hipMemcpyHostToDevice));
            }
            D.kind = 2;
            return upload_plain() < 0 ? ERROR_ALLOC_MEM : FASP_SUCCESS;
        }
    }
    // not coded: plain CSR, rows re-sorted by column where the gathers dominate
    static const bool sort_long = !(std::getenv("FASP_HIP_SORT_LONG_ROWS") && std::atoi(std::getenv("FASP_HIP_SORT_LONG_ROWS")) == 0);
    static const int  sort_stream = std::getenv("FASP_HIP_SORT_STREAM") ? std::atoi(std::getenv("FASP_HIP_SORT_STREAM")) : 0;
    const double avg_len = H.row > 0 ? (double)H.nnz / H.row : 0.0;
    const bool do_sort = sort_long && !g_oneshot_upload && H.nnz > 0 && (D.kind == 0 || (D.kind == 2 && sort_stream > 0 && avg_len >= sort_stream));
    static const bool timing = std::getenv("FASP_HIP_SETUP_TIMING") != nullptr;
    double tp = wall_seconds();
    auto lap = [&](const char* what) {
        if (!timing) return;
        const double now = wall_seconds();
        std::printf("        [upload_csr %d x %d, %d nnz] %-10s %8.3f s\n", H.row, H.col, H.nnz, what, now - tp);
        tp = now;
    };
    if (do_sort && D.kind == 0) {   // (kind 2 wants the diagonal positions of the sorted copy: host path below)
        int maxlen = 0;
#pragma omp parallel for schedule(static) reduction(max : maxlen)
        for (int i = 0; i < H.row; ++i) maxlen = std::max(maxlen, H.ia[i + 1] - H.ia[i]);
        if (g_device_sort && maxlen <= SORT_MAXLEN) {
            const int st = upload_sorted_on_device(H, D, maxlen);
            lap("device sort");
            return st < 0 ? st : build_estream(H.ia.data(), H.row, H.nnz, D);
        }
    }
    if (do_sort) {
        // Operators whose time goes into the x gathers -- one L1 tag lookup per distinct cache line, up to 64
        // per wavefront load when a row's columns come in discovery order: the DEVICE copy keeps every row's
        // entries sorted by column, so neighbouring lanes gather neighbouring entries.  (The sub-wavefront
        // kernel sums lane-strided partials + a shuffle tree, i.e. it never followed the storage order.)
        Buf<int> sj((size_t)H.nnz);
        Buf<double> sv((size_t)H.nnz);
        std::vector<int> dp;
        const bool square = H.row == H.col;
        if (square) dp.assign((size_t)H.row, -1);
#pragma omp parallel
        {
            std::vector<std::pair<int, double>> tmp;
#pragma omp for schedule(dynamic, 64)
            for (int i = 0; i < H.row; ++i) {
                const int kb = H.ia[i], ke = H.ia[i + 1];
                tmp.resize((size_t)(ke - kb));
                for (int k = kb; k < ke; ++k) tmp[(size_t)(k - kb)] = {H.ja[k], H.val[k]};
                std::stable_sort(tmp.begin(), tmp.end(),
                                 [](const std::pair<int, double>& x, const std::pair<int, double>& y) { return x.first < y.first; });
                for (int k = kb; k < ke; ++k) {
                    sj[k] = tmp[(size_t)(k - kb)].first; sv[k] = tmp[(size_t)(k - kb)].second;
                    if (square && sj[k] == i) dp[(size_t)i] = k;  // last diagonal hit (stable sort keeps their order)
                }
            }
        }
        lap("row sort");
        HIPCK(hipMemcpy(D.ja, sj.data(), sizeof(int) * (size_t)H.nnz, hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(D.val, sv.data(), sizeof(double) * (size_t)H.nnz, hipMemcpyHostToDevice));
        lap("memcpy");
        if (square && D.kind == 2) {
            HIPCK(hipMalloc(&D.dpos, sizeof(int) * (size_t)std::max(H.row, 1)));
            HIPCK(hipMemcpy(D.dpos, dp.data(), sizeof(int) * (size_t)H.row, hipMemcpyHostToDevice));
        }
        D.sorted = true;
        if (upload_ja16(D, H.ia.data(), sj.data()) < 0) return ERROR_ALLOC_MEM;
        return build_estream(H.ia.data(), H.row, H.nnz, D);
    }
    if (upload_plain() < 0) return ERROR_ALLOC_MEM;
    if (D.kind == 2 && !g_oneshot_upload && build_xtile(H, D) < 0) return ERROR_ALLOC_MEM;
    // neither row patterns nor a byte dictionary: the value-indexed sliced-ELL form where the operator has few distinct values
    if (D.kind == 2 && compress_enabled() && upload_sell(H, D) < 0) return ERROR_ALLOC_MEM;
    if (upload_ja16(D, H.ia.data(), H.ja.data()) < 0) return ERROR_ALLOC_MEM;
    return build_estream(H.ia.data(), H.row, H.nnz, D);
}

// development knobs (fasp_hip_tune): -1 = automatic
struct Tuning { int bsr_sweep_form = -1, bsr_cycle_sweep = 0, swz_run = -1, swz_run_width = 16, ilu_smooth_fused = 1, gen2 = 2, ws2_bpc = 3, maxgrid = -1, xcd = 16, nt = 1, kind = -1, lanes = -1, wrows = -1, wcap = -1, compress = 1, rpl = -1, lds_tab = 1, xcd_pat = 64, spcg_batch = 16, small_lds = 1, ja16 = 1, spcg_fused = 1, spcg_grid = 0, spcg_persist = 1, split_rows = 0, gs_multicolor = 0, seq_flow = 1, seq_strip_kb = 0, seq_jobs = 1, seq_spine = 1, seq_grid = 0, seq_chain = 1, seq_chain_n1 = 0, seq_chain_grid = 0, seq_chain_ref = 0, seq_test_hang = 0, seq_rest_lanes = 0, local_square = 1, fuse_zr = 1, fuse_presmooth = 1, seq_lanes = 0, xtile = 1, rp5_max = 45, rp_bpc = 5, rp_xcd = -1, rp_strip = 2, spcg_test_hang = 0, small_onewave = 4, lazy_coarse = 1, rp_stream = -1, renumber = 1, renumber_chunk = 262144, pcg_dev_beta = 1, spcg_spec = 1, ev_every = 4, pcg_fold = 1, seq_chain_touch = 8, seq_chain_touch_t1 = 1, seq_zero_skip = 1, estream = 1, es_dbg = 0, ilu_form = -1, str_ilu_form = -1, str_ilu_wgs = 0, str_sweep_form = -1, str_sweep_wgs = 0, sell = 1, safe_fused = 1, rgroup = 1, rgroup_rows = 0, rgroup_waves = 0; };
static Tuning g_tune;

// The row-group form (build_rgroup) of a square long-row operator beside its plain device copy, which stays: row windows, OP_MXV_DOT and
// the distributed path use it.  Built only while fasp_hip_tune("rgroup") is not 0; an operator a rule refuses simply has none.
static int upload_rgroup(const HostCSR& H, DevCSR& D)
{
    if (g_tune.rgroup == 0 || g_oneshot_upload || H.row != H.col || (double)H.nnz < (double)RG_MIN_ROW * H.row) return FASP_SUCCESS;
    static const bool timing = std::getenv("FASP_HIP_SETUP_TIMING") != nullptr;
    const double t0 = wall_seconds();
    RGroupHost G;
    int why = 0;
    const bool ok = build_rgroup(H, g_tune.rgroup_rows == 16 ? 16 : RG_ROWS, RG_MIN_REUSE, G, &why);
    if (timing) std::printf("        [row groups %d x %d, %d nnz] %s (%d) R %d, %d groups, %lld chunks, reuse %.2f, %.2f bytes per entry, %.3f s\n", H.row, H.col, H.nnz,
                            ok ? "coded" : "not coded", why, G.R, G.ng, G.chunks, G.ucols ? (double)H.nnz / (double)G.ucols : 0.0,
                            ok ? rgroup_bytes(H.nnz, G.words, G.ng) / H.nnz : 0.0, wall_seconds() - t0);
    if (!ok) return FASP_SUCCESS;
    const size_t nw = (size_t)((G.words + 3) & ~3ll) + 4;
    HIPCK(hipMalloc(&D.rg_code, sizeof(unsigned) * nw));
    HIPCK(hipMalloc(&D.rg_val, sizeof(double) * ((size_t)H.nnz + 2)));
    HIPCK(hipMalloc(&D.rg_meta, sizeof(int) * G.meta.size()));
    HIPCK(hipMemcpy(D.rg_code, G.code.data(), sizeof(unsigned) * nw, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(D.rg_val, G.val.data(), sizeof(double) * ((size_t)H.nnz + 2), hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(D.rg_meta, G.meta.data(), sizeof(int) * G.meta.size(), hipMemcpyHostToDevice));
    D.rg_R = G.R; D.rg_ng = G.ng; D.rg_words = G.words;
    if (timing) std::printf("        [row groups %d x %d] with the copy to the device %.3f s\n", H.row, H.col, wall_seconds() - t0);
    return FASP_SUCCESS;
}

// Blocks of one kernel instantiation that are co-resident on a CU (VGPR / LDS / wave
// limits), from the occupancy API, cached per instantiation.  The persistent grids
// below are sized to exactly this residency: a grid larger than what is resident
// serialises into two rounds (measured: +35 % time), a smaller one leaves CUs idle.
template <class K>
static int resident_blocks_per_cu(K kernel)
{
    // keyed by the kernel's ADDRESS: K is only the signature, which all CsrArgs kernels share (round 1 cached one
    // value per signature -- whatever kernel ran first decided the grid of all the others)
    static std::vector<std::pair<const void*, int>> cache;
    const void* key = reinterpret_cast<const void*>(kernel);
    for (const auto& e : cache)
        if (e.first == key) return e.second;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, BLOCK, 0) != hipSuccess || nb < 1) nb = 4;
    nb = std::min(nb, 8);
    cache.emplace_back(key, nb);
    return nb;
}

template <class K>
static int launch_persistent(K kernel, int ntiles, CsrArgs& a, int blocks_per_cu = 0)
{
    int cap = (blocks_per_cu > 0 ? std::min(blocks_per_cu, resident_blocks_per_cu(kernel)) : resident_blocks_per_cu(kernel)) * g_ctx.num_cu;
    if (g_tune.maxgrid > 0) cap = g_tune.maxgrid;
    cap = std::min(cap, MAXGRID);
    int grid = std::min(cap, ntiles);
    grid = std::max(8, (grid + 7) / 8 * 8);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), 0, g_ctx.stream, a);
    return grid;
}

// Where k_csr_rgroup replaces the kernel the plan would otherwise pick under fasp_hip_tune("rgroup", 1): on a level only where it measured
// faster by more than the spread of repeated cold timings of that kernel (at most 1.5 us over three repeats of eight launches; one
// outlier).  P7(256), cold, us per launch, y = A x / y -= A x / Jacobi (profiles/rgroup.txt):
//   level (entries per row)   kernel without     8 rows, 2 waves    8 rows, 4 waves    8 rows, 8 waves    16 rows, best of 2 / 4 / 8 waves
//   4 (191)                   49 / 50 / 54       38 / 39 / 43       39 / 40 / 45       55 / 50 / 65       43 / 46 / 52 (2)
//   5 (390)                   56 / 54 / 57       40 / 41 / 42       37 / 38 / 40       44 / 40 / 49       41 / 43 / 46 (4)
//   6 (710)                   58 / 60 / 62       46 / 46 / 47       42 / 42 / 43       44 / 43 / 47       45 / 46 / 49 (8)
//   7 (1 114)                 58 / 55 / 58       44 / 44 / 45       40 / 40 / 41       39 / 40 / 42       43 / 42 / 46 (8)
//   8 (1 356)                 40 / 39 / 41       39 / 39 / 40       33 / 33 / 34       32 / 31 / 33       33 / 33 / 34 (8)
// Groups of 8 rows win on every level that has the copy, by 7-18 us, and beat groups of 16 on every level: 8 is the default.  (The arithmetic
// of a chunk costs the same whether the R x 64 places of its rows are taken or not, and groups of 8 fill 47 % of them where groups of 16
// fill 39 %.)  Waves per group: 2 below a mean row of 256 entries, 4 below 1 000, 8 from there on (RG_W4_MIN_ROW, RG_W8_MIN_ROW; level 7 is a tie
// of 4 and 8).  A copy built with 16 rows per group is used between 256 and 1 200 entries per row, where it won by 8-15 us; on levels 4 and 8
// it wins by less and only with one of the wave counts.
static int rgroup_waves_auto(const DevCSR& M)
{
    const double avg = M.row > 0 ? (double)M.nnz / M.row : 0.0;
    return avg >= RG_W8_MIN_ROW ? 8 : avg >= RG_W4_MIN_ROW ? 4 : 2;
}
static bool rgroup_measured_faster(const DevCSR& M)
{
    const double avg = M.row > 0 ? (double)M.nnz / M.row : 0.0;
    return M.rg_R == 8 || (avg >= 256.0 && avg < 1200.0);
}

// The kernel ONE launch of a row operation runs.  plan_csr decides it -- the only place that does: launch_csr executes the plan, and
// fasp_hip_amg_kernel_info, fasp_hip_matrix_op, fasp_hip_time_matrix and the (z, r) fusion of the smoother read it.  A value per
// instantiation (but OP); the order is part of fasp_hip_csr_plan's report (fasp_hip_dev.h, tests/_csr_cases.py).
enum CsrKernel : int {
    CK_ROWS_2 = 0, CK_ROWS_4, CK_ROWS_8, CK_ROWS_16, CK_ROWS_32, CK_ROWS_64,               // k_csr_rows<L, OP>
    CK_WSTREAM_64_512, CK_WSTREAM_64_1024, CK_WSTREAM_32_512, CK_WSTREAM_32_1024,           // k_csr_wstream<OP, wrows, wcap>
    CK_ROWPAT_0_1, CK_ROWPAT_0_2, CK_ROWPAT_1_1, CK_ROWPAT_1_2, CK_ROWPAT_2_1, CK_ROWPAT_2_2,   // k_csr_rowpat<OP, T, RPL>
    CK_DICT8_8, CK_DICT8_16, CK_DICT8_24,                                                   // k_csr_dict8<OP, U>
    CK_ESTREAM_4, CK_ESTREAM_8, CK_ESTREAM_16, CK_ESTREAM_32,                               // k_csr_estream<L, OP>
    CK_ROWPAT4, CK_ROWPAT5, CK_LSTREAM, CK_XTILE, CK_SELL, CK_WSTREAM2,
    CK_RGROUP_16_4, CK_RGROUP_16_8, CK_RGROUP_8_4, CK_RGROUP_8_8,                           // k_csr_rgroup<R, NW, OP>
    CK_RGROUP_16_2, CK_RGROUP_8_2
};
struct CsrPlan {
    CsrKernel kernel;
    int    family;      // the code of fasp_hip_amg_kernel_info: 0 k_csr_rows (and k_csr_estream), 2 k_csr_wstream, 4 k_csr_dict8, 5 k_csr_rowpat,
                        // 6 k_csr_rowpat4, 7 k_csr_lstream, 8 k_csr_wstream2, 9 k_csr_rowpat5, 10 k_csr_xtile, 11 k_csr_sell
    int    tile_rows;   // rows of a tile (of a workgroup and step)
    int    bpc;         // launch_persistent: blocks per CU at most (0: what is resident)
    int    xcd_map;     // CsrArgs::xcd_map; -2: XCD strips (kernels.hip.h, tile_of) of tpp tiles per grid plane
    int    tpp;         // 0: no strips
    int    nt;          // CsrArgs::nt
    bool   ja16, jbase; // the 16-bit column copy / its row bases are passed
    bool   fused_zr;    // OP_JACOBI with a.partials set asks for the partials of (x_new, b) on the way out (the (z, r) of PCG from the last sweep
                        // of level 0) and this kernel writes them: only those of the fast paths do
    double bytes;       // matrix data one pass reads: row pointers / indices / values, or their coded form
};
// Pure: reads scalar fields of M, whether its pointers are set, and g_tune; calls nothing, dereferences nothing, changes nothing.
// windowed: a row-window launch, or fasp_hip_tune("split_rows") in force; rows: the rows of the window (< 0: the whole operator).
static CsrPlan plan_csr(const DevCSR& M, int op, bool windowed, bool want_partials, int rows = -1)
{
    CsrPlan p{};
    int kind = M.kind;
    if (rows < 0) rows = M.row;
    if (M.code && g_tune.compress) kind = 4;  // dictionary-coded copy present: one byte per entry
    if (M.pat && g_tune.compress) kind = 5;   // row-pattern-coded copy present: two bytes per row
    if (g_tune.kind >= 0 && !(g_tune.kind == 4 && !M.code) && !(g_tune.kind == 5 && !M.pat)) kind = g_tune.kind;
    const int lanes = g_tune.lanes > 0 ? g_tune.lanes : M.lanes, wrows = g_tune.wrows > 0 ? g_tune.wrows : M.wrows, wcap = g_tune.wcap > 0 ? g_tune.wcap : M.wcap;
    const bool jac = op == OP_JACOBI, w64 = wrows == 64 && wcap == 512;
    const bool lstream_ok = g_tune.gen2 && kind == 2 && w64 && (double)M.nnz <= 7.6 * M.row;  // tests c != r itself
    // the other stream kernels take the diagonal from dpos: a Jacobi sweep that needs the c != r test keeps the row kernel
    if (jac && kind != 0 && kind < 4 && (M.dup_diag || !M.dpos) && !lstream_ok) kind = 0;
    p.xcd_map = g_tune.xcd;
    // coded pair kernels: streaming hints on y / pattern ids / b where a vector does not fit the Infinity Cache beside the
    // others anyway (P7(256): level 0 yes -- 0.546 -> 0.519 GB, 93 -> 88 us; level 1, 67 MB vectors, no: 63 -> 73 us with hints)
    p.nt = g_tune.nt | ((g_tune.rp_stream > 0 || (g_tune.rp_stream < 0 && (size_t)M.row * 8 > (size_t)96 << 20)) ? 4 : 0);
    p.ja16 = g_tune.ja16 && M.ja16; p.jbase = g_tune.ja16 && M.jbase;
    if (M.jbase && kind != 0) p.ja16 = p.jbase = false;   // (a tuning knob sent a sub-wavefront operator elsewhere: only k_csr_rows adds the row base)
    if (kind == 1 || kind == 3) kind = 0;   // (block-level stream, one workgroup per row: measured slower, retired to tools/lab/)
    p.tile_rows = kind >= 4 ? BLOCK : kind == 2 ? 4 * wrows : BLOCK / lanes;
    auto ntiles = [&] { return (rows + p.tile_rows - 1) / p.tile_rows; };
    auto strips = [&] {   // where the operator knows its grid plane
        const int rpb = p.tile_rows;
        if (!g_tune.rp_strip || M.plane < 8 * rpb || M.plane % (8 * rpb) != 0 || ntiles() < 4 * (M.plane / rpb)) return;
        p.xcd_map = -2; p.tpp = M.plane / rpb;
    };
    const double avg = M.row > 0 ? (double)M.nnz / M.row : 1.0, ptr_bytes = 4.0 * (M.row + 1.0), base_bytes = M.rowbase ? 4.0 * M.row : 0.0;
    const bool pair = kind == 5 && M.nxrows >= 0 && g_tune.rpl <= 0;   // (fasp_hip_tune("rpl", 1 | 2) asks for k_csr_rowpat's rows-per-lane forms: the pair sweeps step aside)
    p.bytes = kind == 5 ? 2.0 * M.row + base_bytes + 12.0 * M.npent : kind == 4 ? 1.0 * M.nnz + ptr_bytes + base_bytes : 12.0 * M.nnz + ptr_bytes;
    if (pair && g_tune.gen2 && !M.rowbase) {
        // square row-pattern-coded operator: scalar-pattern sweep, other rows through the wave's LDS queue (kernels2.hip.h)
        p.kernel = CK_ROWPAT4; p.family = 6; p.tile_rows = 2 * BLOCK;
        p.xcd_map = ntiles() >= 8 * 64 ? g_tune.rp_xcd : 16;  // slabs: x is fetched once per XCD (PMC: 0.18 GB instead of 0.45 GB per level-0 pass)
        if (p.xcd_map == -1) strips();   // strips instead of slabs where the operator says how long a grid plane is
        // (strips: three blocks per CU -- six planes of an XCD's strip in flight -- measured against two, four, five: level-0 t = A p
        // 87-98 us against 95-105 with five; with four, 108)
        p.bpc = p.xcd_map == -2 && g_tune.rp_bpc == 5 ? 3 : g_tune.rp_bpc;
        p.fused_zr = jac && want_partials;
    }
    else if (pair && g_tune.gen2 >= 2 && M.rowbase && !jac && op != OP_L1DIAG && (double)M.nnz <= 0.1 * g_tune.rp5_max * M.row) {
        // rectangular row-pattern-coded operator (R, P of the coded levels): pair-of-patterns sweep + LDS queue; no smoother instantiations.
        // (measured on P7(256) level 0: prolongation, 1-6 entries per row, 140 -> 131 us; restriction, 7-13 entries per row,
        // 68 -> 80 us: the sweep pays for short lists only)
        p.kernel = CK_ROWPAT5; p.family = 9; p.tile_rows = 2 * BLOCK; p.bpc = 5;
        p.xcd_map = ntiles() >= 8 * 64 ? -1 : 16;
        if (g_tune.rp_strip >= 2) strips();
    }
    else if (kind == 5) {
        const int rpl = g_tune.rpl > 0 ? g_tune.rpl : 1;
        const bool lds = M.npat <= 512 && M.npent <= 2048 && g_tune.lds_tab != 0;
        const int T = !lds ? 0 : M.npat <= 64 && M.npent <= 512 && g_tune.lds_tab != 3 ? 2 : 1;   // 2 = small table: more resident blocks
        p.kernel = CsrKernel(CK_ROWPAT_0_1 + 2 * T + (rpl != 1)); p.family = 5; p.tile_rows = BLOCK * rpl;
        if (g_tune.xcd_pat != 0) p.xcd_map = g_tune.xcd_pat;
        if (g_tune.xcd_pat == 64 && g_tune.rp_strip >= 2) strips();
    }
    else if (kind == 4) { p.kernel = avg <= 8.5 ? CK_DICT8_8 : avg <= 20.0 ? CK_DICT8_16 : CK_DICT8_24; p.family = 4; }
    // short rows (64 rows fit the 512-entry slab with room for ragged tiles): 16-byte staged stream, lane = row
    else if (lstream_ok) { p.kernel = CK_LSTREAM; p.family = 7; p.bpc = 4; p.fused_zr = jac && want_partials; }
    else if (kind == 2 && g_tune.gen2 >= 2 && w64) {
        if (g_tune.xtile && M.lja16) {
            // mid levels (20-60 nonzeros per row): the tile's distinct x entries staged in LDS, 16-bit column positions
            p.kernel = CK_XTILE; p.family = 10; p.bpc = 3;
            p.bytes = 10.0 * M.nnz + ptr_bytes + 4.0 * M.ntcols + 4.0 * ((M.row + 63) / 64 + 1.0);   // values + 16-bit positions + the tiles' column lists
        }
        else if (M.sell_code && g_tune.compress && g_tune.sell) {
            // few distinct values, tiles that share too few columns for k_csr_xtile: sliced ELL (kernels4.hip.h), lane = row, 4 bytes per entry,
            // workgroups of 16 waves (the rows' sums are k_csr_wstream2's)
            p.kernel = CK_SELL; p.family = 11; p.tile_rows = SELL_BLOCK;
            p.bytes = 4.0 * (double)M.sell_slots + 1.0 * M.row + 4.0 * (2.0 * M.sell_nslice + 1.0) + 8.0 * M.sell_nv;   // words + row lengths + slice table + value table
        }
        else { p.kernel = CK_WSTREAM2; p.family = 8; p.bpc = g_tune.ws2_bpc; }   // rows of any length: staged, prefetched stream
        p.fused_zr = jac && want_partials;
    }
    else if (kind == 2) {
        p.kernel = w64 ? CK_WSTREAM_64_512 : wrows == 64 ? CK_WSTREAM_64_1024 : wrows == 32 && wcap == 512 ? CK_WSTREAM_32_512 : CK_WSTREAM_32_1024; p.family = 2;
    }
    else {
        if (p.ja16) p.bytes = 10.0 * M.nnz + ptr_bytes + (p.jbase ? 4.0 * M.row : 0.0);   // 16-bit indices
        // long rows with 16-bit columns, whole-operator launches: the entry-parallel stream (kernels3.hip.h).  Not for the fused dot
        // products (whichever wave completes a cut row would own its term of the sum) and not for row windows (they keep the row kernel).
        // Where it is the faster one (cold, P7(256): profiles/r06_estream.txt): mean rows below 256 entries -- levels 3 and 4 there, 66 -> 50 and
        // 51 -> 48 us per product; on the longer rows the two tie (both sit on the gather rate of the texture-address pipe) and the row
        // kernel's epilogue is lighter.  fasp_hip_tune("estream", 2): wherever the tables exist (tests, A/B runs); 0: never.
        const bool es_rule = g_tune.estream >= 2 || (g_tune.estream == 1 && (double)M.nnz < 256.0 * M.row);
        // row groups (kernels5.hip.h): one gather of x per union column of R consecutive rows.  fasp_hip_tune("rgroup", 2): wherever the coded
        // copy exists; 1 (default): by the measured rule (rgroup_measured_faster) -- and not under fasp_hip_tune("estream", 0), which asks for
        // the row kernel on every long-row operator (row windows against whole launches, bit for bit); 0: never, and no copy is built.
        const bool rg_rule = g_tune.rgroup >= 2 || (g_tune.rgroup == 1 && g_tune.estream != 0 && rgroup_measured_faster(M));
        if (M.rg_code && rg_rule && !windowed && op != OP_MXV_DOT && !(jac && (want_partials || M.dup_diag))) {
            const int tw = g_tune.rgroup_waves, nw = tw == 2 || tw == 4 || tw == 8 ? tw : rgroup_waves_auto(M);
            p.kernel = M.rg_R == 8 ? (nw == 2 ? CK_RGROUP_8_2 : nw == 4 ? CK_RGROUP_8_4 : CK_RGROUP_8_8) : (nw == 2 ? CK_RGROUP_16_2 : nw == 4 ? CK_RGROUP_16_4 : CK_RGROUP_16_8);
            p.tile_rows = M.rg_R;
            p.ja16 = p.jbase = false;
            p.bytes = rgroup_bytes(M.nnz, M.rg_words, M.rg_ng);
        }
        else if (M.es_tab && es_rule && p.ja16 && !windowed && op != OP_MXV_DOT && !(jac && (want_partials || M.dup_diag)))
            // lanes per row: so that the rows a 512-entry chunk touches normally fit one pass of 64 / L rows (kernels3.hip.h)
            p.kernel = avg >= 512.0 ? CK_ESTREAM_32 : avg >= 256.0 ? CK_ESTREAM_16 : avg >= 128.0 ? CK_ESTREAM_8 : CK_ESTREAM_4;
        else
            p.kernel = lanes == 2 ? CK_ROWS_2 : lanes == 4 ? CK_ROWS_4 : lanes == 8 ? CK_ROWS_8 : lanes == 16 ? CK_ROWS_16 : lanes == 32 ? CK_ROWS_32 : CK_ROWS_64;
    }
    return p;
}
// The report of fasp_hip_amg_kernel_info and fasp_hip_matrix_op: family and matrix bytes (may be NULL) of y = M x on the whole operator.
static int kernel_family(const DevCSR& M, double* matrix_bytes)
{
    const CsrPlan p = plan_csr(M, OP_MXV, false, false);
    if (matrix_bytes) *matrix_bytes = p.bytes;
    return p.family;
}

template <int OP>
static int launch_sell(const DevCSR& M, CsrArgs& a)
{
    a.sell_code = M.sell_code; a.sell_sptr = M.sell_meta; a.sell_sbase = M.sell_meta + M.sell_nslice + 1; a.sell_rlen = M.sell_rlen;
    a.sell_tab = M.sell_tab; a.sell_nv = M.sell_nv; a.sell_obits = M.sell_obits;
    const size_t lds = sizeof(double) * ((size_t)M.sell_nv + SELL_NW);
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_csr_sell<OP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * (SELL_MAXV + SELL_NW)));
        attr_set = true;
    }
    static std::vector<std::pair<size_t, int>> cache;   // resident workgroups per CU by table size
    int nb = 0;
    for (const auto& e : cache)
        if (e.first == lds) nb = e.second;
    if (nb == 0) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_csr_sell<OP>, SELL_BLOCK, lds) != hipSuccess || nb < 1) nb = 1;
        nb = std::min(nb, 2);
        cache.emplace_back(lds, nb);
    }
    int cap = nb * g_ctx.num_cu;
    if (g_tune.maxgrid > 0) cap = g_tune.maxgrid;
    cap = std::min(cap, MAXGRID);
    int grid = std::min(cap, a.ntiles);
    grid = std::max(8, (grid + 7) / 8 * 8);
    hipLaunchKernelGGL(k_csr_sell<OP>, dim3(grid), dim3(SELL_BLOCK), lds, g_ctx.stream, a);
    return grid;
}

// One workgroup of NW waves per group of R rows; an XCD's workgroups (blocks b, b + 8, ...) take one contiguous eighth of the groups.
// LDS: a slab of 64 R doubles per wave (a chunk's values: at most R per union column).  No fused dot products: OP_MXV_DOT never gets here.
template <int R, int NW, int OP>
static int launch_rgroup(const DevCSR& M, CsrArgs& a)
{
    if constexpr (OP == OP_MXV_DOT) { (void)M; (void)a; return 0; }
    else {
        a.rg_code = M.rg_code; a.rg_val = M.rg_val; a.rg_meta = M.rg_meta; a.rg_ng = M.rg_ng;
        constexpr int lds = NW * 64 * R * 8;
        static bool attr_set = false;
        if (!attr_set) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_csr_rgroup<R, NW, OP>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            attr_set = true;
        }
        const int grid = 8 * ((M.rg_ng + 7) / 8);
        hipLaunchKernelGGL((k_csr_rgroup<R, NW, OP>), dim3(grid), dim3(NW * 64), lds, g_ctx.stream, a);
        return grid;
    }
}

// (the transfer-operator kernel has no smoother instantiations)
template <int OP>
static int launch_rowpat5(CsrArgs& a)
{
    if constexpr (OP == OP_JACOBI || OP == OP_L1DIAG) { (void)a; return 0; }
    else return launch_persistent(k_csr_rowpat5<OP>, a.ntiles, a, 5);
}

// Launches the row kernel of family M.kind for operation OP; returns the grid size
// (= number of per-block partials written by OP_MXV_DOT).
// Row window of a launch: rows [lo, hi) (lo a multiple of WIN_ALIGN, which every kernel's tile size divides),
// per-block partials written from slot goff on.  hi < 0: the whole operator.
constexpr int WIN_ALIGN = DIST_WIN_ALIGN;
struct RowWin { int lo = 0, hi = -1, goff = 0; };

// numbering bridge of a transfer operator (DevCSR::bridge): gather behind a restriction -- with the next level's first Jacobi sweep from
// the zero guess written along, zx_store's expression -- and scatter in front of a prolongation
__global__ __launch_bounds__(BLOCK) void k_bridge_gather(int n, const int* __restrict__ perm, const double* __restrict__ s, double* __restrict__ y,
                                                         double* __restrict__ zx, const double* __restrict__ zdiag, double zomega)
{
    for (int k = blockIdx.x * BLOCK + threadIdx.x; k < n; k += gridDim.x * BLOCK) {
        const double v = s[perm[k]];
        y[k] = v;
        if (zx) { const double di = zdiag[k]; zx[k] = (fabs(di) > 1e-20) ? (1 - zomega) * 0.0 + zomega * v / di : 0.0; }
    }
}
__global__ __launch_bounds__(BLOCK) void k_bridge_scatter(int n, const int* __restrict__ perm, const double* __restrict__ x, double* __restrict__ s)
{
    for (int k = blockIdx.x * BLOCK + threadIdx.x; k < n; k += gridDim.x * BLOCK) s[perm[k]] = x[k];
}

template <int OP>
static int launch_csr(const DevCSR& M0, CsrArgs a, RowWin win = RowWin())
{
    if (M0.bridge && win.hi < 0) {
        DevCSR Mn = M0;   // (shallow: the operator without its bridge)
        Mn.bridge = nullptr; Mn.bscratch = nullptr; Mn.bridge_dir = 0;
        if (M0.bridge_dir == 1 && OP == OP_MXV) {
            CsrArgs b = a;
            b.y = M0.bscratch; b.zx = nullptr; b.zdiag = nullptr;
            const int G = launch_csr<OP>(Mn, b);
            const int grid = std::max(1, std::min(MAXGRID, (M0.row + BLOCK - 1) / BLOCK));
            hipLaunchKernelGGL(k_bridge_gather, dim3(grid), dim3(BLOCK), 0, g_ctx.stream, M0.row, M0.bridge, (const double*)M0.bscratch, a.y, a.zx, a.zdiag, a.zomega);
            return G;
        }
        if (M0.bridge_dir == 2 && (OP == OP_ADD || OP == OP_SUB || OP == OP_AXPY || OP == OP_MXV)) {
            const int grid = std::max(1, std::min(MAXGRID, (M0.col + BLOCK - 1) / BLOCK));
            hipLaunchKernelGGL(k_bridge_scatter, dim3(grid), dim3(BLOCK), 0, g_ctx.stream, M0.col, M0.bridge, a.x, M0.bscratch);
            CsrArgs b = a;
            b.x = M0.bscratch;
            return launch_csr<OP>(Mn, b);
        }
        std::fprintf(stderr, "### ERROR: fasp_hip: operation %d on a transfer operator with a numbering bridge (direction %d)\n", (int)OP, M0.bridge_dir);
        std::abort();
    }
    if (win.hi < 0 && g_tune.split_rows > 0 && M0.row >= 4 * WIN_ALIGN) {
        // test mode (fasp_hip_tune("split_rows", k)): every operator in three row windows, as dist_launch issues them
        const int lo = std::min(g_tune.split_rows, M0.row / 4) / WIN_ALIGN * WIN_ALIGN, hi = (M0.row - lo) / WIN_ALIGN * WIN_ALIGN;
        RowWin w; w.lo = lo; w.hi = hi; w.goff = 0;
        int G = launch_csr<OP>(M0, a, w);
        w.lo = 0; w.hi = lo; w.goff = G;
        G += launch_csr<OP>(M0, a, w);
        w.lo = hi; w.hi = M0.row; w.goff = G;
        return G + launch_csr<OP>(M0, a, w);
    }
    const DevCSR& M = M0;
    const int w_lo = win.hi >= 0 ? win.lo : 0, w_hi = win.hi >= 0 ? std::min(win.hi, M0.row) : M0.row;
    if (w_hi <= w_lo && win.hi >= 0) return 0;
    if (a.partials) a.partials += win.goff;
    const CsrPlan p = plan_csr(M, OP, win.hi >= 0 || g_tune.split_rows > 0, a.partials != nullptr, w_hi - w_lo);
    const int rpb = p.tile_rows;
    // a row window starts at a multiple of WIN_ALIGN; a kernel whose tile size does not divide it (only reachable through
    // fasp_hip_tune: block-stream tiles beyond 1024 rows, k_csr_rowpat with 8 rows per lane) would compute rows outside
    // the window a second time -- refuse loudly instead
    if (win.hi >= 0 && rpb > 0 && (w_lo % rpb) != 0) {
        std::fprintf(stderr, "### ERROR: fasp_hip: row window at %d with a kernel tile of %d rows (a tuning knob broke the window alignment)\n", w_lo, rpb);
        std::abort();
    }
    a.nrow = w_hi; a.row_lo = w_lo; a.tile0 = w_lo / rpb;
    a.ntiles = (w_hi - w_lo + rpb - 1) / rpb; a.tiles_per_xcd = (a.ntiles + 7) / 8;
    a.xcd_map = p.xcd_map; a.nt = p.nt;
    if (p.tpp) { a.tpp = p.tpp; a.tiles_per_xcd = p.tpp / 8; }
    a.ia = M.ia; a.ja = M.ja; a.val = M.val; a.dpos = M.dpos;
    a.ja16 = p.ja16 ? M.ja16 : nullptr; a.jbase = p.jbase ? M.jbase : nullptr;
    // what the kernel's family reads beyond that (k_csr_sell: launch_sell)
    if (p.family == 5 || p.family == 6 || p.family == 9) {
        a.pat = M.pat; a.pstart = M.pstart; a.plen = M.plen; a.poff = M.poff; a.pval = M.pval; a.rowbase = M.rowbase;
        a.npat = M.npat; a.npent = M.npent; a.ncol = M.col;
    }
    if (p.family == 4) { a.code = M.code; a.rowbase = M.rowbase; a.doff = M.doff; a.dval = M.dval; }
    if (p.kernel == CK_XTILE) { a.lja16 = M.lja16; a.tptr = M.tptr; a.tcols = M.tcols; }
#define PERSIST(...) return launch_persistent(__VA_ARGS__, a.ntiles, a, p.bpc)
    switch (p.kernel) {
        case CK_ROWS_2:  PERSIST(k_csr_rows<2, OP>);
        case CK_ROWS_4:  PERSIST(k_csr_rows<4, OP>);
        case CK_ROWS_8:  PERSIST(k_csr_rows<8, OP>);
        case CK_ROWS_16: PERSIST(k_csr_rows<16, OP>);
        case CK_ROWS_32: PERSIST(k_csr_rows<32, OP>);
        case CK_ROWS_64: PERSIST(k_csr_rows<64, OP>);
        case CK_WSTREAM_64_512:  PERSIST(k_csr_wstream<OP, 64, 512>);
        case CK_WSTREAM_64_1024: PERSIST(k_csr_wstream<OP, 64, 1024>);
        case CK_WSTREAM_32_512:  PERSIST(k_csr_wstream<OP, 32, 512>);
        case CK_WSTREAM_32_1024: PERSIST(k_csr_wstream<OP, 32, 1024>);
        case CK_ROWPAT_0_1: PERSIST(k_csr_rowpat<OP, 0, 1>);
        case CK_ROWPAT_0_2: PERSIST(k_csr_rowpat<OP, 0, 2>);
        case CK_ROWPAT_1_1: PERSIST(k_csr_rowpat<OP, 1, 1>);
        case CK_ROWPAT_1_2: PERSIST(k_csr_rowpat<OP, 1, 2>);
        case CK_ROWPAT_2_1: PERSIST(k_csr_rowpat<OP, 2, 1>);
        case CK_ROWPAT_2_2: PERSIST(k_csr_rowpat<OP, 2, 2>);
        case CK_DICT8_8:  PERSIST(k_csr_dict8<OP, 8>);
        case CK_DICT8_16: PERSIST(k_csr_dict8<OP, 16>);
        case CK_DICT8_24: PERSIST(k_csr_dict8<OP, 24>);
        case CK_ROWPAT4:  PERSIST(k_csr_rowpat4<OP>);
        case CK_ROWPAT5:  return launch_rowpat5<OP>(a);
        case CK_LSTREAM:  PERSIST(k_csr_lstream<OP, 512>);
        case CK_XTILE:    PERSIST(k_csr_xtile<OP>);
        case CK_SELL:     return launch_sell<OP>(M, a);
        case CK_WSTREAM2: PERSIST(k_csr_wstream2<OP>);
        case CK_RGROUP_16_4: return launch_rgroup<16, 4, OP>(M, a);
        case CK_RGROUP_16_8: return launch_rgroup<16, 8, OP>(M, a);
        case CK_RGROUP_8_4:  return launch_rgroup<8, 4, OP>(M, a);
        case CK_RGROUP_8_8:  return launch_rgroup<8, 8, OP>(M, a);
        case CK_RGROUP_16_2: return launch_rgroup<16, 2, OP>(M, a);
        case CK_RGROUP_8_2:  return launch_rgroup<8, 2, OP>(M, a);
        default: break;   // k_csr_estream<L, OP>
    }
#undef PERSIST
    const int W = M.es_W, nc = M.es_nc, lanes = 4 << (p.kernel - CK_ESTREAM_4);
    a.es_wc = M.es_tab; a.es_centry = a.es_wc + W + 1; a.es_crow = a.es_centry + nc + 1; a.es_hw0 = a.es_crow + nc + 1; a.es_np = a.es_hw0 + W;
    a.es_part = M.es_part; a.es_cnt = reinterpret_cast<unsigned*>(M.es_part + 2 * (size_t)W);
    a.es_cbase = M.es_ja16 ? a.es_np + W : nullptr; a.es_ja16 = M.es_ja16;
    static bool attr_set = false;
#define ES_ATTR(LL) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_csr_estream<LL, OP>), hipFuncAttributeMaxDynamicSharedMemorySize, ES_LDS_BYTES)
    if (!attr_set) { ES_ATTR(32); ES_ATTR(16); ES_ATTR(8); ES_ATTR(4); attr_set = true; }
#undef ES_ATTR
#define ES_LAUNCH(LL) hipLaunchKernelGGL((k_csr_estream<LL, OP>), dim3(W / 4), dim3(BLOCK), ES_LDS_BYTES, g_ctx.stream, a)
#ifdef FASP_LAB_DEBUG
    if (OP == OP_MXV && g_tune.es_dbg) {   // (tools/lab: which part of the kernel costs what)
#define ES_DBG(LL, DD) do { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_csr_estream<LL, OP_MXV, DD>), hipFuncAttributeMaxDynamicSharedMemorySize, ES_LDS_BYTES); hipLaunchKernelGGL((k_csr_estream<LL, OP_MXV, DD>), dim3(W / 4), dim3(BLOCK), ES_LDS_BYTES, g_ctx.stream, a); } while (0)
        const int dd = g_tune.es_dbg;
        if (lanes == 32) { if (dd == 1) ES_DBG(32, 1); else if (dd == 2) ES_DBG(32, 2); else if (dd == 3) ES_DBG(32, 3); else if (dd == 4) ES_DBG(32, 4); else ES_DBG(32, 7); }
        else if (lanes == 16) { if (dd == 1) ES_DBG(16, 1); else if (dd == 2) ES_DBG(16, 2); else if (dd == 3) ES_DBG(16, 3); else if (dd == 4) ES_DBG(16, 4); else ES_DBG(16, 7); }
        else if (lanes == 8) { if (dd == 1) ES_DBG(8, 1); else if (dd == 2) ES_DBG(8, 2); else if (dd == 3) ES_DBG(8, 3); else if (dd == 4) ES_DBG(8, 4); else ES_DBG(8, 7); }
        else { if (dd == 1) ES_DBG(4, 1); else if (dd == 2) ES_DBG(4, 2); else if (dd == 3) ES_DBG(4, 3); else if (dd == 4) ES_DBG(4, 4); else ES_DBG(4, 7); }
#undef ES_DBG
        return W / 4;
    }
#endif
    static const bool es_log = std::getenv("FASP_HIP_ES_LOG") != nullptr;   // (debugging: every launch announced and waited for)
    if (es_log) { std::fprintf(stderr, "[es rank %d] op %d rows %d cols %d nnz %d W %d chunks %d lanes %d rel %d x %p y %p b %p\n", comm_rank(), (int)OP, M.row, M.col, M.nnz, W, nc, lanes, M.es_ja16 != nullptr, (const void*)a.x, (void*)a.y, (const void*)a.b); std::fflush(stderr); }
    if (lanes == 32) ES_LAUNCH(32); else if (lanes == 16) ES_LAUNCH(16); else if (lanes == 8) ES_LAUNCH(8); else ES_LAUNCH(4);
#undef ES_LAUNCH
    if (es_log) { const hipError_t e = hipStreamSynchronize(g_ctx.stream); std::fprintf(stderr, "[es rank %d] done: %s\n", comm_rank(), hipGetErrorString(e)); std::fflush(stderr); }
    return W / 4;
}

// y = A x
static void d_mxv(const DevCSR& A, const double* x, double* y)
{
    CsrArgs a{}; a.x = x; a.y = y;
    launch_csr<OP_MXV>(A, a);
}
// y = b - A x
static void d_resid(const DevCSR& A, const double* x, const double* b, double* y)
{
    CsrArgs a{}; a.x = x; a.y = y; a.b = b;
    launch_csr<OP_RESID>(A, a);
}
// y += alpha A x  (three rounding-distinct paths of BlaSpmvCSR.c:494)
static void d_aAxpy(double alpha, const DevCSR& A, const double* x, double* y)
{
    CsrArgs a{}; a.x = x; a.y = y; a.alpha = alpha;
    if (alpha == 1.0) launch_csr<OP_ADD>(A, a);
    else if (alpha == -1.0) launch_csr<OP_SUB>(A, a);
    else launch_csr<OP_AXPY>(A, a);
}

// --- reductions ----------------------------------------------------------------
// local partials -> d_red[slot .. slot+nq) -> (all-reduce over ranks) .  Host copy on demand.
static void d_finalize_to(int G, int nq, unsigned maxmask, double* out, bool dist)
{
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(BLOCK), 0, g_ctx.stream, g_ctx.d_partials, G, nq,
                       maxmask, out);
    if (dist && comm_size() > 1 && comm_allreduce(out, nq, maxmask, g_ctx.stream) < 0) comm_mark_failed();  // seen by fetch_red
}
static void d_finalize(int G, int nq, unsigned maxmask, int slot, bool dist)
{
    d_finalize_to(G, nq, maxmask, g_ctx.d_red + slot, dist);
}
static int fetch_red(int slot, int nq, double* out)
{
    HIPCK(hipMemcpyAsync(g_ctx.h_red + slot, g_ctx.d_red + slot, sizeof(double) * nq,
                         hipMemcpyDeviceToHost, g_ctx.stream));
    HIPCK(hipStreamSynchronize(g_ctx.stream));
    for (int q = 0; q < nq; ++q) out[q] = g_ctx.h_red[slot + q];
    if (comm_failed()) {  // an all-reduce or halo exchange failed: the scalars are local, unreduced values
        std::fprintf(stderr, "### ERROR: fasp_hip: rank %d: a collective failed; the iteration is abandoned\n", comm_rank());
        return ERROR_MISC;
    }
    return FASP_SUCCESS;
}
// (x,y) left on the device in reduction slot `slot` (no host round trip)
static int d_dot_to(int n, const double* x, const double* y, int slot, bool dist)
{
    const int G = vec_grid(n);
    hipLaunchKernelGGL(k_dot, dim3(G), dim3(BLOCK), 0, g_ctx.stream, n, x, y, g_ctx.d_partials);
    d_finalize(G, 1, 0u, slot, dist);
    return 0;
}
static int d_dot(int n, const double* x, const double* y, double* out, bool dist = false)
{
    const int G = vec_grid(n);
    hipLaunchKernelGGL(k_dot, dim3(G), dim3(BLOCK), 0, g_ctx.stream, n, x, y, g_ctx.d_partials);
    d_finalize(G, 1, 0u, 0, dist);
    return fetch_red(0, 1, out);
}
// out[0] = sum x^2, out[1] = max |x|
static int d_norms(int n, const double* x, double* out, bool dist = false)
{
    const int G = vec_grid(n);
    hipLaunchKernelGGL(k_norms, dim3(G), dim3(BLOCK), 0, g_ctx.stream, n, x, g_ctx.d_partials);
    d_finalize(G, 2, 0x2u, 0, dist);
    return fetch_red(0, 2, out);
}
static void d_axpy(int n, double a, const double* x, double* y)
{
    hipLaunchKernelGGL(k_axpy, dim3(vec_grid(n / 2 + 1)), dim3(BLOCK), 0, g_ctx.stream, n, a, x, y);
}
static void d_axpby(int n, double a, const double* x, double b, double* y)
{
    hipLaunchKernelGGL(k_axpby, dim3(vec_grid(n / 2 + 1)), dim3(BLOCK), 0, g_ctx.stream, n, a, x, b, y);
}

