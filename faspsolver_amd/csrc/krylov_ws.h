// krylov_ws.h -- the workspace of the Krylov drivers (krylov.hip.h): it owns its memory.
// Stand-alone header: the memory calls go through the policy Mem, so the growth and free logic also runs over
// malloc / free on the host (tests/krylov_ws_check.cpp).  Mem has
//   static int  alloc(double** q, size_t n);   // n doubles; < 0: failed
//   static int  zero(double* q, size_t n);     // q[0..n) = 0; < 0: failed
//   static void release(double* q);
#pragma once
#include <cstddef>
#include <vector>

template <class Mem>
struct KrylovWsT {
    static constexpr size_t HH_LEN = 1024;   // the Hessenberg column of gmres_device (restart + 3 <= HH_LEN)
    KrylovWsT() = default;
    KrylovWsT(const KrylovWsT&) = delete;
    KrylovWsT& operator=(const KrylovWsT&) = delete;
    ~KrylovWsT() { release(); }

    // at least `count` zero-initialised vectors of nvec doubles; vectors of another length are freed first
    int ensure(size_t count, size_t nvec)
    {
        if (len != nvec) { free_vectors(); len = nvec; }
        while (v.size() < count) {
            double* q = nullptr;
            int st = Mem::alloc(&q, nvec);
            if (st < 0) return st;
            if ((st = Mem::zero(q, nvec)) < 0) { Mem::release(q); return st; }
            v.push_back(q);
        }
        return 0;
    }
    size_t   size() const { return v.size(); }
    double*  operator[](size_t i) const { return v[i]; }
    double** data() { return v.data(); }
    // the Hessenberg buffer, allocated on first use (nullptr: the allocation failed)
    double* hessenberg()
    {
        if (!hh && Mem::alloc(&hh, HH_LEN) < 0) hh = nullptr;
        return hh;
    }
    void release()
    {
        free_vectors();
        len = 0;
        if (hh) Mem::release(hh);
        hh = nullptr;
    }

private:
    void free_vectors()
    {
        for (double* q : v) if (q) Mem::release(q);
        v.clear();
    }
    std::vector<double*> v;
    size_t               len = 0;   // common length of the vectors
    double*              hh = nullptr;
};
