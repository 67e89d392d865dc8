// Host-side check of KrylovWsT (faspsolver_amd/csrc/krylov_ws.h): the growth and free logic of the Krylov workspace over
// malloc / free.  Stand-alone: build with -fsanitize=address,undefined and run; exit status 0 = clean.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I faspsolver_amd/csrc tests/krylov_ws_check.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "krylov_ws.h"

static long g_live = 0, g_allocs = 0;
struct HostMem {
    static int alloc(double** q, size_t n)
    {
        *q = static_cast<double*>(std::malloc(sizeof(double) * (n ? n : 1)));
        if (!*q) return -1;
        std::memset(*q, 0xff, sizeof(double) * (n ? n : 1));   // not zero: ensure() has to zero the vectors itself
        ++g_live; ++g_allocs;
        return 0;
    }
    static int  zero(double* q, size_t n) { std::memset(q, 0, sizeof(double) * n); return 0; }
    static void release(double* q) { std::free(q); --g_live; }
};
using Ws = KrylovWsT<HostMem>;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

static bool all_zero(const Ws& W, size_t n)
{
    for (size_t i = 0; i < W.size(); ++i)
        for (size_t k = 0; k < n; ++k) if (W[i][k] != 0.0) return false;
    return true;
}

int main()
{
    {
        Ws W;
        CHECK(W.size() == 0 && g_live == 0);
        // growth: vectors already there are kept (address and contents), new ones come zeroed
        CHECK(W.ensure(3, 10) == 0 && W.size() == 3 && g_live == 3 && all_zero(W, 10));
        double* first = W[0];
        W[0][9] = 7.0;
        CHECK(W.ensure(2, 10) == 0 && W.size() == 3 && g_allocs == 3);          // a smaller need allocates nothing
        CHECK(W.ensure(6, 10) == 0 && W.size() == 6 && g_live == 6 && W[0] == first && W[0][9] == 7.0);
        for (size_t i = 0; i < W.size(); ++i) W[i][9] = 1.0;                    // writes up to the last entry
        // the Hessenberg buffer: allocated on first use, the same afterwards
        double* hh = W.hessenberg();
        CHECK(hh && g_live == 7 && W.hessenberg() == hh);
        hh[Ws::HH_LEN - 1] = 1.0;
        // a length change with existing vectors: all vectors are freed, the Hessenberg buffer stays
        CHECK(W.ensure(2, 33) == 0 && W.size() == 2 && g_live == 3 && all_zero(W, 33) && W.hessenberg() == hh);
        W[1][32] = 2.0;
        CHECK(W.ensure(4, 0) == 0 && W.size() == 4 && g_live == 5);             // length 0: one-entry allocations, nothing to zero
        // release twice, then ensure again
        W.release();
        CHECK(W.size() == 0 && g_live == 0);
        W.release();
        CHECK(W.size() == 0 && g_live == 0);
        CHECK(W.ensure(5, 17) == 0 && W.size() == 5 && g_live == 5 && all_zero(W, 17));
        CHECK(W.hessenberg() != nullptr && g_live == 6);
        W[4][16] = 3.0;
        W.release();
        CHECK(g_live == 0);
    }   // destruction after release
    CHECK(g_live == 0);
    {
        Ws W[2];   // two sets as a handle holds them, destroyed with vectors in them
        CHECK(W[0].ensure(9, 5) == 0 && W[1].ensure(24, 3) == 0 && W[1].hessenberg() && g_live == 34);
    }
    CHECK(g_live == 0);
    std::printf("krylov_ws_check ok: %ld allocations, none left\n", g_allocs);
    return 0;
}
