// devmem_test.cpp -- TEST INFRASTRUCTURE.  The owners of csrc/pbre_devmem.hpp against counting stand-ins of the HIP calls: construction, move,
// release on an early return, double release.  Host only (tests/test_devmem.py builds it with -fsanitize=address,undefined and runs it).
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <utility>

typedef int hipError_t;
typedef struct Ev_* hipEvent_t;
typedef struct St_* hipStream_t;
static int g_live = 0, g_made = 0, g_freed = 0, g_budget = 1 << 30;      // g_budget: allocations that still succeed
template <class T> static hipError_t make(T** p, size_t bytes) {
    if (g_budget <= 0) { *p = nullptr; return 2; }
    g_budget--; g_made++; g_live++;
    *p = (T*)std::malloc(bytes ? bytes : 1);
    return 0;
}
template <class T> static hipError_t hipMalloc(T** p, size_t bytes) { return make(p, bytes); }
template <class T> static hipError_t hipHostMalloc(T** p, size_t bytes, unsigned) { return make(p, bytes); }
static hipError_t hipEventCreate(hipEvent_t* e) { return make(e, 1); }
static hipError_t hipStreamCreate(hipStream_t* s) { return make(s, 1); }
static hipError_t unmake(void* p) { if (!p) return 1; g_live--; g_freed++; std::free(p); return 0; }
static hipError_t hipFree(void* p) { return unmake(p); }
static hipError_t hipHostFree(void* p) { return unmake(p); }
static hipError_t hipEventDestroy(hipEvent_t e) { return unmake(e); }
static hipError_t hipStreamDestroy(hipStream_t s) { return unmake(s); }

#define PBRE_DEVMEM_STUBS
#include "../../pybullet-robot-envs_amd/csrc/pbre_devmem.hpp"
using namespace pbre;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s (made %d freed %d live %d)\n", __LINE__, #c, g_made, g_freed, g_live); g_fail++; } } while (0)

struct Engine {      // shaped like an engine: several owners, set up by a function that returns at the first error
    DevBuf<float> a, b; HostBuf<int> h; Event ev[2]; Stream s;
    hipError_t init() {
        hipError_t e;
        if ((e = hipMalloc(a.out(), 64)) != 0) return e;
        if ((e = hipStreamCreate(s.out())) != 0) return e;
        for (auto& x : ev) if ((e = hipEventCreate(x.out())) != 0) return e;
        if ((e = hipHostMalloc(h.out(), 8, 0)) != 0) return e;
        return hipMalloc(b.out(), 64);
    }
};

int main() {
    {   // construction: empty owners release nothing
        DevBuf<float> d; Event e; Stream s; HostBuf<int> h;
        CHECK(!d && !e && !s && !h);
    }
    CHECK(g_made == 0 && g_freed == 0);
    {   // scope exit releases; the raw handle is what converts out
        DevBuf<float> d;
        CHECK(hipMalloc(d.out(), 16) == 0 && d);
        float* raw = d; raw[0] = 1.f; raw[3] = 2.f;
        CHECK(d[0] == 1.f && *(d + 3) == 2.f && g_live == 1);
    }
    CHECK(g_live == 0 && g_made == 1 && g_freed == 1);
    {   // move construction and move assignment: one owner at a time, the target's old handle is released
        DevBuf<int> x, y;
        CHECK(hipMalloc(x.out(), 4) == 0 && hipMalloc(y.out(), 4) == 0 && g_live == 2);
        int* px = x;
        DevBuf<int> z(std::move(x));
        CHECK(!x && (int*)z == px && g_live == 2);
        y = std::move(z);
        CHECK(!z && (int*)y == px && g_live == 1);
        y = std::move(y);                                  // self-assignment keeps the handle
        CHECK((int*)y == px && g_live == 1);
    }
    CHECK(g_live == 0 && g_made == g_freed);
    {   // double release, and out() on a live owner (a second hipMalloc into it) releases the first handle
        Event e;
        CHECK(hipEventCreate(e.out()) == 0 && g_live == 1);
        e.release(); e.release();
        CHECK(!e && g_live == 0);
        CHECK(hipEventCreate(e.out()) == 0 && hipEventCreate(e.out()) == 0 && g_live == 1);
    }
    CHECK(g_live == 0 && g_made == g_freed);
    for (int ok = 0; ok <= 6; ok++) {   // early return: a set-up that fails at its (ok + 1)-th allocation gives back exactly the `ok` it made
        const int made0 = g_made;
        g_budget = ok;
        {
            Engine eng;
            const hipError_t e = eng.init();
            CHECK((e == 0) == (ok == 6));
            CHECK(g_made - made0 == ok && g_live == ok);
        }
        CHECK(g_live == 0 && g_made == g_freed);
    }
    g_budget = 1 << 30;
    {   // arrays of owners (the event ring) and owners inside a moved aggregate
        Event ring[4][2];
        for (auto& pr : ring) for (auto& e : pr) CHECK(hipEventCreate(e.out()) == 0);
        CHECK(g_live == 8);
        Engine e1; CHECK(e1.init() == 0 && g_live == 14);
        Engine e2(std::move(e1));
        CHECK(g_live == 14 && !e1.a && e2.a);
    }
    CHECK(g_live == 0 && g_made == g_freed);
    std::printf(g_fail ? "devmem_test: %d check(s) FAILED\n" : "devmem_test OK (%d handles made and released)\n", g_fail ? g_fail : g_made);
    return g_fail ? 1 : 0;
}
