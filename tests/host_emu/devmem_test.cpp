// devmem_test.cpp -- TEST INFRASTRUCTURE.  The owners of csrc/pbre_devmem.hpp against counting stand-ins of the HIP calls: construction, move,
// release on an early return, double release; then the helpers of csrc/pbre_devwork.hpp on top of them -- grow, upload_once, Stage.
// Host only (tests/test_devmem.py builds it with -fsanitize=address,undefined and runs it).
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

typedef int hipError_t;
enum { hipSuccess = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
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
static int g_syncs = 0, g_stream_syncs = 0, g_copies = 0, g_copy_fails = 0;      // g_copy_fails: copies that still fail
static hipError_t hipDeviceSynchronize() { g_syncs++; return 0; }
static hipError_t hipStreamSynchronize(hipStream_t) { g_stream_syncs++; return 0; }
static hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, int) {
    if (g_copy_fails > 0) { g_copy_fails--; return 3; }
    g_copies++; std::memcpy(dst, src, bytes);
    return 0;
}
static hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, int kind, hipStream_t) { return hipMemcpy(dst, src, bytes, kind); }

#define PBRE_DEVMEM_STUBS
#include "../../pybullet-robot-envs_amd/csrc/pbre_devwork.hpp"
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

struct Unit {        // shaped like a unit's record (pbre_scene.hpp): a table uploaded once, a work buffer, the host variant's block
    DevBuf<float> table;
    DevBuf<float> work; size_t cap_work = 0;
    DevBuf<char> out; size_t cap_out = 0;
};

static void test_helpers() {
    {   // grow: allocates on first need, does nothing within the capacity, frees and reallocates beyond it, synchronises only then
        DevBuf<float> b; size_t cap = 0;
        const int made0 = g_made, freed0 = g_freed;
        CHECK(grow(b, cap, 10, true) == 0 && b && cap == 10 && g_made - made0 == 1 && g_syncs == 1);
        b[9] = 1.f;
        float* p0 = b;
        CHECK(grow(b, cap, 10, true) == 0 && grow(b, cap, 3, true) == 0 && grow(b, cap, 0, true) == 0);
        CHECK((float*)b == p0 && cap == 10 && g_made - made0 == 1 && g_freed == freed0 && g_syncs == 1);
        CHECK(grow(b, cap, 11, false) == 0 && cap == 11 && g_made - made0 == 2 && g_freed - freed0 == 1 && g_live == 1 && g_syncs == 1);
        b[10] = 2.f;
        CHECK(grow(b, cap, 40, true) == 0 && cap == 40 && g_live == 1 && g_syncs == 2);
        b[39] = 3.f;
        g_budget = 0;                                      // a failed allocation: nothing stale is left, and the next call tries again
        CHECK(grow(b, cap, 41, true) != 0 && !b && cap == 0 && g_live == 0 && g_syncs == 3);
        CHECK(grow(b, cap, 5, false) != 0 && !b && cap == 0);
        g_budget = 1 << 30;
        CHECK(grow(b, cap, 5, false) == 0 && b && cap == 5 && g_live == 1 && g_syncs == 3);
        b[4] = 4.f;
    }
    CHECK(g_live == 0 && g_made == g_freed);
    {   // upload_once: the table arrives; a failed copy or a failed allocation leaves nothing live
        const std::vector<float> tab = {1.f, 2.f, 3.f};
        DevBuf<float> t;
        CHECK(upload_once(t, tab) == 0 && t && t[0] == 1.f && t[2] == 3.f && g_live == 1);
        DevBuf<float> u;
        g_copy_fails = 1;
        CHECK(upload_once(u, tab) != 0 && !u && g_live == 1);
        g_budget = 0;
        CHECK(upload_once(u, tab) != 0 && !u && g_live == 1);
        g_budget = 1 << 30;
        CHECK(upload_once(u, tab) == 0 && u && u[1] == 2.f && g_live == 2);
    }
    CHECK(g_live == 0 && g_made == g_freed);
    {   // a unit's record, grown a few times and dropped
        Unit u;
        const std::vector<float> tab(7, 1.f);
        CHECK(upload_once(u.table, tab) == 0);
        for (size_t need : {4u, 64u, 16u, 65u, 300u}) CHECK(grow(u.work, u.cap_work, need, true) == 0 && grow(u.out, u.cap_out, 3 * need, false) == 0);
        CHECK(g_live == 3 && u.cap_work == 300 && u.cap_out == 900);
        Unit w(std::move(u));
        CHECK(g_live == 3 && !u.work && w.work);
    }
    CHECK(g_live == 0 && g_made == g_freed);
    const size_t n = 131;
    {   // Stage, the contact query's block: flags | dist[3] | nearest[2] | count[2] | tips at 0, 4n, 16n, 24n, 32n; what is not asked for
        // keeps its place and gets no pointer and no copy
        Unit u;
        std::vector<int> flags(n, -1), nearest(2 * n, -1), tips(n, -1);
        Stage sg;
        const int a = sg.add(flags.data(), n * 4), b = sg.add(nullptr, n * 12), c = sg.add(nearest.data(), n * 8), d = sg.add(nullptr, n * 8), e = sg.add(tips.data(), n * 4);
        const int copies0 = g_copies, ss0 = g_stream_syncs, ds0 = g_syncs;
        CHECK(sg.begin(u.out, u.cap_out, nullptr) == 0 && u.cap_out == 36 * n && g_copies == copies0 && g_syncs == ds0);
        char* base = u.out;
        CHECK(sg.dev<char>(a) == base && !sg.dev<char>(b) && sg.dev<char>(c) == base + 16 * n && !sg.dev<char>(d) && sg.dev<char>(e) == base + 32 * n);
        CHECK(sg.s[b].off == 4 * n && sg.s[d].off == 24 * n);
        for (size_t i = 0; i < n; i++) { sg.dev<int>(a)[i] = (int)i; sg.dev<int>(c)[2 * i + 1] = 7; sg.dev<int>(e)[i] = 9; }
        CHECK(sg.finish(nullptr) == 0 && g_copies - copies0 == 3 && g_stream_syncs - ss0 == 1);
        CHECK(flags[130] == 130 && nearest[261] == 7 && tips[0] == 9);
        Stage again;                                       // the same need: the block stays
        again.add(flags.data(), n * 36);
        CHECK(again.begin(u.out, u.cap_out, nullptr) == 0 && (char*)u.out == base);
    }
    CHECK(g_live == 0 && g_made == g_freed);
    {   // the camera's: depth | seg | rgba at 0, 4 px, 8 px
        Unit u;
        const size_t px = n * 33 * 17;
        std::vector<float> depth(px);
        std::vector<unsigned char> rgba(4 * px);
        Stage sg;
        const int a = sg.add(depth.data(), px * 4), b = sg.add(nullptr, px * 4), c = sg.add(rgba.data(), px * 4);
        CHECK(sg.begin(u.out, u.cap_out, nullptr) == 0 && u.cap_out == 12 * px);
        CHECK(sg.dev<char>(a) == (char*)u.out && !sg.dev<char>(b) && sg.s[b].off == 4 * px && sg.dev<char>(c) == (char*)u.out + 8 * px);
    }
    {   // the kinematics query's: pose | vel | jac | mass | tau | qdd, nothing for what is not asked for (0 bytes), qdd uploaded by begin()
        Unit u;
        const size_t nd = 9, rec = n * 4;
        std::vector<float> vel(6 * n), mass(nd * nd * n), tau(nd * n), qdd(nd * n, 5.f);
        Stage sg;
        const int ip = sg.add(nullptr, 0), iv = sg.add(vel.data(), 6 * rec), ij = sg.add(nullptr, 0), im = sg.add(mass.data(), nd * nd * rec), it = sg.add(tau.data(), nd * rec),
                  iq = sg.add(qdd.data(), nd * rec, true);
        const int copies0 = g_copies;
        CHECK(sg.begin(u.out, u.cap_out, nullptr) == 0 && u.cap_out == (6 + nd * nd + nd + nd) * rec && g_copies - copies0 == 1);
        char* base = u.out;
        CHECK(!sg.dev<char>(ip) && sg.dev<char>(iv) == base && !sg.dev<char>(ij) && sg.dev<char>(im) == base + 6 * rec && sg.dev<char>(it) == base + (6 + nd * nd) * rec);
        CHECK(sg.dev<char>(iq) == base + (6 + nd * nd + nd) * rec && sg.dev<float>(iq)[nd * n - 1] == 5.f);
        CHECK(sg.finish(nullptr) == 0 && g_copies - copies0 == 4);      // (the upload is not copied back)
        Stage none;                                        // nothing but zero-byte outputs: still a block to point into
        none.add(nullptr, 0);
        Unit e;
        CHECK(none.begin(e.out, e.cap_out, nullptr) == 0 && e.out && e.cap_out == 4 && none.finish(nullptr) == 0);
    }
    CHECK(g_live == 0 && g_made == g_freed);
    {   // a block that cannot be allocated: begin() fails, nothing is live
        Unit u;
        Stage sg;
        float x[4];
        sg.add(x, 16);
        g_budget = 0;
        CHECK(sg.begin(u.out, u.cap_out, nullptr) != 0 && !u.out && u.cap_out == 0);
        g_budget = 1 << 30;
    }
    CHECK(g_live == 0 && g_made == g_freed);
}

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
    test_helpers();
    std::printf(g_fail ? "devmem_test: %d check(s) FAILED\n" : "devmem_test OK (%d handles made and released)\n", g_fail ? g_fail : g_made);
    return g_fail ? 1 : 0;
}
