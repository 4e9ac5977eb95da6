// pbre_contacts.hip -- the batched contact query (include/pbre_contacts.h): per env the contact flags, the smallest signed distance of each
// pair, the collision sphere attaining it, the count of spheres within the margin and the fingertip mask, from the state records the
// engines keep on the device.  One kernel on the caller's stream:
//   k_contact_query  one thread per env: forward kinematics of the RobotTable in fp32 (pbre_scene.hpp: scene_fk, the camera's), then a loop
//                    over the collision spheres in table order (runtime count, not unrolled) -- each against the table box and the object --
//                    then the object's candidate points against the table top.  The link frames go through a buffer [n_links][12][N] (one
//                    column per env: coalesced); a sphere on the link of the sphere before it keeps that frame in registers.  The table, the
//                    spheres and the hull are read at wave-uniform addresses.  No scratch, no LDS, no atomics, nothing between workgroups;
//                    an env's outputs are stored by its own thread, consecutive threads to consecutive records.
// The state is never written.  The per-pair functions are in pbre_contacts.hpp (shared with the host tests).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/pbre_contacts.h"
#include "pbre_engine.hpp"
#include "pbre_tables.hpp"
#include "pbre_scene.hpp"
#define PBRE_HD __host__ __device__ __forceinline__
#include "pbre_contacts.hpp"

namespace pbre {

constexpr int CQ_TPB = 64;

struct CqParams {
    const float* tab;                           // CT_HDR | links | spheres (CQ_SPHERE floats each)
    const float* state; int stride, n, obj_lane, ns;
    float* frames;
    float margin;
    int obj_shape;                              // PBRE_SHAPE_*, -1: no object
    float obj_h[3], tab_c[3], tab_h[3];
    const float* hull;
    int32_t* flags; float* dist; int32_t* nearest; int32_t* count; int32_t* tips;
};

__global__ __launch_bounds__(CQ_TPB) void k_contact_query(const CqParams P) {
    const int env = blockIdx.x * CQ_TPB + threadIdx.x;
    if (env >= P.n) return;
    const float* st = P.state + (size_t)env * P.stride;
    const size_t N = (size_t)P.n;
    scene_fk(P.tab, st, env, N, P.frames);
    const float* S = P.tab + CT_HDR + CT_LINK * (int)P.tab[0];
    const bool obj = P.obj_shape >= 0;
    float op[3] = {0.0f, 0.0f, 0.0f}, Ro[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    if (obj) {
        const float* o = st + P.obj_lane;
        op[0] = o[0]; op[1] = o[1]; op[2] = o[2];
        const float q[4] = {o[3], o[4], o[5], o[6]};
        cq::quat_R(q, Ro);
    }
    const float reach = P.margin + (P.obj_shape == PBRE_SHAPE_HULL ? cq::hull_rb_max(P.hull) : 0.0f);      // the hull early-out's (pbre_contacts.hpp)
    float d_ro = cq::CQ_FAR, d_rt = cq::CQ_FAR;
    int i_ro = -1, i_rt = -1, c_ro = 0, c_rt = 0, tips = 0;
    int last = -1;
    float R[9], p[3];
    for (int k = 0; k < 9; k++) R[k] = 0.0f;
    for (int k = 0; k < 3; k++) p[k] = 0.0f;
#pragma unroll 1
    for (int k = 0; k < P.ns; k++) {
        const float* V = S + CQ_SPHERE * k;
        const int link = (int)V[0];
        if (link != last) {                  // (wave-uniform)
            const float* F = P.frames + (size_t)link * 12 * N + env;
            for (int j = 0; j < 9; j++) R[j] = F[j * N];
            for (int j = 0; j < 3; j++) p[j] = F[(9 + j) * N];
            last = link;
        }
        const float sc[3] = {p[0] + (R[0] * V[1] + R[1] * V[2] + R[2] * V[3]), p[1] + (R[3] * V[1] + R[4] * V[2] + R[5] * V[3]),
                             p[2] + (R[6] * V[1] + R[7] * V[2] + R[8] * V[3])};
        const float sr = V[4];
        const float dt = cq::sphere_aabb_dist(sc, sr, P.tab_c, P.tab_h);
        if (dt < d_rt) { d_rt = dt; i_rt = k; }      // (strict: a tie keeps the lower index)
        c_rt += dt < P.margin ? 1 : 0;
        if (obj) {
            const float d_o = cq::sphere_object_dist(P.obj_shape, sc, sr, op, Ro, P.obj_h, P.hull, reach);
            if (d_o < d_ro) { d_ro = d_o; i_ro = k; }
            const bool in = d_o < P.margin;
            c_ro += in ? 1 : 0;
            const int slot = (int)V[5];
            if (in && slot > 0) tips |= 1 << (slot - 1);
        }
    }
    const float d_ot = obj ? cq::object_table_dist(P.obj_shape, op, Ro, P.obj_h, P.hull, P.tab_c, P.tab_h) : cq::CQ_FAR;
    if (P.flags) P.flags[env] = (d_ot < P.margin ? PBRE_CQ_OBJECT_TABLE : 0) | (c_ro > 0 ? PBRE_CQ_ROBOT_OBJECT : 0) | (c_rt > 0 ? PBRE_CQ_ROBOT_TABLE : 0);
    if (P.dist) { float* d = P.dist + (size_t)env * 3; d[0] = d_ot; d[1] = d_ro; d[2] = d_rt; }
    if (P.nearest) { int32_t* q = P.nearest + (size_t)env * 2; q[0] = i_ro; q[1] = i_rt; }
    if (P.count) { int32_t* q = P.count + (size_t)env * 2; q[0] = c_ro; q[1] = c_rt; }
    if (P.tips) P.tips[env] = tips;
}

}  // namespace pbre

using namespace pbre;

// (the ctx: pbre_engine.hpp -- state_view, fail (pbre_capi.hip) and its record pbre_ctx::readers (pbre_scene.hpp: the RobotTable copy, CqBufs))

static int check_query(pbre_ctx* ctx, const pbre_contact_out* o, float margin) {
    if (!ctx) return fail(nullptr, PBRE_E_ARG, "pbre_contact_query: null ctx");
    if (!o) return fail(ctx, PBRE_E_ARG, "pbre_contact_query: null output struct");
    if (std::isnan(margin)) return fail(ctx, PBRE_E_ARG, "pbre_contact_query: margin is NaN");
    return PBRE_OK;
}
static bool nothing_asked(const pbre_contact_out* o) { return !o->flags && !o->dist && !o->nearest && !o->count && !o->tips; }

// enqueue the kernel on v.stream; the outputs are device pointers (null: skipped)
static int query_on(pbre_ctx* ctx, const StateView& v, const pbre_contact_out& o, float margin) {
    Readers& r = ctx->readers;
    CqBufs& s = r.cq;
    if (r.table.empty()) return fail(ctx, PBRE_E_TABLE, "pbre_contact_query: the ctx has no RobotTable");
    hipStream_t st = (hipStream_t)v.stream;
    const int ns = r.ns;
    if (!s.table) {                              // header, links, spheres: once per ctx
        std::vector<float> tab = scene_link_table(r);
        const double* t = r.table.data();
        for (int k = 0; k < ns; k++) {
            const double* q = t + 24 + r.nl * 40 + k * 8;
            const float rec[CQ_SPHERE] = {(float)q[0], (float)q[1], (float)q[2], (float)q[3], (float)q[4], (float)q[6], 0.0f, 0.0f};
            if (!(q[0] >= 0.0 && q[0] < (double)r.nl)) return fail(ctx, PBRE_E_TABLE, "pbre_contact_query: a collision sphere's link index is out of range");
            if (q[6] > 32.0) return fail(ctx, PBRE_E_TABLE, "pbre_contact_query: more than 32 fingertip slots");
            tab.insert(tab.end(), rec, rec + CQ_SPHERE);
        }
        for (int i = 0; i < r.nl; i++) {         // what scene_fk indexes with: parents before children, joint values inside a record
            const float* L = tab.data() + CT_HDR + CT_LINK * i;
            if (!(L[0] < (float)i) || (L[1] != 0.0f && !(L[17] >= 0.0f && L[17] < (float)v.stride)))
                return fail(ctx, PBRE_E_TABLE, "pbre_contact_query: RobotTable links out of order or a joint index outside the state record");
        }
        PBRE_CHK_ON(ctx, upload_once(s.table, tab));
    }
    // (a query in flight on another stream may still use the old buffer)
    PBRE_CHK_ON(ctx, grow(s.frames, s.cap_frames, (size_t)std::max(r.nl, 1) * 12 * v.n, true));
    CqParams P;
    std::memset(&P, 0, sizeof P);
    P.tab = s.table; P.state = v.state; P.stride = v.stride; P.n = v.n; P.obj_lane = v.obj_lane; P.ns = ns;
    P.frames = s.frames;
    P.margin = margin < 0.0f ? (float)v.phys.contact_margin : margin;
    P.obj_shape = (v.flags & PBRE_F_NO_OBJECT) ? -1 : v.phys.obj_shape;
    for (int k = 0; k < 3; k++) { P.tab_c[k] = (float)v.phys.table_c[k]; P.tab_h[k] = (float)v.phys.table_h[k]; P.obj_h[k] = (float)v.phys.obj_h[k]; }
    P.hull = v.hull;
    if (P.obj_shape == PBRE_SHAPE_HULL) {
        if (!P.hull) return fail(ctx, PBRE_E_ARG, "pbre_contact_query: a hull object without a hull table");
    } else if (P.obj_shape > PBRE_SHAPE_HULL || P.obj_shape < -1) return fail(ctx, PBRE_E_UNSUPPORTED, "pbre_contact_query: unknown object shape");
    P.flags = o.flags; P.dist = o.dist; P.nearest = o.nearest; P.count = o.count; P.tips = o.tips;
    hipLaunchKernelGGL(k_contact_query, dim3((v.n + CQ_TPB - 1) / CQ_TPB), dim3(CQ_TPB), 0, st, P);
    PBRE_CHK_ON(ctx, hipGetLastError());
    return PBRE_OK;
}

extern "C" {

int pbre_contact_query_device(pbre_ctx* ctx, const pbre_contact_out* d_out, float margin, void* stream) {
    int rc = check_query(ctx, d_out, margin);
    if (rc != PBRE_OK) return rc;
    if (nothing_asked(d_out)) return PBRE_OK;
    StateView v;
    if ((rc = ctx->state_view(&v, stream, false)) != PBRE_OK) return rc;
    return query_on(ctx, v, *d_out, margin);
}

int pbre_contact_query(pbre_ctx* ctx, const pbre_contact_out* out, float margin) {
    int rc = check_query(ctx, out, margin);
    if (rc != PBRE_OK) return rc;
    if (nothing_asked(out)) return PBRE_OK;
    StateView v;
    if ((rc = ctx->state_view(&v, nullptr, true)) != PBRE_OK) return rc;
    const size_t n = (size_t)v.n;
    hipStream_t st = (hipStream_t)v.stream;
    Stage sg;                                    // flags | dist[3] | nearest[2] | count[2] | tips, 4 bytes each
    const int i_flags = sg.add(out->flags, n * 4), i_dist = sg.add(out->dist, n * 12), i_nearest = sg.add(out->nearest, n * 8), i_count = sg.add(out->count, n * 8),
              i_tips = sg.add(out->tips, n * 4);
    PBRE_CHK_ON(ctx, sg.begin(ctx->readers.cq.out, ctx->readers.cq.cap_out, st));
    const pbre_contact_out d = {sg.dev<int32_t>(i_flags), sg.dev<float>(i_dist), sg.dev<int32_t>(i_nearest), sg.dev<int32_t>(i_count), sg.dev<int32_t>(i_tips)};
    if ((rc = query_on(ctx, v, d, margin)) != PBRE_OK) return rc;
    PBRE_CHK_ON(ctx, sg.finish(st));
    return PBRE_OK;
}

}  // extern "C"
