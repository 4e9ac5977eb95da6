// pbre_ik.hip -- the batched inverse-kinematics query (include/pbre_ik.h): per env the joint positions that bring a point of a link to a
// target pose, by the damped-least-squares iteration of the step (oracle/pbre_oracle.c: orc_ik), from the state records the engines keep on
// the device.  One kernel on the caller's stream, k_ik_query<M> (M = 6: position and orientation, M = 3: position only), one thread per env
// in blocks of 64, the table and the chain at wave-uniform addresses (the mapping of k_contact_query and k_kin_*).
//
// A solve is up to max_iters dependent iterations of four passes over the chain's joints; what an env carries between the passes stays on
// chip: the working q, world axis and world origin of every DoF that moves in dynamic LDS, [7 per DoF][64 lanes] floats (one column per
// thread: consecutive lanes on consecutive banks, no barrier -- nobody reads another thread's column), 1792 B per DoF and block, 12544 B for
// the Panda's seven arm joints; J J^T + lambda^2 I, its Cholesky factor, e and y in registers.  Only the chain from the root to the
// driven link is walked.  A lane whose convergence test passed applies no further update; the wave leaves the loop when none of its lanes
// is active.  Nothing goes through device memory but the inputs and the three small records each env's own thread stores; the state is
// never written.  The per-env solve is in pbre_ik.hpp (shared with the host tests).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include "../../include/pbre_ik.h"
#include "pbre_engine.hpp"
#include "pbre_scene.hpp"
#define PBRE_HD __host__ __device__ __forceinline__
#include "pbre_ik.hpp"

static_assert(PBRE_IK_MAX_CHAIN == pbre::ik::MAX_CHAIN && PBRE_IK_MAX_MOVING == pbre::ik::MAX_MOVING, "include/pbre_ik.h states the limits of pbre_ik.hpp");

namespace pbre {

constexpr int IQ_TPB = ik::IK_LANES;

struct IqParams {
    const float* tab;
    const float* state; int stride, n, nd;
    const float *tpos, *tquat, *qstart;
    float point[3];
    float l2, residual, rot_residual; int max_iters, clamp;
    float *q, *err; int32_t* iters;
    ik::Chain ch;
};

template <int M>
__global__ __launch_bounds__(IQ_TPB) void k_ik_query(const IqParams P) {
    extern __shared__ float ik_cols[];           // [7 nm][64]
    const int env = blockIdx.x * IQ_TPB + threadIdx.x;
    if (env >= P.n) return;
    const size_t e = (size_t)env;
    const float* qsrc = P.qstart ? P.qstart + e * P.nd : P.state + e * P.stride;
    const float tp[3] = {P.tpos[e * 3], P.tpos[e * 3 + 1], P.tpos[e * 3 + 2]};
    const float pt[3] = {P.point[0], P.point[1], P.point[2]};
    float Rt[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    if (M == 6) {
        const float qt[4] = {P.tquat[e * 4], P.tquat[e * 4 + 1], P.tquat[e * 4 + 2], P.tquat[e * 4 + 3]};
        ik::quat_to_R(qt, Rt);
    }
    ik::solve<M>(P.tab, P.ch, qsrc, P.nd, tp, Rt, pt, P.l2, P.residual, P.rot_residual, P.max_iters, P.clamp != 0, ik_cols + threadIdx.x,
                 P.q ? P.q + e * P.nd : nullptr, P.err ? P.err + e * 2 : nullptr, P.iters ? P.iters + e : nullptr,
                 [](bool active) { return __any(active ? 1 : 0) != 0; });
}

}  // namespace pbre

using namespace pbre;

// (the ctx: pbre_engine.hpp -- state_view, fail (pbre_capi.hip) and its record pbre_ctx::readers (pbre_scene.hpp: the RobotTable copy, IkBufs))

static int check_query(pbre_ctx* ctx, const pbre_ik_query_t* q) {
    if (!ctx) return fail(nullptr, PBRE_E_ARG, "pbre_ik_query: null ctx");
    if (!q) return fail(ctx, PBRE_E_ARG, "pbre_ik_query: null query struct");
    for (int k = 0; k < 3; k++) if (std::isnan(q->point[k])) return fail(ctx, PBRE_E_ARG, "pbre_ik_query: point is NaN");
    if (!q->target_pos) return fail(ctx, PBRE_E_ARG, "pbre_ik_query: target_pos is null");
    if (q->max_iters > 1000) return fail(ctx, PBRE_E_ARG, "pbre_ik_query: max_iters is above 1000");
    return PBRE_OK;
}
static bool nothing_asked(const pbre_ik_query_t* q) { return !q->q && !q->err && !q->iters; }

// the checks that need the table; fills the chain and the scalars
static int check_table(pbre_ctx* ctx, const pbre_ik_query_t& q, int stride, IqParams& P) {
    const Readers& s = ctx->readers;
    if (s.table.empty()) return fail(ctx, PBRE_E_TABLE, "pbre_ik_query: the ctx has no RobotTable");
    const double* t = s.table.data();
    const int nl = s.nl, nd = s.ndof;
    if (t[18] == 0.0) return fail(ctx, PBRE_E_UNSUPPORTED, "pbre_ik_query: a RobotTable with fixed_base = 0 (a free-floating base) is not supported");
    if (nl > 128 || nd > 64 || nd < 0) return fail(ctx, PBRE_E_UNSUPPORTED, "pbre_ik_query: more than 128 links or 64 DoF");
    const int link = q.link == -1 ? (int)t[4] : q.link;
    if (link < 0 || link >= nl) return fail(ctx, PBRE_E_ARG, "pbre_ik_query: link is outside the table");
    const int W = (stride - 16) / 2;
    if (nd > W) return fail(ctx, PBRE_E_TABLE, "pbre_ik_query: the RobotTable has more DoFs than the state record has lanes");
    for (int i = 0; i < nl; i++) {           // what the walk indexes with: parents before children, joint values inside a record's lanes
        const double* r = t + 24 + i * 40;
        if (!(r[0] < (double)i) || !(r[0] >= -1.0) || (r[1] != 0.0 && !(r[33] >= 0.0 && r[33] < (double)std::min(nd, W))) || r[1] < 0.0 || r[1] > 2.0)
            return fail(ctx, PBRE_E_TABLE, "pbre_ik_query: RobotTable links out of order or a joint index outside the state record");
    }
    const int rc = ik::resolve_chain(t, link, q.dof_mask, P.ch);
    if (rc == 1) return fail(ctx, PBRE_E_UNSUPPORTED, "pbre_ik_query: the chain from the root to the link has more than 64 links (PBRE_IK_MAX_CHAIN)");
    if (rc == 2) return fail(ctx, PBRE_E_UNSUPPORTED, "pbre_ik_query: more than 24 DoFs of the chain move (PBRE_IK_MAX_MOVING: their working set is kept in LDS)");
    const double damping = q.damping < 0.0 ? ctx->cfg.ik_damping : q.damping;
    P.l2 = (float)(damping * damping);
    P.residual = (float)(q.residual < 0.0 ? ctx->cfg.ik_residual : q.residual);
    P.rot_residual = q.rot_residual > 0.0 ? (float)q.rot_residual : 0.0f;
    P.max_iters = q.max_iters < 0 ? ctx->cfg.ik_max_iters : q.max_iters;
    if (P.max_iters > 1000) return fail(ctx, PBRE_E_ARG, "pbre_ik_query: the ctx's ik_max_iters is above 1000");
    if (P.max_iters < 0) P.max_iters = 0;
    P.clamp = q.clamp_limits != 0;
    for (int k = 0; k < 3; k++) P.point[k] = q.point[k];
    return PBRE_OK;
}

// enqueue the kernel on v.stream; the inputs and outputs are device pointers
static int query_on(pbre_ctx* ctx, const StateView& v, const pbre_ik_query_t& q, IqParams& P) {
    hipStream_t st = (hipStream_t)v.stream;
    const Readers& r = ctx->readers;
    IkBufs& s = ctx->readers.ik;
    if (!s.table) PBRE_CHK_ON(ctx, upload_once(s.table, ik::ik_table(r.table.data())));      // once per ctx: the RobotTable never changes
    P.tab = s.table; P.state = v.state; P.stride = v.stride; P.n = v.n; P.nd = r.ndof;
    P.tpos = q.target_pos; P.tquat = q.target_quat; P.qstart = q.q_start;
    P.q = q.q; P.err = q.err; P.iters = q.iters;
    const dim3 grid((v.n + IQ_TPB - 1) / IQ_TPB), block(IQ_TPB);
    const size_t lds = (size_t)P.ch.nm * ik::IK_SLOT * ik::IK_LANES * sizeof(float);
    if (q.target_quat) hipLaunchKernelGGL((k_ik_query<6>), grid, block, lds, st, P);
    else hipLaunchKernelGGL((k_ik_query<3>), grid, block, lds, st, P);
    PBRE_CHK_ON(ctx, hipGetLastError());
    return PBRE_OK;
}

extern "C" {

int pbre_ik_query_device(pbre_ctx* ctx, const pbre_ik_query_t* q, void* stream) {
    int rc = check_query(ctx, q);
    if (rc != PBRE_OK) return rc;
    StateView v;
    if ((rc = ctx->state_view(&v, stream, false)) != PBRE_OK) return rc;
    IqParams P;
    std::memset(&P, 0, sizeof P);
    if ((rc = check_table(ctx, *q, v.stride, P)) != PBRE_OK) return rc;
    if (nothing_asked(q)) return PBRE_OK;
    return query_on(ctx, v, *q, P);
}

int pbre_ik_query(pbre_ctx* ctx, const pbre_ik_query_t* q) {
    int rc = check_query(ctx, q);
    if (rc != PBRE_OK) return rc;
    StateView v;
    if ((rc = ctx->state_view(&v, nullptr, true)) != PBRE_OK) return rc;
    IqParams P;
    std::memset(&P, 0, sizeof P);
    if ((rc = check_table(ctx, *q, v.stride, P)) != PBRE_OK) return rc;
    if (nothing_asked(q)) return PBRE_OK;
    const size_t nd = (size_t)ctx->readers.ndof, rec = (size_t)v.n * sizeof(float);
    hipStream_t st = (hipStream_t)v.stream;
    Stage sg;                                    // q | err | iters | target_pos | target_quat | q_start; what is not given takes no space
    auto add = [&](const void* host, size_t words, bool in) { return sg.add(host, host ? words * rec : 0, in); };
    const int i_q = add(q->q, nd, false), i_err = add(q->err, 2, false), i_it = add(q->iters, 1, false), i_tp = add(q->target_pos, 3, true),
              i_tq = add(q->target_quat, 4, true), i_qs = add(q->q_start, nd, true);
    PBRE_CHK_ON(ctx, sg.begin(ctx->readers.ik.out, ctx->readers.ik.cap_out, st));
    pbre_ik_query_t d = *q;
    d.q = sg.dev<float>(i_q); d.err = sg.dev<float>(i_err); d.iters = sg.dev<int32_t>(i_it);
    d.target_pos = sg.dev<float>(i_tp); d.target_quat = sg.dev<float>(i_tq); d.q_start = sg.dev<float>(i_qs);
    if ((rc = query_on(ctx, v, d, P)) != PBRE_OK) return rc;
    PBRE_CHK_ON(ctx, sg.finish(st));
    return PBRE_OK;
}

}  // extern "C"
