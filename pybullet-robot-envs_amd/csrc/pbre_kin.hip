// pbre_kin.hip -- the batched kinematics / dynamics query (include/pbre_kin.h): per env the pose and velocity of the links asked for, the
// Jacobian of a point, M(q) and the inverse-dynamics torques, from the state records the engines keep on the device.  Up to seven small
// kernels on the caller's stream, each only when an output needs it, all one thread per env in blocks of 64, the table at wave-uniform
// addresses, runtime loops over the links, no scratch, no atomics, nothing between workgroups (the mapping of k_contact_query):
//   k_kin_fk<VEL, ACC>  the forward walk: per link R, p, the world axis, and (VEL) w, v, (ACC) al, acc into the column buffer [link][27][N]
//   k_kin_links         pose / vel records of the links asked for, stored by the env's own thread
//   k_kin_jac           the walk from jac_link to the root: the non-zero Jacobian columns into the staging columns [6 nd][N]
//   k_kin_tau           RNEA's backward pass through wrench columns [link][6][N]; tau stored by the env's own thread
//   k_kin_mass          composite rigid bodies through composite columns [link][10][N]; the entries of DoF pairs on one path to the root
//                       into the staging columns [nd nd][N]
//   k_kin_rows<MASS>    staging columns -> the env-major `jac` / `mass` records: a 64 env x 64 element tile goes through LDS (rows padded
//                       to 65 floats: the transposed read is conflict-free) and leaves with consecutive lanes on consecutive addresses.
//                       Entries that the walks never write (columns of DoFs that are no ancestors; DoF pairs on different branches) are
//                       zeros the kernel knows from the table, not loads.
// The state is never written.  The per-env walks are in pbre_kin.hpp (shared with the host tests).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "../../include/pbre_kin.h"
#include "pbre_engine.hpp"
#include "pbre_scene.hpp"
#define PBRE_HD __host__ __device__ __forceinline__
#include "pbre_kin.hpp"

namespace pbre {

constexpr int KQ_TPB = 64, KQ_TILE = 64, KQ_LD = KQ_TILE + 1;

struct KqParams {
    const float* tab;
    const float* state; int stride, W, n, nd;
    float *cols, *comp, *wr, *stage;
    const float* qdd; float g_up;
    int n_links, at_com, jac_link, jac_at_com;
    float jac_point[3];
    float *pose, *vel, *tau;
    unsigned char links[kin::MAX_LINKS];
};

template <bool VEL, bool ACC>
__global__ __launch_bounds__(KQ_TPB) void k_kin_fk(const KqParams P) {
    const int env = blockIdx.x * KQ_TPB + threadIdx.x;
    if (env >= P.n) return;
    const float* st = P.state + (size_t)env * P.stride;
    kin::fk<VEL, ACC>(P.tab, st, st + P.W, P.qdd ? P.qdd + (size_t)env * P.nd : nullptr, P.g_up, env, (size_t)P.n, P.cols);
}

__global__ __launch_bounds__(KQ_TPB) void k_kin_links(const KqParams P) {
    const int env = blockIdx.x * KQ_TPB + threadIdx.x;
    if (env >= P.n) return;
#pragma unroll 1
    for (int j = 0; j < P.n_links; j++) {
        const size_t rec = (size_t)env * P.n_links + j;
        kin::link_out(P.tab, P.cols, (int)P.links[j], P.at_com != 0, env, (size_t)P.n, P.pose ? P.pose + rec * 7 : nullptr, P.vel ? P.vel + rec * 6 : nullptr);
    }
}

__global__ __launch_bounds__(KQ_TPB) void k_kin_jac(const KqParams P) {
    const int env = blockIdx.x * KQ_TPB + threadIdx.x;
    if (env >= P.n) return;
    kin::jac(P.tab, P.cols, P.jac_link, P.jac_point, P.jac_at_com != 0, env, (size_t)P.n, P.stage);
}

__global__ __launch_bounds__(KQ_TPB) void k_kin_tau(const KqParams P) {
    const int env = blockIdx.x * KQ_TPB + threadIdx.x;
    if (env >= P.n) return;
    kin::rnea(P.tab, P.cols, P.wr, env, (size_t)P.n, P.tau + (size_t)env * P.nd);
}

__global__ __launch_bounds__(KQ_TPB) void k_kin_mass(const KqParams P) {
    const int env = blockIdx.x * KQ_TPB + threadIdx.x;
    if (env >= P.n) return;
    kin::crba(P.tab, P.cols, P.comp, env, (size_t)P.n, P.stage);
}

// out[env][k] = stage[k][env] for k in [0, K), or 0 where the table says the entry is never written.  Block (x, y): envs 64 x .. + 63,
// elements 64 y .. + 63.  dofs: the DoFs whose Jacobian columns were written (MASS = false).
template <bool MASS>
__global__ __launch_bounds__(KQ_TPB) void k_kin_rows(const float* __restrict__ tab, const float* __restrict__ stage, float* __restrict__ out, int K, int n, int nd,
                                                     unsigned long long dofs) {
    __shared__ float tile[KQ_TILE * KQ_LD];
    const int lane = threadIdx.x, env0 = blockIdx.x * KQ_TILE, k0 = blockIdx.y * KQ_TILE, env = env0 + lane;
    const int kn = min(KQ_TILE, K - k0), en = min(KQ_TILE, n - env0);
    const size_t N = (size_t)n;
#pragma unroll 8
    for (int kk = 0; kk < kn; kk++) {            // (unrolled: eight independent loads in flight instead of one)
        const int k = k0 + kk;
        const bool nz = MASS ? kin::mass_entry(tab, k) : (bool)((dofs >> (k % nd)) & 1ull);      // (the same in every lane)
        float v = 0.0f;
        if (nz && lane < en) v = stage[(size_t)k * N + env];
        tile[kk * KQ_LD + lane] = v;
    }
    __syncthreads();
    if (lane < kn) {
        float* o = out + (size_t)env0 * K + k0 + lane;
#pragma unroll 8
        for (int e = 0; e < en; e++) o[(size_t)e * K] = tile[lane * KQ_LD + e];
    }
}

}  // namespace pbre

using namespace pbre;

// (the ctx: pbre_engine.hpp -- state_view, fail (pbre_capi.hip) and its record pbre_ctx::readers (pbre_scene.hpp: the RobotTable copy, KinBufs))

static int check_query(pbre_ctx* ctx, const pbre_kin_query_t* q) {
    if (!ctx) return fail(nullptr, PBRE_E_ARG, "pbre_kin_query: null ctx");
    if (!q) return fail(ctx, PBRE_E_ARG, "pbre_kin_query: null query struct");
    for (int k = 0; k < 3; k++) if (std::isnan(q->jac_point[k])) return fail(ctx, PBRE_E_ARG, "pbre_kin_query: jac_point is NaN");
    if (q->n_links < 0 || (q->n_links > 0 && !q->links)) return fail(ctx, PBRE_E_ARG, "pbre_kin_query: n_links links asked for but links is null (or n_links < 0)");
    return PBRE_OK;
}
static bool nothing_asked(const pbre_kin_query_t* q) { return !q->pose && !q->vel && !q->jac && !q->mass && !q->tau; }

// the checks that need the table; fills the link list and the Jacobian's link
static int check_table(pbre_ctx* ctx, const pbre_kin_query_t& q, int stride, KqParams& P) {
    const Readers& s = ctx->readers;
    if (s.table.empty()) return fail(ctx, PBRE_E_TABLE, "pbre_kin_query: the ctx has no RobotTable");
    const double* t = s.table.data();
    const int nl = s.nl, nd = s.ndof;
    if (t[18] == 0.0) return fail(ctx, PBRE_E_UNSUPPORTED, "pbre_kin_query: a RobotTable with fixed_base = 0 (a free-floating base) is not supported");
    if (nl > kin::MAX_LINKS || nd > kin::MAX_DOF || nd < 0) return fail(ctx, PBRE_E_UNSUPPORTED, "pbre_kin_query: more than 128 links or 64 DoF");
    if (q.n_links > nl) return fail(ctx, PBRE_E_ARG, "pbre_kin_query: n_links is above the table's link count");
    for (int j = 0; j < q.n_links; j++) {
        if (q.links[j] < 0 || q.links[j] >= nl) return fail(ctx, PBRE_E_ARG, "pbre_kin_query: a link index is outside the table");
        P.links[j] = (unsigned char)q.links[j];
    }
    P.jac_link = q.jac_link == -1 ? (int)t[4] : q.jac_link;
    if (P.jac_link < 0 || P.jac_link >= nl) return fail(ctx, PBRE_E_ARG, "pbre_kin_query: jac_link is outside the table");
    const int W = (stride - 16) / 2;
    for (int i = 0; i < nl; i++) {           // what the walks index with: parents before children, joint values inside a record's lanes
        const double* r = t + 24 + i * 40;
        if (!(r[0] < (double)i) || !(r[0] >= -1.0) || (r[1] != 0.0 && !(r[33] >= 0.0 && r[33] < (double)std::min(nd, W))) || r[1] < 0.0 || r[1] > 2.0)
            return fail(ctx, PBRE_E_TABLE, "pbre_kin_query: RobotTable links out of order or a joint index outside the state record");
    }
    return PBRE_OK;
}

// enqueue the kernels on v.stream; the outputs (and qdd) are device pointers (null: skipped)
static int query_on(pbre_ctx* ctx, const StateView& v, const pbre_kin_query_t& q, KqParams& P) {
    hipStream_t st = (hipStream_t)v.stream;
    const Readers& r = ctx->readers;
    KinBufs& s = ctx->readers.kin;
    const int nl = r.nl, nd = r.ndof, n = v.n;
    const bool links = q.n_links > 0 && (q.pose || q.vel), vel = links && q.vel;
    const bool want_jac = q.jac && nd > 0, want_mass = q.mass && nd > 0, want_tau = q.tau && nd > 0;
    if (!links && !want_jac && !want_mass && !want_tau) return PBRE_OK;
    if (!s.table) PBRE_CHK_ON(ctx, upload_once(s.table, kin::kin_table(r.table.data())));      // once per ctx: the RobotTable never changes
    // column buffers of this query: frames | composites | wrenches | staging (jac and mass use it one after the other)
    const size_t N = (size_t)n;
    const size_t f_frames = (size_t)std::max(nl, 1) * kin::KC * N, f_comp = want_mass ? (size_t)nl * kin::KCOMP * N : 0, f_wr = want_tau ? (size_t)nl * kin::KWR * N : 0;
    const size_t f_stage = std::max(want_jac ? (size_t)6 * nd : 0, want_mass ? (size_t)nd * nd : 0) * N;
    // (a query in flight on another stream may still use the old buffer)
    PBRE_CHK_ON(ctx, grow(s.cols, s.cap_cols, f_frames + f_comp + f_wr + f_stage, true));
    P.tab = s.table; P.state = v.state; P.stride = v.stride; P.W = (v.stride - 16) / 2; P.n = n; P.nd = nd;
    P.cols = s.cols; P.comp = P.cols + f_frames; P.wr = P.comp + f_comp; P.stage = P.wr + f_wr;
    P.qdd = q.qdd; P.g_up = (float)(-v.phys.gravity_z);
    P.n_links = q.n_links; P.at_com = q.at_com; P.jac_at_com = q.jac_at_com;
    for (int k = 0; k < 3; k++) P.jac_point[k] = q.jac_point[k];
    P.pose = q.pose; P.vel = q.vel; P.tau = q.tau;
    const dim3 grid((n + KQ_TPB - 1) / KQ_TPB), block(KQ_TPB);
    if (want_tau) hipLaunchKernelGGL((k_kin_fk<true, true>), grid, block, 0, st, P);
    else if (vel) hipLaunchKernelGGL((k_kin_fk<true, false>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((k_kin_fk<false, false>), grid, block, 0, st, P);
    if (links) hipLaunchKernelGGL(k_kin_links, grid, block, 0, st, P);
    if (want_jac) {
        unsigned long long dofs = 0;
        const double* t = r.table.data();
        for (int i = P.jac_link; i >= 0; i = (int)t[24 + i * 40]) if (t[24 + i * 40 + 1] != 0.0) dofs |= 1ull << (int)t[24 + i * 40 + 33];
        hipLaunchKernelGGL(k_kin_jac, grid, block, 0, st, P);
        const int K = 6 * nd;
        hipLaunchKernelGGL((k_kin_rows<false>), dim3((n + KQ_TILE - 1) / KQ_TILE, (K + KQ_TILE - 1) / KQ_TILE), block, 0, st, P.tab, P.stage, q.jac, K, n, nd, dofs);
    }
    if (want_tau) hipLaunchKernelGGL(k_kin_tau, grid, block, 0, st, P);
    if (want_mass) {
        hipLaunchKernelGGL(k_kin_mass, grid, block, 0, st, P);
        const int K = nd * nd;
        hipLaunchKernelGGL((k_kin_rows<true>), dim3((n + KQ_TILE - 1) / KQ_TILE, (K + KQ_TILE - 1) / KQ_TILE), block, 0, st, P.tab, P.stage, q.mass, K, n, nd, 0ull);
    }
    PBRE_CHK_ON(ctx, hipGetLastError());
    return PBRE_OK;
}

extern "C" {

int pbre_kin_query_device(pbre_ctx* ctx, const pbre_kin_query_t* q, void* stream) {
    int rc = check_query(ctx, q);
    if (rc != PBRE_OK) return rc;
    StateView v;
    if ((rc = ctx->state_view(&v, stream, false)) != PBRE_OK) return rc;
    KqParams P;
    std::memset(&P, 0, sizeof P);
    if ((rc = check_table(ctx, *q, v.stride, P)) != PBRE_OK) return rc;
    if (nothing_asked(q)) return PBRE_OK;
    return query_on(ctx, v, *q, P);
}

int pbre_kin_query(pbre_ctx* ctx, const pbre_kin_query_t* q) {
    int rc = check_query(ctx, q);
    if (rc != PBRE_OK) return rc;
    StateView v;
    if ((rc = ctx->state_view(&v, nullptr, true)) != PBRE_OK) return rc;
    KqParams P;
    std::memset(&P, 0, sizeof P);
    if ((rc = check_table(ctx, *q, v.stride, P)) != PBRE_OK) return rc;
    if (nothing_asked(q)) return PBRE_OK;
    const size_t nd = (size_t)ctx->readers.ndof, nlq = (size_t)q->n_links, rec = (size_t)v.n * sizeof(float);
    hipStream_t st = (hipStream_t)v.stream;
    Stage sg;                                    // pose | vel | jac | mass | tau | qdd; what is not asked for takes no space
    auto add = [&](const void* host, size_t floats, bool in) { return sg.add(host, host ? floats * rec : 0, in); };
    const int i_pose = add(q->pose, nlq * 7, false), i_vel = add(q->vel, nlq * 6, false), i_jac = add(q->jac, 6 * nd, false), i_mass = add(q->mass, nd * nd, false),
              i_tau = add(q->tau, nd, false), i_qdd = add(q->tau ? q->qdd : nullptr, nd, true);
    PBRE_CHK_ON(ctx, sg.begin(ctx->readers.kin.out, ctx->readers.kin.cap_out, st));
    pbre_kin_query_t d = *q;
    d.pose = sg.dev<float>(i_pose); d.vel = sg.dev<float>(i_vel); d.jac = sg.dev<float>(i_jac); d.mass = sg.dev<float>(i_mass); d.tau = sg.dev<float>(i_tau);
    d.qdd = sg.dev<float>(i_qdd);
    if ((rc = query_on(ctx, v, d, P)) != PBRE_OK) return rc;
    PBRE_CHK_ON(ctx, sg.finish(st));
    return PBRE_OK;
}

}  // extern "C"
