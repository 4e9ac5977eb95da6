// pbre_ik.hpp -- the per-env solve of the inverse-kinematics query (include/pbre_ik.h): damped least squares on the chain from the root to
// one link, the iteration of oracle/pbre_oracle.c: orc_ik.  PBRE_HD as in pbre_math.hpp: the same header compiles for the device
// (pbre_ik.hip) and for the host (tests/ik_host).  One env per thread, fp32, no fast-math, contraction off and fmaf where a fused
// operation is meant: host and device run the same operations.
//
// What an env carries from pass to pass of an iteration lives in its column of a [k][IK_LANES] float block (the device's LDS: consecutive
// lanes on consecutive banks): per DoF that moves, slot s, 7 floats -- the working q at 7 s, the joint's world axis at 7 s + 1 .. 3, its world
// origin at 7 s + 4 .. 6.  The link table and the chain are read at addresses that are the same for every thread.  J J^T + lambda^2 I, its
// Cholesky factor, e and y are locals with compile-time indices only (registers); nothing here indexes a per-thread array at run time.
//
// One iteration: (1) the walk along the chain: frames, the axis and origin of every moving joint, then e and the convergence test;
// (2) the Jacobian columns from the stored axes and origins, A += c c^T; (3) A = L L^T, L L^T y = e; (4) the columns again, q_s += c . y.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>
#include "pbre_math.hpp"
#include "pbre_kin.hpp"
PBRE_FP_CONTRACT_OFF

namespace pbre {
namespace ik {

constexpr int IK_LANES = 64;                        // columns of the working block: the threads of a block
constexpr int IK_SLOT = 7;                          // floats per moving DoF and env
constexpr int MAX_CHAIN = 64, MAX_MOVING = 24;      // (PBRE_IK_MAX_CHAIN, PBRE_IK_MAX_MOVING: 24 x 7 x 64 x 4 B = 43008 B of LDS at most)
// device table: [0] n_links [1] n_dof [2..4] base position [5..13] base rotation; IT_LINK floats per link:
// 0 parent 1 joint type 2..4 axis 5..7 origin 8..16 origin rotation 17 DoF 18 lower 19 upper
constexpr int IT_HDR = 16, IT_LINK = 20;

// the chain of one query, resolved by the host: links from the root to the driven link; per link the slot of its DoF if it moves, else
// -1; per slot its link
struct Chain {
    int n, nm;
    unsigned char link[MAX_CHAIN];
    signed char slot[MAX_CHAIN];
    unsigned char mlink[MAX_MOVING];
};

inline std::vector<float> ik_table(const double* t) {
    const int nl = (int)t[2];
    std::vector<float> out(IT_HDR + (size_t)IT_LINK * nl, 0.0f);
    out[0] = (float)nl; out[1] = (float)t[3];
    for (int k = 0; k < 3; k++) out[2 + k] = (float)t[6 + k];
    for (int k = 0; k < 9; k++) out[5 + k] = (float)t[9 + k];
    for (int i = 0; i < nl; i++) {
        const double* r = t + 24 + i * 40;
        float* L = out.data() + IT_HDR + IT_LINK * i;
        L[0] = (float)r[0]; L[1] = (float)r[1];
        for (int k = 0; k < 3; k++) { L[2 + k] = (float)r[2 + k]; L[5 + k] = (float)r[5 + k]; }
        for (int k = 0; k < 9; k++) L[8 + k] = (float)r[8 + k];
        L[17] = (float)r[33]; L[18] = (float)r[30]; L[19] = (float)r[31];
    }
    return out;
}

// The chain from the root to `link` of a RobotTable whose links are in order (parents first); mask: nd bytes or null.  Returns 0, or 1: more
// than MAX_CHAIN links, 2: more than MAX_MOVING DoFs that move.
inline int resolve_chain(const double* t, int link, const uint8_t* mask, Chain& ch) {
    const int nl = (int)t[2];
    int rev[MAX_CHAIN], n = 0;
    for (int i = link; i >= 0 && i < nl; i = (int)t[24 + i * 40]) {
        if (n == MAX_CHAIN) return 1;
        rev[n++] = i;
    }
    ch.n = n; ch.nm = 0;
    for (int c = 0; c < MAX_CHAIN; c++) { ch.link[c] = 0; ch.slot[c] = -1; }
    for (int s = 0; s < MAX_MOVING; s++) ch.mlink[s] = 0;
    for (int c = 0; c < n; c++) {
        const int i = rev[n - 1 - c];
        const double* r = t + 24 + i * 40;
        ch.link[c] = (unsigned char)i;
        const bool moves = r[1] != 0.0 && r[37] == 0.0 && (!mask || mask[(int)r[33]] != 0);
        if (!moves) continue;
        if (ch.nm == MAX_MOVING) return 2;
        ch.mlink[ch.nm] = (unsigned char)i;
        ch.slot[c] = (signed char)ch.nm++;
    }
    return 0;
}

// rotation (row major) of the quaternion x, y, z, w, which is normalised first
static PBRE_HD void quat_to_R(const float* q, float* R) {
    const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float x = q[0] / n, y = q[1] / n, z = q[2] / n, w = q[3] / n;
    R[0] = 1.0f - 2.0f * (y * y + z * z); R[1] = 2.0f * (x * y - z * w); R[2] = 2.0f * (x * z + y * w);
    R[3] = 2.0f * (x * y + z * w); R[4] = 1.0f - 2.0f * (x * x + z * z); R[5] = 2.0f * (y * z - x * w);
    R[6] = 2.0f * (x * z - y * w); R[7] = 2.0f * (y * z + x * w); R[8] = 1.0f - 2.0f * (x * x + y * y);
}

// Pass 1: the walk along the chain at the working q (a joint that does not move: its start value).  Stores the world axis and origin of
// every moving joint into the env's column; returns the driven point x and the driven link's rotation R.
static PBRE_HD void walk(const float* __restrict__ tab, const Chain& ch, const float* qsrc, const float* point, float* col, float* x, float* R) {
    float pp[3];
    for (int k = 0; k < 9; k++) R[k] = tab[5 + k];
    for (int k = 0; k < 3; k++) pp[k] = tab[2 + k];
#pragma unroll 1
    for (int c = 0; c < ch.n; c++) {
        const float* L = tab + IT_HDR + IT_LINK * (int)ch.link[c];
        const int jt = (int)L[1], s = (int)ch.slot[c];
        float Rl[9], pl[3] = {L[5], L[6], L[7]};
        const float ax[3] = {L[2], L[3], L[4]};
        for (int k = 0; k < 9; k++) Rl[k] = L[8 + k];
        float a0[3];                         // the axis in the parent's frame: R0 axis (the joint's own rotation leaves it where it is)
        kin::mat_v(Rl, ax, a0);
        float qi = 0.0f;
        if (jt != 0) qi = s >= 0 ? col[(IK_SLOT * s) * IK_LANES] : qsrc[(int)L[17]];
        if (jt == 1) {                       // revolute: R0 (I + s K + (1 - c) K^2)
            const float sn = sinf(qi), c1 = 1.0f - cosf(qi);
            const float A[9] = {1.0f - c1 * (ax[1] * ax[1] + ax[2] * ax[2]), -sn * ax[2] + c1 * ax[0] * ax[1], sn * ax[1] + c1 * ax[0] * ax[2],
                                sn * ax[2] + c1 * ax[0] * ax[1], 1.0f - c1 * (ax[0] * ax[0] + ax[2] * ax[2]), -sn * ax[0] + c1 * ax[1] * ax[2],
                                -sn * ax[1] + c1 * ax[0] * ax[2], sn * ax[0] + c1 * ax[1] * ax[2], 1.0f - c1 * (ax[0] * ax[0] + ax[1] * ax[1])};
            float M[9];
            for (int r = 0; r < 3; r++) for (int cc = 0; cc < 3; cc++) M[3 * r + cc] = Rl[3 * r] * A[cc] + Rl[3 * r + 1] * A[3 + cc] + Rl[3 * r + 2] * A[6 + cc];
            for (int k = 0; k < 9; k++) Rl[k] = M[k];
        } else if (jt == 2) {                // prismatic: xyz + (R0 axis) q
            for (int r = 0; r < 3; r++) pl[r] += a0[r] * qi;
        }
        float Rw[9], r[3], a[3];
        for (int rr = 0; rr < 3; rr++) for (int cc = 0; cc < 3; cc++) Rw[3 * rr + cc] = R[3 * rr] * Rl[cc] + R[3 * rr + 1] * Rl[3 + cc] + R[3 * rr + 2] * Rl[6 + cc];
        kin::mat_v(R, pl, r);
        kin::mat_v(R, a0, a);
        for (int k = 0; k < 3; k++) pp[k] = pp[k] + r[k];
        if (s >= 0) {
            float* S = col + (IK_SLOT * s) * IK_LANES;
            for (int k = 0; k < 3; k++) { S[(1 + k) * IK_LANES] = a[k]; S[(4 + k) * IK_LANES] = pp[k]; }
        }
        for (int k = 0; k < 9; k++) R[k] = Rw[k];
    }
    float c[3];
    kin::mat_v(R, point, c);
    for (int k = 0; k < 3; k++) x[k] = pp[k] + c[k];
}

// the Jacobian column of slot s at the point x from the stored axis and origin: linear rows, then (M = 6) angular rows
template <int M>
static PBRE_HD void column(const float* __restrict__ tab, const Chain& ch, const float* col, int s, const float* x, float* c) {
    const bool rev = (int)tab[IT_HDR + IT_LINK * (int)ch.mlink[s] + 1] == 1;
    const float* S = col + (IK_SLOT * s) * IK_LANES;
    const float a[3] = {S[IK_LANES], S[2 * IK_LANES], S[3 * IK_LANES]};
    if (rev) {
        const float d[3] = {x[0] - S[4 * IK_LANES], x[1] - S[5 * IK_LANES], x[2] - S[6 * IK_LANES]};
        kin::cross3(a, d, c);
    } else { c[0] = a[0]; c[1] = a[1]; c[2] = a[2]; }
    if (M == 6) for (int k = 0; k < 3; k++) c[3 + k] = rev ? a[k] : 0.0f;
}

constexpr int tri(int a, int b) { return a * (a + 1) / 2 + b; }      // entry (a, b), b <= a, of a packed lower triangle

// The whole solve of one env.  M = 6: position and orientation (Rt: the target rotation); M = 3: position only.  col: the env's column of
// the working block.  qsrc: its start values [nd] (q_start or the state record).  any(active): true while some env of the group that runs
// in lockstep (the wave; on the host the env itself) is still iterating -- the result of an env does not depend on it.  Outputs may be null.
template <int M, class Any>
static PBRE_HD void solve(const float* __restrict__ tab, const Chain& ch, const float* qsrc, int nd, const float* tp, const float* Rt,
                          const float* point, float l2, float residual, float rot_residual, int max_iters, bool clamp, float* col,
                          float* qout, float* errout, int32_t* itout, Any any) {
#pragma unroll 1
    for (int s = 0; s < ch.nm; s++) col[(IK_SLOT * s) * IK_LANES] = qsrc[(int)tab[IT_HDR + IT_LINK * (int)ch.mlink[s] + 17]];
    bool active = true;
    int it = 0;
    float perr = 0.0f, ang = 0.0f, x[3], e[M];
#pragma unroll 1
    for (;;) {
        if (active) {
            float R[9];
            walk(tab, ch, qsrc, point, col, x, R);
            for (int k = 0; k < 3; k++) e[k] = tp[k] - x[k];
            perr = sqrtf(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
            if (M == 6) {                    // the rotation vector of Rt R^T (orc_ik: the s2 > 1e-9 branch)
                float E[9];
                for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) E[3 * r + c] = Rt[3 * r] * R[3 * c] + Rt[3 * r + 1] * R[3 * c + 1] + Rt[3 * r + 2] * R[3 * c + 2];
                const float sx = E[7] - E[5], sy = E[2] - E[6], sz = E[3] - E[1];
                const float s2 = sqrtf(sx * sx + sy * sy + sz * sz) * 0.5f, c2 = (E[0] + E[4] + E[8] - 1.0f) * 0.5f;
                ang = atan2f(s2, c2);
                const float f = s2 > 1e-9f ? ang / (2.0f * s2) : 0.5f;
                e[M - 3] = f * sx; e[M - 2] = f * sy; e[M - 1] = f * sz;
            }
            const bool conv = perr < residual && (!(rot_residual > 0.0f) || ang < rot_residual);
            if (it >= max_iters || conv) active = false;
        }
        if (!any(active)) break;
        if (active) {
            float A[M * (M + 1) / 2], y[M];
            for (int a = 0; a < M; a++) for (int b = 0; b <= a; b++) A[tri(a, b)] = a == b ? l2 : 0.0f;
#pragma unroll 1
            for (int s = 0; s < ch.nm; s++) {
                float c[M];
                column<M>(tab, ch, col, s, x, c);
                for (int a = 0; a < M; a++) for (int b = 0; b <= a; b++) A[tri(a, b)] = fmaf(c[a], c[b], A[tri(a, b)]);
            }
            for (int a = 0; a < M; a++) for (int b = 0; b <= a; b++) {        // A = L L^T in place
                float sum = A[tri(a, b)];
                for (int k = 0; k < b; k++) sum = fmaf(-A[tri(a, k)], A[tri(b, k)], sum);
                A[tri(a, b)] = a == b ? sqrtf(sum) : sum / A[tri(b, b)];
            }
            for (int a = 0; a < M; a++) {
                float sum = e[a];
                for (int k = 0; k < a; k++) sum = fmaf(-A[tri(a, k)], y[k], sum);
                y[a] = sum / A[tri(a, a)];
            }
            for (int a = M - 1; a >= 0; a--) {
                float sum = y[a];
                for (int k = a + 1; k < M; k++) sum = fmaf(-A[tri(k, a)], y[k], sum);
                y[a] = sum / A[tri(a, a)];
            }
#pragma unroll 1
            for (int s = 0; s < ch.nm; s++) {
                float c[M];
                column<M>(tab, ch, col, s, x, c);
                float dq = 0.0f;
                for (int a = 0; a < M; a++) dq = fmaf(c[a], y[a], dq);
                float qn = col[(IK_SLOT * s) * IK_LANES] + dq;
                if (clamp) {
                    const float* L = tab + IT_HDR + IT_LINK * (int)ch.mlink[s];
                    qn = fminf(fmaxf(qn, L[18]), L[19]);
                }
                col[(IK_SLOT * s) * IK_LANES] = qn;
            }
            it++;
        }
    }
    if (qout) {
#pragma unroll 1
        for (int d = 0; d < nd; d++) qout[d] = qsrc[d];
#pragma unroll 1
        for (int s = 0; s < ch.nm; s++) qout[(int)tab[IT_HDR + IT_LINK * (int)ch.mlink[s] + 17]] = col[(IK_SLOT * s) * IK_LANES];
    }
    if (errout) { errout[0] = perr; errout[1] = M == 6 ? ang : 0.0f; }
    if (itout) *itout = it;
}

}  // namespace ik
}  // namespace pbre
