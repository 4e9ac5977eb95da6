// pbre_kin.hpp -- the per-env walks of the kinematics / dynamics query (include/pbre_kin.h): forward kinematics with link velocities and
// accelerations, the pose and velocity of a link, the Jacobian of a point, inverse dynamics (RNEA) and the joint-space inertia matrix
// (composite rigid bodies).  PBRE_HD as in pbre_math.hpp: the same header compiles for the device (pbre_kin.hip) and for the host
// (tests/kin_host).  One env per thread, fp32, no fast-math, contraction off: host and device agree.
//
// Nothing here keeps a per-thread array that is indexed at run time.  Per-link quantities travel through column buffers, one column per
// env (element k of link i at [(i KC + k) N + env]: consecutive threads on consecutive addresses), as in pbre_scene.hpp: scene_fk.  The
// link table is read at addresses that are the same for every thread.
//
// Formulas (world frame; link i with parent p, joint axis a_i = R_i axis_i, r = p_i - p_p, base at rest accelerated by (0, 0, g_up)):
//   revolute   w_i = w_p + a_i qd          v_i = v_p + w_p x r
//              al_i = al_p + a_i qdd + (w_p x a_i) qd          acc_i = acc_p + al_p x r + w_p x (w_p x r)
//   prismatic  w_i = w_p, al_i = al_p      v_i = v_p + w_p x r + a_i qd        acc_i = ... + a_i qdd + 2 (w_p x a_i) qd
// v and acc are those of the link frame's origin.  RNEA: f = m acc_com, n = Ic al + w x Ic w about the centre of mass, moved to the link's
// own origin, summed over the subtree through the column buffer (levers are link offsets), tau = a . n (revolute) or a . f (prismatic).
// M: composite inertias (mass, first moment, inertia tensor) about each link's OWN origin, handed to the parent's origin by the parallel-axis
// terms of the link offset -- never about the world origin: the finger joints of the hands model have M_jj ~ 1e-3 where m |c|^2 about the
// world origin is of order 1, and fp32 would lose them.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include "pbre_math.hpp"
#include <vector>
PBRE_FP_CONTRACT_OFF

namespace pbre {
namespace kin {

// device table: [0] n_links [1] n_dof [2..4] base position [5..13] base rotation; KT_LINK floats per link; then 2 words per DoF: the DoFs
// on one path to the root with it (the non-zero pattern of a row of M)
constexpr int KT_HDR = 16, KT_LINK = 36;
// per link: 0 parent 1 joint type 2..4 axis 5..7 origin 8..16 origin rotation 17 DoF 18 mass 19..21 centre of mass 22..30 inertia about it
// (link axes, symmetrised) 31: 1 = the first link, in descending order, that hands something to its parent (it stores, the others add)
// 32: 1 = has children
constexpr int KC = 27;          // frame columns per link: 0..8 R  9..11 p  12..14 a  15..17 w  18..20 v  21..23 al  24..26 acc
constexpr int KCOMP = 10;       // composite columns: mass, first moment[3], inertia xx xy xz yy yz zz
constexpr int KWR = 6;          // wrench columns: force[3], moment about the link's origin[3]
constexpr int MAX_LINKS = 128, MAX_DOF = 64;

// the device table from a RobotTable (include/pbre.h)
inline std::vector<float> kin_table(const double* t) {
    const int nl = (int)t[2], nd = (int)t[3];
    std::vector<float> out(KT_HDR + (size_t)KT_LINK * nl + 2 * (size_t)nd, 0.0f);
    out[0] = (float)nl; out[1] = (float)nd;
    for (int k = 0; k < 3; k++) out[2 + k] = (float)t[6 + k];
    for (int k = 0; k < 9; k++) out[5 + k] = (float)t[9 + k];
    std::vector<int> seen(nl > 0 ? nl : 1, 0);
    for (int i = nl - 1; i >= 0; i--) {
        const double* r = t + 24 + i * 40;
        float* L = out.data() + KT_HDR + KT_LINK * i;
        L[0] = (float)r[0]; L[1] = (float)r[1];
        for (int k = 0; k < 3; k++) { L[2 + k] = (float)r[2 + k]; L[5 + k] = (float)r[5 + k]; L[19 + k] = (float)r[18 + k]; }
        for (int k = 0; k < 9; k++) L[8 + k] = (float)r[8 + k];
        L[17] = (float)r[33]; L[18] = (float)r[17];
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) L[22 + 3 * a + b] = (float)(0.5 * (r[21 + 3 * a + b] + r[21 + 3 * b + a]));
        const int par = (int)r[0];
        L[32] = seen[i] ? 1.0f : 0.0f;
        if (par >= 0 && par < nl) { L[31] = seen[par] ? 0.0f : 1.0f; seen[par] = 1; }
    }
    uint32_t* rel = reinterpret_cast<uint32_t*>(out.data() + KT_HDR + (size_t)KT_LINK * nl);
    for (int i = 0; i < nl; i++) {
        const double* r = t + 24 + i * 40;
        const int di = (int)r[33];
        if ((int)r[1] == 0 || di < 0 || di >= nd) continue;
        for (int j = i, guard = 0; j >= 0 && j < nl && guard <= nl; j = (int)t[24 + j * 40], guard++) {
            const int dj = (int)t[24 + j * 40 + 33];
            if ((int)t[24 + j * 40 + 1] == 0 || dj < 0 || dj >= nd) continue;
            rel[2 * di + (dj >> 5)] |= 1u << (dj & 31);
            rel[2 * dj + (di >> 5)] |= 1u << (di & 31);
        }
    }
    return out;
}

static PBRE_HD void cross3(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
static PBRE_HD float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static PBRE_HD void mat_v(const float* R, const float* v, float* o) {           // R v
    for (int r = 0; r < 3; r++) o[r] = R[3 * r] * v[0] + R[3 * r + 1] * v[1] + R[3 * r + 2] * v[2];
}
static PBRE_HD void matT_v(const float* R, const float* v, float* o) {          // R^T v
    for (int c = 0; c < 3; c++) o[c] = R[c] * v[0] + R[3 + c] * v[1] + R[6 + c] * v[2];
}
static PBRE_HD void load3(const float* C, size_t N, float* o) { o[0] = C[0]; o[1] = C[N]; o[2] = C[2 * N]; }
static PBRE_HD void store3(float* C, size_t N, const float* v) { C[0] = v[0]; C[N] = v[1]; C[2 * N] = v[2]; }
// R Ic R^T v: the link's inertia about its centre of mass (link axes) applied to a world vector
static PBRE_HD void inertia_v(const float* R, const float* Ic, const float* v, float* o) {
    float l[3], m[3];
    matT_v(R, v, l); mat_v(Ic, l, m); mat_v(R, m, o);
}

// Forward pass of one env.  q, qd: the Q and V lanes of its state record; qdd: its nd accelerations or null (zeros).  VEL: also w, v.
// ACC: also al, acc (needs VEL).  g_up: the base's acceleration along z (-gravity_z).
template <bool VEL, bool ACC>
static PBRE_HD void fk(const float* __restrict__ tab, const float* __restrict__ q, const float* __restrict__ qd, const float* __restrict__ qdd,
                       float g_up, int env, size_t N, float* __restrict__ cols) {
    const int nl = (int)tab[0];
#pragma unroll 1
    for (int i = 0; i < nl; i++) {
        const float* L = tab + KT_HDR + KT_LINK * i;
        const int par = (int)L[0], jt = (int)L[1], dof = (int)L[17];
        float Rp[9], pp[3], wp[3] = {0.0f, 0.0f, 0.0f}, vp[3] = {0.0f, 0.0f, 0.0f}, alp[3] = {0.0f, 0.0f, 0.0f}, accp[3] = {0.0f, 0.0f, g_up};
        if (par >= 0) {
            const float* F = cols + (size_t)par * KC * N + env;
            for (int k = 0; k < 9; k++) Rp[k] = F[k * N];
            load3(F + 9 * N, N, pp);
            if (VEL) { load3(F + 15 * N, N, wp); load3(F + 18 * N, N, vp); }
            if (ACC) { load3(F + 21 * N, N, alp); load3(F + 24 * N, N, accp); }
        } else {
            for (int k = 0; k < 9; k++) Rp[k] = tab[5 + k];
            for (int k = 0; k < 3; k++) pp[k] = tab[2 + k];
        }
        float Rl[9], pl[3] = {L[5], L[6], L[7]};
        const float ax[3] = {L[2], L[3], L[4]};
        for (int k = 0; k < 9; k++) Rl[k] = L[8 + k];
        float a0[3];                         // the axis in the parent's frame: R0 axis (the joint's own rotation leaves it where it is)
        mat_v(Rl, ax, a0);
        if (jt == 1) {                       // revolute: R0 (I + s K + (1 - c) K^2)
            const float qi = q[dof], s = sinf(qi), c1 = 1.0f - cosf(qi);
            const float A[9] = {1.0f - c1 * (ax[1] * ax[1] + ax[2] * ax[2]), -s * ax[2] + c1 * ax[0] * ax[1], s * ax[1] + c1 * ax[0] * ax[2],
                                s * ax[2] + c1 * ax[0] * ax[1], 1.0f - c1 * (ax[0] * ax[0] + ax[2] * ax[2]), -s * ax[0] + c1 * ax[1] * ax[2],
                                -s * ax[1] + c1 * ax[0] * ax[2], s * ax[0] + c1 * ax[1] * ax[2], 1.0f - c1 * (ax[0] * ax[0] + ax[1] * ax[1])};
            float M[9];
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) M[3 * r + c] = Rl[3 * r] * A[c] + Rl[3 * r + 1] * A[3 + c] + Rl[3 * r + 2] * A[6 + c];
            for (int k = 0; k < 9; k++) Rl[k] = M[k];
        } else if (jt == 2) {                // prismatic: xyz + (R0 axis) q
            const float qi = q[dof];
            for (int r = 0; r < 3; r++) pl[r] += a0[r] * qi;
        }
        float Rw[9], r[3], pw[3], a[3];
        for (int rr = 0; rr < 3; rr++) for (int c = 0; c < 3; c++) Rw[3 * rr + c] = Rp[3 * rr] * Rl[c] + Rp[3 * rr + 1] * Rl[3 + c] + Rp[3 * rr + 2] * Rl[6 + c];
        mat_v(Rp, pl, r);
        mat_v(Rp, a0, a);
        for (int k = 0; k < 3; k++) pw[k] = pp[k] + r[k];
        float* F = cols + (size_t)i * KC * N + env;
        for (int k = 0; k < 9; k++) F[k * N] = Rw[k];
        store3(F + 9 * N, N, pw);
        store3(F + 12 * N, N, a);
        if (VEL) {
            const float qdi = jt != 0 ? qd[dof] : 0.0f;
            const float qddi = (ACC && jt != 0 && qdd) ? qdd[dof] : 0.0f;
            float w[3], v[3], wr[3], wa[3];
            cross3(wp, r, wr);
            cross3(wp, a, wa);
            for (int k = 0; k < 3; k++) {
                w[k] = wp[k] + (jt == 1 ? a[k] * qdi : 0.0f);
                v[k] = vp[k] + wr[k] + (jt == 2 ? a[k] * qdi : 0.0f);
            }
            store3(F + 15 * N, N, w);
            store3(F + 18 * N, N, v);
            if (ACC) {
                float al[3], acc[3], ar[3], wwr[3];
                cross3(alp, r, ar);
                cross3(wp, wr, wwr);
                for (int k = 0; k < 3; k++) {
                    al[k] = alp[k] + (jt == 1 ? a[k] * qddi + wa[k] * qdi : 0.0f);
                    acc[k] = accp[k] + ar[k] + wwr[k] + (jt == 2 ? a[k] * qddi + 2.0f * wa[k] * qdi : 0.0f);
                }
                store3(F + 21 * N, N, al);
                store3(F + 24 * N, N, acc);
            }
        }
    }
}

// rotation (row major) -> quaternion x, y, z, w with w >= 0: the branch on the largest of the trace and the diagonal terms (Shepperd)
static PBRE_HD void quat_of(const float* R, float* o) {
    const float tr = R[0] + R[4] + R[8];
    float x, y, z, w;
    if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
        const float s = 2.0f * sqrtf(1.0f + tr);
        w = 0.25f * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s;
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        const float s = 2.0f * sqrtf(1.0f + R[0] - R[4] - R[8]);
        w = (R[7] - R[5]) / s; x = 0.25f * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s;
    } else if (R[4] >= R[8]) {
        const float s = 2.0f * sqrtf(1.0f + R[4] - R[0] - R[8]);
        w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25f * s; z = (R[5] + R[7]) / s;
    } else {
        const float s = 2.0f * sqrtf(1.0f + R[8] - R[0] - R[4]);
        w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25f * s;
    }
    const float sg = w < 0.0f ? -1.0f : 1.0f;
    o[0] = sg * x; o[1] = sg * y; o[2] = sg * z; o[3] = sg * w;
}

// pose[7] / vel[6] of one link of one env (either may be null); at_com: the centre of mass instead of the frame's origin
static PBRE_HD void link_out(const float* __restrict__ tab, const float* __restrict__ cols, int link, bool at_com, int env, size_t N,
                             float* __restrict__ pose, float* __restrict__ vel) {
    const float* L = tab + KT_HDR + KT_LINK * link;
    const float* F = cols + (size_t)link * KC * N + env;
    float R[9], p[3], c[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 9; k++) R[k] = F[k * N];
    load3(F + 9 * N, N, p);
    if (at_com) { const float cl[3] = {L[19], L[20], L[21]}; mat_v(R, cl, c); }
    if (pose) {
        float qt[4];
        quat_of(R, qt);
        for (int k = 0; k < 3; k++) pose[k] = p[k] + c[k];
        for (int k = 0; k < 4; k++) pose[3 + k] = qt[k];
    }
    if (vel) {
        float w[3], v[3], wc[3];
        load3(F + 15 * N, N, w); load3(F + 18 * N, N, v);
        cross3(w, c, wc);
        for (int k = 0; k < 3; k++) { vel[k] = v[k] + wc[k]; vel[3 + k] = w[k]; }
    }
}

// The non-zero columns of the Jacobian of the point `pt` (link frame; at_com: the centre of mass) of link jl, into stage[(r nd + dof) N +
// env]: the walk from jl to the root.  The columns of the other DoFs are not written.
static PBRE_HD void jac(const float* __restrict__ tab, const float* __restrict__ cols, int jl, const float* pt, bool at_com, int env, size_t N,
                        float* __restrict__ stage) {
    const int nd = (int)tab[1];
    float x[3];
    {
        const float* L = tab + KT_HDR + KT_LINK * jl;
        const float* F = cols + (size_t)jl * KC * N + env;
        float R[9], p[3], c[3];
        for (int k = 0; k < 9; k++) R[k] = F[k * N];
        load3(F + 9 * N, N, p);
        const float cl[3] = {at_com ? L[19] : pt[0], at_com ? L[20] : pt[1], at_com ? L[21] : pt[2]};
        mat_v(R, cl, c);
        for (int k = 0; k < 3; k++) x[k] = p[k] + c[k];
    }
#pragma unroll 1
    for (int i = jl; i >= 0;) {
        const float* L = tab + KT_HDR + KT_LINK * i;
        const int jt = (int)L[1], dof = (int)L[17];
        if (jt != 0) {
            const float* F = cols + (size_t)i * KC * N + env;
            float a[3], p[3], lin[3];
            load3(F + 12 * N, N, a);
            if (jt == 1) {
                load3(F + 9 * N, N, p);
                const float d[3] = {x[0] - p[0], x[1] - p[1], x[2] - p[2]};
                cross3(a, d, lin);
            } else { lin[0] = a[0]; lin[1] = a[1]; lin[2] = a[2]; }
            float* S = stage + (size_t)dof * N + env;
            for (int k = 0; k < 3; k++) {
                S[(size_t)k * nd * N] = lin[k];
                S[(size_t)(3 + k) * nd * N] = jt == 1 ? a[k] : 0.0f;
            }
        }
        i = (int)L[0];
    }
}

// RNEA's backward pass of one env from the columns of fk<true, true>: tau[nd].  wr: wrench columns [n_links][KWR][N].
static PBRE_HD void rnea(const float* __restrict__ tab, const float* __restrict__ cols, float* __restrict__ wr, int env, size_t N, float* __restrict__ tau) {
    const int nl = (int)tab[0];
#pragma unroll 1
    for (int i = nl - 1; i >= 0; i--) {
        const float* L = tab + KT_HDR + KT_LINK * i;
        const int par = (int)L[0], jt = (int)L[1], dof = (int)L[17];
        const float* F = cols + (size_t)i * KC * N + env;
        float R[9], p[3], a[3], w[3], al[3], acc[3];
        for (int k = 0; k < 9; k++) R[k] = F[k * N];
        load3(F + 9 * N, N, p); load3(F + 12 * N, N, a); load3(F + 15 * N, N, w); load3(F + 21 * N, N, al); load3(F + 24 * N, N, acc);
        const float m = L[18], cl[3] = {L[19], L[20], L[21]};
        float Ic[9];
        for (int k = 0; k < 9; k++) Ic[k] = L[22 + k];
        float c[3], alc[3], wc[3], wwc[3], f[3], Ial[3], Iw[3], wIw[3], cf[3], n[3];
        mat_v(R, cl, c);
        cross3(al, c, alc); cross3(w, c, wc); cross3(w, wc, wwc);
        for (int k = 0; k < 3; k++) f[k] = m * (acc[k] + alc[k] + wwc[k]);
        inertia_v(R, Ic, al, Ial); inertia_v(R, Ic, w, Iw);
        cross3(w, Iw, wIw); cross3(c, f, cf);
        for (int k = 0; k < 3; k++) n[k] = Ial[k] + wIw[k] + cf[k];
        float* Wi = wr + (size_t)i * KWR * N + env;
        if (L[32] != 0.0f) for (int k = 0; k < 3; k++) { f[k] += Wi[k * N]; n[k] += Wi[(3 + k) * N]; }
        if (jt != 0) tau[dof] = jt == 1 ? dot3(a, n) : dot3(a, f);
        if (par >= 0) {
            float pp[3], rf[3];
            load3(cols + ((size_t)par * KC + 9) * N + env, N, pp);
            const float r[3] = {p[0] - pp[0], p[1] - pp[1], p[2] - pp[2]};
            cross3(r, f, rf);
            float* Wp = wr + (size_t)par * KWR * N + env;
            const bool first = L[31] != 0.0f;
            for (int k = 0; k < 3; k++) {
                Wp[k * N] = first ? f[k] : Wp[k * N] + f[k];
                Wp[(3 + k) * N] = first ? n[k] + rf[k] : Wp[(3 + k) * N] + (n[k] + rf[k]);
            }
        }
    }
}

// M(q) of one env by composite rigid bodies, the entries of DoF pairs on one path to the root into stage[(i nd + j) N + env] (both
// triangles); the other entries are zero and are not written.  comp: composite columns [n_links][KCOMP][N].
static PBRE_HD void crba(const float* __restrict__ tab, const float* __restrict__ cols, float* __restrict__ comp, int env, size_t N, float* __restrict__ stage) {
    const int nl = (int)tab[0], nd = (int)tab[1];
#pragma unroll 1
    for (int i = nl - 1; i >= 0; i--) {
        const float* L = tab + KT_HDR + KT_LINK * i;
        const int par = (int)L[0], jt = (int)L[1], dof = (int)L[17];
        const float* F = cols + (size_t)i * KC * N + env;
        float R[9], p[3];
        for (int k = 0; k < 9; k++) R[k] = F[k * N];
        load3(F + 9 * N, N, p);
        float m = L[18];
        const float cl[3] = {L[19], L[20], L[21]};
        float Ic[9], c[3], h[3];
        for (int k = 0; k < 9; k++) Ic[k] = L[22 + k];
        mat_v(R, cl, c);
        // the link's own inertia about its origin, world axes: R Ic R^T + m (|c|^2 1 - c c^T); xx xy xz yy yz zz
        float T[9], I[6];
        for (int r = 0; r < 3; r++) for (int cc = 0; cc < 3; cc++) T[3 * r + cc] = R[3 * r] * Ic[cc] + R[3 * r + 1] * Ic[3 + cc] + R[3 * r + 2] * Ic[6 + cc];
        const float c2 = dot3(c, c);
        I[0] = T[0] * R[0] + T[1] * R[1] + T[2] * R[2] + m * (c2 - c[0] * c[0]);
        I[1] = T[0] * R[3] + T[1] * R[4] + T[2] * R[5] - m * c[0] * c[1];
        I[2] = T[0] * R[6] + T[1] * R[7] + T[2] * R[8] - m * c[0] * c[2];
        I[3] = T[3] * R[3] + T[4] * R[4] + T[5] * R[5] + m * (c2 - c[1] * c[1]);
        I[4] = T[3] * R[6] + T[4] * R[7] + T[5] * R[8] - m * c[1] * c[2];
        I[5] = T[6] * R[6] + T[7] * R[7] + T[8] * R[8] + m * (c2 - c[2] * c[2]);
        for (int k = 0; k < 3; k++) h[k] = m * c[k];
        float* Ci = comp + (size_t)i * KCOMP * N + env;
        if (L[32] != 0.0f) {
            m += Ci[0];
            for (int k = 0; k < 3; k++) h[k] += Ci[(1 + k) * N];
            for (int k = 0; k < 6; k++) I[k] += Ci[(4 + k) * N];
        }
        if (jt != 0) {
            // the composite's momentum under a unit velocity of joint i: linear l, angular n about p_i
            float a[3], l[3], n[3];
            load3(F + 12 * N, N, a);
            if (jt == 1) {
                cross3(a, h, l);
                n[0] = I[0] * a[0] + I[1] * a[1] + I[2] * a[2];
                n[1] = I[1] * a[0] + I[3] * a[1] + I[4] * a[2];
                n[2] = I[2] * a[0] + I[4] * a[1] + I[5] * a[2];
            } else {
                for (int k = 0; k < 3; k++) l[k] = m * a[k];
                cross3(h, a, n);
            }
            stage[((size_t)dof * nd + dof) * N + env] = jt == 1 ? dot3(a, n) : dot3(a, l);
#pragma unroll 1
            for (int j = par; j >= 0;) {
                const float* Lj = tab + KT_HDR + KT_LINK * j;
                const int jtj = (int)Lj[1], dj = (int)Lj[17];
                if (jtj != 0) {
                    const float* Fj = cols + (size_t)j * KC * N + env;
                    float aj[3], v;
                    load3(Fj + 12 * N, N, aj);
                    if (jtj == 1) {
                        float pj[3], rl[3];
                        load3(Fj + 9 * N, N, pj);
                        const float r[3] = {p[0] - pj[0], p[1] - pj[1], p[2] - pj[2]};
                        cross3(r, l, rl);
                        v = aj[0] * (n[0] + rl[0]) + aj[1] * (n[1] + rl[1]) + aj[2] * (n[2] + rl[2]);
                    } else v = dot3(aj, l);
                    stage[((size_t)dof * nd + dj) * N + env] = v;
                    stage[((size_t)dj * nd + dof) * N + env] = v;
                }
                j = (int)Lj[0];
            }
        }
        if (par >= 0) {
            // about the parent's origin: x' = x + r, r = p_i - p_p
            float pp[3];
            load3(cols + ((size_t)par * KC + 9) * N + env, N, pp);
            const float r[3] = {p[0] - pp[0], p[1] - pp[1], p[2] - pp[2]};
            const float hr = dot3(h, r), r2 = dot3(r, r);
            float J[6];
            J[0] = I[0] + 2.0f * hr - 2.0f * h[0] * r[0] + m * (r2 - r[0] * r[0]);
            J[1] = I[1] - (h[0] * r[1] + r[0] * h[1]) - m * r[0] * r[1];
            J[2] = I[2] - (h[0] * r[2] + r[0] * h[2]) - m * r[0] * r[2];
            J[3] = I[3] + 2.0f * hr - 2.0f * h[1] * r[1] + m * (r2 - r[1] * r[1]);
            J[4] = I[4] - (h[1] * r[2] + r[1] * h[2]) - m * r[1] * r[2];
            J[5] = I[5] + 2.0f * hr - 2.0f * h[2] * r[2] + m * (r2 - r[2] * r[2]);
            float* Cp = comp + (size_t)par * KCOMP * N + env;
            const bool first = L[31] != 0.0f;
            Cp[0] = first ? m : Cp[0] + m;
            for (int k = 0; k < 3; k++) { const float v = h[k] + m * r[k]; Cp[(1 + k) * N] = first ? v : Cp[(1 + k) * N] + v; }
            for (int k = 0; k < 6; k++) Cp[(4 + k) * N] = first ? J[k] : Cp[(4 + k) * N] + J[k];
        }
    }
}

// is entry k of a row-major [nd][nd] matrix one that crba writes?  (the words behind the links of the table)
static PBRE_HD bool mass_entry(const float* tab, int k) {
    const int nl = (int)tab[0], nd = (int)tab[1];
    const int i = k / nd, j = k - i * nd;
    uint32_t w;
    memcpy(&w, tab + KT_HDR + (size_t)KT_LINK * nl + 2 * i + (j >> 5), 4);
    return (w >> (j & 31)) & 1u;
}

}  // namespace kin
}  // namespace pbre
