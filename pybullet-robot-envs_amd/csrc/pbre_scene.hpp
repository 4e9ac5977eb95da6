// pbre_scene.hpp -- what the units that read an engine's state records without stepping them share: the camera (pbre_camera.hip), the
// contact query (pbre_contacts.hip), the kinematics query (pbre_kin.hip) and the inverse-kinematics query (pbre_ik.hip).  The per-ctx record (pbre_ctx::readers): the one host copy of
// the RobotTable and each unit's own buffers; the float link table the camera and the contact query upload, and the one
// forward-kinematics loop both their kernels run.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "pbre_devwork.hpp"

namespace pbre {

constexpr int CT_HDR = 16, CT_LINK = 20;        // device table: [0] n_links [1] n_prims [2..4] base position [5..13] base rotation; links; primitives / spheres
constexpr int CQ_SPHERE = 8;                    // contact query: a sphere is link | centre[3] | radius | fingertip slot + 1 | 0 | 0

// Each unit keeps buffers of its own, so that queries on different streams cannot race.  A capacity follows the buffer it describes
// (grow, pbre_devwork.hpp); `out` is the block of the host-buffer variant (Stage).
struct CamBufs {
    std::vector<float> visuals;                 // the caller's list (12 floats each); empty: the collision spheres
    int nprims = 0;
    bool dirty = true;                          // the device table is older than the list
    DevBuf<float> table; size_t cap_table = 0;
    DevBuf<float> work; size_t cap_work = 0;    // of one render: link frames | scene | per-env views
    DevBuf<char> out; size_t cap_out = 0;
};
struct CqBufs {
    DevBuf<float> table;                        // links + collision spheres, uploaded once: the RobotTable never changes
    DevBuf<float> frames; size_t cap_frames = 0;
    DevBuf<char> out; size_t cap_out = 0;
};
struct KinBufs {
    DevBuf<float> table;                        // the link table with masses and inertias, uploaded once
    DevBuf<float> cols; size_t cap_cols = 0;    // the column buffers of one query
    DevBuf<char> out; size_t cap_out = 0;
};
struct IkBufs {
    DevBuf<float> table;                        // the link table with joint limits, uploaded once
    DevBuf<char> out; size_t cap_out = 0;
};
struct Readers {
    std::vector<double> table;                  // the RobotTable (include/pbre.h); empty: the ctx was made without a valid one
    int nl = 0, ns = 0, ndof = 0;
    CamBufs cam; CqBufs cq; KinBufs kin; IkBufs ik;
    void set_table(const double* t, size_t len) {
        if (!t || len < 24 || t[0] != 1346523717.0) return;
        const int l = (int)t[2], sp = (int)t[5];
        if (l >= 0 && sp >= 0 && len >= (size_t)(24 + l * 40 + sp * 8)) { table.assign(t, t + 24 + l * 40 + sp * 8); nl = l; ns = sp; ndof = (int)t[3]; }
    }
};

// header and links of the device table (see CT_HDR), from the RobotTable
inline std::vector<float> scene_link_table(const Readers& s) {
    const double* t = s.table.data();
    std::vector<float> out(CT_HDR + (size_t)CT_LINK * s.nl, 0.0f);
    out[0] = (float)s.nl;
    for (int k = 0; k < 3; k++) out[2 + k] = (float)t[6 + k];
    for (int k = 0; k < 9; k++) out[5 + k] = (float)t[9 + k];
    for (int i = 0; i < s.nl; i++) {
        const double* r = t + 24 + i * 40;
        float* L = out.data() + CT_HDR + CT_LINK * i;
        L[0] = (float)r[0]; L[1] = (float)r[1];
        for (int k = 0; k < 3; k++) { L[2 + k] = (float)r[2 + k]; L[5 + k] = (float)r[5 + k]; }
        for (int k = 0; k < 9; k++) L[8 + k] = (float)r[8 + k];
        L[17] = (float)r[33];
    }
    return out;
}

// Forward kinematics of one env (one thread) in fp32, links in table order (parent before child): the frame of link i -- rotation, row
// major, then origin -- goes to frames[(12 i + k) N + env], one column per env (coalesced), so no kernel keeps per-thread frame arrays.
// A link whose parent is the previous link (a chain) takes the parent's frame from registers instead of loading it back.
__device__ __forceinline__ void scene_fk(const float* __restrict__ tab, const float* __restrict__ st, int env, size_t N, float* __restrict__ frames) {
    const int nl = (int)tab[0];
    float Rw[9], pw[3];                      // the previous link's world frame
    for (int k = 0; k < 9; k++) Rw[k] = 0.0f;
    for (int k = 0; k < 3; k++) pw[k] = 0.0f;
#pragma unroll 1
    for (int i = 0; i < nl; i++) {
        const float* L = tab + CT_HDR + CT_LINK * i;
        const int par = (int)L[0], jt = (int)L[1], dof = (int)L[17];
        float Rp[9], pp[3];
        if (par >= 0) {
            if (par == i - 1) {
                for (int k = 0; k < 9; k++) Rp[k] = Rw[k];
                for (int k = 0; k < 3; k++) pp[k] = pw[k];
            } else {
                const float* F = frames + (size_t)par * 12 * N + env;
                for (int k = 0; k < 9; k++) Rp[k] = F[k * N];
                for (int k = 0; k < 3; k++) pp[k] = F[(9 + k) * N];
            }
        } else {
            for (int k = 0; k < 9; k++) Rp[k] = tab[5 + k];
            for (int k = 0; k < 3; k++) pp[k] = tab[2 + k];
        }
        float Rl[9], pl[3] = {L[5], L[6], L[7]};
        for (int k = 0; k < 9; k++) Rl[k] = L[8 + k];
        if (jt == 1) {                       // revolute: R0 (I + s K + (1 - c) K^2)
            const float q = st[dof], s = sinf(q), c1 = 1.0f - cosf(q);
            const float ax = L[2], ay = L[3], az = L[4];
            const float A[9] = {1.0f - c1 * (ay * ay + az * az), -s * az + c1 * ax * ay, s * ay + c1 * ax * az,
                                s * az + c1 * ax * ay, 1.0f - c1 * (ax * ax + az * az), -s * ax + c1 * ay * az,
                                -s * ay + c1 * ax * az, s * ax + c1 * ay * az, 1.0f - c1 * (ax * ax + ay * ay)};
            float M[9];
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) M[3 * r + c] = Rl[3 * r] * A[c] + Rl[3 * r + 1] * A[3 + c] + Rl[3 * r + 2] * A[6 + c];
            for (int k = 0; k < 9; k++) Rl[k] = M[k];
        } else if (jt == 2) {                // prismatic: xyz + (R0 axis) q
            const float q = st[dof];
            for (int r = 0; r < 3; r++) pl[r] += (Rl[3 * r] * L[2] + Rl[3 * r + 1] * L[3] + Rl[3 * r + 2] * L[4]) * q;
        }
        float* F = frames + (size_t)i * 12 * N + env;
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) Rw[3 * r + c] = Rp[3 * r] * Rl[c] + Rp[3 * r + 1] * Rl[3 + c] + Rp[3 * r + 2] * Rl[6 + c];
            pw[r] = pp[r] + Rp[3 * r] * pl[0] + Rp[3 * r + 1] * pl[1] + Rp[3 * r + 2] * pl[2];
        }
        for (int k = 0; k < 9; k++) F[k * N] = Rw[k];
        for (int k = 0; k < 3; k++) F[(9 + k) * N] = pw[k];
    }
}

}  // namespace pbre
