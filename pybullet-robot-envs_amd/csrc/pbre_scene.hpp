// pbre_scene.hpp -- what the units that read an engine's state records without stepping them share: the camera (pbre_camera.hip) and the
// contact query (pbre_contacts.hip).  The per-ctx record with the one host copy of the RobotTable (pbre_ctx::cam), the float link table
// both upload, and the one forward-kinematics loop both kernels run.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>

namespace pbre {

constexpr int CT_HDR = 16, CT_LINK = 20;        // device table: [0] n_links [1] n_prims [2..4] base position [5..13] base rotation; links; primitives / spheres
constexpr int CQ_SPHERE = 8;                    // contact query: a sphere is link | centre[3] | radius | fingertip slot + 1 | 0 | 0

struct CamState {
    std::vector<double> table;                  // the RobotTable (include/pbre.h)
    int nl = 0, ns = 0, ndof = 0;
    std::vector<float> visuals;                 // the caller's list (12 floats each); empty: the collision spheres
    int nprims = 0;
    bool dirty = true;                          // the device table is older than the list
    int device = -1;
    float *d_table = nullptr, *d_frames = nullptr, *d_scene = nullptr, *d_views = nullptr;
    int cap_n = 0, cap_prims = -1;
    size_t cap_table = 0;
    void* d_img = nullptr; size_t cap_img = 0;  // images of the host-buffer render
    // the contact query's (pbre_contacts.hip): links + collision spheres (uploaded once: the RobotTable never changes), link frames, and
    // the outputs of the host-buffer query
    float *d_cq_table = nullptr, *d_cq_frames = nullptr;
    void* d_cq_out = nullptr;
    int cq_cap_n = 0, cq_cap_out = 0;
    // the kinematics query's (pbre_kin.hip), its own so that a contact query on another stream cannot race with it: the link table with
    // masses and inertias (uploaded once), the column buffers of one query, and the outputs of the host-buffer query
    float *d_kin_table = nullptr, *d_kin_cols = nullptr;
    void* d_kin_out = nullptr;
    size_t kin_cap_cols = 0, kin_cap_out = 0;
};

// header and links of the device table (see CT_HDR), from the RobotTable
inline std::vector<float> scene_link_table(const CamState& s) {
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
