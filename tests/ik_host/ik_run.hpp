// One inverse-kinematics query for an array of envs with the per-env solve of csrc/pbre_ik.hpp, as the device runs it: the chain resolved
// once, the float table of ik_table, a working block of exactly the device's size ([7 per moving DoF][64 lanes]; env e uses column e % 64),
// each env on its own.  Shared by ik_host.cpp (the library tests/test_ik_host.py loads) and ik_san.cpp (the sanitizer run).
#pragma once
#include <cstdint>
#include <vector>
#include "pbre_ik.hpp"

namespace ik_host {

struct Query {
    int link = 0;
    float point[3] = {0.0f, 0.0f, 0.0f};
    const float* target_pos = nullptr; const float* target_quat = nullptr; const float* q_start = nullptr;   // q_start: [n][nd], required here
    const uint8_t* dof_mask = nullptr;
    float damping = 0.1f, residual = 1e-3f, rot_residual = 0.0f;
    int max_iters = 100, clamp = 0;
    float* q = nullptr; float* err = nullptr; int32_t* iters = nullptr;
};

// returns resolve_chain's code (0: solved)
inline int run(const double* table, int n, const Query& Q) {
    using namespace pbre::ik;
    Chain ch;
    const int rc = resolve_chain(table, Q.link, Q.dof_mask, ch);
    if (rc != 0) return rc;
    const std::vector<float> tab = ik_table(table);
    const int nd = (int)table[3];
    std::vector<float> block((size_t)ch.nm * IK_SLOT * IK_LANES);      // (empty when nothing moves: no column is touched then)
    const float l2 = (float)((double)Q.damping * (double)Q.damping);
    for (int e = 0; e < n; e++) {
        float Rt[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
        float* col = block.data() + e % IK_LANES;
        const float* qs = Q.q_start + (size_t)e * nd;
        float* qo = Q.q ? Q.q + (size_t)e * nd : nullptr;
        float* eo = Q.err ? Q.err + (size_t)e * 2 : nullptr;
        int32_t* io = Q.iters ? Q.iters + e : nullptr;
        auto own = [](bool active) { return active; };
        if (Q.target_quat) {
            quat_to_R(Q.target_quat + (size_t)e * 4, Rt);
            solve<6>(tab.data(), ch, qs, nd, Q.target_pos + (size_t)e * 3, Rt, Q.point, l2, Q.residual, Q.rot_residual, Q.max_iters, Q.clamp != 0, col, qo, eo, io, own);
        } else {
            solve<3>(tab.data(), ch, qs, nd, Q.target_pos + (size_t)e * 3, Rt, Q.point, l2, Q.residual, Q.rot_residual, Q.max_iters, Q.clamp != 0, col, qo, eo, io, own);
        }
    }
    return 0;
}

}  // namespace ik_host
