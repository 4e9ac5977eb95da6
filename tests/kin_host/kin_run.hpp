// The query of csrc/pbre_kin.hip on the host: the same per-env walks (csrc/pbre_kin.hpp) in the same order over column buffers of exactly
// the size the device allocates, then the staging columns turned into env-major records with the zeros the table implies.
#pragma once
#include <cstdint>
#include <vector>
#include "pbre_kin.hpp"

namespace kin_host {
using namespace pbre;

struct Query {
    int n_links = 0; const int32_t* links = nullptr; int at_com = 0, jac_link = 0, jac_at_com = 0;
    float jac_point[3] = {0.0f, 0.0f, 0.0f};
    const float* qdd = nullptr;
    float *pose = nullptr, *vel = nullptr, *jac = nullptr, *mass = nullptr, *tau = nullptr;
};

// table: a RobotTable; state: [n][stride] records with lane width W
inline void run(const double* table, int n, const float* state, int stride, int W, float g_up, const Query& q) {
    const std::vector<float> tab = kin::kin_table(table);
    const int nl = (int)table[2], nd = (int)table[3];
    const size_t N = (size_t)n;
    std::vector<float> cols((size_t)nl * kin::KC * N), comp(q.mass ? (size_t)nl * kin::KCOMP * N : 0), wr(q.tau ? (size_t)nl * kin::KWR * N : 0);
    std::vector<float> stage(((q.mass ? (size_t)nd * nd : 0) > (q.jac ? (size_t)6 * nd : 0) ? (size_t)nd * nd : (q.jac ? (size_t)6 * nd : 0)) * N);
    for (int e = 0; e < n; e++) {
        const float* st = state + (size_t)e * stride;
        const float* dd = q.qdd ? q.qdd + (size_t)e * nd : nullptr;
        if (q.tau) kin::fk<true, true>(tab.data(), st, st + W, dd, g_up, e, N, cols.data());
        else if (q.vel) kin::fk<true, false>(tab.data(), st, st + W, dd, g_up, e, N, cols.data());
        else kin::fk<false, false>(tab.data(), st, st + W, dd, g_up, e, N, cols.data());
    }
    for (int e = 0; e < n; e++) for (int j = 0; j < q.n_links && (q.pose || q.vel); j++) {
        const size_t rec = (size_t)e * q.n_links + j;
        kin::link_out(tab.data(), cols.data(), q.links[j], q.at_com != 0, e, N, q.pose ? q.pose + rec * 7 : nullptr, q.vel ? q.vel + rec * 6 : nullptr);
    }
    if (q.jac) {
        uint64_t dofs = 0;
        for (int i = q.jac_link; i >= 0; i = (int)table[24 + i * 40]) if (table[24 + i * 40 + 1] != 0.0) dofs |= 1ull << (int)table[24 + i * 40 + 33];
        for (int e = 0; e < n; e++) kin::jac(tab.data(), cols.data(), q.jac_link, q.jac_point, q.jac_at_com != 0, e, N, stage.data());
        const int K = 6 * nd;
        for (int e = 0; e < n; e++) for (int k = 0; k < K; k++) q.jac[(size_t)e * K + k] = ((dofs >> (k % nd)) & 1) ? stage[(size_t)k * N + e] : 0.0f;
    }
    if (q.tau) for (int e = 0; e < n; e++) kin::rnea(tab.data(), cols.data(), wr.data(), e, N, q.tau + (size_t)e * nd);
    if (q.mass) {
        for (int e = 0; e < n; e++) kin::crba(tab.data(), cols.data(), comp.data(), e, N, stage.data());
        const int K = nd * nd;
        for (int e = 0; e < n; e++) for (int k = 0; k < K; k++) q.mass[(size_t)e * K + k] = kin::mass_entry(tab.data(), k) ? stage[(size_t)k * N + e] : 0.0f;
    }
}

}  // namespace kin_host
