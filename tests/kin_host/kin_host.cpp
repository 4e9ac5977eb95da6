// The per-env walks of csrc/pbre_kin.hpp behind a C interface: one call answers a whole query for an array of state records
// (tests/test_kin_host.py), through kin_run.hpp.
#include "kin_run.hpp"

extern "C" {

// outputs as in include/pbre_kin.h (null: skipped); jac_link must be a link index
void kin_query(const double* table, int n, const float* state, int stride, int W, float g_up, int n_links, const int32_t* links, int at_com,
               int jac_link, const float* jac_point, int jac_at_com, const float* qdd, float* pose, float* vel, float* jac, float* mass, float* tau) {
    kin_host::Query q;
    q.n_links = n_links; q.links = links; q.at_com = at_com; q.jac_link = jac_link; q.jac_at_com = jac_at_com;
    for (int k = 0; k < 3; k++) q.jac_point[k] = jac_point[k];
    q.qdd = qdd; q.pose = pose; q.vel = vel; q.jac = jac; q.mass = mass; q.tau = tau;
    kin_host::run(table, n, state, stride, W, g_up, q);
}
void kin_quat(int n, const float* R, float* out) {
    for (int i = 0; i < n; i++) pbre::kin::quat_of(R + 9 * i, out + 4 * i);
}

}
