// The per-env solve of csrc/pbre_ik.hpp behind a C interface: one call answers a whole query for an array of start values
// (tests/test_ik_host.py), through ik_run.hpp.
#include "ik_run.hpp"

extern "C" {

// inputs and outputs as in include/pbre_ik.h (null outputs: skipped; target_quat null: position only); link must be a link index, q_start
// is required.  Returns 0, or 1 / 2 when the chain is longer than the on-chip layout holds.
int ik_query(const double* table, int n, const float* q_start, int link, const float* point, const float* target_pos, const float* target_quat,
             const uint8_t* dof_mask, float damping, float residual, float rot_residual, int max_iters, int clamp, float* q, float* err, int32_t* iters) {
    ik_host::Query Q;
    Q.link = link;
    for (int k = 0; k < 3; k++) Q.point[k] = point[k];
    Q.target_pos = target_pos; Q.target_quat = target_quat; Q.q_start = q_start; Q.dof_mask = dof_mask;
    Q.damping = damping; Q.residual = residual; Q.rot_residual = rot_residual; Q.max_iters = max_iters; Q.clamp = clamp;
    Q.q = q; Q.err = err; Q.iters = iters;
    return ik_host::run(table, n, Q);
}

}
