// The reset sequence (csrc/pbre_reset_seq.hpp) run by a recording executor, and make_motor_cmd (csrc/pbre_host.hpp), behind a flat C
// interface (tests/test_reset_seq_host.py; reset_seq_san.cpp links this file too).
#include "pbre_host.hpp"
#include "pbre_reset_seq.hpp"

using namespace pbre;

// in[6] = robot, use_ik, task, mrec, cfg_flags, fail_at: the executor records (op, count, flags) per operation into out[3 * cap] and fails
// the fail_at-th one (0-based; -1: none) with -7.  Returns the number of operations it was asked for; *rc: what the sequence returned.
extern "C" int reset_seq_record(const int* in, int* out, int cap, int* rc) {
    int n = 0;
    *rc = reset_sequence(in[0], in[1] != 0, in[2], in[3] != 0, in[4], [&](ResetOp op, int count, int flags) {
        if (n < cap) { out[3 * n] = (int)op; out[3 * n + 1] = count; out[3 * n + 2] = flags; }
        return n++ == in[5] ? -7 : 0;
    });
    return n;
}

// pbre_set_motors' command: 0 and out = {n, kp, fscale, vmax}, dof_out[n], target_out[n]; or PBRE_E_ARG and the refusal in msg[128]
extern "C" int motor_cmd(int cnt, const int32_t* dofs, const float* targets, double kp, double max_force, double max_vel, int ndof, double dt,
                         double max_motor_impulse, float* out, int* dof_out, float* target_out, char* msg) {
    pbre_physics ph;
    default_physics(ph);
    ph.dt = dt; ph.max_motor_impulse = max_motor_impulse;
    MotorCmd cmd;
    if (const char* no = make_motor_cmd(cmd, cnt, dofs, targets, kp, max_force, max_vel, ndof, ph)) { std::strncpy(msg, no, 127); msg[127] = 0; return PBRE_E_ARG; }
    out[0] = (float)cmd.n; out[1] = cmd.kp; out[2] = cmd.fscale; out[3] = cmd.vmax;
    for (int k = 0; k < cnt; k++) { dof_out[k] = cmd.dof[k]; target_out[k] = cmd.target[k]; }
    return PBRE_OK;
}
