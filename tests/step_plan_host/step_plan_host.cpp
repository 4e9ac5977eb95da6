// The step planner of the Panda engine behind a flat C interface (tests/test_step_plan_host.py; field orders: KNOBS, QUERY, PLAN there).
#include "pbre_step_plan.hpp"

using namespace pbre;

// knobs[11], query[15] -> plan[18]
extern "C" void step_plan(const int* kn, const int* qu, int* out) {
    StepKnobs k;
    k.rc_first_min = kn[0]; k.idle_touch = kn[1]; k.idle_single = kn[2]; k.row_max = kn[3]; k.pair = kn[4]; k.tail_pair = kn[5];
    k.fast3 = kn[6]; k.fused = kn[7]; k.ksample = kn[8]; k.zero_copy = kn[9]; k.objv_seq0 = kn[10];
    StepQuery q;
    q.n = qu[0]; q.n_simd = qu[1]; q.nb = qu[2]; q.hint = qu[3]; q.recent = qu[4]; q.cfg_flags = qu[5]; q.step_flags = qu[6];
    q.rt = qu[7] != 0; q.inner = qu[8] != 0; q.fusable = qu[9] != 0; q.obj_iso = qu[10] != 0; q.obj_shape = qu[11];
    q.action_repeat = qu[12]; q.have_pair_g = qu[13] != 0; q.launches = qu[14];
    const StepPlan p = plan_step(k, q);
    const int v[18] = {(int)p.form, p.rows, p.pair, p.rblocks, p.ntail, p.fast3, p.single, p.rc_first, p.touch_side, p.rc_on_caller, p.fast_on_caller,
                       p.fork_join, p.grid_fused, p.threads_fused, p.grid_rc, p.threads_rc, p.grid_fast, p.threads_fast};
    for (int i = 0; i < 18; i++) out[i] = v[i];
}

// knobs[11]: the defaults (from_env = 0) or what the process's environment says
extern "C" void step_knobs(int from_env, int* out) {
    const StepKnobs k = from_env ? StepKnobs::from_env() : StepKnobs();
    const int v[11] = {k.rc_first_min, k.idle_touch, k.idle_single, k.row_max, k.pair, k.tail_pair, k.fast3, k.fused, k.ksample, k.zero_copy, k.objv_seq0};
    for (int i = 0; i < 11; i++) out[i] = v[i];
}
