// pbre_wide.hip -- the wide lane-group engine: robots with more than 9 DoF (iCub) are stepped by the lane-group core
// (pbre_core.hpp) with one env per half-wave (Shape32: <= 20 DoF, 2 envs per wavefront -- the iCub as the engine simulates
// it, i.e. without the legs, model/table.py prune_base_branches) or one env per wavefront (Shape64: <= 32 DoF).  Lane k of
// the group owns DoF k (robot lanes, 6 object lanes, the constant lane); M^-1 rows, constraint rows and the 150-iteration
// PGS state live in VGPRs; cross-lane traffic is DPP / ds_swizzle (all-reduce), ds_bpermute (gathers, broadcasts inside a
// half-wave) and v_readlane (broadcasts inside a whole wave).  No LDS memory, no barriers; a block is 4 independent waves.
// State: Q[W] | V[W] | X[16] floats per env (80 for Shape32, 144 for Shape64).  The kernels and the shape-specific engine half
// are templates in pbre_wide_impl.hpp; the iCub with hands (Shape128, 60 DoF) is instantiated in pbre_hands.hip.
//
// Replaces, per env (reference file:line): iCubReachGymEnv / iCubPushGymEnv / iCubPushGymGoalEnv .step and .reset
// (icub_reach_gym_env.py:114-259, icub_push_gym_env.py:116-282, icub_push_gym_goal_env.py:69-139), iCubEnv.apply_action /
// get_observation (icub_env.py:202-361) and the p.stepSimulation / p.calculateInverseKinematics calls inside them.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "pbre_wide_impl.hpp"

namespace pbre {

hipError_t WideEngine::wstep(int kind, float* st, float* tg, int cnt, const float* act, float* out, int flags, hipStream_t s, bool timed) {
    const Event* ek = ev_k[k_steps % KRING];
    if (timed) (void)hipEventRecord(ek[0], s);
    launch_step(kind, st, tg, cnt, act, out, flags, s);
    if (timed) { (void)hipEventRecord(ek[1], s); k_steps++; }
    return hipGetLastError();
}
hipError_t WideEngine::wsettle(float* st, float* tg, int cnt, int count, int flags, hipStream_t s) {
    const int kind = (P.use_ik || mrec) ? K_SETTLE_TGT : K_SETTLE;
    // settle steps of the whole batch in place: through the lane-per-env pipeline where it is the step path (pbre_lane.hip); the object's
    // presence decides the classes, so they are recomputed for this run of steps and left invalid after it
    const bool lane = lane_ok() && st == state && tg == tgt && cnt == n;
    if (lane) lane_invalidate();
    for (int i = 0; i < count; i++) {
        hipError_t e = lane ? launch_lane_step(kind, nullptr, nullptr, flags, s, false) : wstep(kind, st, tg, cnt, nullptr, nullptr, flags, s);
        if (e != hipSuccess) return e;
    }
    if (lane) lane_invalidate();
    return hipSuccess;
}
hipError_t WideEngine::step_repeat(bool last, const float* d_actions, float* d_rows, int flags, hipStream_t s) {
    if (lane_ok()) {     // lane-per-env path (pbre_lane.hpp)
        if (P.use_ik) launch_lane_ik(d_actions, s);
        return launch_lane_step(P.use_ik ? (last ? K_STEP_TGT : K_INNER_TGT) : (last ? K_STEP_ACT : K_INNER_ACT), d_actions, last ? d_rows : nullptr, flags, s, last);
    }
    if (!P.use_ik) return wstep(last ? K_STEP_ACT : K_INNER_ACT, state, tgt, n, d_actions, last ? d_rows : nullptr, flags, s, last);
    launch_ik(false, state, d_actions, tgt, n, s, true);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { obj_done = nullptr; return e; }
    return wstep(last ? K_STEP_TGT : K_INNER_TGT, state, tgt, n, nullptr, last ? d_rows : nullptr, flags, s, last);
}

pbre_ctx* new_lane_group_engine(const pbre_config& cfg) {
    const int nd = table_ndof(cfg);
    return nd > Shape64::NJ ? make_hands_engine()
         : (cfg.robot_level && nd <= ShapePA::NJ ? static_cast<WideEngine*>(new WideImpl<ShapePA, DevLanes32>())     // pandaEnv alone
         : (cfg.robot_level && nd <= ShapeIA::NJ ? make_icub_arm_engine()                                             // iCubEnv alone
         : (nd <= Shape32::NJ ? make_lane_engine()
                              : static_cast<WideEngine*>(new WideImpl<Shape64, DevLanes64>()))));
}

int WideEngine::init(const pbre_config& c) {
    cfg = c;
    const std::string e = tables(c);
    if (!e.empty()) return fail(table_error_code(e), e.c_str());
    cfg.robot_table = nullptr;
    n = c.num_envs; act_dim = act_dim_of(c); ow = obs_dim + 2; device = c.device_id;
    if (const int rc = open_device()) return rc;
    const size_t ne = (size_t)n, tg = (size_t)tgs;
    HIPCHK(upload_tables());
    HIPCHK(hipMalloc(state_buf.out(), ne * sf * sizeof(float)));
    state = state_buf;
    HIPCHK(hipMalloc(tmp.out(), ne * sf * sizeof(float)));
    scratch = tmp;
    HIPCHK(hipMalloc(tgt.out(), ne * tg * sizeof(float)));
    HIPCHK(hipMalloc(tgt_tmp.out(), ne * tg * sizeof(float)));
    HIPCHK(hipMemset(tgt, 0, ne * tg * sizeof(float)));
    HIPCHK(hipMemset(tgt_tmp, 0, ne * tg * sizeof(float)));
    {   // side records of the per-env object solve (pbre_objstep.hpp); PBRE_OBJ_SPLIT=0 keeps every object row in kw_step (A/B runs)
        const char* knob = getenv("PBRE_OBJ_SPLIT");
        if (!(knob && knob[0] == '0')) {
            const size_t wl = ((size_t)sf - 16) / 2;
            HIPCHK(hipMalloc(objv.out(), ne * wl * sizeof(float)));
            HIPCHK(hipMemset(objv, 0, ne * wl * sizeof(float)));
        }
    }
    if (const int rc = alloc_step_io(ne)) return rc;
    if (const int rc = alloc_counters(ne)) return rc;
    HIPCHK(lane_alloc());
    if (const int rc = alloc_reset_ids(ne, ne)) return rc;
    // every record holds a valid (un-settled) state with episode -1
    launch_init(state, n, stream);
    launch_init(tmp, n, stream);
    launch_mrec_init(tgt, n, stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    return PBRE_OK;
}

int WideEngine::settle(int32_t count, int32_t flags) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    HIPCHK(wsettle(state, tgt, n, count, flags & PBRE_F_NO_OBJECT, stream));
    lane_invalidate();
    HIPCHK(hipStreamSynchronize(stream));
    return PBRE_OK;
}
// reset(): reset_sequence's operations on the batch (state, tgt) or the scratch buffers (tmp, tgt_tmp)
hipError_t WideEngine::reset_op(ResetOp op, bool in_scratch, int cnt, int count, int flags) {
    float* st = in_scratch ? (float*)tmp : state;
    float* tg = in_scratch ? (float*)tgt_tmp : (float*)tgt;
    switch (op) {
        case RS_INIT: launch_init(st, cnt, stream); break;
        case RS_MOTORS: launch_mrec_init(tg, cnt, stream); break;
        case RS_HOME_IK: launch_ik(true, st, nullptr, tg, cnt, stream); break;
        case RS_SETTLE: return wsettle(st, tg, cnt, count, flags, stream);
        case RS_TARGETS: launch_target(st, cnt, stream); break;
        case RS_INITD: launch_observe(true, st, nullptr, cnt, stream); break;
    }
    return hipGetLastError();
}
int WideEngine::reset_snapshot(const uint8_t* mask) {
    if (mrec) return fail(PBRE_E_UNSUPPORTED, "pbre_reset_snapshot: task envs only (the robot-level interfaces have no episodes)");
    return pbre_ctx::reset_snapshot(mask);
}
int WideEngine::set_motors(int32_t cnt, const int32_t* dofs, const float* targets, double kp, double max_force, double max_vel, const uint8_t* mask) {
    if (!mrec) return fail(PBRE_E_UNSUPPORTED, "pbre_set_motors: only the robot-level engines keep a motor record");
    MotorCmd cmd;
    if (const char* no = make_motor_cmd(cmd, cnt, dofs, targets, kp, max_force, max_vel, ndof(), cfg.phys)) return fail(PBRE_E_ARG, no);
    if (cnt == 0) return PBRE_OK;
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    if (mask) {
        if (!d_mask) HIPCHK(hipMalloc(d_mask.out(), (size_t)n));
        HIPCHK(hipMemcpyAsync(d_mask, mask, (size_t)n, hipMemcpyHostToDevice, stream));
    }
    launch_set_motors(cmd, mask ? (const unsigned char*)d_mask : nullptr, stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    return PBRE_OK;
}
int WideEngine::apply_action(const float* actions, double max_vel) {
    if (!mrec) return fail(PBRE_E_UNSUPPORTED, "pbre_apply_action: only the robot-level engines keep a motor record");
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    hipStream_t s = stream;
    HIPCHK(hipMemcpyAsync(d_act, actions, (size_t)n * act_dim * 4, hipMemcpyHostToDevice, s));
    const Params P0 = P;
    const float vm = apply_action_cmd(P, max_vel);
    if (P.use_ik) launch_ik(false, state, d_act, tgt, n, s);
    else launch_cmd_joints(d_act, P.robot == PBRE_ROBOT_PANDA ? 0.f : vm, s);      // the joint branch passes maxVelocity on the iCub only (icub_env.py:353-360)
    P = P0;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return PBRE_OK;
}
int WideEngine::motor_state(float* out, const float* in) {
    if (!mrec) return fail(PBRE_E_UNSUPPORTED, "pbre_get/set_motor_state: only the iCub-with-hands engine keeps a motor record");
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    if (out) HIPCHK(hipMemcpy(out, tgt, (size_t)n * tgs * 4, hipMemcpyDeviceToHost));
    if (in) HIPCHK(hipMemcpy(tgt, in, (size_t)n * tgs * 4, hipMemcpyHostToDevice));
    return PBRE_OK;
}
int WideEngine::kernel_info(int32_t* info, int32_t cnt) const {
    int lv = -1, cn = 0;
    const bool lane = lane_ok() && const_cast<WideEngine*>(this)->lane_info(&lv, &cn);      // (classifies the batch if its classes are stale)
    // same slots as the Panda engine: [0] VGPRs of the lane-per-env kernel, [1] of the lane-group kernel, [2] lane-per-env path in use,
    // [3] envs in the simple class, [4] envs the lane-group kernel steps when the lane path is off, [5] complex envs,
    // [12] env-steps that met a non-finite state (NaN / Inf guard)
    const int v[13] = {lane ? lv : -1, vgprs(), lane ? 1 : 0, lane ? n - cn : 0, lane ? 0 : n, lane ? cn : 0, -1, 0, 0, 0, 0, 0, read_bad()};
    for (int i = 0; i < cnt; i++) info[i] = i < 13 ? v[i] : 0;
    return PBRE_OK;
}

}  // namespace pbre
