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

__global__ void kw_next_episode(const float* __restrict__ state, const int* __restrict__ idx, int cnt, unsigned* __restrict__ ep, int sf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt) ep[i] = (unsigned)((int)state[(size_t)idx[i] * sf + (sf - 16) + 5] + 1);
}
__global__ void kw_scatter(float* __restrict__ dst, const float* __restrict__ src, const int* __restrict__ idx, int cnt, int sf) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = t / sf, k = t % sf;
    if (i < cnt) dst[(size_t)idx[i] * sf + k] = src[(size_t)i * sf + k];
}

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
int WideEngine::reset(const uint8_t* mask) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    lane_invalidate();
    std::vector<int> idx;
    for (int e = 0; e < n; e++) if (!mask || mask[e]) idx.push_back(e);
    const int cnt = (int)idx.size();
    if (cnt > 0) {
        std::vector<unsigned long long> ids(cnt);
        for (int i = 0; i < cnt; i++) ids[i] = P.env_id_base + (unsigned long long)idx[i];
        hipStream_t s = stream;
        HIPCHK(hipMemcpyAsync(d_ids, ids.data(), (size_t)cnt * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_idx, idx.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(kw_next_episode, dim3((cnt + 127) / 128), dim3(128), 0, s, state, d_idx, cnt, d_ep, sf);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));                      // host vectors go out of scope below
        const bool full = cnt == n;
        float* st = full ? state : (float*)tmp;               // a partial reset settles a compacted copy
        float* tg = full ? tgt : tgt_tmp;
        const int f0 = cfg.flags & PBRE_F_NO_OBJECT;
        launch_init(st, cnt, s);
        launch_mrec_init(tg, cnt, s);
        HIPCHK(hipGetLastError());
        // iCubEnv.reset (icub_env.py:88-151): joints at their initial positions, IK targets of the home hand pose when
        // use_IK, one stepSimulation; then reset_simulation (icub_reach_gym_env.py:135-148): 100 steps robot alone,
        // world loaded, 100 + 1 steps
        if (P.use_ik) {
            launch_ik(true, st, nullptr, tg, cnt, s);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(wsettle(st, tg, cnt, (P.use_ik || P.robot != PBRE_ROBOT_PANDA ? 1 : 0) + 100, PBRE_F_NO_OBJECT, s));
        HIPCHK(wsettle(st, tg, cnt, 101, f0, s));
        launch_target(st, cnt, s);
        HIPCHK(hipGetLastError());
        if (P.task >= 1) {   // iCubPushGymEnv.reset (icub_push_gym_env.py:124-127): distances the normalised reward divides by
            launch_observe(true, st, nullptr, cnt, s);
            HIPCHK(hipGetLastError());
        }
        if (!full) {
            // the IK targets of the reset envs are only needed while settling; the next step recomputes them
            hipLaunchKernelGGL(kw_scatter, dim3((cnt * sf + 255) / 256), dim3(256), 0, s, state, st, d_idx, cnt, sf);
            if (mrec) hipLaunchKernelGGL(kw_scatter, dim3((cnt * tgs + 255) / 256), dim3(256), 0, s, tgt, tg, d_idx, cnt, tgs);   // motors persist
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(s));
        if (full) {   // snapshot for PBRE_F_AUTO_RESET: settled robot pose and object height (identical in every env)
            std::vector<float> rec(sf);
            HIPCHK(hipMemcpy(rec.data(), state, (size_t)sf * sizeof(float), hipMemcpyDeviceToHost));
            snapshot(rec.data());
            HIPCHK(upload_tables());
            have_snapshot = true; stale_snapshot = false;
            // end-effector pose of the settled robot (the first 6 observation entries of env 0) for the lane-per-env pipeline's in-kernel
            // restart (Lane::finish): valid while the settled state is in the simple class (no robot sphere at the object)
            P.rst_ok = 0;
            if (lane_ok() && !mrec) {
                launch_observe_all(s);
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(s));
                float row[6]; int vg = 0, cn = 1;
                HIPCHK(hipMemcpy(row, d_out, sizeof row, hipMemcpyDeviceToHost));
                for (int k = 0; k < 6; k++) P.rst_ee[k] = row[k];
                if (lane_info(&vg, &cn) && cn == 0) P.rst_ok = 1;
            }
        }
    }
    return PBRE_OK;
}
int WideEngine::reset_snapshot(const uint8_t* mask) {
    if (mrec) return fail(PBRE_E_UNSUPPORTED, "pbre_reset_snapshot: task envs only (the robot-level interfaces have no episodes)");
    return pbre_ctx::reset_snapshot(mask);
}
int WideEngine::set_motors(int32_t cnt, const int32_t* dofs, const float* targets, double kp, double max_force, double max_vel, const uint8_t* mask) {
    if (!mrec) return fail(PBRE_E_UNSUPPORTED, "pbre_set_motors: only the robot-level engines keep a motor record");
    if (cnt > 64) return fail(PBRE_E_ARG, "pbre_set_motors: more than 64 joints");
    MotorCmd cmd;
    cmd.n = cnt; cmd.kp = (float)kp;
    cmd.fscale = max_force > 0 ? (float)(max_force * cfg.phys.dt / cfg.phys.max_motor_impulse) : 1.f;
    cmd.vmax = max_vel > 0 ? (float)max_vel : 0.f;
    for (int k = 0; k < cnt; k++) {
        if (dofs[k] < 0 || dofs[k] >= ndof()) return fail(PBRE_E_ARG, "pbre_set_motors: bad DoF index");
        cmd.dof[k] = dofs[k]; cmd.target[k] = targets[k];
    }
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
