// emu_capi.cpp -- TEST INFRASTRUCTURE.  Builds libpbre_emu.so: the same C-ABI symbols as
// libpbre.so (include/pbre.h), but the lane-generic step (csrc/pbre_core.hpp) runs through the
// CPU lane emulation (lanes_host.hpp) over host memory.  Purpose: check the device algorithm
// against the oracle in the GPU-less dev container (pytest -m "not gpu").  The product never
// loads this library; it is neither shipped nor a fallback.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>
#include "lanes_host.hpp"
#ifdef PBRE_FIXPOINT_PROBE
// instrumented build (make build/libpbre_emu_probe.so): histograms of the sweep at which the solver blocks of Fast::step_t stop changing
static long g_fix_obj[152], g_fix_mot[152], g_fix_per2[152];
static void pbre_fixpoint_record(int fo, int fm, int po) { g_fix_obj[fo < 0 ? 151 : fo]++; g_fix_mot[fm < 0 ? 151 : fm]++; g_fix_per2[po < 0 ? 151 : po]++; }
extern "C" void pbre_fixpoint_hist(long* o, long* m, long* p2, int clear) {
    for (int i = 0; i < 152; i++) { o[i] = g_fix_obj[i]; m[i] = g_fix_mot[i]; p2[i] = g_fix_per2[i]; if (clear) g_fix_obj[i] = g_fix_mot[i] = g_fix_per2[i] = 0; }
}
#endif
#ifdef PBRE_IK_PROBE
// instrumented build (make build/libpbre_emu_ikprobe.so, tools/ik_cycle_probe.py): per call of Lane::ik_targets, the iteration at which the
// env's IK sequence converged (kind 0), reached a bitwise fixed point (1), a two-cycle (2), or none of these within the cap (3)
static long g_ik_hist[4][128];
static void pbre_ik_probe_record(int kind, int at) { g_ik_hist[kind & 3][at < 0 ? 127 : (at > 126 ? 126 : at)]++; }
extern "C" void pbre_ik_probe_hist(long* h, int clear) {
    for (int k = 0; k < 4; k++) for (int i = 0; i < 128; i++) { h[k * 128 + i] = g_ik_hist[k][i]; if (clear) g_ik_hist[k][i] = 0; }
}
#endif
#include "../../pybullet-robot-envs_amd/csrc/pbre_host.hpp"
#include "../../pybullet-robot-envs_amd/csrc/pbre_reset_seq.hpp"
#include "../../pybullet-robot-envs_amd/csrc/pbre_core.hpp"
static long g_oc_stats[2] = {0, 0};      // lanes that failed / passed the validity bound of the object block's closed form (Fast::obj_closed)
#define PBRE_OC_PROBE(ok) (g_oc_stats[(ok) ? 1 : 0]++)
static long g_rt_why[16] = {0};           // residual exit, closed form: lanes by reason mask (1 object rows not through after OC_K sweeps, 2 a motor may clamp, 4 trial residuals not decreasing, 8 object bound)
static float g_rt_speed[16][2] = {{0}};   // ... and the smallest object speed |v|, |w| seen among the lanes of each mask (is "the cube moves" a predictor?)
#define PBRE_RT_PROBE(why, st) do { int w_ = (why); g_rt_why[w_]++; float v_ = sqrtf((st)[25]*(st)[25] + (st)[26]*(st)[26] + (st)[27]*(st)[27]), o_ = sqrtf((st)[28]*(st)[28] + (st)[29]*(st)[29] + (st)[30]*(st)[30]); \
    if (g_rt_why[w_] == 1 || v_ + o_ < g_rt_speed[w_][0] + g_rt_speed[w_][1]) { g_rt_speed[w_][0] = v_; g_rt_speed[w_][1] = o_; } } while (0)
#include "../../pybullet-robot-envs_amd/csrc/pbre_fast.hpp"
#include "../../pybullet-robot-envs_amd/csrc/pbre_objstep.hpp"
#include "../../pybullet-robot-envs_amd/csrc/pbre_lane.hpp"
#include "../../pybullet-robot-envs_amd/csrc/pbre_comm_impl.hpp"

#include <type_traits>

using namespace pbre;
using FastH = Fast<TopoPanda>;
using LaneH = Lane<TopoICub, Shape32>;

struct pbre_ctx {                       // shape-independent part + the virtual interface of the shape-specific part
    pbre_config cfg;
    Params P;
    int n = 0, obs_dim = 0, act_dim = 0, sf = 0, nj = 0;
    std::vector<float> state, tgt;
    std::string err;
    bool fast_ok = false;
    bool lane_ok = false;                // the iCub's lane-per-env path (pbre_lane.hpp; PBRE_ICUB_LANE=0 switches it off as on the device)
    long n_fast = 0, n_rc = 0, n_general = 0, n_pair = 0;
    int n_bad = 0;                       // NaN / Inf guard counter (Params::bad_count points here)
    std::vector<int> sweeps;             // pbre_get_sweeps (pbre_physics.solver_residual_threshold > 0)
    bool pair = getenv("PBRE_PAIR") && getenv("PBRE_PAIR")[0] == '1';
    bool obj_split = !(getenv("PBRE_OBJ_SPLIT") && getenv("PBRE_OBJ_SPLIT")[0] == '0');
    virtual ~pbre_ctx() {}
    virtual void reset(const uint8_t* mask) = 0;
    virtual int reset_snapshot(const uint8_t* mask) = 0;
    bool have_snapshot = false, stale_snapshot = false;
    virtual void step(const float* actions, float* out) = 0;
    virtual void observe(float* obs) = 0;
    virtual void settle_all(int n, int flags) = 0;
    virtual void limits(float* lo, float* hi) = 0;
    virtual int set_motors(int n, const int32_t* dofs, const float* targets, double kp, double max_force, double max_vel, const uint8_t* mask) = 0;
    virtual int apply_action(const float* actions, double max_vel) = 0;
    bool mrec = false;
};

template <class S>
struct Emu : pbre_ctx {
    using L = pbre_emu::HostLanesT<S::W>;
    using CoreH = Core<L, S>;
    static constexpr bool PANDA = std::is_same<S, Shape16>::value;
    static constexpr int STATE = S::STATE, NJ = S::NJ, W = S::W, TG = S::TGT;
    TablesT<S> T;

    // same dispatch as the device: lane-per-env fast path first (Panda), general lane-group kernel otherwise
    void count_bad(int c) { if (c & FastH::BAD_BIT) n_bad++; }      // (as the device's publish_class: the NaN / Inf guard's counter)
    void step_env(float* st, const float* act, float* out, int mode, int flags, unsigned long long env_id = 0, const float* tg = nullptr) {
        if (P.res_lim > 0.f) { step_env_rt(st, act, out, mode, flags, env_id, tg); return; }
        if constexpr (PANDA) {
            if (fast_ok && !(cfg.flags & PBRE_F_FORCE_GENERAL) && P.obj_shape != PBRE_SHAPE_HULL) {
                // the class is recomputed here instead of being carried from the previous step
                if (FastH::classify_state(T, P, st, flags) == 0) {
                    n_fast++;
                    // PBRE_PAIR=1: the device's pair kernel (k_fast_pair) -- the object's half of the step (ROLE 2), then the robot's half with
                    // the observation (ROLE 1), handing the object's new pose over through the exchange area as the two waves do in LDS
                    if (pair && !(flags & 1) && !(mode & FastH::M_INNER) && st[46] == 0.f) {
                        PairX px;
                        (void)FastH::step_t<false, 2>(T, P, st, nullptr, nullptr, mode, flags, 0ull, nullptr, &px, 0);
                        count_bad(FastH::step_t<false, 1>(T, P, st, act, out, mode, flags, env_id, tg, &px, 0));
                        n_pair++;
                    } else count_bad(FastH::step(T, P, st, act, out, mode, flags, env_id, tg));
                }
                else if ((cfg.flags & PBRE_F_COMPLEX_ROWS) || !P.obj_iso || P.obj_shape != 0) {
                    // the device's k_row_list: physics by the row kernel, observation / reward / done / auto-reset by Fast::finish
                    n_rc++;
                    // (as on the device: the object's half of the step by ObjStep, one lane per env -- the row kernel's fifth wave --, used by
                    // Core::step for an env without robot-object contact)
                    float objv[W] = {0};
                    const bool obj_on = !(flags & 1);
                    if (obj_on) {
                        float pose[7], tw[6], o[6];
                        for (int k = 0; k < 7; k++) pose[k] = st[S::LC + k];
                        for (int k = 0; k < 6; k++) tw[k] = st[W + S::LC + k];
                        const float o_m = st[44] > 0.f ? st[44] : P.obj_m, o_mu = st[45] > 0.f ? st[45] : P.obj_mu, o_kl = st[47] > 0.f ? st[47] - 1.f : P.kl;
                        ObjStep::run_p(P, pose, tw, o, o_m, o_mu, o_kl);
                        for (int k = 0; k < 6; k++) objv[S::LC + k] = o[k];
                    }
                    CoreH::step(T, P, st, act, nullptr, mode & (CoreH::M_ACTION | CoreH::M_TGT), flags, tg, 0ull, obj_on ? objv : nullptr);
                    float q[NJ], qd[NJ];
                    for (int j = 0; j < NJ; j++) { q[j] = st[j]; qd[j] = st[16 + j]; }
                    FastH::V3 op; op.x = st[9]; op.y = st[10]; op.z = st[11];
                    FastH::Q4 oq; oq.x = st[12]; oq.y = st[13]; oq.z = st[14]; oq.w = st[15];
                    count_bad(FastH::finish(T, P, st, q, qd, op, oq, out, mode, flags, env_id));
                }
                else { n_rc++; count_bad(FastH::step_rc(T, P, st, act, out, mode, flags, env_id, tg)); }
                return;
            }
        }
        if constexpr (std::is_same<S, Shape32>::value) {
            // the device's kw_lane / kw_list pair (pbre_wide.hip): task-env steps of the whole batch; settle steps stay on the lane-group kernel
            if (lane_ok && P.obj_shape != PBRE_SHAPE_HULL && (mode & (CoreH::M_OBS | CoreH::M_TASK))) {
                if (LaneH::classify_state(T, P, st, flags) == 0) {
                    n_fast++;
                    float mi[LaneH::NM];
                    LaneH::step(T, P, st, act, out, mode, flags, env_id, tg, mi);
                } else {
                    n_rc++;
                    CoreH::step(T, P, st, act, nullptr, mode & (CoreH::M_ACTION | CoreH::M_TGT), flags, tg, env_id, nullptr);
                    float q[LaneH::ND], qd[LaneH::ND];
                    for (int j = 0; j < LaneH::ND; j++) { q[j] = st[j]; qd[j] = st[W + j]; }
                    LaneH::V3 op; op.x = st[S::LC]; op.y = st[S::LC + 1]; op.z = st[S::LC + 2];
                    LaneH::Q4 oq; oq.x = st[S::LC + 3]; oq.y = st[S::LC + 4]; oq.z = st[S::LC + 5]; oq.w = st[S::LC + 6];
                    LaneH::finish(T, P, st, q, qd, op, oq, out, mode, flags, env_id);
                }
                return;
            }
        }
        n_general++;
        if constexpr (!PANDA) {
            // the device's kw_obj + kw_step pair (pbre_wide_impl.hpp): the object's half of the step per env, used by Core::step
            // when the group has no robot-object contact
            if (obj_split && !(flags & 1) && P.obj_shape != PBRE_SHAPE_HULL) {
                float side[W] = {0.f}, pose[7], tw[6], o[6];
                for (int k = 0; k < 7; k++) pose[k] = st[S::LC + k];
                for (int k = 0; k < 6; k++) tw[k] = st[W + S::LC + k];
                ObjStep::run(P, pose, tw, o);
                for (int k = 0; k < 6; k++) side[S::LC + k] = o[k];
                CoreH::step(T, P, st, act, out, mode, flags, tg, env_id, side);
                return;
            }
        }
        CoreH::step(T, P, st, act, out, mode, flags, tg, env_id);
    }
    // pbre_physics.solver_residual_threshold > 0: the device's RT kernel variants -- one solve over all rows of an env (no pair kernel,
    // no side solve of the object, no lane-per-env iCub pipeline), same choice of kernel otherwise
    void step_env_rt(float* st, const float* act, float* out, int mode, int flags, unsigned long long env_id, const float* tg) {
        int* sw = &sweeps[(size_t)(st - state.data()) / STATE];
        if constexpr (PANDA) {
            if (fast_ok && !(cfg.flags & PBRE_F_FORCE_GENERAL) && P.obj_shape != PBRE_SHAPE_HULL) {
                if (FastH::classify_state(T, P, st, flags) == 0) { n_fast++; count_bad(FastH::template step<true>(T, P, st, act, out, mode, flags, env_id, tg, sw)); }
                else if ((cfg.flags & PBRE_F_COMPLEX_ROWS) || !P.obj_iso || P.obj_shape != 0) {
                    n_rc++;
                    CoreH::template step<true>(T, P, st, act, nullptr, mode & (CoreH::M_ACTION | CoreH::M_TGT), flags, tg, 0ull, nullptr, nullptr, sw);
                    float q[NJ], qd[NJ];
                    for (int j = 0; j < NJ; j++) { q[j] = st[j]; qd[j] = st[16 + j]; }
                    FastH::V3 op; op.x = st[9]; op.y = st[10]; op.z = st[11];
                    FastH::Q4 oq; oq.x = st[12]; oq.y = st[13]; oq.z = st[14]; oq.w = st[15];
                    count_bad(FastH::finish(T, P, st, q, qd, op, oq, out, mode, flags, env_id));
                }
                else { n_rc++; count_bad(FastH::template step_rc<true>(T, P, st, act, out, mode, flags, env_id, tg, sw)); }
                return;
            }
        }
        n_general++;
        CoreH::template step<true>(T, P, st, act, out, mode, flags, tg, env_id, nullptr, nullptr, sw);
    }
    void ik(float* st, const float* act, float* tg, bool rst) {
        if constexpr (PANDA) FastH::ik_targets(T, P, st, act, tg, rst);
        else {
            if constexpr (std::is_same<S, Shape32>::value) { if (lane_ok && !rst && !(P.res_lim > 0.f)) { LaneH::ik_targets(T, P, st, act, tg); return; } }
            CoreH::ik_targets(T, P, st, act, tg, rst);
        }
    }
    void settle(int e, int cnt, int flags) {
        flags |= cfg.flags & (PBRE_F_SEQ_MOTORS | PBRE_F_SEQ_OBJECT);
        const int mode = (P.use_ik || S::MREC) ? CoreH::M_TGT : 0;
        for (int i = 0; i < cnt; i++) step_env(&state[(size_t)e * STATE], nullptr, nullptr, mode, flags, 0, &tgt[(size_t)e * TG]);
    }
    void settle_all(int cnt, int flags) override { for (int e = 0; e < n; e++) settle(e, cnt, flags); }
    void reset(const uint8_t* mask) override {
        int cnt = 0;
        for (int e = 0; e < n; e++) {
            float* st = &state[(size_t)e * STATE];
            float* m = &tgt[(size_t)e * TG];
            if (mask && !mask[e]) continue;
            cnt++;
            unsigned long long id = P.env_id_base + (unsigned long long)e;
            unsigned ep = (unsigned)((int)st[2 * W + 5] + 1);      // episode numbers live in the state records
            // the sequence the device engines run (csrc/pbre_reset_seq.hpp), env by env
            reset_sequence(P.robot, P.use_ik != 0, P.task, S::MREC, cfg.flags, [&](ResetOp op, int count, int flags) {
                switch (op) {
                    case RS_INIT: CoreH::init_state(T, P, id, ep, st); break;
                    case RS_MOTORS: for (int l = 0; l < W; l++) mrec_init<S>(T, m, l); break;
                    case RS_HOME_IK: ik(st, nullptr, m, true); break;
                    case RS_SETTLE: settle(e, count, flags); break;
                    case RS_TARGETS: CoreH::sample_target(P, id, ep, st); break;
                    case RS_INITD: {
                        auto Q = L::load(st), V = L::load(st + W), X = L::loadm(st + 2 * W, L::lti(L::lane(), 16));
                        CoreH::observe(T, P, st, Q, V, X, nullptr, CoreH::M_INITD);
                    }
                }
                return 0;
            });
        }
        if (cnt == n) {      // (as on the device: also a mask of all ones)
            for (int k = 0; k < NJ; k++) { P.rst_q[k] = state[k]; T.rst_q[k] = state[k]; } P.rst_objz = state[S::LC + 2]; have_snapshot = true; stale_snapshot = false;
            std::vector<float> row(obs_dim + 2);
            float* st = &state[0];
            auto Q = L::load(st), V = L::load(st + W), X = L::loadm(st + 2 * W, L::lti(L::lane(), 16));
            CoreH::observe(T, P, st, Q, V, X, row.data(), CoreH::M_OBS);
            for (int k = 0; k < 6; k++) P.rst_ee[k] = row[k];
            if constexpr (PANDA) { bool ok = true; for (int e = 0; e < n; e++) ok = ok && FastH::classify_state(T, P, &state[(size_t)e * STATE], cfg.flags & PBRE_F_NO_OBJECT) == 0; P.rst_ok = ok ? 1 : 0; }
        }
    }
    int reset_snapshot(const uint8_t* mask) override {
        if (S::MREC) { err = "pbre_reset_snapshot: task envs only"; return PBRE_E_UNSUPPORTED; }
        if (!have_snapshot) { err = stale_snapshot ? stale_snapshot_msg() : "pbre_reset_snapshot: no settled snapshot yet (call pbre_reset for the whole batch first)"; return PBRE_E_ARG; }
        for (int e = 0; e < n; e++) {
            if (!mask[e]) continue;
            float* st = &state[(size_t)e * STATE];
            CoreH::snapshot_reset(T, P, P.env_id_base + (unsigned long long)e, st);
            if (P.robot != PBRE_ROBOT_PANDA && P.task >= 1) {
                auto Q = L::load(st), V = L::load(st + W), X = L::loadm(st + 2 * W, L::lti(L::lane(), 16));
                CoreH::observe(T, P, st, Q, V, X, nullptr, CoreH::M_INITD);
            }
        }
        return PBRE_OK;
    }
    void step(const float* actions, float* out) override {
        const int ow = obs_dim + 2;
        const int reps = cfg.action_repeat > 1 ? cfg.action_repeat : 1;
        const Params P0 = P;
        for (int r = 0; r < reps; r++) {
            repeat_scale(P, P0, r);        // all but the last iteration only simulate, test termination and count
            const bool last = r + 1 == reps;
            const int tail = last ? (CoreH::M_OBS | CoreH::M_TASK) : (CoreH::M_TASK | CoreH::M_INNER);
            for (int e = 0; e < n; e++) {
                float* st = &state[(size_t)e * STATE];
                const int fl = cfg.flags & (PBRE_F_NO_OBJECT | PBRE_F_AUTO_RESET | PBRE_F_SEQ_MOTORS | PBRE_F_SEQ_OBJECT);
                const unsigned long long id = P.env_id_base + (unsigned long long)e;
                float* o = last ? out + (size_t)e * ow : nullptr;
                if (P.use_ik) {
                    ik(st, actions + (size_t)e * act_dim, &tgt[(size_t)e * TG], false);
                    step_env(st, nullptr, o, CoreH::M_TGT | tail, fl, id, &tgt[(size_t)e * TG]);
                } else
                    step_env(st, actions + (size_t)e * act_dim, o, CoreH::M_ACTION | tail, fl, id, S::MREC ? &tgt[(size_t)e * TG] : nullptr);
            }
        }
        P = P0;
    }
    void observe(float* obs) override {
        std::vector<float> row(obs_dim + 2);
        for (int e = 0; e < n; e++) {
            float* st = &state[(size_t)e * STATE];
            auto Q = L::load(st), V = L::load(st + W), X = L::loadm(st + 2 * W, L::lti(L::lane(), 16));
            CoreH::observe(T, P, st, Q, V, X, row.data(), CoreH::M_OBS);
            std::memcpy(obs + (size_t)e * obs_dim, row.data(), obs_dim * 4);
        }
    }
    void limits(float* lo, float* hi) override { obs_limits(cfg, T, lo, hi); }
    int apply_action(const float* actions, double max_vel) override {
        if (!S::MREC) { err = "pbre_apply_action: only the robot-level engines keep a motor record"; return PBRE_E_UNSUPPORTED; }
        const bool panda = P.robot == PBRE_ROBOT_PANDA;
        const Params P0 = P;
        const float vm = apply_action_cmd(P, max_vel);
        for (int e = 0; e < n; e++) {
            float* m = &tgt[(size_t)e * TG];
            const float* a = actions + (size_t)e * act_dim;
            if (P.use_ik) ik(&state[(size_t)e * STATE], a, m, false);
            else for (int l = 0; l < T.ndof; l++) mrec_cmd_joint<S>(T, m, l, a, panda ? 0.f : vm);
        }
        P = P0;
        return PBRE_OK;
    }
    int set_motors(int cnt, const int32_t* dofs, const float* targets, double kp, double max_force, double max_vel, const uint8_t* mask) override {
        if (!S::MREC) { err = "pbre_set_motors: only the robot-level engines keep a motor record"; return PBRE_E_UNSUPPORTED; }
        MotorCmd cmd;
        if (const char* no = make_motor_cmd(cmd, cnt, dofs, targets, kp, max_force, max_vel, T.ndof, cfg.phys)) { err = no; return PBRE_E_ARG; }
        for (int e = 0; e < n; e++) {
            if (mask && !mask[e]) continue;
            for (int k = 0; k < cnt; k++) mrec_set<S>(&tgt[(size_t)e * TG], cmd, k);
        }
        return PBRE_OK;
    }
};
static std::string g_err;

template <class S>
static int create(const pbre_config* cfg, pbre_ctx** out) {
    Emu<S>* c = new Emu<S>();
    c->cfg = *cfg;
    std::string e = make_tables<S>(*cfg, c->T, c->P);
    if (!e.empty()) { g_err = e; delete c; return table_error_code(e); }
    c->cfg.robot_table = nullptr;
    c->P.bad_count = &c->n_bad;
    c->n = cfg->num_envs; c->obs_dim = obs_dim_of(c->T, c->P); c->act_dim = act_dim_of(*cfg); c->sf = S::STATE; c->nj = S::NJ;
    c->state.assign((size_t)c->n * S::STATE, 0.f);
    c->sweeps.assign((size_t)c->n, 0);
    c->tgt.assign((size_t)c->n * S::TGT, 0.f);
    c->mrec = S::MREC;
    for (int e = 0; e < c->n; e++) c->state[(size_t)e * S::STATE + 2 * S::W + 5] = -1.f;      // never reset
    if constexpr (std::is_same<S, Shape16>::value) c->fast_ok = topo_matches<TopoPanda>(c->T) && fast_scene_ok(c->P);
    if constexpr (std::is_same<S, Shape32>::value) c->lane_ok = lane_topo_matches<TopoICub, Shape32>(c->T) && (getenv("PBRE_ICUB_LANE") ? getenv("PBRE_ICUB_LANE")[0] != '0' : c->n >= 16384);      // the device's rule (pbre_lane.hip)
    *out = c;
    return PBRE_OK;
}

// runtime policy of csrc/pbre_comm_impl.hpp for the emulation: buffers are host memory, a "stream" is the calling thread
struct HostRuntime {
    typedef int stream_t;
    typedef int event_t;
    static stream_t to_stream(void* abi, bool& own) { own = false; (void)abi; return 0; }
    static void* raw(stream_t) { return nullptr; }
    static std::string set_device(int) { return ""; }
    static std::string current_device(int* d) { *d = 0; return ""; }
    static std::string stream_create_high_priority(stream_t* s) { *s = 0; return ""; }
    static void stream_destroy(stream_t) {}
    static std::string stream_sync(stream_t) { return ""; }
    static std::string event_create(event_t* e) { *e = 0; return ""; }
    static void event_destroy(event_t) {}
    static std::string event_record(event_t, stream_t) { return ""; }
    static std::string stream_wait(stream_t, event_t) { return ""; }
    static std::string event_sync(event_t) { return ""; }
    static std::string copy_async(void* dst, const void* src, size_t bytes, stream_t) { std::memcpy(dst, src, bytes); return ""; }
    static int step(pbre_ctx* ctx, const float* act, float* rows, void*) { return pbre_step(ctx, act, rows); }
};
typedef pbre_comm_detail::Comm<HostRuntime> EmuComm;

extern "C" {

int pbre_default_config(pbre_config* cfg, int32_t robot, int32_t task) { return default_config(cfg, robot, task); }

int pbre_create(const pbre_config* cfg, pbre_ctx** out) {
    if (!cfg || !out) { g_err = "null argument"; return PBRE_E_ARG; }
    const int nd = table_ndof(*cfg);
    if (nd > Shape64::NJ) return create<Shape128>(cfg, out);
    if (cfg->robot_level && nd <= ShapePA::NJ) return create<ShapePA>(cfg, out);
    if (cfg->robot_level && nd <= ShapeIA::NJ) return create<ShapeIA>(cfg, out);
    return nd > Shape32::NJ ? create<Shape64>(cfg, out) : (nd > Shape16::NJ ? create<Shape32>(cfg, out) : create<Shape16>(cfg, out));
}
void pbre_destroy(pbre_ctx* c) { if (c) EmuComm::release(c); delete c; }
const char* pbre_last_error(const pbre_ctx* c) { return c ? c->err.c_str() : g_err.c_str(); }
int pbre_dims(const pbre_ctx* c, int32_t* od, int32_t* ad, int32_t* n) {
    if (!c) return PBRE_E_ARG;
    if (od) *od = c->obs_dim; if (ad) *ad = c->act_dim; if (n) *n = c->n;
    return PBRE_OK;
}
int pbre_state_floats(const pbre_ctx* c) { return c ? c->sf : PBRE_E_ARG; }

int pbre_reset(pbre_ctx* c, const uint8_t* mask, float* obs) {
    if (!c) return PBRE_E_ARG;
    c->reset(mask);
    if (obs) c->observe(obs);
    return PBRE_OK;
}
int pbre_reset_snapshot(pbre_ctx* c, const uint8_t* mask, float* obs) {
    if (!c || !mask) return PBRE_E_ARG;
    const int rc = c->reset_snapshot(mask);
    if (rc != PBRE_OK) return rc;
    if (obs) c->observe(obs);
    return PBRE_OK;
}
int pbre_step(pbre_ctx* c, const float* actions, float* out) {
    if (!c || !actions || !out) return PBRE_E_ARG;
    if (c->stale_snapshot && (c->cfg.flags & PBRE_F_AUTO_RESET)) { c->err = stale_snapshot_msg(); return PBRE_E_ARG; }
    c->step(actions, out);
    return PBRE_OK;
}
// (the pipelined host path: on the host runtime a step is done when the call returns; the bookkeeping -- at most two in flight, wait needs
// one -- is the device library's)
static thread_local long g_async_in_flight = 0;
int pbre_step_async(pbre_ctx* c, const float* actions, float* out) {
    if (!c || !actions || !out) return PBRE_E_ARG;
    if (c->sf != 48) { c->err = "pbre_step_async: implemented for the Panda task envs"; return PBRE_E_UNSUPPORTED; }
    if (g_async_in_flight >= 2) { c->err = "pbre_step_async: two steps are in flight already -- pbre_step_wait first"; return PBRE_E_ARG; }
    const int rc = pbre_step(c, actions, out);
    if (rc == PBRE_OK) g_async_in_flight++;
    return rc;
}
int pbre_step_wait(pbre_ctx* c) {
    if (!c) return PBRE_E_ARG;
    if (g_async_in_flight <= 0) { c->err = "pbre_step_wait: no step in flight"; return PBRE_E_ARG; }
    g_async_in_flight--;
    return PBRE_OK;
}
int pbre_step_device(pbre_ctx* c, const float* a, float* o, void*) { return pbre_step(c, a, o); }
int pbre_sync(pbre_ctx*) { return PBRE_OK; }

int pbre_get_state(pbre_ctx* c, float* s) { if (!c || !s) return PBRE_E_ARG; std::memcpy(s, c->state.data(), c->state.size() * 4); return PBRE_OK; }
int pbre_set_state(pbre_ctx* c, const float* s) { if (!c || !s) return PBRE_E_ARG; std::memcpy(c->state.data(), s, c->state.size() * 4); return PBRE_OK; }

int pbre_get_state_cols(pbre_ctx* c, int32_t first, int32_t count, float* out) {
    if (!c || !out || first < 0 || count <= 0 || first + count > c->sf) return PBRE_E_ARG;
    for (int e = 0; e < c->n; e++) std::memcpy(out + (size_t)e * count, c->state.data() + (size_t)e * c->sf + first, (size_t)count * 4);
    return PBRE_OK;
}
void* pbre_host_alloc(size_t bytes) { return std::malloc(bytes ? bytes : 1); }
void pbre_host_free(void* p) { std::free(p); }
int pbre_observe(pbre_ctx* c, float* obs) {
    if (!c || !obs) return PBRE_E_ARG;
    c->observe(obs);
    return PBRE_OK;
}
int pbre_settle(pbre_ctx* c, int32_t n, int32_t flags) {
    if (!c || n < 0) return PBRE_E_ARG;
    c->settle_all(n, flags & PBRE_F_NO_OBJECT);
    return PBRE_OK;
}
int pbre_set_motors(pbre_ctx* c, int32_t n, const int32_t* dofs, const float* targets, double kp, double max_force, double max_vel, const uint8_t* mask) {
    if (!c || n < 0 || (n > 0 && (!dofs || !targets))) return PBRE_E_ARG;
    return c->set_motors(n, dofs, targets, kp, max_force, max_vel, mask);
}
int pbre_apply_action(pbre_ctx* c, const float* actions, double max_vel) {
    if (!c || !actions) return PBRE_E_ARG;
    return c->apply_action(actions, max_vel);
}
int pbre_get_motor_state(pbre_ctx* c, float* m) {
    if (!c || !m) return PBRE_E_ARG;
    if (!c->mrec) { c->err = "pbre_get_motor_state: only the robot-level engines keep a motor record"; return PBRE_E_UNSUPPORTED; }
    std::memcpy(m, c->tgt.data(), c->tgt.size() * 4);
    return PBRE_OK;
}
int pbre_set_motor_state(pbre_ctx* c, const float* m) {
    if (!c || !m) return PBRE_E_ARG;
    if (!c->mrec) { c->err = "pbre_set_motor_state: only the robot-level engines keep a motor record"; return PBRE_E_UNSUPPORTED; }
    std::memcpy(c->tgt.data(), m, c->tgt.size() * 4);
    return PBRE_OK;
}
int pbre_get_physics(const pbre_ctx* c, pbre_physics* phys) {
    if (!c || !phys) return PBRE_E_ARG;
    *phys = c->cfg.phys;
    return PBRE_OK;
}
void pbre_emu_rt_why(long* out, float* speed, int reset) { for (int i = 0; i < 16; i++) { out[i] = g_rt_why[i]; speed[2 * i] = g_rt_speed[i][0]; speed[2 * i + 1] = g_rt_speed[i][1]; if (reset) g_rt_why[i] = 0; } }
void pbre_emu_oc_stats(long* out, int reset) { out[0] = g_oc_stats[0]; out[1] = g_oc_stats[1]; if (reset) g_oc_stats[0] = g_oc_stats[1] = 0; }
int pbre_get_sweeps(pbre_ctx* c, int32_t* sweeps) {
    if (!c || !sweeps) return PBRE_E_ARG;
    if (!(c->P.res_lim > 0.f)) { c->err = "pbre_get_sweeps: pbre_physics.solver_residual_threshold is 0 (every env runs all solver_iters sweeps)"; return PBRE_E_UNSUPPORTED; }
    for (int e = 0; e < c->n; e++) sweeps[e] = c->sweeps[e];
    return PBRE_OK;
}
int pbre_set_physics(pbre_ctx* c, const pbre_physics* phys) {
    if (!c || !phys) return PBRE_E_ARG;
    pbre_config cfg = c->cfg;
    cfg.phys = *phys;
    Params P2 = c->P;
    if (!apply_physics(*phys, P2)) { c->err = "bad physics parameters"; return PBRE_E_ARG; }
    if (c->fast_ok && !fast_scene_ok(P2)) { c->err = "the lane-per-env kernels need explicit joint damping"; return PBRE_E_UNSUPPORTED; }
    if (snapshot_relevant_change(c->cfg.phys, *phys)) invalidate_snapshot(c->have_snapshot, c->stale_snapshot, P2);
    c->cfg = cfg; c->P = P2;
    return PBRE_OK;
}
int pbre_set_object_hull(pbre_ctx* c, const double* verts, int32_t n_verts) {      // same host code as the device library (csrc/pbre_host.hpp: build_hull); the table stays in host memory
    if (!c) return PBRE_E_ARG;
    static thread_local std::vector<std::unique_ptr<HullTable>> keep;      // (tables live as long as the process: a ctx's Params points into one)
    std::unique_ptr<HullTable> H(new HullTable);
    const std::string e = build_hull(verts, n_verts, *H);
    if (!e.empty()) { c->err = e; return PBRE_E_ARG; }
    apply_hull(*H, H->data, c->cfg, c->P, c->have_snapshot, c->stale_snapshot);
    keep.push_back(std::move(H));
    return PBRE_OK;
}
int pbre_set_physics_per_env(pbre_ctx* c, const uint8_t* mask, const float* obj_mass, const float* obj_mu, const float* obj_lin_damping,
                             const float* robot_lin_damping) {
    if (!c) return PBRE_E_ARG;
    if (c->sf != 48) { c->err = "pbre_set_physics_per_env: implemented for the Panda task envs"; return PBRE_E_UNSUPPORTED; }
    for (int e = 0; e < c->n; e++) {
        if (mask && !mask[e]) continue;
        float* X = c->state.data() + (size_t)e * 48 + 32;
        if (obj_mass) X[12] = obj_mass[e];
        if (obj_mu) X[13] = obj_mu[e];
        if (obj_lin_damping) X[15] = obj_lin_damping[e] + 1.f;
        if (robot_lin_damping) c->state[(size_t)e * 48 + 31] = robot_lin_damping[e] + 1.f;
    }
    return PBRE_OK;
}
int pbre_obs_limits(const pbre_ctx* c, float* lo, float* hi) { if (!c || !lo || !hi) return PBRE_E_ARG; const_cast<pbre_ctx*>(c)->limits(lo, hi); return PBRE_OK; }
int pbre_timing(const pbre_ctx*, double* ms, int32_t n) { for (int i = 0; i < n; i++) ms[i] = 0; return PBRE_OK; }
int pbre_kernel_info(const pbre_ctx* c, int32_t* info, int32_t n) {
    const long v[13] = {0, 0, (c->fast_ok || c->lane_ok) ? 1 : 0, c->n_fast, c->n_general, c->n_rc, 0, 0, 0, 0, c->n_pair, 0, c->n_bad};      // ([10]: env-steps taken by the pair split, PBRE_PAIR=1; [12]: NaN / Inf guard)
    for (int i = 0; i < n; i++) info[i] = i < 13 ? (int32_t)v[i] : 0;
    return PBRE_OK;
}

// the context-owned exchanges of the sharded batch: the SAME source as the product's (csrc/pbre_comm_impl.hpp) on a host runtime -- host
// buffers, no streams, everything synchronous.  With tests/fake_rccl as PBRE_RCCL_LIB the world > 1 branch of pbre_step_gather_device /
// pbre_scatter_actions_device runs between the processes of a CPU test (tests/test_comm_fake_rccl.py).
int pbre_comm_probe(void) { return EmuComm::probe(); }
int pbre_comm_unique_id(void* id) { return EmuComm::unique_id(id); }
int pbre_comm_init(pbre_ctx* c, const void* id, int32_t rank, int32_t world) { return EmuComm::init(c, id, rank, world); }
int pbre_step_gather_device(pbre_ctx* c, const float* a, float* rl, float* ra, void* s) { return EmuComm::step_gather(c, a, rl, ra, s); }
int pbre_gather_wait(pbre_ctx* c, void* s, int32_t h) { return EmuComm::gather_wait(c, s, h); }
int pbre_scatter_actions_device(pbre_ctx* c, const float* all, float* local, void* s) { return EmuComm::scatter_actions(c, all, local, s); }
int pbre_comm_info(const pbre_ctx* c, int32_t* info, int32_t n) { return EmuComm::info(c, info, n); }
const char* pbre_comm_last_error(const pbre_ctx* c) { return EmuComm::last_error(c); }

}  // extern "C"
