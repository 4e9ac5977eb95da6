// pbre_engine.hpp -- pbre_ctx, the one engine type behind the C-ABI (include/pbre.h): the shape-independent half of an engine -- buffers,
// stream, events, the host logic of every entry point -- and the virtual interface of the half that depends on the robot's kernels.
// Implementations: PandaEngine (pbre_panda.hpp / pbre_capi.hip, the Panda task envs) and WideEngine (pbre_wide_impl.hpp / pbre_wide.hip:
// the lane-group engines of the iCub, the iCub with hands and the robot-level pandaEnv / iCubEnv).  pbre_capi.hip's extern "C" functions
// check their arguments and call one method.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include "pbre_devmem.hpp"
#include "pbre_host.hpp"
#include "pbre_reset_seq.hpp"
#include "pbre_scene.hpp"

// the one HIP error check of the library, with an engine `eng`; HIPCHK is its spelling inside a method of an engine.  (Set-up helpers that
// hand a hipError_t on to such a check -- alloc_buf, lane_alloc, SidePick::create -- test their calls themselves.)
#define PBRE_CHK_ON(eng, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return (eng)->hip_fail(#call, e_); } while (0)
#define HIPCHK(call) PBRE_CHK_ON(this, call)

namespace pbre {
// What a unit that reads an engine's state without stepping it gets (the camera, the contact query, the kinematics query) -- it writes
// none of it: the state records [n][stride] floats on the device (object pose at float obj_lane of a record), the scene, the hull table
// (null without one; its piece directory is in its header, pbre_tables.hpp) and the stream the unit's kernels go to.
struct StateView {
    const float* state; int stride, n, obj_lane, flags;
    pbre_physics phys;
    const float* hull;
    void* stream;         // a hipStream_t
};
struct ResetKeep { int pad, n, slot[4]; };      // pbre_ctx::rst_keep (by value to the next-episode kernel)
}  // namespace pbre

struct pbre_ctx {
    pbre_config cfg;
    pbre::Params P;
    int n = 0, obs_dim = 0, act_dim = 0, ow = 0, device = 0;
    int sf = 0, lc = 0;                       // floats per state record, float of the object's pose in it
    float* state = nullptr;                   // [n][sf] the batch's records (a view: the engine's buffers own them)
    float* scratch = nullptr;                 // ... and as many in which a partial reset settles a compacted copy of the selected envs
    bool mrec = false;                        // the shape keeps persistent motor records (the robot-level interfaces)
    pbre::ResetKeep rst_keep = {1, 0, {0}};   // reset: a multiple of `pad` records is initialised (the last env repeated); n floats of its record an env keeps
    pbre::DevBuf<float> d_act, d_out;         // staging of pbre_step's actions / rows
    pbre::DevBuf<int> d_bad;                  // NaN / Inf guard: env-steps that met a non-finite state (Params::bad_count)
    pbre::DevBuf<float> d_hull;               // PBRE_SHAPE_HULL: the object's vertex / face table (Params::hull; pbre_set_object_hull)
    pbre::DevBuf<int> d_sweeps;               // sweeps every env's solver ran in the last step (Params::sweeps; solver_residual_threshold > 0)
    pbre::DevBuf<unsigned long long> d_ids; pbre::DevBuf<unsigned> d_ep; pbre::DevBuf<int> d_idx;      // reset: env ids, episodes, indices
    pbre::DevBuf<unsigned char> d_mask;
    pbre::Stream stream;
    pbre::Event ev[4];                        // pbre_step: upload | step | download
    static constexpr int KRING = 64;          // HIP event pairs around the dominant kernel of the last KRING sampled steps (pbre_timing[3])
    pbre::Event ev_k[KRING][2];
    long k_steps = 0;
    double ms[3] = {0, 0, 0};
    bool have_snapshot = false;               // a full pbre_reset has recorded the settled snapshot (rst_q, rst_objz)
    bool stale_snapshot = false;              // ... and a later scene change invalidated it
    bool ext_dirty = false;                   // a step was enqueued on a caller-supplied stream since the last quiesce()
    std::string err;
    pbre::Readers readers;                    // the RobotTable copy and the buffers of the units that read the state (pbre_scene.hpp)

    virtual ~pbre_ctx() {}
    // the only way an engine is deleted: device set, its streams drained, then its owners release (also after a failed init)
    static void destroy(pbre_ctx* c);
    int hip_fail(const char* what, hipError_t e) { err = std::string(what) + ": " + hipGetErrorString(e); return PBRE_E_DEVICE; }
    int fail(int code, const char* msg) { err = msg; return code; }

    // ---- set-up: tables, buffers and a valid state in every record; on failure the text is in err
    virtual int init(const pbre_config& c) = 0;
    int open_device();                        // device count and range checks, the stream and the events
    int alloc_step_io(size_t rows);           // d_act / d_out
    int alloc_counters(size_t rows);          // d_bad, d_sweeps (Params::bad_count / sweeps)
    int alloc_reset_ids(size_t rows, size_t ids);      // d_ids / d_ep for `ids` records, all of episode -1; d_idx

    // ---- host logic written once
    hipError_t quiesce();                     // all work the ctx has in flight is complete on return
    hipStream_t stream_of(void* abi);         // PBRE_STREAM_LEGACY / a hipStream_t / null = the ctx's own
    hipError_t full_step(const float* d_actions, float* d_rows, hipStream_t s);      // the action-repeat loop
    int timed_step(const float* actions, float* out, bool za, bool zo);              // za / zo: the kernels access that host buffer themselves
    int check_stale() { return (stale_snapshot && (cfg.flags & PBRE_F_AUTO_RESET)) ? fail(PBRE_E_ARG, pbre::stale_snapshot_msg()) : PBRE_OK; }
    int begin_step();                         // pbre_step: the device, the order behind work on a caller's stream, the stale-snapshot refusal
    int read_bad() const;                     // pbre_kernel_info[12]
    int sync();
    int observe(float* obs);
    int step_device(const float* d_actions, float* d_rows, void* stream);
    int get_state(float* s);
    int set_state(const float* s);
    int get_state_cols(int32_t first, int32_t count, float* out);
    int get_sweeps(int32_t* sweeps);
    int set_physics(const pbre_physics* phys);
    int set_object_hull(const double* verts, int32_t n_verts);
    int timing(double* out, int32_t cnt) const;
    int state_view(pbre::StateView* v, void* stream, bool host_sync);

    // ---- hooks of the shared logic
    virtual hipError_t state_changed() = 0;   // the records or the scene were changed by something other than a step
    virtual hipError_t drain_side() { return hipSuccess; }                           // streams beside `stream` that hold work of the ctx
    virtual hipError_t step_repeat(bool last, const float* d_actions, float* d_rows, int flags, hipStream_t s) = 0;   // one iteration of full_step
    virtual void launch_observe_all(hipStream_t s) = 0;                              // every env's observation into d_out
    virtual void launch_snapshot_reset(const unsigned char* mask, hipStream_t s) = 0;
    virtual const char* physics_objection(const pbre::Params&) const { return nullptr; }   // pbre_set_physics: what the engine cannot step
    virtual void limits(float* lo, float* hi) const = 0;
    virtual int kernel_info(int32_t* info, int32_t cnt) const = 0;

    // ---- entry points whose substance differs between the engines
    virtual int reset(const uint8_t* mask);   // (written once, pbre_capi.hip; an engine's override brackets it)
    virtual int settle(int32_t count, int32_t flags) = 0;
    virtual int reset_snapshot(const uint8_t* mask);
    virtual int step(const float* actions, float* out) { const int rc = begin_step(); return rc ? rc : timed_step(actions, out, false, false); }
    // ... and those only one family implements
    virtual int step_async(const float*, float*) { return fail(PBRE_E_UNSUPPORTED, "pbre_step_async: implemented for the Panda task envs (the BASELINE metric's path); use pbre_step"); }
    virtual int step_wait() { return fail(PBRE_E_UNSUPPORTED, "pbre_step_wait: no pbre_step_async on this engine"); }
    virtual int set_physics_per_env(const uint8_t*, const float*, const float*, const float*, const float*) {
        return fail(PBRE_E_UNSUPPORTED, "pbre_set_physics_per_env: implemented for the Panda task envs (change_physics_params, panda_push_gym_env.py:362-368)");
    }
    virtual int set_motors(int32_t, const int32_t*, const float*, double, double, double, const uint8_t*) {
        return fail(PBRE_E_UNSUPPORTED, "pbre_set_motors: only the robot-level engines (pbre_config.robot_level) keep a motor record");
    }
    virtual int apply_action(const float*, double) { return fail(PBRE_E_UNSUPPORTED, "pbre_apply_action: only the robot-level engines (pbre_config.robot_level) keep a motor record"); }
    virtual int motor_state(float* out, const float*) {
        return fail(PBRE_E_UNSUPPORTED, out ? "pbre_get_motor_state: only the robot-level engines keep a motor record" : "pbre_set_motor_state: only the robot-level engines keep a motor record");
    }

    // ---- hooks of reset(): one operation of reset_sequence on the first cnt records of the batch in place or of the scratch buffer; what
    // is left to do once a partial reset's records are scattered back; the settled record of env 0 into rst_q / rst_objz of the uploaded
    // tables; whether steps restart envs in-kernel (rst_ee / rst_ok) and, if so, how many envs of the batch are complex now
    hipError_t scatter_records(float* dst, const float* src, int cnt, int floats);      // dst[d_idx[i]] <- src[i], i < cnt
    virtual hipError_t reset_op(pbre::ResetOp op, bool in_scratch, int cnt, int count, int flags) = 0;
    virtual hipError_t reset_scattered(int cnt) = 0;
    virtual hipError_t record_snapshot(const float* rec) = 0;
    virtual bool restarts_in_kernel() const = 0;
    virtual hipError_t complex_now(int* count) = 0;
};

namespace pbre {
int fail(pbre_ctx* c, int code, const char* msg);             // pbre_capi.hip: the text to c->err, or without a ctx to the calling thread's slot; returns code
pbre_ctx* new_lane_group_engine(const pbre_config& cfg);      // pbre_wide.hip: the implementation for a robot of more than 9 DoF / the robot level
}
