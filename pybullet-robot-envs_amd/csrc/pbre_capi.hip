// pbre_capi.hip -- libpbre.so: HIP kernels (gfx950) + the C-ABI of include/pbre.h.
//
// Four stepping kernels:
//   k_fast      lane-per-env (one thread = one env, 64 envs per wave), everything in VGPRs.  Steps the "simple" envs (class 0: no robot
//               contact, no joint-limit row): 9 motor rows (in closed form) + <= 4 object-table contacts.  Two builds: 256 VGPRs / 2 waves
//               per SIMD, and 168 VGPRs / 3 per SIMD for the steps in which the complex envs' waves need room (launch_step picks).
//   k_row_list  complex envs (class 1), few of them: the 16-lane row physics of k_step over the compacted list + Fast::finish,
//               concurrently with k_fast on a second stream.
//   k_fast_rc   complex envs, many of them: lane-per-env with dense robot-contact rows and limit rows, whole register file (1 wave/SIMD).
//   k_step      general 16-lane-row kernel (pbre_core.hpp): one env per DPP row, 4 envs per wave.  Any robot the
//               RobotTable describes (<= 9 DoF); used when the table does not match the compiled-in Panda topology
//               or when PBRE_F_FORCE_GENERAL is set (validation).
// Every step kernel ends by classifying the state it produced and appends complex envs to the list the next step's complex-env
// kernel consumes, so there is no classification pre-pass on the hot path.
//
// State lives in HBM as one 192-byte record per env (three 64-byte lane records).  No kernel uses LDS or barriers; blocks
// are independent, so the block -> XCD mapping is irrelevant (there is no inter-block reuse to be XCD-aware about).
#include "pbre_panda.hpp"

#ifdef PBRE_UNITY
PBRE_STEP_INST_ALL()
#else
PBRE_STEP_INST_ALL(extern)      // pbre_step_inst.hip, one translation unit per (MODE, RT)
#endif

// use_IK = 1: hand-pose update + inverse kinematics -> joint targets (one thread per env).  RESET: targets of the home hand pose.
template <bool RESET>
__global__ __launch_bounds__(FTPB) void k_ik(const FTables* __restrict__ T, const Params P, float* __restrict__ state,
                                             const float* __restrict__ actions, float* __restrict__ tgt, int n, int act_dim) {
    const int env = blockIdx.x * FTPB + threadIdx.x;
    if (env >= n) return;
    FastD::ik_targets(*T, P, state + (size_t)env * STATE, RESET ? nullptr : actions + (size_t)env * act_dim, tgt + (size_t)env * NJ, RESET);
}

// Class of every env's current state (after reset / set_state / a change of the NO_OBJECT flag).
__global__ __launch_bounds__(FTPB) void k_classify(const FTables* __restrict__ T, const Params P, const float* __restrict__ state, int n, int flags,
                                                   signed char* __restrict__ cls, int* __restrict__ list, int* __restrict__ count, int cap) {
    const int env = blockIdx.x * FTPB + threadIdx.x;
    if (env >= n) return;
    publish_class(env, FastD::classify_state(*T, P, state + (size_t)env * STATE, flags), cls, list, count, cap);
}

__global__ void k_total(const int* __restrict__ count, int* __restrict__ host_total, int* __restrict__ recent) {
    int t = 0;
    for (int b = 0; b < NB; b++) t += count[b];
    *recent = 0;
    const int acc = recent[1];
    report_hint(t, recent, host_total);
    recent[1] = acc;                    // a (re)classification is not a step
}

__global__ __launch_bounds__(TPB) void k_observe(const Tables* __restrict__ T, const Params P, float* __restrict__ state,
                                                 float* __restrict__ out, float* __restrict__ scratch_row, int n, int ow) {
    const int env = blockIdx.x * EPB + (threadIdx.x >> 4);
    float* st = state + (size_t)env * STATE;
    float Q = DevLanes::load(st), V = DevLanes::load(st + 16), X = DevLanes::load(st + 32);
    CoreD::observe(*T, P, st, Q, V, X, env < n ? out + (size_t)env * ow : scratch_row, CoreD::M_OBS);
}

// robot.reset + WorldEnv._sample_pose: one thread per env.  ids: global env id per record, ep: episode per record
__global__ void k_init(const Tables* __restrict__ T, const Params P, float* __restrict__ state,
                       const unsigned long long* __restrict__ ids, const unsigned* __restrict__ ep, int cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt) CoreD::init_state(*T, P, ids[i], ep[i], state + (size_t)i * STATE);
}
__global__ void k_target(const Params P, float* __restrict__ state, const unsigned long long* __restrict__ ids,
                         const unsigned* __restrict__ ep, int cnt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt) CoreD::sample_target(P, ids[i], ep[i], state + (size_t)i * STATE);
}
// pbre_reset_snapshot: the selected envs start their next episode from the settled snapshot (what PBRE_F_AUTO_RESET does in-kernel)
__global__ void k_snapshot_reset(const Tables* __restrict__ T, const Params P, float* __restrict__ state, const unsigned char* __restrict__ mask, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n && mask[e]) CoreD::snapshot_reset(*T, P, P.env_id_base + (unsigned long long)e, state + (size_t)e * STATE);
}
// episode number of the next reset of env idx[i]: one more than the episode stored in its record (-1 = never reset)
// (also hands the floats a reset keeps -- the Panda's per-env object parameters X[12], X[13], X[15], V[15] -- to the record the env is
// re-initialised in; records cnt .. cpad - 1 repeat the last env).  sf floats per record, the episode at X[5]
__global__ void k_next_episode(const float* __restrict__ state, const int* __restrict__ idx, int cnt, int cpad, int sf, unsigned* __restrict__ ep,
                               float* __restrict__ work, const ResetKeep keep) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cpad) return;
    const float* src = state + (size_t)idx[i < cnt ? i : cnt - 1] * sf;
    ep[i] = (unsigned)((int)src[sf - 16 + 5] + 1);
    if (work != state) for (int k = 0; k < keep.n; k++) work[(size_t)i * sf + keep.slot[k]] = src[keep.slot[k]];
}
// dst[idx[i]] <- src[i], sf floats per record
__global__ void k_scatter(float* __restrict__ dst, const float* __restrict__ src, const int* __restrict__ idx, int cnt, int sf) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = t / sf, k = t % sf;
    if (i < cnt) dst[(size_t)idx[i] * sf + k] = src[(size_t)i * sf + k];
}

static thread_local std::string g_err;      // errors without a ctx (pbre_create): per calling thread (MultiEngine creates its shards from one thread per device)

int pbre::fail(pbre_ctx* c, int code, const char* msg) { (c ? c->err : g_err) = msg; return code; }

extern "C" {
__attribute__((visibility("hidden"))) void pbre_comm_release(const pbre_ctx* c);      // pbre_comm.hip: the ctx's RCCL communicator, if any
}

// ------------------------------------------------------------------ pbre_ctx: the host logic every engine shares
void pbre_ctx::destroy(pbre_ctx* c) {
    if (!c) return;
    pbre_comm_release(c);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)c->quiesce();        // (a SidePick waits for its candidate streams itself, before the engine's buffers go)
    delete c;
}

int pbre_ctx::open_device() {
    int ndev = 0;
    hipError_t he = hipGetDeviceCount(&ndev);
    if (he != hipSuccess || ndev <= 0) { err = std::string("no HIP device available (") + hipGetErrorString(he) + "); libpbre has no CPU fallback"; return PBRE_E_DEVICE; }
    if (device < 0 || device >= ndev) return fail(PBRE_E_ARG, "device_id out of range");
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(stream.out(), hipStreamNonBlocking));
    for (auto& e : ev) HIPCHK(hipEventCreate(e.out()));
    // (timing-only events around the dominant kernel: no system-scope fence at the markers)
    for (auto& pr : ev_k) for (auto& e : pr) HIPCHK(hipEventCreateWithFlags(e.out(), hipEventDisableSystemFence));
    return PBRE_OK;
}

int pbre_ctx::alloc_step_io(size_t rows) {
    HIPCHK(hipMalloc(d_act.out(), rows * act_dim * sizeof(float)));
    HIPCHK(hipMalloc(d_out.out(), rows * ow * sizeof(float)));
    return PBRE_OK;
}
int pbre_ctx::alloc_counters(size_t rows) {
    HIPCHK(hipMalloc(d_bad.out(), 2 * sizeof(int)));
    HIPCHK(hipMemset(d_bad, 0, 2 * sizeof(int)));
    P.bad_count = d_bad;
    HIPCHK(hipMalloc(d_sweeps.out(), rows * sizeof(int)));
    HIPCHK(hipMemset(d_sweeps, 0, rows * sizeof(int)));
    P.sweeps = d_sweeps;
    return PBRE_OK;
}
int pbre_ctx::alloc_reset_ids(size_t rows, size_t ids) {
    HIPCHK(hipMalloc(d_ids.out(), ids * sizeof(unsigned long long)));
    HIPCHK(hipMalloc(d_ep.out(), ids * sizeof(unsigned)));
    HIPCHK(hipMalloc(d_idx.out(), rows * sizeof(int)));
    // every record starts as a valid (un-settled) state with episode -1: the ids and episodes the engine's init kernel reads
    std::vector<unsigned long long> id0(ids, P.env_id_base); std::vector<unsigned> ep0(ids, 0xFFFFFFFFu);
    HIPCHK(hipMemcpy(d_ids, id0.data(), ids * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_ep, ep0.data(), ids * 4, hipMemcpyHostToDevice));
    return PBRE_OK;
}

// Every host-synchronous entry point starts here: all work the ctx has in flight is complete on return.  Steps enqueued on a
// caller-supplied stream (pbre_step_device) are not ordered against the ctx's own non-blocking streams, so after one of those the
// whole device is drained (these entry points are not on the hot path).
hipError_t pbre_ctx::quiesce() {
    hipError_t e;
    if (ext_dirty) {
        if ((e = hipDeviceSynchronize()) != hipSuccess) return e;
        ext_dirty = false;
        return hipSuccess;
    }
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    return drain_side();
}
// PBRE_STREAM_LEGACY: the null stream (HIP's legacy default stream; the runtime torch bundles dereferences the symbolic
// hipStreamLegacy handle, so it is passed as stream 0)
hipStream_t pbre_ctx::stream_of(void* abi) { return abi == PBRE_STREAM_LEGACY ? (hipStream_t) nullptr : (abi ? (hipStream_t)abi : (hipStream_t)stream); }

hipError_t pbre_ctx::full_step(const float* d_actions, float* d_rows, hipStream_t s) {
    const int flags = cfg.flags & (PBRE_F_NO_OBJECT | PBRE_F_AUTO_RESET);
    const int reps = cfg.action_repeat > 1 ? cfg.action_repeat : 1;
    const Params P0 = P;
    hipError_t e = hipSuccess;
    for (int r = 0; r < reps && e == hipSuccess; r++) {
        repeat_scale(P, P0, r);        // all but the last iteration only simulate, test termination and count
        e = step_repeat(r + 1 == reps, d_actions, d_rows, flags, s);
    }
    P = P0;
    return e;
}
int pbre_ctx::timed_step(const float* actions, float* out, bool za, bool zo) {
    HIPCHK(hipEventRecord(ev[0], stream));
    if (!za) HIPCHK(hipMemcpyAsync(d_act, actions, (size_t)n * act_dim * 4, hipMemcpyHostToDevice, stream));
    HIPCHK(hipEventRecord(ev[1], stream));
    HIPCHK(full_step(za ? actions : (const float*)d_act, zo ? out : (float*)d_out, stream));
    HIPCHK(hipEventRecord(ev[2], stream));
    if (!zo) HIPCHK(hipMemcpyAsync(out, d_out, (size_t)n * ow * 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipEventRecord(ev[3], stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (int i = 0; i < 3; i++) { float t = 0; HIPCHK(hipEventElapsedTime(&t, ev[i], ev[i + 1])); ms[i] = t; }
    return PBRE_OK;
}
int pbre_ctx::begin_step() {
    HIPCHK(hipSetDevice(device));
    if (ext_dirty) HIPCHK(quiesce());
    return check_stale();
}
int pbre_ctx::step_device(const float* d_actions, float* d_rows, void* abi_stream) {
    HIPCHK(hipSetDevice(device));
    if (abi_stream) ext_dirty = true;
    if (const int rc = check_stale()) return rc;
    HIPCHK(full_step(d_actions, d_rows, stream_of(abi_stream)));
    return PBRE_OK;
}
int pbre_ctx::sync() {
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    return PBRE_OK;
}
int pbre_ctx::observe(float* obs) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    launch_observe_all(stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy2DAsync(obs, (size_t)obs_dim * 4, d_out, (size_t)ow * 4, (size_t)obs_dim * 4, n, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return PBRE_OK;
}
hipError_t pbre_ctx::scatter_records(float* dst, const float* src, int cnt, int floats) {
    hipLaunchKernelGGL(k_scatter, dim3((cnt * floats + 255) / 256), dim3(256), 0, stream, dst, src, d_idx, cnt, floats);
    return hipGetLastError();
}
// The selected envs (null: all) begin their next episode: reset_sequence (pbre_reset_seq.hpp) on the batch in place or, for a part of it,
// on a compacted copy in the scratch buffer that is scattered back
int pbre_ctx::reset(const uint8_t* mask) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    std::vector<int> idx;
    for (int e = 0; e < n; e++) if (!mask || mask[e]) idx.push_back(e);
    const int cnt = (int)idx.size(), cpad = (cnt + rst_keep.pad - 1) / rst_keep.pad * rst_keep.pad;
    if (cnt == 0) return PBRE_OK;
    std::vector<unsigned long long> ids(cpad);
    for (int i = 0; i < cpad; i++) ids[i] = P.env_id_base + (unsigned long long)idx[i < cnt ? i : cnt - 1];
    HIPCHK(hipMemcpyAsync(d_ids, ids.data(), (size_t)cpad * 8, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_idx, idx.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, stream));
    // episode numbers live in the state records (the device advances them on auto-reset)
    const bool full = cnt == n;
    hipLaunchKernelGGL(k_next_episode, dim3((cpad + 127) / 128), dim3(128), 0, stream, state, d_idx, cnt, cpad, sf, d_ep, full ? state : scratch, rst_keep);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));          // host vectors go out of scope below
    if (const int rc = reset_sequence(P.robot, P.use_ik != 0, P.task, mrec, cfg.flags, [&](ResetOp op, int count, int flags) {
            const hipError_t e = reset_op(op, !full, cnt, count, flags);
            return e == hipSuccess ? PBRE_OK : hip_fail("pbre_reset", e);
        })) return rc;
    if (!full) { HIPCHK(scatter_records(state, scratch, cnt, sf)); HIPCHK(reset_scattered(cnt)); }
    HIPCHK(hipStreamSynchronize(stream));
    if (!full) return PBRE_OK;
    // snapshot for PBRE_F_AUTO_RESET: settled robot pose and object height (identical in every env)
    std::vector<float> rec(sf);
    HIPCHK(hipMemcpy(rec.data(), state, (size_t)sf * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(record_snapshot(rec.data()));
    have_snapshot = true; stale_snapshot = false;
    P.rst_ok = 0;
    if (restarts_in_kernel()) {   // the settled end-effector pose (the first 6 observation entries of env 0); valid while no env of the batch is complex
        launch_observe_all(stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        int nc = 1;
        HIPCHK(hipMemcpy(P.rst_ee, d_out, sizeof P.rst_ee, hipMemcpyDeviceToHost));
        HIPCHK(complex_now(&nc));
        P.rst_ok = nc == 0 ? 1 : 0;
    }
    return PBRE_OK;
}
int pbre_ctx::reset_snapshot(const uint8_t* mask) {
    if (!have_snapshot) return fail(PBRE_E_ARG, stale_snapshot ? stale_snapshot_msg() : "pbre_reset_snapshot: no settled snapshot yet (call pbre_reset for the whole batch first)");
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    if (!d_mask) HIPCHK(hipMalloc(d_mask.out(), (size_t)n));
    HIPCHK(hipMemcpyAsync(d_mask, mask, (size_t)n, hipMemcpyHostToDevice, stream));
    launch_snapshot_reset(d_mask, stream);
    HIPCHK(hipGetLastError());
    HIPCHK(state_changed());
    HIPCHK(hipStreamSynchronize(stream));
    return PBRE_OK;
}
int pbre_ctx::get_state(float* s) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    HIPCHK(hipMemcpy(s, state, (size_t)n * sf * 4, hipMemcpyDeviceToHost));
    return PBRE_OK;
}
int pbre_ctx::set_state(const float* s) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    HIPCHK(hipMemcpy(state, s, (size_t)n * sf * 4, hipMemcpyHostToDevice));
    HIPCHK(state_changed());
    return PBRE_OK;
}
int pbre_ctx::get_state_cols(int32_t first, int32_t count, float* out) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    HIPCHK(hipMemcpy2D(out, (size_t)count * 4, state + first, (size_t)sf * 4, (size_t)count * 4, n, hipMemcpyDeviceToHost));
    return PBRE_OK;
}
int pbre_ctx::get_sweeps(int32_t* sweeps) {
    if (!(P.res_lim > 0.f)) return fail(PBRE_E_UNSUPPORTED, "pbre_get_sweeps: pbre_physics.solver_residual_threshold is 0 (every env runs all solver_iters sweeps)");
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    HIPCHK(hipMemcpy(sweeps, d_sweeps, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    return PBRE_OK;
}
int pbre_ctx::set_physics(const pbre_physics* phys) {
    Params P2 = P;
    if (!apply_physics(*phys, P2)) return fail(PBRE_E_ARG, "bad physics parameters");
    if (const char* no = physics_objection(P2)) return fail(PBRE_E_UNSUPPORTED, no);
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    // (round-2 advice) restarts would put the object at the old scene's rest height
    if (snapshot_relevant_change(cfg.phys, *phys)) invalidate_snapshot(have_snapshot, stale_snapshot, P2);
    cfg.phys = *phys; P = P2;
    HIPCHK(state_changed());           // the contact margin may have changed
    return PBRE_OK;
}
int pbre_ctx::set_object_hull(const double* verts, int32_t n_verts) {
    HullTable H;
    const std::string e = build_hull(verts, n_verts, H);
    if (!e.empty()) return fail(PBRE_E_ARG, e.c_str());
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    if (!d_hull) HIPCHK(hipMalloc(d_hull.out(), sizeof H.data));
    HIPCHK(hipMemcpy(d_hull, H.data, sizeof H.data, hipMemcpyHostToDevice));
    apply_hull(H, d_hull, cfg, P, have_snapshot, stale_snapshot);
    HIPCHK(state_changed());
    return PBRE_OK;
}
int pbre_ctx::timing(double* out, int32_t cnt) const {
    double kd = 0.0;
    if (cnt > 3 && k_steps > 0) {      // mean over the last min(k_steps, KRING) steps
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
        const long last = std::min<long>(k_steps, KRING);
        int ok = 0;
        for (long i = 0; i < last; i++) {
            float t = 0.f;
            const Event* ek = ev_k[(k_steps - 1 - i) % KRING];
            if (hipEventElapsedTime(&t, ek[0], ek[1]) == hipSuccess) { kd += t; ok++; }
        }
        kd = ok ? kd / ok : 0.0;
    }
    for (int i = 0; i < cnt; i++) out[i] = i < 3 ? ms[i] : (i == 3 ? kd : 0.0);
    return PBRE_OK;
}
int pbre_ctx::read_bad() const {
    int bad = 0;
    if (d_bad) { (void)hipSetDevice(device); (void)hipDeviceSynchronize(); (void)hipMemcpy(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost); }
    return bad;
}
// Fills *v for a unit's kernels on `abi_stream` (as for pbre_step_device).  host_sync: a host-synchronous call -- all work of the engine
// is complete on return (then abi_stream must be null).
int pbre_ctx::state_view(StateView* v, void* abi_stream, bool host_sync) {
    HIPCHK(hipSetDevice(device));
    if (host_sync) HIPCHK(quiesce());
    else if (abi_stream) ext_dirty = true;
    v->state = state; v->stride = sf; v->n = n; v->obj_lane = lc; v->flags = cfg.flags;
    v->phys = cfg.phys; v->hull = P.obj_shape == PBRE_SHAPE_HULL ? P.hull : nullptr;
    v->stream = (void*)stream_of(abi_stream);
    return PBRE_OK;
}

// ------------------------------------------------------------------ the Panda task engine
hipError_t PandaEngine::alloc_buf(EnvBuf& b, int cap) {
    b.cap = cap;
    hipError_t e;
    // cap records + EPB pristine dummy records (read by the idle rows of the row kernels) + EPB scratch records (written by them)
    if ((e = hipMalloc(b.state.out(), (size_t)(cap + 2 * EPB) * STATE * sizeof(float))) != hipSuccess) return e;
    if ((e = hipMemset(b.state, 0, (size_t)(cap + 2 * EPB) * STATE * sizeof(float))) != hipSuccess) return e;     // k_init keeps X[12], X[13], X[15]
    if ((e = hipMalloc(b.cls.out(), (size_t)2 * cap)) != hipSuccess) return e;
    if ((e = hipMalloc(b.tgt.out(), (size_t)(cap + EPB) * NJ * sizeof(float))) != hipSuccess) return e;
    if ((e = hipMemset(b.tgt, 0, (size_t)(cap + EPB) * NJ * sizeof(float))) != hipSuccess) return e;
    if ((e = hipMemset(b.cls, 0, (size_t)2 * cap)) != hipSuccess) return e;
    for (int k = 0; k < 2; k++) if ((e = hipMalloc(b.list[k].out(), (size_t)NB * cap * sizeof(int))) != hipSuccess) return e;
    if ((e = hipMalloc(b.count.out(), (3 * NB + 2) * sizeof(int))) != hipSuccess) return e;      // + the device copy of the "recent" hint
    if ((e = hipMalloc(b.objv_g.out(), (size_t)(cap + 32) * W * sizeof(float))) != hipSuccess) return e;
    if ((e = hipMemset(b.objv_g, 0, (size_t)(cap + 32) * W * sizeof(float))) != hipSuccess) return e;
    if ((e = hipMalloc(b.pair_g.out(), (size_t)((cap + FTPB - 1) / FTPB) * PBRE_PAIR_G_BYTES)) != hipSuccess) return e;
    if ((e = hipMemset(b.pair_g, 0, (size_t)((cap + FTPB - 1) / FTPB) * PBRE_PAIR_G_BYTES)) != hipSuccess) return e;
    if ((e = hipHostMalloc(b.h_total.out(), 2 * sizeof(int), hipHostMallocDefault)) != hipSuccess) return e;
    b.h_total[0] = 1; b.h_total[1] = 16;   // unknown until the first step has run
    return hipMemset(b.count, 0, (3 * NB + 2) * sizeof(int));
}

hipError_t PandaEngine::classify(EnvBuf& b, int cnt, int flags, hipStream_t s) {
    if (!lane_per_env(this)) return hipSuccess;
    hipError_t e = hipMemsetAsync(b.count + b.ccur * NB, 0, NB * sizeof(int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_classify, dim3((cnt + FTPB - 1) / FTPB), dim3(FTPB), 0, s, dFT, P, b.state, cnt, flags, b.cls + (size_t)b.cur * b.cap, b.list[b.cur], b.count + b.ccur * NB, b.cap);
    hipLaunchKernelGGL(k_total, dim3(1), dim3(1), 0, s, b.count + b.ccur * NB, b.h_total, b.count + 3 * NB);
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) return le;
    // The complex-env count k_total just wrote is what the next launch_step sizes its complex-env kernel by.  Every caller is a
    // host-synchronous entry point off the hot path (reset, set_state, settle, set_physics), so wait for it: launched against the count
    // of an EARLIER state, a batch that has just become entirely complex (IK control: the home hand pose's IK solution lies beyond
    // joint 4's limit) was walked by an 8-block row kernel -- 11 ms per launch at 16384 envs, 19 s per reset at 131072.
    return hipStreamSynchronize(s);
}

template <int MODE>
static hipError_t launch_step(PandaEngine* c, EnvBuf& b, int n, const float* act, float* out, int flags, hipStream_t s) {
    return c->P.res_lim > 0.f ? launch_step_t<MODE, true>(c, b, n, act, out, flags, s) : launch_step_t<MODE, false>(c, b, n, act, out, flags, s);
}

// settle steps (hold motors; IK mode: hold the IK targets)
hipError_t PandaEngine::settle_steps(EnvBuf& b, int cnt, int count, int flags, hipStream_t s) {
    for (int i = 0; i < count; i++) {
        hipError_t e = P.use_ik ? launch_step<MODE_SETTLE_IK>(this, b, cnt, nullptr, nullptr, flags, s) : launch_step<0>(this, b, cnt, nullptr, nullptr, flags, s);
        if (e != hipSuccess) return e;
        // (a settle loop is host-synchronous anyway: every 16 launches let the device catch up, so that the complex-env count the next
        // launches are sized and scheduled by is at most 16 steps old)
        if ((i & 15) == 15 && (e = hipStreamSynchronize(s)) != hipSuccess) return e;
    }
    return hipSuccess;
}
hipError_t PandaEngine::step_repeat(bool last, const float* d_actions, float* d_rows, int flags, hipStream_t s) {
    if (!P.use_ik)
        return last ? launch_step<MODE_STEP>(this, main, n, d_actions, d_rows, flags, s) : launch_step<MODE_INNER>(this, main, n, d_actions, nullptr, flags, s);
    hipLaunchKernelGGL(k_ik<false>, dim3((n + FTPB - 1) / FTPB), dim3(FTPB), 0, s, dFT, P, main.state, d_actions, main.tgt, n, act_dim);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return last ? launch_step<MODE_STEP_IK>(this, main, n, nullptr, d_rows, flags, s) : launch_step<MODE_INNER_IK>(this, main, n, nullptr, nullptr, flags, s);
}
void PandaEngine::launch_observe_all(hipStream_t s) {
    hipLaunchKernelGGL(k_observe, dim3(npad / EPB), dim3(TPB), 0, s, dT, P, main.state, d_out, d_scratch, n, ow);
}
void PandaEngine::launch_snapshot_reset(const unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_snapshot_reset, dim3((n + 127) / 128), dim3(128), 0, s, dT, P, main.state, mask, n);
}

// the model constants in both layouts: `Tables` for the row kernels, its per-joint packing for the lane-per-env ones (one source: T)
hipError_t PandaEngine::upload_tables() {
    fast_tables(T, FT);
    const hipError_t e = hipMemcpy(dT, &T, sizeof(Tables), hipMemcpyHostToDevice);
    return e != hipSuccess ? e : hipMemcpy(dFT, &FT, sizeof(FTables), hipMemcpyHostToDevice);
}

int PandaEngine::init(const pbre_config& c) {
    cfg = c;
    const std::string e = make_tables<Shape16>(c, T, P);
    if (!e.empty()) return fail(table_error_code(e), e.c_str());
    cfg.robot_table = nullptr;
    n = c.num_envs; npad = ceil16(n); obs_dim = obs_dim_of(T, P); act_dim = act_dim_of(c);
    ow = obs_dim + 2; device = c.device_id; sf = STATE; lc = LC;
    fast_ok = topo_matches<TopoPanda>(T) && fast_scene_ok(P);
    knobs = StepKnobs::from_env();       // A/B knobs
    main.objv_seq = tmp.objv_seq = knobs.objv_seq0;      // (tests: start k_fused's sequence numbers next to their wrap)
    if (const int rc = open_device()) return rc;
    { hipDeviceProp_t pr; HIPCHK(hipGetDeviceProperties(&pr, device)); n_simd = std::max(1, pr.multiProcessorCount * 4); }
    HIPCHK(sp.create(0, false));
    side = sp.side;
    {   // fork / join of the two step kernels: both ends are on this GPU, so the events need no system-scope fence (cache write-back
        // and invalidate at every marker); PBRE_EVENT_FENCE=1 keeps it (A/B)
        const char* ef = getenv("PBRE_EVENT_FENCE");
        const unsigned fl = hipEventDisableTiming | ((ef && ef[0] == '1') ? 0u : (unsigned)hipEventDisableSystemFence);
        HIPCHK(hipEventCreateWithFlags(ev_fork.out(), fl));
        HIPCHK(hipEventCreateWithFlags(ev_join.out(), fl));
        HIPCHK(hipEventCreateWithFlags(ev_join_sys.out(), hipEventDisableTiming));
    }
    HIPCHK(hipMalloc(dT.out(), sizeof(Tables)));
    HIPCHK(hipMalloc(dFT.out(), sizeof(FTables)));
    HIPCHK(upload_tables());
    HIPCHK(alloc_buf(main, npad));
    HIPCHK(alloc_buf(tmp, npad));
    state = main.state; scratch = tmp.state;
    rst_keep = {EPB, 4, {44, 45, 47, 31}};      // groups of 16 records; the per-env object parameters X[12], X[13], X[15] and V[15] (pbre_set_physics_per_env)
    if (const int rc = alloc_step_io((size_t)npad)) return rc;
    HIPCHK(hipMalloc(d_scratch.out(), 64 * sizeof(float)));
    if (const int rc = alloc_counters((size_t)npad)) return rc;
    // every record of both buffers (incl. padding and dummy records) must hold a valid state: the un-settled reset pose
    const int tot = npad + EPB;
    if (const int rc = alloc_reset_ids((size_t)npad, (size_t)tot)) return rc;
    hipLaunchKernelGGL(k_init, dim3((tot + 127) / 128), dim3(128), 0, stream, dT, P, main.state, d_ids, d_ep, tot);
    hipLaunchKernelGGL(k_init, dim3((tot + 127) / 128), dim3(128), 0, stream, dT, P, tmp.state, d_ids, d_ep, tot);
    HIPCHK(hipGetLastError());
    HIPCHK(state_changed());
    HIPCHK(hipStreamSynchronize(stream));
    return PBRE_OK;
}

int PandaEngine::settle(int32_t count, int32_t flags) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    const int f = flags & PBRE_F_NO_OBJECT, f0 = cfg.flags & PBRE_F_NO_OBJECT;
    if (f != f0) HIPCHK(classify(main, n, f, stream));           // classes depend on whether the object is present
    HIPCHK(settle_steps(main, n, count, f, stream));
    if (f != f0) HIPCHK(classify(main, n, f0, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return PBRE_OK;
}

// reset(): reset_sequence's operations on the first cnt envs of `main` or `tmp` (k_init / k_target: whole groups of 16 records)
hipError_t PandaEngine::reset_op(ResetOp op, bool in_scratch, int cnt, int count, int flags) {
    EnvBuf& b = in_scratch ? tmp : main;
    const int cpad = ceil16(cnt);
    if (op == RS_INIT) hipLaunchKernelGGL(k_init, dim3((cpad + 127) / 128), dim3(128), 0, stream, dT, P, b.state, d_ids, d_ep, cpad);
    if (op == RS_HOME_IK) hipLaunchKernelGGL(k_ik<true>, dim3((cnt + FTPB - 1) / FTPB), dim3(FTPB), 0, stream, dFT, P, b.state, (const float*)nullptr, b.tgt, cnt, act_dim);
    if (op == RS_TARGETS) hipLaunchKernelGGL(k_target, dim3((cpad + 127) / 128), dim3(128), 0, stream, P, b.state, d_ids, d_ep, cpad);
    hipError_t e = hipGetLastError();
    // classes depend on whether the object is present: built for the fresh records (the robot alone) and again when a run of steps changes it
    const int cf = op == RS_INIT ? PBRE_F_NO_OBJECT : flags;
    if (e == hipSuccess && (op == RS_INIT || (op == RS_SETTLE && cf != rst_cls_flags))) { rst_cls_flags = cf; e = classify(b, cnt, cf, stream); }
    return (e == hipSuccess && op == RS_SETTLE) ? settle_steps(b, cnt, count, flags, stream) : e;
}
hipError_t PandaEngine::record_snapshot(const float* rec) {
    for (int k = 0; k < NJ; k++) { P.rst_q[k] = rec[k]; T.rst_q[k] = rec[k]; }
    P.rst_objz = rec[11];
    return upload_tables();
}
hipError_t PandaEngine::complex_now(int* count) {
    int cn[NB] = {0};
    const hipError_t e = lane_per_env(this) ? hipMemcpy(cn, main.count + main.ccur * NB, sizeof cn, hipMemcpyDeviceToHost) : hipSuccess;
    *count = 0;
    for (int k = 0; k < NB; k++) *count += cn[k];
    return e;
}
int PandaEngine::reset(const uint8_t* mask) {
    const int rc = pbre_ctx::reset(mask);
    k_steps = 0; launches = 0; launches3 = 0; launches_pair = 0; launches_fused = 0; launches_tail = 0;      // pbre_timing[3] averages env steps only, not the settle launches above
    return rc;
}

int PandaEngine::step(const float* actions, float* out) {
    if (const int rc = begin_step()) return rc;
    // zero-copy (PBRE_ZERO_COPY bit 0: actions, bit 1: rows): a page-locked buffer (pbre_host_alloc) is accessed by the kernels
    // themselves, over PCIe, instead of being staged through HBM with a copy
    bool za = false, zo = false;
    if (knobs.zero_copy) {
        hipPointerAttribute_t pa;
        za = (knobs.zero_copy & 1) && hipPointerGetAttributes(&pa, actions) == hipSuccess && pa.type == hipMemoryTypeHost;
        zo = (knobs.zero_copy & 2) && hipPointerGetAttributes(&pa, out) == hipSuccess && pa.type == hipMemoryTypeHost;
        (void)hipGetLastError();
    }
    rows_to_host = zo;
    const int rc = timed_step(actions, out, za, zo);
    rows_to_host = false;
    return rc;
}

// ---- the pipelined host path (SURVEY 8(d)'s literal metric: action upload + kernels + row download).  pbre_step is host-synchronous: upload,
// kernels and download of ONE step follow each other (or, zero-copy, the kernels reach over PCIe themselves and are stretched by it:
// 0.44 ms instead of 0.15 at 131072 envs).  Here the three run on three streams with two buffer slots, so that in an open loop the DMA
// engines download the rows of step t (18.4 MB at 131072 envs: the PCIe floor, ~0.33 ms) while the kernels of step t + 1 run and the
// actions of step t + 2 come up.  Same kernels, same order per env: rows bit-equal to pbre_step's.
// rows out by a copy KERNEL (PBRE_ASYNC_D2H=1; A/B): coalesced 16-byte stores into the page-locked host buffer from a few waves on the
// download stream.  Measured (profiles/r06k_host_async_probe.txt): 54 GB/s alone, but beside k_fused -- which holds every wave slot -- the
// pipelined step is 0.56 ms against 0.47 with the DMA engine (hipMemcpyAsync, the default: 55 GB/s and no wave slots)
extern "C" __global__ __launch_bounds__(256) void k_rows_out(const float4* __restrict__ src, float4* __restrict__ dst, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
int PandaEngine::async_setup() {
    if (ap.ready) return PBRE_OK;
    for (int b = 0; b < 2; b++) {
        HIPCHK(hipMalloc(ap.d_act[b].out(), (size_t)n * act_dim * 4));
        HIPCHK(hipMalloc(ap.d_rows[b].out(), (size_t)n * ow * 4));
        for (Event* e : {&ap.ev_step[b], &ap.ev_out[b]}) HIPCHK(hipEventCreateWithFlags(e->out(), hipEventDisableTiming));
    }
    if (const char* e = getenv("PBRE_ASYNC_BLOCKS")) async_blocks = std::max(1, atoi(e));
    ap.ready = true;
    return PBRE_OK;
}
int PandaEngine::step_async(const float* actions, float* out) {
    HIPCHK(hipSetDevice(device));
    if (const int rc = check_stale()) return rc;
    if (const int rc = async_setup()) return rc;
    AsyncPath& A = ap;
    if (A.issued - A.waited >= 2) return fail(PBRE_E_ARG, "pbre_step_async: two steps are in flight already -- pbre_step_wait first");
    if (ext_dirty) HIPCHK(quiesce());
    const int b = (int)(A.issued & 1);
    hipStream_t dl = sp.pick(stream);      // the stream that really runs beside the ctx's
    // upload (in stream order: the step that last read this slot's action buffer is two steps back on the same stream), then the step --
    // behind the download that last read this slot's row buffer
    HIPCHK(hipMemcpyAsync(A.d_act[b], actions, (size_t)n * act_dim * 4, hipMemcpyHostToDevice, stream));
    if (A.issued >= 2) HIPCHK(hipStreamWaitEvent(stream, A.ev_out[b], 0));
    // PBRE_ASYNC_D2H: how the rows reach the host buffer -- 0 the DMA engine (hipMemcpyAsync), 1 a copy kernel on the download stream, 2 the
    // step kernels write them into the page-locked buffer themselves (pbre_step's zero-copy, minus its host synchronisation)
    static const int d2h_mode = [] { const char* e = getenv("PBRE_ASYNC_D2H"); return e ? atoi(e) : 0; }();
    const size_t bytes = (size_t)n * ow * 4;
    bool host_mapped = false;
    if (d2h_mode != 0) {
        hipPointerAttribute_t pa;
        host_mapped = hipPointerGetAttributes(&pa, out) == hipSuccess && pa.type == hipMemoryTypeHost;
        (void)hipGetLastError();
    }
    const bool direct = d2h_mode == 2 && host_mapped;
    rows_to_host = direct;
    const hipError_t fe = full_step(A.d_act[b], direct ? out : (float*)A.d_rows[b], stream);
    rows_to_host = false;
    HIPCHK(fe);
    HIPCHK(hipEventRecord(A.ev_step[b], stream));
    // download
    HIPCHK(hipStreamWaitEvent(dl, A.ev_step[b], 0));
    if (!direct) {
        const bool mapped = d2h_mode == 1 && (bytes % 16) == 0 && ((uintptr_t)out % 16) == 0 && host_mapped;
        if (mapped) {
            hipLaunchKernelGGL(k_rows_out, dim3(async_blocks), dim3(256), 0, dl, (const float4*)(float*)A.d_rows[b], (float4*)out, bytes / 16);
            HIPCHK(hipGetLastError());
        } else HIPCHK(hipMemcpyAsync(out, A.d_rows[b], bytes, hipMemcpyDeviceToHost, dl));
    }
    HIPCHK(hipEventRecord(A.ev_out[b], dl));
    A.issued++;
    return PBRE_OK;
}
int PandaEngine::step_wait() {
    AsyncPath& A = ap;
    if (!A.ready || A.waited >= A.issued) return fail(PBRE_E_ARG, "pbre_step_wait: no step in flight");
    HIPCHK(hipSetDevice(device));
    // (poll the slot's event: hipEventSynchronize returned only once the NEWER download enqueued on the same stream was done too -- the
    // pipeline then runs one step deep)
    for (;;) {
        const hipError_t q = hipEventQuery(A.ev_out[A.waited & 1]);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) return hip_fail("hipEventQuery", q);
        for (int i = 0; i < 64; i++) __builtin_ia32_pause();
    }
    (void)hipGetLastError();
    A.waited++;
    return PBRE_OK;
}

int PandaEngine::set_physics_per_env(const uint8_t* mask, const float* obj_mass, const float* obj_mu, const float* obj_lin_damping, const float* robot_lin_damping) {
    for (int e = 0; e < n; e++) {
        if (mask && !mask[e]) continue;
        if ((obj_mass && !(obj_mass[e] > 0.f)) || (obj_mu && !(obj_mu[e] > 0.f)) || (obj_lin_damping && !(obj_lin_damping[e] >= 0.f)) ||
            (robot_lin_damping && !(robot_lin_damping[e] >= 0.f)))
            return fail(PBRE_E_ARG, "pbre_set_physics_per_env: mass and friction must be > 0, damping >= 0");
    }
    HIPCHK(hipSetDevice(device));
    HIPCHK(quiesce());
    // strided columns of the state records: X[12] mass, X[13] lateral friction, X[15] 1 + linear damping of the object, V[15] 1 + linear
    // damping of the robot's links (0 = batch value)
    std::vector<float> col((size_t)n);
    const float* src[4] = {obj_mass, obj_mu, obj_lin_damping, robot_lin_damping};
    const int slot[4] = {44, 45, 47, 31};
    for (int k = 0; k < 4; k++) {
        if (!src[k]) continue;
        HIPCHK(hipMemcpy2D(col.data(), 4, state + slot[k], (size_t)STATE * 4, 4, n, hipMemcpyDeviceToHost));
        for (int e = 0; e < n; e++) if (!mask || mask[e]) col[e] = src[k][e] + (k >= 2 ? 1.f : 0.f);
        HIPCHK(hipMemcpy2D(state + slot[k], (size_t)STATE * 4, col.data(), 4, 4, n, hipMemcpyHostToDevice));
    }
    return PBRE_OK;
}

int PandaEngine::kernel_info(int32_t* info, int32_t cnt) const {
    hipFuncAttributes fa;
    int rf = -1, rg = -1, rr = -1, rf3 = -1, rp = -1, ru = -1;
    if (hipFuncGetAttributes(&fa, (const void*)k_fused<MODE_STEP, false>) == hipSuccess) ru = fa.numRegs;
    if (hipFuncGetAttributes(&fa, (const void*)k_fused<MODE_STEP, true>) == hipSuccess) ru = std::max(ru, (int)fa.numRegs);
    if (hipFuncGetAttributes(&fa, (const void*)k_fast<MODE_STEP, 3>) == hipSuccess) rf3 = fa.numRegs;
    if (hipFuncGetAttributes(&fa, (const void*)k_fast_pair<MODE_STEP>) == hipSuccess) rp = fa.numRegs;
    if (hipFuncGetAttributes(&fa, (const void*)k_fast<MODE_STEP, 2>) == hipSuccess) rf = fa.numRegs;
    if (hipFuncGetAttributes(&fa, (const void*)k_step<MODE_STEP>) == hipSuccess) rg = fa.numRegs;
    if (hipFuncGetAttributes(&fa, (const void*)k_fast_rc<MODE_STEP>) == hipSuccess) rr = fa.numRegs;
    int complex_now = 0, complex_sum = 0;       // envs whose current state is "complex" (what the next step's k_fast_rc will take)
    const bool lpe = lane_per_env(this);
    if (lpe) {
        (void)hipSetDevice(device); (void)hipDeviceSynchronize();
        (void)const_cast<PandaEngine*>(this)->complex_now(&complex_now);
        (void)hipMemcpy(&complex_sum, main.count + 3 * NB + 1, sizeof(int), hipMemcpyDeviceToHost);
    }
    const int bad = read_bad();
    const int v[16] = {lpe ? rf : -1, rg, lpe ? 1 : 0, lpe ? n - complex_now : 0, lpe ? 0 : n, complex_now, lpe ? rr : -1, complex_sum,
                       (int)(launches3 & 0x7fffffff), lpe ? rf3 : -1, (int)(launches_pair & 0x7fffffff), lpe ? rp : -1, bad,
                       (int)(launches_fused & 0x7fffffff), lpe ? ru : -1, (int)(launches_tail & 0x7fffffff)};
    for (int i = 0; i < cnt; i++) info[i] = i < 16 ? v[i] : 0;
    return PBRE_OK;
}

// ------------------------------------------------------------------ the C-ABI: argument checks and one call
extern "C" {

int pbre_default_config(pbre_config* cfg, int32_t robot, int32_t task) { return default_config(cfg, robot, task); }

void pbre_destroy(pbre_ctx* c) { pbre_ctx::destroy(c); }

int pbre_create(const pbre_config* cfg, pbre_ctx** out) {
    if (!cfg || !out) { g_err = "null argument"; return PBRE_E_ARG; }
    *out = nullptr;
    // iCub shapes, and the robot-level interface (motor records) of either robot: the lane-group engines
    pbre_ctx* c = (table_ndof(*cfg) > NJ || cfg->robot_level) ? new_lane_group_engine(*cfg) : new PandaEngine();
    const int rc = c->init(*cfg);
    if (rc != PBRE_OK) { g_err = c->err; pbre_ctx::destroy(c); return rc; }
    c->readers.set_table(cfg->robot_table, cfg->robot_table_len);      // (the engines keep lane tables only)
    *out = c;
    return PBRE_OK;
}

const char* pbre_last_error(const pbre_ctx* c) { return c ? c->err.c_str() : g_err.c_str(); }

int pbre_dims(const pbre_ctx* c, int32_t* od, int32_t* ad, int32_t* n) {
    if (!c) return PBRE_E_ARG;
    if (od) *od = c->obs_dim;
    if (ad) *ad = c->act_dim;
    if (n) *n = c->n;
    return PBRE_OK;
}
int pbre_state_floats(const pbre_ctx* c) { return c ? c->sf : PBRE_E_ARG; }
int pbre_sync(pbre_ctx* c) { return c ? c->sync() : PBRE_E_ARG; }
int pbre_observe(pbre_ctx* c, float* obs) { return (c && obs) ? c->observe(obs) : PBRE_E_ARG; }
int pbre_settle(pbre_ctx* c, int32_t n, int32_t flags) { return (c && n >= 0) ? c->settle(n, flags) : PBRE_E_ARG; }
int pbre_reset(pbre_ctx* c, const uint8_t* mask, float* obs) {
    if (!c) return PBRE_E_ARG;
    const int rc = c->reset(mask);
    return (rc == PBRE_OK && obs) ? c->observe(obs) : rc;
}
int pbre_reset_snapshot(pbre_ctx* c, const uint8_t* mask, float* obs) {
    if (!c || !mask) return PBRE_E_ARG;
    const int rc = c->reset_snapshot(mask);
    return (rc == PBRE_OK && obs) ? c->observe(obs) : rc;
}
int pbre_step_device(pbre_ctx* c, const float* d_actions, float* d_out, void* stream) { return (c && d_actions && d_out) ? c->step_device(d_actions, d_out, stream) : PBRE_E_ARG; }
int pbre_step(pbre_ctx* c, const float* actions, float* out) { return (c && actions && out) ? c->step(actions, out) : PBRE_E_ARG; }
int pbre_step_async(pbre_ctx* c, const float* actions, float* out) { return (c && actions && out) ? c->step_async(actions, out) : PBRE_E_ARG; }
int pbre_step_wait(pbre_ctx* c) { return c ? c->step_wait() : PBRE_E_ARG; }
int pbre_get_state(pbre_ctx* c, float* s) { return (c && s) ? c->get_state(s) : PBRE_E_ARG; }
int pbre_set_state(pbre_ctx* c, const float* s) { return (c && s) ? c->set_state(s) : PBRE_E_ARG; }
int pbre_get_state_cols(pbre_ctx* c, int32_t first, int32_t count, float* out) {
    return (c && out && first >= 0 && count > 0 && first + count <= c->sf) ? c->get_state_cols(first, count, out) : PBRE_E_ARG;
}
void* pbre_host_alloc(size_t bytes) {
    void* p = nullptr;
    // PBRE_HOST_NONCOHERENT=1 (A/B with PBRE_ZERO_COPY): coarse-grained host memory, device writes are cached in L2 and written back at
    // the end of the kernel in full lines instead of going out as they are issued
    const char* nc = getenv("PBRE_HOST_NONCOHERENT");
    const unsigned flags = (nc && nc[0] == '1') ? (hipHostMallocNonCoherent | hipHostMallocMapped) : hipHostMallocDefault;
    return hipHostMalloc(&p, bytes ? bytes : 1, flags) == hipSuccess ? p : nullptr;
}
void pbre_host_free(void* p) { if (p) (void)hipHostFree(p); }

int pbre_set_motors(pbre_ctx* c, int32_t n, const int32_t* dofs, const float* targets, double kp, double max_force, double max_vel, const uint8_t* mask) {
    return (c && n >= 0 && !(n > 0 && (!dofs || !targets))) ? c->set_motors(n, dofs, targets, kp, max_force, max_vel, mask) : PBRE_E_ARG;
}
int pbre_apply_action(pbre_ctx* c, const float* actions, double max_vel) { return (c && actions) ? c->apply_action(actions, max_vel) : PBRE_E_ARG; }
int pbre_get_motor_state(pbre_ctx* c, float* m) { return (c && m) ? c->motor_state(m, nullptr) : PBRE_E_ARG; }
int pbre_set_motor_state(pbre_ctx* c, const float* m) { return (c && m) ? c->motor_state(nullptr, m) : PBRE_E_ARG; }
int pbre_get_physics(const pbre_ctx* c, pbre_physics* phys) {
    if (!c || !phys) return PBRE_E_ARG;
    *phys = c->cfg.phys;
    return PBRE_OK;
}
int pbre_get_sweeps(pbre_ctx* c, int32_t* sweeps) { return (c && sweeps) ? c->get_sweeps(sweeps) : PBRE_E_ARG; }
int pbre_set_physics(pbre_ctx* c, const pbre_physics* phys) { return (c && phys) ? c->set_physics(phys) : PBRE_E_ARG; }
int pbre_set_object_hull(pbre_ctx* c, const double* verts, int32_t n_verts) { return c ? c->set_object_hull(verts, n_verts) : PBRE_E_ARG; }
int pbre_set_physics_per_env(pbre_ctx* c, const uint8_t* mask, const float* obj_mass, const float* obj_mu, const float* obj_lin_damping,
                             const float* robot_lin_damping) {
    return c ? c->set_physics_per_env(mask, obj_mass, obj_mu, obj_lin_damping, robot_lin_damping) : PBRE_E_ARG;
}
int pbre_obs_limits(const pbre_ctx* c, float* lo, float* hi) {
    if (!c || !lo || !hi) return PBRE_E_ARG;
    c->limits(lo, hi);
    return PBRE_OK;
}
int pbre_timing(const pbre_ctx* c, double* ms, int32_t n) { return (c && ms) ? c->timing(ms, n) : PBRE_E_ARG; }
int pbre_kernel_info(const pbre_ctx* c, int32_t* info, int32_t n) { return (c && info) ? c->kernel_info(info, n) : PBRE_E_ARG; }

#ifdef PBRE_PHASE_PROBE
int pbre_debug_probe(unsigned long long* out, int reset) {      // (probe builds only; not part of include/pbre.h)
    unsigned long long z[64] = {0};
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_probe), sizeof z) != hipSuccess) return -1;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_probe), z, sizeof z) != hipSuccess) return -1;
    return 0;
}
#endif

}  // extern "C"
