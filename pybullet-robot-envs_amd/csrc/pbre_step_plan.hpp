// pbre_step_plan.hpp -- how the Panda engine launches one batched step: the A/B knobs (StepKnobs), what the decision reads (StepQuery),
// the decision (StepPlan) and the pure function between them (plan_step).  No HIP in here: launch_step_t (pbre_panda.hpp) fills the query,
// calls plan_step and executes the plan -- launches, events, counters -- and tests/step_plan_host compiles this header with the host
// compiler alone, so every rule below is pinned by tests/test_step_plan_host.py without a GPU.  Every rule was paid for with a measurement.
#pragma once
#include <algorithm>
#include <cstdlib>
#include "../../include/pbre.h"

namespace pbre {

// the step kernels' block shapes the grids below are counted in (pbre_panda.hpp asserts that they are its own)
constexpr int PLAN_FTPB = 64;             // lane-per-env kernels: one wave per block, 64 envs
constexpr int PLAN_REPB = 12;             // envs per row block (three row waves of four envs + the object wave)
constexpr int PLAN_FUSED_WAVES = 4;       // waves of a row block
constexpr int PLAN_RTPB = PLAN_FUSED_WAVES * PLAN_FTPB;
constexpr int PLAN_PTPB = 2 * PLAN_FTPB;  // k_fast_pair: robot wave + object wave

// The A/B knobs of the Panda engine (environment variables PBRE_<NAME>, read once per engine: PandaEngine::init).
struct StepKnobs {
    int rc_first_min = 1;              // complex envs (reported by the device) from which their kernel is scheduled ahead of k_fast
    int idle_touch = 16;               // in that mode, an (empty) fork / join through the side stream every idle_touch-th step: a side stream
                                       // left idle for hundreds of steps makes the first steps after the switch back ~8 % slower (0: never)
    int idle_single = 1;               // with no complex envs reported, both kernels go to the caller's stream in order (no fork / join events); 0: A/B
    int row_max = 4096;                // up to this many complex envs they are stepped by the row kernel (1 wave per 4 envs)
    int pair = 2;                      // k_fast_pair (robot wave + object wave per 64 envs): 0 never, 1 whenever it applies, 2 while its waves fit two per SIMD (PBRE_PAIR)
    int tail_pair = 0;                 // k_fused's 64-thread grid: the chunks the row waves displace into a second round as robot / object wave pairs (PBRE_TAIL_PAIR: 0 never,
                                       // 1 by the hint, n > 1: always the last n chunks -- tests).  Measured (profiles/r06s_final_structure_ab.txt, r06t_bench_tail_pairs_by_hint.json):
                                       // by the hint the stationary mix at 131072 envs gains 1.3 % (0.1494 -> 0.1476 ms) and a batch with FEW complex envs -- synchronised
                                       // episode clocks, ~30 per step -- loses 34 % (0.091 -> 0.122: two dozen pairs at the end of the grid start when the first round ends): off
    int fast3 = 2;                     // k_fast variant limited to 3 waves per SIMD: 0 never, 1 whenever complex envs are reported, 2 when they would displace k_fast waves (PBRE_FAST3)
                                       // -- only where the step is NOT one fused launch (PBRE_FUSED=0, residual exit, action_repeat's inner steps).  (Round 5 also measured the
                                       // spill-free build in two half-grid launches back to back, one wave per SIMD each: 0.21 ms against 0.177, profiles/r05_fast3_halves_ab.txt.)
    int fused = 1;                     // the step as ONE launch (k_fused: row-list blocks + fast / pair blocks in one grid); 0: the two kernels on two streams (PBRE_FUSED)
    int ksample = 8;                   // every ksample-th launch is sampled into ev_k, on the stream the dominant kernel runs on (PBRE_KSAMPLE: A/B of the sampling interval)
    int zero_copy = 3;                 // PBRE_ZERO_COPY: pbre_step lets the kernels access page-locked host buffers directly (bit 0 actions, bit 1 rows; 0: staged copies)
    int objv_seq0 = 0;                 // PBRE_OBJV_SEQ0 (tests): start k_fused's sequence numbers here, next to their wrap

    static StepKnobs from_env() {
        StepKnobs k;
        if (const char* ev = getenv("PBRE_RC_FIRST_MIN")) k.rc_first_min = atoi(ev);
        if (const char* ev = getenv("PBRE_IDLE_SINGLE")) k.idle_single = atoi(ev);
        if (const char* ev = getenv("PBRE_KSAMPLE")) k.ksample = std::max(1, atoi(ev));
        if (const char* ev = getenv("PBRE_IDLE_TOUCH")) k.idle_touch = atoi(ev);
        if (const char* ev = getenv("PBRE_ROW_MAX")) k.row_max = atoi(ev);
        if (const char* ev = getenv("PBRE_FAST3")) k.fast3 = atoi(ev);
        if (const char* ev = getenv("PBRE_FUSED")) k.fused = atoi(ev);
        if (const char* ev = getenv("PBRE_OBJV_SEQ0")) k.objv_seq0 = atoi(ev);
        if (const char* ev = getenv("PBRE_PAIR")) k.pair = atoi(ev);
        if (const char* ev = getenv("PBRE_TAIL_PAIR")) k.tail_pair = atoi(ev);      // (0: A/B; n > 1: tests -- always the last n chunks)
        if (const char* ev = getenv("PBRE_ZERO_COPY")) k.zero_copy = atoi(ev);
        return k;
    }
};

// Everything the decision reads, as launch_step_t<MODE, RT> finds it when a step is enqueued.
struct StepQuery {
    int n = 0;                         // envs of the step
    int n_simd = 1024;                 // SIMDs of the device
    int nb = 2;                        // complex-env bucket lists (NB = NCLASS - 1)
    int hint = 0;                      // h_total[0]: complex envs of the last step the DEVICE has finished (report_hint)
    int recent = 0;                    // h_total[1]: 16 while there were any, counting down by one per step once there are none
    int cfg_flags = 0, step_flags = 0; // pbre_config.flags / the flags of this step (PBRE_F_*)
    bool rt = false;                   // residual-exit variants of the kernels
    bool inner = false;                // MODE & M_INNER: a non-final iteration of action_repeat > 1
    bool fusable = true;               // k_fused exists for this MODE: NB <= 2 && (MODE == MODE_STEP || MODE == 0)
    bool obj_iso = true;               // Params::obj_iso, obj_shape (PBRE_SHAPE_*)
    int obj_shape = 0;
    int action_repeat = 1;
    bool have_pair_g = true;           // the buffer has the tail pairs' global records
    long launches = 0;                 // the engine's launch counter BEFORE this step
};

struct StepPlan {
    // FUSED_PAIR: k_fused<MODE, true>, 256-thread blocks; FUSED_64: k_fused<MODE, false, RT>, FUSED_64_TAIL: k_fused<MODE, false, false, true>,
    // 64-thread blocks; TWO_KERNELS: the complex envs' kernel (k_row_list / k_fast_rc) and the simple envs' (k_fast_pair / k_fast<3> / k_fast<2>)
    enum Form { FUSED_PAIR = 0, FUSED_64 = 1, FUSED_64_TAIL = 2, TWO_KERNELS = 3 };
    Form form = TWO_KERNELS;
    bool rows = false;                 // the complex envs go to the row kernel (else k_fast_rc)
    bool pair = false;                 // the simple envs in the pair mapping
    int rblocks = 0;                   // row blocks (k_row_list's grid; k_fused's first blocks)
    int ntail = 0;                     // FUSED_64*: tail pairs
    // TWO_KERNELS only (false in the fused forms):
    bool fast3 = false;                // k_fast<MODE, 3> (decided whether or not `pair` overrides it: only a k_fast step counts as a 3-wave step)
    bool single = false;               // both kernels in order on the caller's stream
    bool rc_first = false;             // the complex envs' kernel is scheduled ahead of k_fast
    bool touch_side = false;           // single, and yet an (empty) fork / join through the side stream
    bool rc_on_caller = false, fast_on_caller = false;      // which kernel gets the caller's stream (the other: the side stream)
    bool fork_join = false;            // the fork / join events are needed
    // grids: blocks x threads of the one launch, or of the two
    int grid_fused = 0, threads_fused = 0;
    int grid_rc = 0, threads_rc = 0;
    int grid_fast = 0, threads_fast = 0;
};

inline StepPlan plan_step(const StepKnobs& k, const StepQuery& q) {
    StepPlan p;
    const int FTPB = PLAN_FTPB, REPB = PLAN_REPB, FUSED_WAVES = PLAN_FUSED_WAVES;
    const int blocks = (q.n + FTPB - 1) / FTPB, hint = q.hint;
    // The two kernels of a step run concurrently on two streams (fork/join events) and both append to list[nxt].
    // Which one gets the caller's stream is a scheduling choice made from the complex-env count the device reported for
    // an earlier step (a hint; either order is correct):
    //  * complex envs present: k_fast_rc (few waves, each needs a whole SIMD's register file, long latency) is enqueued first on
    //    the caller's stream so that its waves claim their SIMDs before k_fast floods the chip from the side stream;
    //  * none (e.g. the first steps after a reset): the (empty) complex-env kernel and k_fast are enqueued in order on the caller's
    //    stream, with no fork / join events at all: the event packets and the concurrently dispatched empty kernel cost 6 % of the
    //    step (613 M -> 650 M env-steps/s at 131072 envs).  Taken only when the device has reported no complex env for 16 steps in a
    //    row (a count that flickers between 0 and a few would otherwise serialise the two kernels every other step); a stale
    //    hint only serialises them for that step.
    // complex envs: row kernel while they are few (latency), lane-per-env k_fast_rc when many (throughput)
    bool rows = q.nb <= 2 && hint <= k.row_max;
    if (q.cfg_flags & PBRE_F_COMPLEX_ROWS) rows = q.nb <= 2;
    if (q.cfg_flags & PBRE_F_COMPLEX_LANES) rows = false;
    if (!q.obj_iso || q.obj_shape != 0) rows = q.nb <= 2;      // k_fast_rc's object rows assume a cube: other boxes and the round objects' complex envs go to the row kernel
    p.rows = rows;
    // (the host knows the complex envs' total, not how many of them are coupled -- one env per wave: about a tenth, generously)
    // At least 64 blocks whatever the hint says: the hint is the count of a step the DEVICE has finished, and a host that runs ahead
    // of it (the 201 launches of a reset are enqueued in ~1 ms) sizes every launch by a count that may be a hundred steps old --
    // 16384 envs that had all become complex meanwhile were walked by 8 blocks, 11 ms per launch.  Blocks without work exit at once.
    const int rblocks_estimate = (hint + REPB - 1) / REPB + (q.nb > 1 ? std::min(hint, 8 + hint / 4) / (REPB / 4) : 0) + 8;
    p.rblocks = std::max(64, std::min(q.n_simd / 4, rblocks_estimate));
    // small batches: the pair kernel (two waves per 64 envs) while all of its waves are resident at once, two per SIMD at most
    if (!q.rt && k.pair != 0 && !(q.step_flags & PBRE_F_NO_OBJECT) && !q.inner)
        p.pair = k.pair == 1 || 2 * blocks <= 2 * q.n_simd;
    // (env.step() under joint control, and the settle steps of reset(): 201 launches per reset)
    // the whole step as one launch on the caller's stream (k_fused): no fork / join through the side stream
    if (q.fusable && k.fused && rows) {
        if (p.pair) {
            p.form = StepPlan::FUSED_PAIR;
            p.grid_fused = p.rblocks + (blocks + FUSED_WAVES / 2 - 1) / (FUSED_WAVES / 2);
            p.threads_fused = PLAN_RTPB;
            return p;
        }
        // tail pairs: as many of the last chunks as the row blocks' waves (the hint's complex envs: the coupled ones -- about a quarter,
        // generously -- one per wave, the others four, an object wave per 12) will keep k_fast waves out of the first round
        if (!q.rt && k.tail_pair != 0 && q.action_repeat <= 1 && !(q.step_flags & PBRE_F_NO_OBJECT) && q.have_pair_g) {
            const int coupled = q.nb > 1 ? std::min(hint, 8 + hint / 4) : 0;
            const int tail_estimate = coupled + (hint - coupled + 3) / 4 + (hint + REPB - 1) / REPB;
            const int ntail = k.tail_pair > 1 ? k.tail_pair : (hint > 0 ? blocks + tail_estimate - 2 * q.n_simd : 0);
            p.ntail = std::max(0, std::min(ntail, blocks - 1));
        }
        p.form = p.ntail ? StepPlan::FUSED_64_TAIL : StepPlan::FUSED_64;
        p.grid_fused = FUSED_WAVES * p.rblocks + blocks + p.ntail;
        p.threads_fused = FTPB;
        return p;
    }
    p.rc_first = hint >= k.rc_first_min;
    p.single = k.idle_single && hint == 0 && q.recent == 0;      // both kernels in order on the caller's stream
    p.rc_on_caller = p.rc_first || p.single;
    p.fast_on_caller = !(p.rc_first && !p.single);
    p.touch_side = p.single && k.idle_touch > 0 && (q.launches % k.idle_touch) == 0;   // keep the side stream's queue mapped
    p.fork_join = !p.single || p.touch_side;
    p.grid_rc = rows ? p.rblocks : std::min(q.n_simd, blocks + q.nb);
    p.threads_rc = rows ? PLAN_RTPB : FTPB;
    // the 3-waves-per-SIMD variant when the complex envs' waves would push k_fast waves of the 2-wave variant into an extra round
    if (!p.single && k.fast3 != 0 && !q.rt) {      // (RT: the sweep loop of the residual-exit variant needs ~170 live registers -- at 168 it spills inside the loop)
        const int slots2 = 2 * q.n_simd;
        const int fast3_estimate = (rows ? (hint + 3) / 4 + (hint + REPB - 1) / REPB : (hint + FTPB - 1) / FTPB * 2) + 8;
        p.fast3 = k.fast3 == 1 || ((blocks + fast3_estimate + slots2 - 1) / slots2 > (blocks + slots2 - 1) / slots2 && blocks + fast3_estimate <= 3 * q.n_simd);
    }
    p.grid_fast = blocks;
    p.threads_fast = p.pair ? PLAN_PTPB : FTPB;
    return p;
}

}  // namespace pbre
