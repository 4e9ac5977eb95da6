// pbre_reset_seq.hpp -- what a reset does to an env, in order: the reference's robot.reset() + reset_simulation() choreography, stated once.
// No HIP in here: pbre_ctx::reset (pbre_capi.hip) runs it over a batch through the engines' reset_op hooks, the lane emulation
// (tests/host_emu) runs it env by env, and tests/reset_seq_host compiles this header with the host compiler alone and records it, so the
// operation lists of tests/test_reset_seq_host.py -- written out from the reference's lines -- pin the sequence every engine executes.
#pragma once
#include "../../include/pbre.h"

namespace pbre {

// RS_INIT: the records of the episode that begins (joints at their initial positions, object pose sampled); RS_MOTORS: the motor records
// (every motor at its initial position, gain 0.2, default force); RS_HOME_IK: the joint targets of the home hand pose; RS_SETTLE: `count`
// steps with `flags` (PBRE_F_NO_OBJECT: the robot alone), motors holding; RS_TARGETS: the episode's target pose; RS_INITD: the distances
// the normalised reward divides by
enum ResetOp { RS_INIT, RS_MOTORS, RS_HOME_IK, RS_SETTLE, RS_TARGETS, RS_INITD };

// run(op, count, flags) executes one operation on the envs being reset (count, flags: RS_SETTLE's) and returns 0 or an error code, which
// ends the sequence and is returned.  mrec: the engine's shape keeps motor records (the robot-level interfaces).
template <class Run>
int reset_sequence(int robot, bool use_ik, int task, bool mrec, int cfg_flags, Run&& run) {
    int rc;
    // robot.reset (panda_env.py:60-91, icub_env.py:103-151, icub_env_with_hands.py:108-121): every joint at its initial position and held
    // there; with use_IK the home hand pose is commanded (panda_env.py:90, icub_env.py:148-149)
    if ((rc = run(RS_INIT, 0, 0))) return rc;
    if (mrec && (rc = run(RS_MOTORS, 0, 0))) return rc;
    if (use_ik && (rc = run(RS_HOME_IK, 0, 0))) return rc;
    // ... and it ends with one stepSimulation: on the Panda only behind the IK command (panda_env.py:91), on the iCub always
    // (icub_env.py:151).  reset_simulation then runs 100 steps with the robot alone (panda_push_gym_env.py:129-133,
    // icub_reach_gym_env.py:135-137)
    const int extra = (use_ik || robot != PBRE_ROBOT_PANDA) ? 1 : 0;
    if ((rc = run(RS_SETTLE, extra + 100, PBRE_F_NO_OBJECT))) return rc;
    // the world is loaded, 100 steps and one more behind the debug drawing (panda_push_gym_env.py:136-148, icub_reach_gym_env.py:139-149)
    if ((rc = run(RS_SETTLE, 100 + 1, cfg_flags & PBRE_F_NO_OBJECT))) return rc;
    // reset() samples the target (panda_push_gym_env.py:108-110, icub_push_gym_env.py:118-120) and, for the iCub push envs, takes the
    // distances hand-object and object-target of the settled state (icub_push_gym_env.py:123-127)
    if ((rc = run(RS_TARGETS, 0, 0))) return rc;
    if (task >= PBRE_TASK_PUSH && robot != PBRE_ROBOT_PANDA && (rc = run(RS_INITD, 0, 0))) return rc;
    return 0;
}

}  // namespace pbre
