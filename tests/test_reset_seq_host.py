"""What a reset does, without a GPU: csrc/pbre_reset_seq.hpp (reset_sequence -- the text pbre_ctx::reset of the device library and the lane
emulation both execute) compiled by the host compiler (tests/reset_seq_host) and run by a recording executor.  The operation lists below
are written out BY HAND from the reference's lines (R = pybullet_robot_envs/envs), not taken from the function:

  R/panda_envs/panda_env.py:60-77      resetJointState + position motors at the initial positions            -> INIT
  R/panda_envs/panda_env.py:83-91      use_IK: apply_action(home hand pose), ONE stepSimulation               -> HOME_IK, 1 step
  R/icub_envs/icub_env.py:103-119      the same joint loop                                                    -> INIT
  R/icub_envs/icub_env.py:148-151      use_IK: apply_action(home hand pose); ONE stepSimulation either way    -> [HOME_IK], 1 step
  R/icub_envs/icub_env_with_hands.py:108-121   every motor at its initial position, gain 0.2                  -> INIT, MOTORS (the engines
                                       that keep motor records: the iCub with hands and the robot-level pandaEnv / iCubEnv)
  R/panda_envs/panda_push_gym_env.py:129-133, R/icub_envs/icub_reach_gym_env.py:133-137   robot.reset(), 100 steps, no object yet
  R/panda_envs/panda_push_gym_env.py:136-148, R/icub_envs/icub_reach_gym_env.py:139-149   world.reset(), 100 steps, debug drawing, 1 step
  R/panda_envs/panda_push_gym_env.py:108-110, R/icub_envs/icub_push_gym_env.py:118-120    the target pose                       -> TARGETS
  R/icub_envs/icub_push_gym_env.py:123-127     _init_dist_hand_obj, _max_dist_obj_tg of the settled state     -> INITD (iCub push only)

A run of steps is one SETTLE(count, flags); the robot-alone run always carries PBRE_F_NO_OBJECT, the run with the world loaded carries
that bit of the config's flags (a config without an object never loads one) and no other bit."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INIT, MOTORS, HOME_IK, SETTLE, TARGETS, INITD = range(6)       # csrc/pbre_reset_seq.hpp: ResetOp
PANDA, ICUB, HANDS = 0, 1, 2                                    # include/pbre.h: PBRE_ROBOT_*
REACH, PUSH, PUSH_GOAL = 0, 1, 2                                # PBRE_TASK_*
NO_OBJECT, AUTO_RESET = 1, 2                                    # PBRE_F_*


@pytest.fixture(scope="module")
def host():
    d = os.path.join(ROOT, "tests", "reset_seq_host")
    subprocess.check_call(["make", "-s", "-C", d])
    lib = C.CDLL(os.path.join(d, "build", "libpbre_reset_seq_host.so"))
    lib.reset_seq_record.restype = C.c_int
    lib.motor_cmd.restype = C.c_int
    return lib


def record(host, robot, use_ik, task, mrec, flags=0, fail_at=-1):
    out, rc = (C.c_int * (3 * 16))(), C.c_int(99)
    n = host.reset_seq_record((C.c_int * 6)(robot, use_ik, task, mrec, flags, fail_at), out, 16, C.byref(rc))
    assert n <= 16
    ops = [(out[3 * i],) if out[3 * i] != SETTLE else tuple(out[3 * i:3 * i + 3]) for i in range(n)]
    return ops, rc.value


def alone(steps):
    return (SETTLE, steps, NO_OBJECT)


def loaded(flags=0):
    return (SETTLE, 100 + 1, flags & NO_OBJECT)


# every engine kind: (robot, use_ik, task, mrec) -> the operations with the object in the scene
KINDS = {
    "panda_push_joint": ((PANDA, 0, PUSH, 0), [(INIT,), alone(100), loaded(), (TARGETS,)]),
    "panda_push_ik": ((PANDA, 1, PUSH, 0), [(INIT,), (HOME_IK,), alone(1 + 100), loaded(), (TARGETS,)]),
    "panda_reach_ik": ((PANDA, 1, REACH, 0), [(INIT,), (HOME_IK,), alone(1 + 100), loaded(), (TARGETS,)]),
    "panda_push_goal_joint": ((PANDA, 0, PUSH_GOAL, 0), [(INIT,), alone(100), loaded(), (TARGETS,)]),
    "icub_reach_joint": ((ICUB, 0, REACH, 0), [(INIT,), alone(1 + 100), loaded(), (TARGETS,)]),
    "icub_reach_ik": ((ICUB, 1, REACH, 0), [(INIT,), (HOME_IK,), alone(1 + 100), loaded(), (TARGETS,)]),
    "icub_push_joint": ((ICUB, 0, PUSH, 0), [(INIT,), alone(1 + 100), loaded(), (TARGETS,), (INITD,)]),
    "icub_push_ik": ((ICUB, 1, PUSH, 0), [(INIT,), (HOME_IK,), alone(1 + 100), loaded(), (TARGETS,), (INITD,)]),
    "icub_push_goal_ik": ((ICUB, 1, PUSH_GOAL, 0), [(INIT,), (HOME_IK,), alone(1 + 100), loaded(), (TARGETS,), (INITD,)]),
    "hands": ((HANDS, 0, REACH, 1), [(INIT,), (MOTORS,), alone(1 + 100), loaded(), (TARGETS,)]),
    "hands_ik": ((HANDS, 1, REACH, 1), [(INIT,), (MOTORS,), (HOME_IK,), alone(1 + 100), loaded(), (TARGETS,)]),
    "panda_arm": ((PANDA, 0, REACH, 1), [(INIT,), (MOTORS,), alone(100), loaded(), (TARGETS,)]),
    "panda_arm_ik": ((PANDA, 1, REACH, 1), [(INIT,), (MOTORS,), (HOME_IK,), alone(1 + 100), loaded(), (TARGETS,)]),
    "icub_arm": ((ICUB, 0, REACH, 1), [(INIT,), (MOTORS,), alone(1 + 100), loaded(), (TARGETS,)]),
    "icub_arm_ik": ((ICUB, 1, REACH, 1), [(INIT,), (MOTORS,), (HOME_IK,), alone(1 + 100), loaded(), (TARGETS,)]),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_operations_of_every_engine_kind(host, kind):
    args, want = KINDS[kind]
    assert record(host, *args) == (want, 0)
    # without the object: the same operations, and the second run of steps is the robot's alone too
    no_obj = [loaded(NO_OBJECT) if op == loaded() else op for op in want]
    assert no_obj != want
    assert record(host, *args, flags=NO_OBJECT) == (no_obj, 0)


def test_the_extra_step_is_the_panda_ik_commands_and_every_icubs(host):
    steps = lambda *a: [op[1] for op in record(host, *a)[0] if op[0] == SETTLE]
    assert steps(PANDA, 0, PUSH, 0) == [100, 101]                # panda_env.py:83: the step is inside `if self._use_IK`
    assert steps(PANDA, 1, PUSH, 0) == [1 + 100, 101]
    assert steps(PANDA, 0, REACH, 1) == [100, 101]               # ... also when pandaEnv is used alone
    assert steps(ICUB, 0, REACH, 0) == [1 + 100, 101]            # icub_env.py:151: outside the `if`
    assert steps(ICUB, 1, REACH, 0) == [1 + 100, 101]
    assert steps(HANDS, 0, REACH, 1) == [1 + 100, 101]


def test_motor_records_are_initialised_only_where_they_are_kept(host):
    for robot in (PANDA, ICUB, HANDS):
        for ik in (0, 1):
            assert [op for op in record(host, robot, ik, REACH, 1)[0] if op == (MOTORS,)] == [(MOTORS,)]
            assert (MOTORS,) not in record(host, robot, ik, REACH, 0)[0]
            assert record(host, robot, ik, REACH, 1)[0][:2] == [(INIT,), (MOTORS,)]      # before the IK command and the first step read them


def test_home_pose_ik_only_under_cartesian_control(host):
    for robot in (PANDA, ICUB, HANDS):
        for mrec in (0, 1):
            assert (HOME_IK,) not in record(host, robot, 0, REACH, mrec)[0]
            ops = record(host, robot, 1, REACH, mrec)[0]
            assert ops.count((HOME_IK,)) == 1 and ops[ops.index((HOME_IK,)) + 1][0] == SETTLE


def test_initial_distances_only_for_the_icub_push_envs(host):
    for robot in (PANDA, ICUB, HANDS):
        for task in (REACH, PUSH, PUSH_GOAL):
            for ik in (0, 1):
                ops = record(host, robot, ik, task, 0)[0]
                assert ((INITD,) in ops) == (robot != PANDA and task != REACH), (robot, task, ik)
                if (INITD,) in ops:
                    assert ops[-2:] == [(TARGETS,), (INITD,)]      # the object-target distance needs the target


def test_only_the_loaded_run_follows_the_no_object_bit(host):
    for flags in (0, NO_OBJECT, AUTO_RESET, AUTO_RESET | NO_OBJECT, 0x7ffffffe, 0x7fffffff):
        runs = [op for op in record(host, ICUB, 1, PUSH, 0, flags=flags)[0] if op[0] == SETTLE]
        assert runs == [(SETTLE, 101, NO_OBJECT), (SETTLE, 101, flags & 1)]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_an_executor_error_stops_the_sequence_there(host, kind):
    args, want = KINDS[kind]
    for at in range(len(want)):
        assert record(host, *args, fail_at=at) == (want[:at + 1], -7)
    assert record(host, *args, fail_at=len(want)) == (want, 0)


# ---------------------------------------------------------------------------------------------- pbre_set_motors' command
def motor_cmd(host, dofs, targets, kp, max_force, max_vel, ndof, dt=1 / 240, imp=100000 / 240):
    n = len(dofs)
    out, d, t, msg = (C.c_float * 4)(), (C.c_int * max(n, 1))(), (C.c_float * max(n, 1))(), C.create_string_buffer(128)
    rc = host.motor_cmd(n, (C.c_int32 * max(n, 1))(*dofs), (C.c_float * max(n, 1))(*targets), C.c_double(kp), C.c_double(max_force), C.c_double(max_vel),
                        ndof, C.c_double(dt), C.c_double(imp), out, d, t, msg)
    return rc, list(out), list(d)[:n], list(t)[:n], msg.value.decode()


def test_motor_command_arithmetic(host):
    import numpy as np
    # a force of 10 N as a fraction of the default 1e5 N: 10 * dt / (1e5 * dt) = 1e-4, in double, rounded once
    rc, out, d, t, _ = motor_cmd(host, [7, 8, 0], [0.04, 0.04, -0.5], 0.3, 10.0, 1.0, 9)
    assert rc == 0 and d == [7, 8, 0] and t == [np.float32(0.04), np.float32(0.04), np.float32(-0.5)]
    assert out == [3.0, np.float32(0.3), np.float32(10.0 * (1 / 240) / (100000 / 240)), 1.0]
    # no force / velocity given: the default force (scale 1), no velocity bound
    assert motor_cmd(host, [0], [0.0], 0.2, 0.0, 0.0, 9)[1] == [1.0, np.float32(0.2), 1.0, 0.0]
    assert motor_cmd(host, [0], [0.0], 0.2, -1.0, -1.0, 9)[1][2:] == [1.0, 0.0]
    assert motor_cmd(host, [], [], 0.2, 0.0, 0.0, 9)[0] == 0


def test_motor_command_refusals(host):
    assert motor_cmd(host, [9], [0.0], 0.2, 0.0, 0.0, 9)[::4] == (-1, "pbre_set_motors: bad DoF index")
    assert motor_cmd(host, [0, -1], [0.0, 0.0], 0.2, 0.0, 0.0, 9)[::4] == (-1, "pbre_set_motors: bad DoF index")
    assert motor_cmd(host, [8], [0.0], 0.2, 0.0, 0.0, 9)[0] == 0
    assert motor_cmd(host, list(range(60)) + [0, 1, 2, 3], [0.0] * 64, 0.2, 0.0, 0.0, 60)[0] == 0
    assert motor_cmd(host, list(range(60)) + [0, 1, 2, 3, 4], [0.0] * 65, 0.2, 0.0, 0.0, 60)[::4] == (-1, "pbre_set_motors: more than 64 joints")


def test_sanitized_sequence_and_motor_commands(host):
    """AddressSanitizer + UBSan over the recording executor at every failure position of every configuration, make_motor_cmd at 0 / 64 / 65
    joints and the three motor-record writers on records of exactly 4 W floats (its own main: nothing is loaded into python)."""
    out = subprocess.run([os.path.join(ROOT, "tests", "reset_seq_host", "build", "reset_seq_san")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "reset_seq_san OK" in out.stdout, out.stdout + out.stderr
