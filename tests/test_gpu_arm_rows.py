"""Every row kind of the robot-level Panda and iCub solves on the GPU, joint by joint (generator and checks: tests/arm_rows.py; CPU half:
test_emu_arm_rows.py).

pandaEnv and iCubEnv used alone are stepped by kw_step of WideImpl<ShapePA, DevLanes32> and WideImpl<ShapeIA, DevLanes32>
(pbre_icub_arm.hip): one env per 32 lanes, env = block * EPB + thread / 32, so envs 2 k and 2 k + 1 share a wave.
WHOEVER REMAPS ENVS TO WAVES IN kw_step UPDATES tests/arm_rows.py KNOWINGLY.
 (a) one step of every pool state against the fp64 oracle, per pool and, for the limit and `vel` pools, per joint: TOL_PANDA_ARM /
     TOL_ICUB_ARM, the contact tables where the robot touches something, max(entry, 4 x d32) where the oracle's own fp32 build misses an
     entry, nothing skipped; fingertip forces and counts in the observation and in the state record; the contact query's classes of
     pairs, fingertip slots and sphere counts must be the oracle's.  Stepped by command + step (C) and from the motor record (S:
     eng.settle(1), the K_SETTLE_TGT instantiation, where force scale and max velocity reach the solve); at 150 sweeps and, for the
     limit, `vel` and resting-cube pools, at 1 and 2; the Panda with PBRE_OBJ_SPLIT unset and 0 (both only_ot loops).
 (b) a probe env is bit-identical beside a free mate and beside mates that make its wave take every other path: each joint at a limit,
     robot contacts, a force-limited mate, a velocity-bounded mate, a fast mate; in either half-wave; U, B, M; C and S.
 (c) under M the fast mate alone leaves the bound (from the oracle), so its wave hands back: the probe beside it stays bit-identical.
 (d) the residual exit on the Panda's `ro` pools: sweep counts, and each env's own fingertip forces where the two envs of a wave leave
     the loop at different sweeps."""
import pytest

import arm_rows
from pybullet_robot_envs import _capi

pytestmark = pytest.mark.gpu

ROBOTS = ["panda", "icub"]
SPLITS = [("panda", None), ("panda", "0"), ("icub", None)]


def _split(monkeypatch, split):
    """PBRE_OBJ_SPLIT is read when an engine is created: set it first"""
    if split is None:
        monkeypatch.delenv("PBRE_OBJ_SPLIT", raising=False)
    else:
        monkeypatch.setenv("PBRE_OBJ_SPLIT", split)


@pytest.mark.parametrize("robot", ROBOTS)
def test_the_checks_start_from_the_resets_motor_record(hip_lib, robot):
    arm_rows.check_reset_record(_capi.Engine, hip_lib, robot)


@pytest.mark.parametrize("robot", ROBOTS)
def test_the_records_are_what_the_engines_commands_write(hip_lib, robot):
    arm_rows.check_records_agree(_capi.Engine, hip_lib, robot)


@pytest.mark.parametrize("robot,variant,mode,sweeps,split", arm_rows.a_cases())
def test_pool_states_against_the_oracle(hip_lib, monkeypatch, robot, variant, mode, sweeps, split):
    _split(monkeypatch, split)
    arm_rows.check_rows_against_oracle(_capi.Engine, hip_lib, robot, variant, mode, sweeps, split, kernel=arm_rows.ROBOTS[robot].kernel)


@pytest.mark.parametrize("mode", ["C", "S"])
@pytest.mark.parametrize("variant", ["U", "B", "M"])
@pytest.mark.parametrize("robot,split", SPLITS)
def test_wave_mates_do_not_matter(hip_lib, monkeypatch, robot, split, variant, mode):
    _split(monkeypatch, split)
    arm_rows.check_wave_mates(_capi.Engine, hip_lib, robot, variant, mode, split)


@pytest.mark.parametrize("variant,mode", arm_rows.RT_CASES)
def test_residual_exit_reports_each_envs_own_forces(hip_lib, variant, mode):
    arm_rows.check_residual_exit(_capi.Engine, hip_lib, variant, mode)
