"""Every row kind of the robot-level Panda and iCub solves, joint by joint (tests/arm_rows.py), CPU half.

The generator's own promises -- all 18 + 40 (joint, side) limit pools hold states in which the ORACLE's result depends on the limit row by at
least 0.05 rad/s (m/s) under bounded motors, all 18 + 40 `vel` pools states in which it depends on the velocity bound as much, every pool
is full after the oracle's conditioning probe, so nothing is skipped downstream -- and the checks (a) - (d) through the host emulation,
which runs Core<Lanes32, ShapePA / ShapeIA>::step env by env: the wave-mate checks (b) and (c) are trivially true here and run all the
same, so that both halves use the same batches."""
import pytest

import arm_rows
from pybullet_robot_envs import _capi

ROBOTS = ["panda", "icub"]
A_CASES = arm_rows.a_cases()
SPLITS = [("panda", None), ("panda", "0"), ("icub", None)]


def _split(monkeypatch, split):
    """PBRE_OBJ_SPLIT is read when an engine is created: set it first"""
    if split is None:
        monkeypatch.delenv("PBRE_OBJ_SPLIT", raising=False)
    else:
        monkeypatch.setenv("PBRE_OBJ_SPLIT", split)


@pytest.mark.parametrize("robot", ROBOTS)
def test_pools_are_full_and_the_rows_decide(emu_lib, robot):
    R = arm_rows.rows(_capi.Engine, emu_lib, robot)
    arm_rows.assert_pools(R)
    print("%s row pools: %d states drawn, %d re-drawn after the conditioning probe, %.1f s of CPU time" % (robot, sum(R.drawn.values()), R.redrawn, R.seconds))


@pytest.mark.parametrize("robot", ROBOTS)
def test_the_checks_start_from_the_resets_motor_record(emu_lib, robot):
    arm_rows.check_reset_record(_capi.Engine, emu_lib, robot)


@pytest.mark.parametrize("robot", ROBOTS)
def test_the_records_are_what_the_engines_commands_write(emu_lib, robot):
    arm_rows.check_records_agree(_capi.Engine, emu_lib, robot)


@pytest.mark.parametrize("robot,variant,mode,sweeps,split", A_CASES)
def test_pool_states_against_the_oracle(emu_lib, monkeypatch, robot, variant, mode, sweeps, split):
    """check (a); split "0": PBRE_OBJ_SPLIT=0 keeps the resting cube's rows in kw_step (the two only_ot loops)"""
    _split(monkeypatch, split)
    arm_rows.check_rows_against_oracle(_capi.Engine, emu_lib, robot, variant, mode, sweeps, split, kernel="emulation")


@pytest.mark.parametrize("mode", ["C", "S"])
@pytest.mark.parametrize("variant", ["U", "B", "M"])
@pytest.mark.parametrize("robot,split", SPLITS)
def test_wave_mates_do_not_matter(emu_lib, monkeypatch, robot, split, variant, mode):
    """checks (b) and, under M, (c)"""
    _split(monkeypatch, split)
    arm_rows.check_wave_mates(_capi.Engine, emu_lib, robot, variant, mode, split)


@pytest.mark.parametrize("variant,mode", arm_rows.RT_CASES)
def test_residual_exit_reports_each_envs_own_forces(emu_lib, variant, mode):
    arm_rows.check_residual_exit(_capi.Engine, emu_lib, variant, mode)
