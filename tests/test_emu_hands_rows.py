"""Every row kind of the hands engine's solve, joint by joint (tests/hands_rows.py), CPU half.

The generator's own promises -- every (joint, side) limit pool that is not listed as left out holds states in which the ORACLE's result
depends on the limit row by at least 0.05 rad/s under bounded motors, every pool is full after the oracle's conditioning probe, so nothing
is skipped downstream -- and the checks (a) - (d) through the host emulation, which runs Core<Lanes128, Shape128>::step env by env: the
block-mate check (b) is trivially true here and runs all the same, so that both halves use the same batches."""
import pytest

import hands_rows
from pybullet_robot_envs import _capi


def test_pools_are_full_and_the_limit_rows_decide(emu_lib):
    R = hands_rows.rows(_capi.Engine, emu_lib)
    hands_rows.assert_pools(R)
    print("hands row pools: %d states drawn, %d re-drawn after the conditioning probe, %.1f s of CPU time, left out: %r"
          % (sum(R.drawn.values()), R.redrawn, R.seconds, R.left_out))


def test_the_checks_start_from_the_resets_motor_record(emu_lib):
    hands_rows.check_reset_record(_capi.Engine, emu_lib)


@pytest.mark.parametrize("variant,hull", hands_rows.ENGINES)
def test_pool_states_against_the_oracle(emu_lib, variant, hull):
    """check (a): UF = the pools without limit rows twice in one engine, as they are (U: the clamp-free attempt) and with every joint
    force-limited through set_motors(mask=...) (F: the clamping loops); B / B2 the limit pools under the bound they were found with;
    hull: the brick as a hull object at rest on the table, whose object-table rows stay in the step kernel (the only_ot loops)"""
    hands_rows.check_rows_against_oracle(_capi.Engine, emu_lib, variant, hull, kernel="emulation")


@pytest.mark.parametrize("sweeps", hands_rows.FEW_SWEEPS)
@pytest.mark.parametrize("variant,hull", hands_rows.FEW_ENGINES)
def test_pool_states_against_the_oracle_after_few_sweeps(emu_lib, variant, hull, sweeps):
    """check (a) at solver_iters = 1 (the backward half-sweep alone) and 2 (backward, then forward): at 150 a row left out of every
    second half-sweep converges to the same impulse and goes unseen"""
    hands_rows.check_rows_against_oracle(_capi.Engine, emu_lib, variant, hull, kernel="emulation", sweeps=sweeps)


@pytest.mark.parametrize("variant", ["U", "F"])
def test_block_mates_do_not_matter(emu_lib, variant):
    hands_rows.check_block_mates(_capi.Engine, emu_lib, variant)


def test_same_value_whichever_loop(emu_lib):
    hands_rows.check_same_value_whichever_loop(_capi.Engine, emu_lib)


def test_residual_exit_reports_the_exit_sweep(emu_lib):
    hands_rows.check_residual_exit(_capi.Engine, emu_lib)
