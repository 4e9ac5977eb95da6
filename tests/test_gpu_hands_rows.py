"""Every row kind of the hands engine's solve on the GPU, joint by joint (generator and checks: tests/hands_rows.py; CPU half:
test_emu_hands_rows.py).

pbre_hands.hip steps the 60-DoF iCub with hands with Core<DevLanes128, Shape128>::step, one env per wave and four waves per block:
env = block * 4 + thread / 64.  WHOEVER REMAPS ENVS TO WAVES AND BLOCKS IN THIS KERNEL UPDATES tests/hands_rows.py KNOWINGLY.
 (a) one step of every pool state against the fp64 oracle, per pool and, for the limit pools, per joint: TOL_HANDS_CONTACT (TOL_HANDS for
     free states), max(TOL, 4 x d32) where the oracle's own fp32 build misses a bound, nothing skipped; fingertip forces and counts; the
     contact query's classes of pairs, fingertip slots and sphere counts must be the oracle's.  U and F share an engine (UF), the F envs
     force-limited through set_motors(mask=...).  U: the clamp-free attempt runs through; F: it is skipped, the clamping loops run; B / B2:
     it hands back, and the oracle's own result depends on every limit row by >= 0.05 rad/s; hull: the two only_ot loops.
 (b) a probe env is bit-identical alone, at each position of a block of `ro5` envs and as the last env of a ragged batch (the per-wave
     regions of the LDS row store).
 (c) max_motor_impulse = 30: pool states bit-identical to an engine with the default bound; fast states hand back and are held to the
     oracle like any other group.
 (d) the residual exit: sweep counts, and the fingertip forces of envs that leave early."""
import pytest

import hands_rows
from pybullet_robot_envs import _capi

pytestmark = pytest.mark.gpu


def test_the_checks_start_from_the_resets_motor_record(hip_lib):
    hands_rows.check_reset_record(_capi.Engine, hip_lib)


@pytest.mark.parametrize("variant,hull", hands_rows.ENGINES)
def test_pool_states_against_the_oracle(hip_lib, variant, hull):
    hands_rows.check_rows_against_oracle(_capi.Engine, hip_lib, variant, hull, kernel="kw_step<Shape128>")


@pytest.mark.parametrize("sweeps", hands_rows.FEW_SWEEPS)
@pytest.mark.parametrize("variant,hull", hands_rows.FEW_ENGINES)
def test_pool_states_against_the_oracle_after_few_sweeps(hip_lib, variant, hull, sweeps):
    """(a) at solver_iters = 1 (motors 59 .. 0, limits_bwd, contact rows) and 2 (then limits_fwd, motors 0 .. 59, contact rows): each
    half-sweep's body on its own, where 150 sweeps would converge past a row that is missing from one of them"""
    hands_rows.check_rows_against_oracle(_capi.Engine, hip_lib, variant, hull, kernel="kw_step<Shape128>", sweeps=sweeps)


@pytest.mark.parametrize("variant", ["U", "F"])
def test_block_mates_do_not_matter(hip_lib, variant):
    hands_rows.check_block_mates(_capi.Engine, hip_lib, variant)


def test_same_value_whichever_loop(hip_lib):
    hands_rows.check_same_value_whichever_loop(_capi.Engine, hip_lib)


def test_residual_exit_reports_the_exit_sweep(hip_lib):
    hands_rows.check_residual_exit(_capi.Engine, hip_lib)
