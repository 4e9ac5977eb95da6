"""Every row kind of the iCub solve kernels, joint by joint (tests/icub_rows.py), CPU half.

The generator's own promises -- all 40 (joint, side) limit pools hold states in which the ORACLE's result depends on the limit row by at
least 0.05 rad/s under bounded motors, every pool is full after the oracle's conditioning probe, so nothing is skipped downstream -- and
check (a), one step of every pool state against the oracle, through the host emulation: Lane::step (PBRE_ICUB_LANE=1; the device runs
quad_step in its place) and Core::step on the half-wave shape (PBRE_ICUB_LANE=0).  The emulation steps env by env (its PBRE_ANY is per
env), so the wave-mate checks (b) are trivially true here; they run all the same, for the batches and the plumbing."""
import pytest

import icub_rows
from pybullet_robot_envs import _capi


def test_pools_are_full_and_the_limit_rows_decide():
    R = icub_rows.rows()
    icub_rows.assert_pools(R)
    print("iCub row pools: %d states drawn, %d re-drawn after the conditioning probe" % (sum(R.drawn.values()), R.redrawn))


@pytest.mark.parametrize("variant", ["B", "U"])
@pytest.mark.parametrize("lane", ["1", "0"])
def test_pool_states_against_the_oracle(emu_lib, monkeypatch, variant, lane):
    """check (a): B = bounded motors, every pool (the limit rows decide where a joint goes); U = the defaults, the contact pools"""
    monkeypatch.setenv("PBRE_ICUB_LANE", lane)
    icub_rows.check_rows_against_oracle(_capi.Engine, emu_lib, variant, int(lane), device=False, kernel="emulation: " + ("Lane::step" if lane == "1" else "Core::step"))


@pytest.mark.parametrize("variant", ["B", "U", "M"])
def test_wave_mates_of_the_pipeline(emu_lib, monkeypatch, variant):
    """check (b), the batches of kw_quad (a probe per kind, one position) and of kw_quad_rc; M: the motor bound that only a fast mate exceeds"""
    monkeypatch.setenv("PBRE_ICUB_LANE", "1")
    icub_rows.check_quad_wave_mates(_capi.Engine, emu_lib, variant, probes=["free", "lim:12:1", "rt1"], positions=(6,))
    if variant != "M":
        icub_rows.check_quad_rc_wave_mates(_capi.Engine, emu_lib, variant, device=False)


@pytest.mark.parametrize("variant", ["B", "U"])
def test_wave_mates_of_the_lane_group_kernel(emu_lib, monkeypatch, variant):
    monkeypatch.setenv("PBRE_ICUB_LANE", "0")
    icub_rows.check_group_wave_mates(_capi.Engine, emu_lib, variant)
