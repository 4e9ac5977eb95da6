"""Every row kind of the iCub solve kernels on the GPU, joint by joint (generator and checks: tests/icub_rows.py; CPU half:
test_emu_icub_rows.py).

The lane-per-env pipeline kw_dyn -> kw_quad / kw_quad_rc -> kw_fin (csrc/pbre_lane.hip) steps every iCub batch from 16384 envs on, and its
solve, quad_step, has no host twin.  It decides per WAVE which rows run: limit row j if any env of the wave has joint j at a limit (a
ballot mask, the row owned by quad lane j / 5), contact slot c if any env uses it, the clamp-free motor attempt if no env has a contact row,
and the clamping repeat if any env's motor went over its bound.  These tests place envs so that the wave is known -- kw_quad: global lane
gl serves env gl >> 2, so wave w holds envs 16 w .. 16 w + 15; kw_quad_rc: at most 16 envs with robot-object contact share wave 0
whatever order the atomics produce; kw_step (PBRE_ICUB_LANE=0): envs 2 k and 2 k + 1 share a wave.  WHOEVER REMAPS ENVS TO WAVES IN THESE
KERNELS UPDATES tests/icub_rows.py KNOWINGLY.
 (a) one step of every pool state against the oracle, per pool and, for the limit pools, per joint: TOL_ICUB_CONTACT (TOL_ICUB for free
     states), nothing skipped.  With bounded motors (variant B) the oracle's own result depends on each limit row by >= 0.05 rad/s; with
     the default motors a limit row is invisible (the position motor undoes it), so U runs the contact pools.
 (b) a probe env's state record and output row are bit-identical whatever its wave-mates make the wave do: a limit row of each of the
     20 joints that is not the probe's, robot-table slots (no clamp-free attempt), a mate that forces the clamping repeat; in kw_quad_rc a
     second robot-object slot, limit rows of each quad lane, robot-table rows; and one env per wave against 16 (PBRE_QUAD_RC_EPW)."""
import pytest

import icub_rows
from pybullet_robot_envs import _capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", ["B", "U"])
@pytest.mark.parametrize("lane", ["1", "0"])
def test_pool_states_against_the_oracle(hip_lib, monkeypatch, variant, lane):
    """(a) lane = 1: quad_step<false> (kw_quad) for the pools without robot-object contact, quad_step<true> (kw_quad_rc) for those with --
    the engine's classes must be the oracle's contact sets; lane = 0: kw_step"""
    monkeypatch.setenv("PBRE_ICUB_LANE", lane)
    icub_rows.check_rows_against_oracle(_capi.Engine, hip_lib, variant, int(lane), kernel="kw_quad / kw_quad_rc" if lane == "1" else "kw_step")


@pytest.mark.parametrize("variant", ["U", "B", "M"])
def test_kw_quad_results_do_not_depend_on_wave_mates(hip_lib, monkeypatch, variant):
    """(b) kw_quad: probes free / a limit joint of each quad lane / robot-table contact, at positions 0, 6 and 15 of the wave.  U: every wave
    without robot-table rows ends on the clamp-free motor rows; B: none does; M (max_motor_impulse = 30): only the wave with the fast mate
    repeats the attempt with clamping rows -- asserted from the oracle: of all envs, only the fast mate's motors reach that bound"""
    monkeypatch.setenv("PBRE_ICUB_LANE", "1")
    icub_rows.check_quad_wave_mates(_capi.Engine, hip_lib, variant)


@pytest.mark.parametrize("variant", ["U", "B"])
def test_kw_quad_rc_results_do_not_depend_on_wave_mates(hip_lib, monkeypatch, variant):
    """(b) kw_quad_rc: the ro1 probe alone in wave 0 and beside ro2 / lim+ro1 (a joint of each quad lane) / ro1+rt1 / all of them / a fast mate"""
    monkeypatch.setenv("PBRE_ICUB_LANE", "1")
    monkeypatch.delenv("PBRE_QUAD_RC_EPW", raising=False)
    icub_rows.check_quad_rc_wave_mates(_capi.Engine, hip_lib, variant)


@pytest.mark.parametrize("variant", ["U", "B"])
def test_kw_quad_rc_results_do_not_depend_on_envs_per_wave(hip_lib, monkeypatch, variant):
    monkeypatch.setenv("PBRE_ICUB_LANE", "1")
    icub_rows.check_quad_rc_epw(_capi.Engine, hip_lib, variant, monkeypatch.setenv, monkeypatch.delenv)


@pytest.mark.parametrize("variant", ["U", "B"])
@pytest.mark.parametrize("split", ["1", "0"])
def test_kw_step_results_do_not_depend_on_the_other_half_wave(hip_lib, monkeypatch, variant, split):
    """(b) kw_step: free / limit / robot-table / robot-object probes beside free, limit, rt2 and ro2 mates, in either half of the wave; with
    the object rows split off (the default) and kept in the kernel (PBRE_OBJ_SPLIT=0)"""
    monkeypatch.setenv("PBRE_ICUB_LANE", "0")
    monkeypatch.setenv("PBRE_OBJ_SPLIT", split)
    icub_rows.check_group_wave_mates(_capi.Engine, hip_lib, variant)
