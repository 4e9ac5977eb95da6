"""The solver at sweep counts other than 150 (checks: tests/sweep_counts.py), CPU half: the device code through the host lane emulation.

Shows without a GPU that every check holds for the reference arithmetic with the existing tolerances, and records the emulation's obj_w
figures (profiles/r14_sweep_counts.json).  What only the GPU has -- the kernels the env vars select between, waves with more than one
env, lanes of a wave that leave the sweep loop apart -- is in tests/test_gpu_sweep_counts.py."""
import numpy as np
import pytest

import parity
import sweep_counts as sc
from pybullet_robot_envs import _capi

E = _capi.Engine


@pytest.mark.parametrize("k", sc.CLOSED_COUNTS)
def test_closed_forms_against_the_sequential_rows(panda, emu_lib, k):
    """A1: Fast::motor_closed's exponent k / 2 by binary powering (1, 2, 3, 4, 5, 25, 26, 27, 28, 75, 150, 500), the object block's closed
    form on either side of its threshold (52 / 54), both refused at odd counts and below 4"""
    c, s, st = sc.cached(("closed", id(emu_lib)), lambda: sc.closed_form_engines(E, emu_lib, panda["table"], 48))
    print(sc.check_closed_forms(c, s, st, k))


@pytest.mark.parametrize("k", sc.FREE_COUNTS)
def test_free_space_steps_against_the_oracle(panda, emu_lib, k):
    """A2: 3 steps of 48 envs after a default reset, TOL (obj_w below 54 sweeps: max(TOL, 4 x the fp32 oracle's own deviation))"""
    eng, ora, ora32, st = sc.cached(("free", id(emu_lib)), lambda: sc.free_pair(E, emu_lib, panda["table"], 48))
    fig = sc.check_free_steps(eng, ora, ora32, st, k, label="emulation")
    assert fig["obj_w_engine"] <= fig["obj_w_bound"]


@pytest.mark.parametrize("flags", [0, _capi.F_COMPLEX_ROWS, _capi.F_COMPLEX_LANES, _capi.F_FORCE_GENERAL])
@pytest.mark.parametrize("k", sc.CONTACT_COUNTS)
def test_contact_rich_states_against_the_oracle(panda, emu_lib, k, flags):
    """A2: 12 robot-table + 12 robot-object contact states, one step, TOL_CONTACT: the lane-per-env complex step, the row kernel's
    Core::step + Fast::finish, the general row kernel -- each with its odd-count exit at 1, 3 and 51"""
    eng, ora, S = sc.cached(("contact", id(emu_lib), flags), lambda: sc.contact_pair(E, emu_lib, panda, flags))
    sc.check_contact_steps(eng, ora, S, k)


@pytest.mark.parametrize("kind", ["ro", "zip"])
@pytest.mark.parametrize("k", sc.FAMILY_COUNTS)
def test_row_path_families_against_the_oracle(panda, emu_lib, k, kind):
    """A3: every single-env wave pattern of the row kernels (all nine one-limit-joint copies of the robot-only chain, the zipped chains, the
    loops with per-slot tests) at 3 and 51 sweeps -- each copy's `if (it + 1 >= P.iters) break` -- and at 300: check (a), and with the
    residual exit on check (c) at 51 and 300"""
    fam = sc.family_at(panda, kind, k)
    sc.row_paths.assert_coverage(fam)
    eng = sc.family_engine(fam, emu_lib, k)
    for v in range(len(fam.variants)):
        sc.row_paths.check_oracle(fam, eng, v)
    if k in sc.FAMILY_RT_COUNTS:
        for v in range(len(fam.variants)):
            sc.row_paths.check_residual_exit(fam, eng, v)
    eng.close()


@pytest.mark.parametrize("kind", ["ro_clamp", "clamp"])
def test_bounded_motor_families_at_an_odd_count(panda, emu_lib, kind):
    """A3: motors that reach their impulse bound (the limit rows decide where a joint goes, so the oracle sees a wrong one) at 51 sweeps"""
    fam = sc.family_at(panda, kind, 51)
    sc.row_paths.assert_coverage(fam)
    eng = sc.family_engine(fam, emu_lib, 51)
    for v in range(len(fam.variants)):
        sc.row_paths.check_oracle(fam, eng, v)
    eng.close()


@pytest.mark.parametrize("k", sc.RT_COUNTS)
def test_residual_exit_against_the_oracle(panda, emu_lib, k):
    """A4: threshold 1e-7 on either side of the closed form's threshold (52 / 54) and far above it; sweep counts equal the oracle's"""
    rep = sc.check_residual_exit_at(E, emu_lib, panda["table"], k, n=16)
    print({kk: v for kk, v in rep.items() if kk not in ("worst", "worst_flip")})
    if k >= 100:
        assert rep["early"] == rep["compared"] + rep["flips"], "in the oracle every env leaves the loop before sweep %d" % k


@pytest.mark.parametrize("k", [56, 300])
def test_residual_exit_lanes_leave_apart(panda, emu_lib, k):
    """A4: the batch of the GPU's wave-mates / sharding check at 32 envs: its actions do make the envs leave at different sweeps"""
    exits = sc.check_residual_exit_wave_mates_and_sharding(E, emu_lib, panda, k, n=32, steps=4)
    assert len(exits) >= 4 and exits[-1] <= k, exits


@pytest.mark.parametrize("task", [0, 1])
@pytest.mark.parametrize("k", sc.GROUP_COUNTS)
def test_icub_against_the_oracle(emu_lib, k, task):
    """A5: iCub reach / push, joint control, TOL_ICUB"""
    eng, ora, st = sc.cached(("icub", id(emu_lib), task), lambda: sc.icub_group(E, emu_lib, task, 2))
    sc.check_icub_steps(eng, ora, st, k)


@pytest.mark.parametrize("k", sc.GROUP_COUNTS)
def test_hands_against_the_oracle(emu_lib, k):
    """A5: iCub with hands, TOL_HANDS"""
    eng, ora, st, mrec, home = sc.cached(("hands", id(emu_lib)), lambda: sc.hands_group(E, emu_lib, 2))
    sc.check_hands_steps(eng, ora, st, mrec, home, k)


@pytest.mark.parametrize("task", [0, 1])
@pytest.mark.parametrize("k", [1, 3])
def test_icub_leaves_the_sweep_loop_at_an_odd_count(emu_lib, k, task):
    """A5: at 1 and 3 sweeps the result is the k-sweep one, not the (k + 1)-sweep one (sweep_counts.assert_odd_exit)"""
    eng, ora, st = sc.cached(("icub", id(emu_lib), task), lambda: sc.icub_group(E, emu_lib, task, 2))
    sc.check_icub_odd_exit(eng, ora, st, k)


@pytest.mark.parametrize("k", [1, 3])
def test_hands_leave_the_sweep_loop_at_an_odd_count(emu_lib, k):
    eng, ora, st, mrec, home = sc.cached(("hands", id(emu_lib)), lambda: sc.hands_group(E, emu_lib, 2))
    sc.check_hands_odd_exit(eng, ora, st, mrec, home, k)


@pytest.mark.parametrize("k", sc.GROUP_COUNTS)
def test_robot_level_panda_against_the_oracle(emu_lib, k):
    """A5: parity.check_panda_arm with everything after its reset at k sweeps, TOL_PANDA_ARM"""
    parity.check_panda_arm(E, emu_lib, use_ik=0, solver_iters=k).close()
