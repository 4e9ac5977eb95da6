"""The solver at sweep counts other than 150 on the GPU (checks: tests/sweep_counts.py; CPU half: test_emu_sweep_counts.py).

pbre_physics.solver_iters is a runtime parameter, and the kernels branch and index on it: the motors' closed form (binary powering of
iters / 2) at even counts >= 4, the object block's closed form and the closed form of the residual exit at even counts >= PBRE_OC_K + 32,
and at odd counts the `if (it + 1 >= P.iters) break` of every two-sweeps-per-trip loop -- about ten copies in the row kernels alone.  Code of
this kind has failed on the GPU only before (the early loop exit of k_fast_rc<., RT>), so every check of the CPU half runs here
again, under each kernel selection the env vars offer, with waves of several envs and lanes that leave the sweep loop apart.

 A1  closed forms against Bullet's sequential rows, bit-identical where no closed form applies       k_fast, k_fast_pair, k_fused's waves
 A2  the Panda against the fp64 oracle: free space (TOL) and crafted contact states (TOL_CONTACT)    + k_row_list, k_fast_rc, k_step
 A3  the per-wave path families of tests/row_paths.py at 3, 51 and 300 sweeps: checks (a), (b), (c)  k_step's copies of Core::step
 A4  the residual exit (threshold 1e-7) at 50 .. 300 sweeps; wave-mates and sharding at 56 and 300   the RT instantiations
 A5  iCub (lane-group kernel and lane-per-env pipeline), iCub with hands, robot-level Panda          kw_step, pbre_lane.hip, pbre_objstep.hpp

`PBRE_PARITY_MEASURE=1 python -m pytest tests/test_gpu_sweep_counts.py -m gpu -s` prints the SWEEP_COUNTS lines recorded in
profiles/r14_sweep_counts.json."""
import numpy as np
import pytest

import parity
import sweep_counts as sc
from pybullet_robot_envs import _capi

pytestmark = pytest.mark.gpu

E = _capi.Engine


@pytest.mark.parametrize("pair,fused", [("1", "1"), ("1", "0"), ("0", "1"), ("0", "0")])
@pytest.mark.parametrize("k", sc.CLOSED_COUNTS)
def test_closed_forms_against_the_sequential_rows(panda, hip_lib, monkeypatch, k, pair, fused):
    """A1, 131 envs (two full waves and a partial one), under the kernel selections of test_pair_kernel_is_bit_identical_to_k_fast
    (PBRE_PAIR) and test_one_launch_step_is_bit_identical_to_the_two_kernel_step (PBRE_FUSED): every kernel that steps simple envs"""
    monkeypatch.setenv("PBRE_PAIR", pair)
    monkeypatch.setenv("PBRE_FUSED", fused)
    c, s, st = sc.cached(("closed", pair, fused), lambda: sc.closed_form_engines(E, hip_lib, panda["table"], 131))
    print(sc.check_closed_forms(c, s, st, k))
    info = c.kernel_info()
    assert (info[10] > 0) == (pair == "1") and (info[13] > 0) == (fused == "1") and info[12] == 0, info


@pytest.mark.parametrize("pair", ["1", "0"])
@pytest.mark.parametrize("k", sc.FREE_COUNTS)
def test_free_space_steps_against_the_oracle(panda, hip_lib, monkeypatch, k, pair):
    """A2: 3 steps of 131 envs after a default reset, TOL (obj_w below 54 sweeps: max(TOL, 4 x the fp32 oracle's own deviation))"""
    monkeypatch.setenv("PBRE_PAIR", pair)
    eng, ora, ora32, st = sc.cached(("free", pair), lambda: sc.free_pair(E, hip_lib, panda["table"], 131))
    sc.check_free_steps(eng, ora, ora32, st, k, label="MI355X, PBRE_PAIR=" + pair)


@pytest.mark.parametrize("flags", [0, _capi.F_COMPLEX_ROWS, _capi.F_COMPLEX_LANES, _capi.F_FORCE_GENERAL])
@pytest.mark.parametrize("k", sc.CONTACT_COUNTS)
def test_contact_rich_states_against_the_oracle(panda, hip_lib, k, flags):
    """A2: 12 robot-table + 12 robot-object contact states, one step, TOL_CONTACT: k_row_list (the engine's choice and pinned), k_fast_rc,
    k_step -- each with its odd-count exit at 1, 3 and 51"""
    eng, ora, S = sc.cached(("contact", flags), lambda: sc.contact_pair(E, hip_lib, panda, flags))
    sc.check_contact_steps(eng, ora, S, k)


@pytest.mark.parametrize("kind", ["ro", "zip"])
@pytest.mark.parametrize("k", sc.FAMILY_COUNTS)
def test_row_path_families(panda, hip_lib, k, kind):
    """A3: every per-wave path of k_step's Core::step at 3 and 51 sweeps (each copy's odd exit) and at 300: (a) against the oracle, (b) a
    probe's record and row bit-identical whichever path its wave-mates put the wave on; at 51 and 300 (c), the RT copies, sweep counts
    included"""
    fam = sc.family_at(panda, kind, k)
    sc.row_paths.assert_coverage(fam)
    eng = sc.family_engine(fam, hip_lib, k)
    assert eng.kernel_info()[4] == fam.n
    for v in range(len(fam.variants)):
        sc.row_paths.check_oracle(fam, eng, v)
    sc.row_paths.check_path_independence(fam, eng)
    if k in sc.FAMILY_RT_COUNTS:
        for v in range(len(fam.variants)):
            sc.row_paths.check_residual_exit(fam, eng, v)
        eng.set_physics(solver_residual_threshold=1e-7)
        sc.row_paths.check_path_independence(fam, eng, sweeps=True)
    eng.close()


@pytest.mark.parametrize("kind", ["ro_clamp", "clamp"])
def test_bounded_motor_families_at_an_odd_count(panda, hip_lib, kind):
    """A3: motors that reach their impulse bound at 51 sweeps: (a) and (b)"""
    fam = sc.family_at(panda, kind, 51)
    sc.row_paths.assert_coverage(fam)
    eng = sc.family_engine(fam, hip_lib, 51)
    for v in range(len(fam.variants)):
        sc.row_paths.check_oracle(fam, eng, v)
    sc.row_paths.check_path_independence(fam, eng)
    eng.close()


@pytest.mark.parametrize("pair", ["1", "0"])
@pytest.mark.parametrize("k", [50, 52, 54, 56, 100, 300])
def test_residual_exit_against_the_oracle(panda, hip_lib, monkeypatch, k, pair):
    """A4: k_fast<MODE, WPS, RT> with the threshold on, on either side of the closed form's threshold (52 / 54) and far above it: sweep
    counts equal the oracle's, none above k"""
    monkeypatch.setenv("PBRE_PAIR", pair)
    rep = sc.check_residual_exit_at(E, hip_lib, panda["table"], k, n=48)
    print({kk: v for kk, v in rep.items() if kk not in ("worst", "worst_flip")})
    if k >= 100:
        assert rep["early"] == rep["compared"] + rep["flips"], "in the oracle every env leaves the loop before sweep %d" % k


@pytest.mark.parametrize("k", [56, 300])
def test_residual_exit_results_do_not_depend_on_wave_mates_or_sharding(panda, hip_lib, k):
    """A4: the lane-divergent code of the residual exit's closed form (obj_closed<PERLANE>'s per-lane exponents, motor_scan's exit pair) at
    counts other than 150: two engines side by side and a 2-shard split, bit-identical, sweep counts included"""
    exits = sc.check_residual_exit_wave_mates_and_sharding(E, hip_lib, panda, k)
    assert len(exits) >= 4 and exits[-1] <= k, exits


@pytest.mark.parametrize("lane", ["1", "0"])
@pytest.mark.parametrize("task", [0, 1])
@pytest.mark.parametrize("k", sc.GROUP_COUNTS)
def test_icub_against_the_oracle(hip_lib, monkeypatch, k, task, lane):
    """A5: iCub reach / push, joint control, the lane-per-env pipeline (pbre_lane.hip) and the lane-group kernel, 5 envs, TOL_ICUB"""
    monkeypatch.setenv("PBRE_ICUB_LANE", lane)
    eng, ora, st = sc.cached(("icub", task, lane), lambda: sc.icub_group(E, hip_lib, task, 5))
    assert eng.kernel_info()[2] == int(lane)
    sc.check_icub_steps(eng, ora, st, k)


@pytest.mark.parametrize("k", sc.GROUP_COUNTS)
def test_hands_against_the_oracle(hip_lib, k):
    """A5: iCub with hands, 3 envs, TOL_HANDS"""
    eng, ora, st, mrec, home = sc.cached(("hands",), lambda: sc.hands_group(E, hip_lib, 3))
    sc.check_hands_steps(eng, ora, st, mrec, home, k)


@pytest.mark.parametrize("k", sc.GROUP_COUNTS)
def test_robot_level_panda_against_the_oracle(hip_lib, k):
    """A5: parity.check_panda_arm with everything after its reset at k sweeps, TOL_PANDA_ARM"""
    parity.check_panda_arm(E, hip_lib, use_ik=0, n=3, solver_iters=k).close()
