"""The per-wave path matrix of the Panda row kernels on the GPU (generators and checks: tests/row_paths.py; CPU half: test_emu_row_paths.py).

Core::step picks its sweep code per WAVE from the union of the row sets of the wave's four envs.  These tests place envs so that the
union is known -- k_step (F_FORCE_GENERAL): envs 4k .. 4k+3 share a wave; k_row_list / k_fused's row blocks (F_COMPLEX_ROWS): at most four
uncoupled complex envs in the batch share wave 0, a coupled env has a wave to itself -- and drive every path on purpose:
 (a) one step against the oracle, TOL_CONTACT, nothing skipped, no outlier;
 (b) a probe env's state record and output row are bit-identical whichever path its three wave-mates put the wave on (no tolerance: this is
     the check that catches ONE wrong copy of a row -- the comments of pbre_core.hpp promise "the same arithmetic, bit for bit");
 (c) the same with solver_residual_threshold = 1e-7 (the RT copies), sweep counts included.
A limit row that is missing or lands on the wrong joint is invisible to (a) while the motors are unbounded (the position motor of the same
joint undoes its impulse within the sweep; the difference is rounding) -- (b) sees it, and (a) does in the families with bounded motors
("ro_clamp", "clamp"), where the limit rows decide where the joint goes.  Tried on a scratch build with the joint index of one inlined
limit-row copy changed (`limit2(LJ)` -> `limit2(LJ == 4 ? 3 : LJ)`): on the GPU (b) and (c) of the robot-only family fail for the joint-4
probes and nothing else does; on the emulation (a) of "ro_clamp" fails for the joint-4 probes only (qd off by 0.8 rad/s)."""
import pytest

import row_paths
from pybullet_robot_envs import _capi

pytestmark = pytest.mark.gpu

K_STEP_FAMILIES = ["ro", "ro_clamp", "zip", "clamp"]


def k_step_engine(fam, hip_lib):
    eng = fam.lab.engine(_capi.Engine, hip_lib, fam.n, fam.flags)
    assert eng.kernel_info()[4] == fam.n, "F_FORCE_GENERAL: every env is a row of k_step (env i: row i % 16 of block i / 16)"
    return eng


@pytest.mark.parametrize("kind", K_STEP_FAMILIES)
def test_k_step_waves_against_the_oracle(panda, hip_lib, kind):
    """(a) "ro": F_NO_OBJECT, the robot-only chain -- no limit, each LJ = 0..8 copy (lower and upper side), the loop with per-joint tests,
    with and without robot-table rows; "zip": the zipped chains by robot-object slot mask (1, 3, anything else), e_zip on and off, fewer than
    four object-table slots, the loops with per-slot tests; "ro_clamp" / "clamp": the same with motors that reach their impulse bound (the
    clamping motor stages bind, and the limit rows decide where a joint past its limit goes)."""
    fam = row_paths.family(panda, kind)
    row_paths.assert_coverage(fam)
    eng = k_step_engine(fam, hip_lib)
    for v in range(len(fam.variants)):
        row_paths.check_oracle(fam, eng, v)
    eng.close()


@pytest.mark.parametrize("kind", K_STEP_FAMILIES)
def test_k_step_results_do_not_depend_on_the_path_of_their_wave(panda, hip_lib, kind):
    """(b) env 4w is the same state with the same action in every variant of the family; its wave-mates put the wave on the LJ = j copy
    or the loop with per-joint tests, with or without the robot-table rows; on the zipped sweeps for slot mask 1, 3 or the generic ones,
    with e_zip or without, or on the loops with per-slot tests (row_paths.assert_coverage: every probe sees more than one path)."""
    fam = row_paths.family(panda, kind)
    row_paths.assert_coverage(fam)
    eng = k_step_engine(fam, hip_lib)
    row_paths.check_path_independence(fam, eng)
    eng.close()


@pytest.mark.parametrize("kind", ["ro", "zip"])
def test_k_step_waves_with_the_residual_exit(panda, hip_lib, kind):
    """(c) the RT copies: sweep counts equal the oracle's but for the one-sweep flips parity.check_residual_threshold allows, and a probe's
    result AND sweep count are bit-identical across wave-mates."""
    fam = row_paths.family(panda, kind)
    eng = k_step_engine(fam, hip_lib)
    for v in range(len(fam.variants)):
        row_paths.check_residual_exit(fam, eng, v)
    eng.set_physics(solver_residual_threshold=1e-7)
    row_paths.check_path_independence(fam, eng, sweeps=True)
    eng.close()


@pytest.mark.parametrize("fused", ["0", "1"])
def test_row_list_waves(panda, hip_lib, monkeypatch, fused):
    """F_COMPLEX_ROWS, 64 envs, one pattern per step: one to four crafted uncoupled envs (wave 0 of the only item, whatever order the atomics
    produce; the object is the object wave's, so the wave sweeps the robot-only chain: each LJ copy, the loop with per-joint tests, with and
    without robot-table rows) and a coupled env in a wave of its own, among simple envs -- (a) and (b), as k_row_list (PBRE_FUSED=0) and as
    k_fused's row blocks (the default)."""
    monkeypatch.setenv("PBRE_FUSED", fused)
    fams = row_paths.family(panda, "rows")
    row_paths.assert_rows_coverage(fams)
    eng = fams[0].lab.engine(_capi.Engine, hip_lib, row_paths.ROWS_N, fams[0].flags)
    for f in fams:
        for v, (S, A) in enumerate(f.variants):
            eng.set_state(S)
            assert eng.kernel_info()[5] == row_paths.complex_envs(f, v), "the engine classes other envs as complex than the oracle's contact sets say"
            row_paths.check_oracle(f, eng, v)
        row_paths.check_path_independence(f, eng)
    info = eng.kernel_info()
    assert (info[13] > 0) == (fused == "1") and info[12] == 0, info
    eng.close()
