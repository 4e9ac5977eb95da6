"""The per-wave path matrix of the Panda row kernels (tests/row_paths.py), CPU half.

The generator's own assertions -- every wave pattern is in the batches it returns, and no state in them is one the oracle calls
ill-conditioned -- and the comparison with the oracle through the host lane emulation.  A wave of the emulation holds ONE env
(tests/host_emu/emu_capi.cpp steps env by env), so this covers every single-env pattern, all nine one-limit-joint copies of the
robot-only chain among them, and shows without a GPU that the states are well conditioned and within TOL_CONTACT for the reference
arithmetic; the unions over wave-mates exist on the GPU only (tests/test_gpu_row_paths.py)."""
import numpy as np
import pytest

import row_paths
from pybullet_robot_envs import _capi

K_STEP_FAMILIES = ["ro", "ro_clamp", "zip", "clamp"]


@pytest.mark.parametrize("kind", K_STEP_FAMILIES)
def test_k_step_families_cover_every_wave_pattern(panda, kind):
    """robot-only chain: no limit / each LJ = 0..8 (lower and upper side, beside free envs, beside table-contact envs, beside a second group
    with the same joint) / two limit joints (in one env, in two envs), each with and without robot-table rows; zipped chains: 0 / 1 / 2 / 3-4
    robot-object slots, masks 1 and 3 in one wave, fewer than four object-table slots, the loops with per-slot tests, each with and
    without a limit joint and robot-table rows (e_zip on and off); and the pre-filter left nothing for check_single_steps to skip."""
    fam = row_paths.family(panda, kind)
    row_paths.assert_coverage(fam)
    if kind.startswith("ro"):
        sides = set((nm, pv[e // 4]) for nm_v, pv in zip(fam.names, fam.patterns) for e, nm in enumerate(nm_v) if e in fam.probes)
        for j in range(row_paths.NJ):
            for side in (0, 1):
                for rt in (0, 1):
                    assert ("lim:%d:%d" % (j, side), "ro/LJ%d/rt%d" % (j, rt)) in sides
                assert ("lim:%d:%d" % (j, side), "ro/multi/rt0") in sides      # ... and the same probe on the loop with per-joint tests
    for S, A in fam.variants:
        assert S.dtype == np.float32 and not row_paths.flagged(fam.lab, S, A).any()
        q = S[:, :row_paths.NJ].astype(np.float64)
        gap = np.minimum(np.abs(q - fam.lab.lo), np.abs(q - fam.lab.hi))
        assert gap.min() > 4e-4, "a joint ON its limit: fp32 rounding of the limit would flip the row"


def test_row_list_batches_cover_every_wave_pattern(panda):
    fams = row_paths.family(panda, "rows")
    row_paths.assert_rows_coverage(fams)
    for f in fams:
        for S, A in f.variants:
            assert not row_paths.flagged(f.lab, S, A).any()


@pytest.mark.parametrize("kind", K_STEP_FAMILIES)
def test_single_env_waves_against_the_oracle(panda, emu_lib, kind):
    """check (a) on the emulation: one step of every variant, TOL_CONTACT, nothing skipped, no outlier"""
    fam = row_paths.family(panda, kind)
    eng = fam.lab.engine(_capi.Engine, emu_lib, fam.n, fam.flags)
    for v in range(len(fam.variants)):
        row_paths.check_oracle(fam, eng, v)
    eng.close()


def test_row_list_batches_against_the_oracle(panda, emu_lib):
    fams = row_paths.family(panda, "rows")
    eng = fams[0].lab.engine(_capi.Engine, emu_lib, row_paths.ROWS_N, fams[0].flags)
    for f in fams:
        for v in range(len(f.variants)):
            before = eng.kernel_info()[5]         # (the emulation counts the env-steps its complex-env path has taken so far)
            row_paths.check_oracle(f, eng, v)
            assert eng.kernel_info()[5] - before == row_paths.complex_envs(f, v), "the engine classes other envs as complex than the oracle's contact sets say"
    eng.close()


@pytest.mark.parametrize("kind", ["ro", "zip"])
def test_single_env_waves_with_the_residual_exit(panda, emu_lib, kind):
    """check (c) on the emulation: the RT copies of the same paths, sweep counts against the oracle's"""
    fam = row_paths.family(panda, kind)
    eng = fam.lab.engine(_capi.Engine, emu_lib, fam.n, fam.flags)
    for v in range(len(fam.variants)):
        row_paths.check_residual_exit(fam, eng, v)
    eng.close()
