"""The lane-per-env step kernels reading the per-joint packed model constants (csrc/pbre_tables.hpp: FastTables) compute what they
computed from the lane-SoA `Tables`: the batch of tests/step_batch.py -- 130 envs, 40 steps, default dispatch (k_fused: the simple envs'
waves, the row waves with Fast::finish on all 16 lanes of a group) -- against tests/golden/step_batch_panda.npz, recorded with the GPU
build of the commit before the packed tables (tools/make_golden_step_batch.py), bit for bit: the start state after reset(), the SHA-256 of
the rows and of the states of every step, and steps 1, 3 and 40 in full (so that a mismatch says where)."""
import os

import numpy as np
import pytest

import step_batch
from pybullet_robot_envs import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_step_batch_matches_golden_of_lane_soa_tables(panda, hip_lib):
    g = np.load(os.path.join(ROOT, "tests", "golden", "step_batch_panda.npz"))
    eng = _capi.Engine(panda["table"], lib=hip_lib, num_envs=step_batch.N, flags=step_batch.F_AUTO_RESET, **step_batch.KW)
    st0 = step_batch.start_state(eng, g["crafted"])
    assert np.array_equal(st0, g["st0"]), "the state after reset() differs"
    complex0 = eng.kernel_info()[7]                # running sum of complex env-steps (the settle steps of reset() included)
    rows, states = step_batch.run(eng)
    for i, k in enumerate(g["full_steps"]):
        bad = np.nonzero((rows[k] != g["rows"][i]).any(1) | (states[k] != g["states"][i]).any(1))[0]
        assert len(bad) == 0, "step %d: envs %s differ from the golden" % (k + 1, bad.tolist())
    for k in range(step_batch.STEPS):
        assert step_batch.digest(rows[k]) == str(g["rows_sha256"][k]), "step %d: rows differ from the golden" % (k + 1)
        assert step_batch.digest(states[k]) == str(g["states_sha256"][k]), "step %d: states differ from the golden" % (k + 1)
    # the run took the paths the sorted sphere indexing changes on the device: the one-launch step in its pair form (130 envs: a robot and an
    # object wave per 64 envs -- the sphere centres parked by one, tested by the other) and complex envs on the row waves (Fast::finish<3>: the
    # sphere tests dealt out over the 16 lanes of a group) -- the host emulation never instantiates that role
    info = eng.kernel_info()
    assert info[3] > 0                                          # the lane-per-env path
    assert info[13] >= step_batch.STEPS and info[10] >= step_batch.STEPS, info      # fused launches, of them with robot / object wave pairs
    assert info[7] - complex0 >= len(g["crafted"]), (info, complex0)              # complex env-steps among the 40 steps
    eng.close()
