"""Robot-object contacts region by region at arbitrary object poses (tests/contact_regions.py), CPU half.

The generator's own assertions -- every region of every object is in its batch, the fp64 oracle's normal, distance and contact point equal
the region's closed form, the oracle lists that one contact and nothing else, and it calls every state well conditioned -- and the
comparison of one step with the oracle through the host lane emulation, every env compared, no outlier allowance, the worst error
reported per region.  tests/test_gpu_contact_regions.py replays the same batches on the device."""
import numpy as np
import pytest

import contact_regions as cr
import row_paths
from pybullet_robot_envs import _capi

SETS = [False, True]         # at rest / moving
FLAGS = {"general": _capi.F_FORCE_GENERAL, "rows": _capi.F_COMPLEX_ROWS, "lanes": _capi.F_COMPLEX_LANES, "default": 0}


@pytest.mark.parametrize("moving", SETS)
@pytest.mark.parametrize("name", cr.OBJECTS)
def test_states_are_single_contacts_in_every_region(panda, name, moving):
    """the batch exists (cr.build raises otherwise: a region without a single-contact state, a closed form the oracle disagrees with, states
    that stay ill conditioned), holds every region at least six times, and the probe of parity.check_single_steps would skip nothing"""
    b = cr.batch(panda, name, moving)
    cr.assert_coverage(b)
    assert b.S.dtype == np.float32 and not row_paths.flagged(b.lab, b.S, b.A).any()
    for e in range(b.n):                                             # (again, on the batch as it is replayed)
        assert cr.accept(b.lab, b.S[e], int(b.sphere[e]), b.forms[e]) is not None, (name, b.region[e], e)
    q = b.S[:, :cr.NJ].astype(np.float64)
    assert np.minimum(q - b.lab.lo, b.lab.hi - q).min() > 1e-3
    assert (np.abs(b.S[:, 16:31]).max() > 0) == moving


def step_counts(eng):
    i = eng.kernel_info()
    return np.array([i[3], i[4], i[5]])          # env-steps so far: lane-per-env simple path, general kernel, complex-env path


@pytest.mark.parametrize("kernel", list(FLAGS))
@pytest.mark.parametrize("moving", SETS)
@pytest.mark.parametrize("name", [n for n in cr.OBJECTS if n not in cr.HULLS])
def test_primitives_against_the_oracle(panda, emu_lib, name, moving, kernel):
    """box, cube, ball and cans: the lane form (Core::sphere_box / sphere_round) under every flag, and for the cube under "lanes" / "default"
    the scalar form Fast::sphere_box of the lane-per-env robot-contact code -- the emulation sends every other primitive's complex envs
    to the row code whatever the flag (emu_capi.cpp: step_env), as the device does."""
    b = cr.batch(panda, name, moving)
    eng = b.lab.engine(_capi.Engine, emu_lib, b.n, FLAGS[kernel])
    before = step_counts(eng)
    cr.compare(b, eng, tag=kernel)
    took = step_counts(eng) - before
    want = [0, b.n, 0] if kernel == "general" else [0, 0, b.n]       # every env has a robot-object contact: none is simple
    assert took.tolist() == want, (kernel, took)
    eng.close()


@pytest.mark.parametrize("moving", SETS)
@pytest.mark.parametrize("name", cr.HULLS)
def test_hulls_against_the_oracle(panda, emu_lib, name, moving):
    """Core::sphere_hull: face, each edge select (the tetrahedron's six edges: AB, AC or BC of some triangle decides), vertex, inside"""
    b = cr.batch(panda, name, moving)
    eng = b.lab.engine(_capi.Engine, emu_lib, b.n, 0)
    before = step_counts(eng)
    cr.compare(b, eng, tag="general")
    assert (step_counts(eng) - before).tolist() == [0, b.n, 0], "a hull is stepped by the general kernel"
    eng.close()


def test_icub_states_are_single_contacts():
    b = cr.icub_batch()
    import parity
    assert b.S.dtype == np.float32 and not b.lab.flagged(b.S, b.A, parity.TOL_ICUB_CONTACT).any()
    for e in range(b.n):
        assert b.lab.accept(b.S[e], int(b.sphere[e]), b.forms[e]) is not None, (b.region[e], e)
    for e in range(b.n):
        if b.region[e] == "in_lat":
            s = b.S[e].astype(np.float64)
            c, _ = b.lab.centre(s[:b.lab.nd], int(b.sphere[e]))
            p = cr.quat_R(s[b.lab.nd + 3:b.lab.nd + 7]).T @ (c - s[b.lab.nd:b.lab.nd + 3])
            assert 0.016 < np.hypot(p[0], p[1]) < b.shape.r


@pytest.mark.parametrize("lane", ["1", "0"])
def test_icub_push_with_the_can_against_the_oracle(emu_lib, monkeypatch, lane):
    """a hand sphere of the iCub's controlled arm on the cap, the lateral surface, the rim and inside the soup can: the lane-per-env
    pipeline (its complex envs: Core at 32 lanes behind the classifier's scalar distance) and the lane-group kernel, TOL_ICUB_CONTACT"""
    monkeypatch.setenv("PBRE_ICUB_LANE", lane)
    b = cr.icub_batch()
    eng = b.lab.engine(_capi.Engine, emu_lib, b.n)
    assert eng.kernel_info()[2] == int(lane)
    before = step_counts(eng)
    cr.icub_compare(b, eng, tag="icub_lane" + lane)
    assert (step_counts(eng) - before).tolist() == ([0, 0, b.n] if lane == "1" else [0, b.n, 0])
    eng.close()
