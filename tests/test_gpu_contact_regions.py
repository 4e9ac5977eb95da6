"""Robot-object contacts region by region at arbitrary object poses, on the GPU (generator and comparison: tests/contact_regions.py; CPU
half, with the generator's own assertions: test_emu_contact_regions.py).

One collision sphere of the Panda's hand in a named region of the object -- face, edge, vertex, inside of a box or a hull; cap, lateral
surface, rim, axis, inside of a can; a ball -- at a uniformly random orientation, at rest and moving; one step from the identical float32
states against the fp64 oracle, parity.TOL_CONTACT, every env compared, no outlier allowance, the worst error per region.  Which kernel
stepped the envs is read back from pbre_kernel_info, not assumed:
  general   F_FORCE_GENERAL: k_step, env i is row i % 16 of block i / 16 ([4] = the batch);
  rows      F_COMPLEX_ROWS: every env is complex ([5] = the batch) and the step is the one launch whose row blocks take them ([13] counts it);
  lanes     F_COMPLEX_LANES: for the CUBE the lane-per-env robot-contact kernel k_fast_rc (Fast::sphere_box; [13] stays 0) -- for every other
            primitive the launcher sends complex envs to the row blocks whatever the flag (pbre_panda.hpp: launch_step_t), and [13] says so;
  default   a batch this small: the row blocks.
A batch is 12 to 78 envs: full 16-row blocks and a partial one on the general kernel, four envs per wave.

What these tests see, tried on scratch builds of the lane emulation (CPU half of this file's cases):
  * without the rule "a centre with rho <= radius and |z| <= half height is inside" every can case and both iCub cases fail in the regions
    in_lat and in_cap (object velocity off by up to 3.3 m/s, angular velocity by up to 57 rad/s after one step); everything else passes;
  * Core::sphere_round rotating its normal with the transposed matrix: every can case and both iCub cases fail;
    test_emu_parity.py::test_round_objects (identity poses) passes;
  * Core::sphere_hull with the edge select rAB forced off: all four hull cases fail, and so does test_emu_parity.py::test_convex_hull_objects;
  * Shapes::sphere_round rotating its normal with the transposed matrix: NOTHING fails on the emulation -- it executes that function for
    distances only (the classifiers); its normal and contact point are used by the device's iCub pipeline alone (kw_dyn's robot-object
    candidates), which the emulation replaces by Core::step.  The iCub case with PBRE_ICUB_LANE=1 below is the one test that runs it."""
import pytest

import contact_regions as cr
from pybullet_robot_envs import _capi

pytestmark = pytest.mark.gpu

SETS = [False, True]
FLAGS = {"general": _capi.F_FORCE_GENERAL, "rows": _capi.F_COMPLEX_ROWS, "lanes": _capi.F_COMPLEX_LANES, "default": 0}


@pytest.mark.parametrize("kernel", list(FLAGS))
@pytest.mark.parametrize("moving", SETS)
@pytest.mark.parametrize("name", [n for n in cr.OBJECTS if n not in cr.HULLS])
def test_primitives_against_the_oracle(panda, hip_lib, name, moving, kernel):
    b = cr.batch(panda, name, moving)
    eng = b.lab.engine(_capi.Engine, hip_lib, b.n, FLAGS[kernel])
    eng.set_state(b.S)
    info = eng.kernel_info()
    if kernel == "general":
        assert info[2] == 0 and info[4] == b.n, info
    else:
        assert info[2] == 1 and info[3] == 0 and info[5] == b.n, ("every env has a robot-object contact: the engine must class all of them as complex", info)
    cr.compare(b, eng, tag=kernel)
    info = eng.kernel_info()
    assert info[12] == 0, "NaN / Inf guard counted a bad env"
    if kernel != "general":
        rc_kernel = kernel == "lanes" and name == "cube_small"
        assert info[13] == (0 if rc_kernel else 1), ("k_fast_rc" if rc_kernel else "the row blocks of the one-launch step", info)
    eng.close()


@pytest.mark.parametrize("moving", SETS)
@pytest.mark.parametrize("name", cr.HULLS)
def test_hulls_against_the_oracle(panda, hip_lib, name, moving):
    """Core::sphere_hull on k_step: face, every edge select (the tetrahedron's six edges), vertex, inside"""
    b = cr.batch(panda, name, moving)
    eng = b.lab.engine(_capi.Engine, hip_lib, b.n, 0)
    eng.set_state(b.S)
    info = eng.kernel_info()
    assert info[2] == 0 and info[4] == b.n, ("a hull is stepped by the general kernel", info)
    cr.compare(b, eng, tag="general")
    assert eng.kernel_info()[12] == 0
    eng.close()


@pytest.mark.parametrize("lane", ["1", "0"])
def test_icub_push_with_the_can_against_the_oracle(hip_lib, monkeypatch, lane):
    """a hand sphere of the iCub's controlled arm on the cap, the lateral surface, the rim and inside the soup can: the lane-per-env
    pipeline (every env is in its complex class) and the lane-group kernel, TOL_ICUB_CONTACT"""
    monkeypatch.setenv("PBRE_ICUB_LANE", lane)
    b = cr.icub_batch()
    eng = b.lab.engine(_capi.Engine, hip_lib, b.n)
    eng.set_state(b.S)
    info = eng.kernel_info()
    assert info[2] == int(lane) and (info[5] == b.n and info[3] == 0 if lane == "1" else info[4] == b.n), info
    cr.icub_compare(b, eng, tag="icub_lane" + lane)
    assert eng.kernel_info()[12] == 0
    eng.close()
