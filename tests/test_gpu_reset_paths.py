"""The shared reset() of the device engines, branch by branch (tests/reset_paths.py): full reset in place and partial reset through the
compacted scratch buffer, for the Panda engine, the iCub (a full reset settles through the lane-per-env pipeline, a partial one through
the lane-group kernel), the iCub with hands and the two robot-level engines."""
import pytest

import reset_paths
from pybullet_robot_envs import _capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", sorted(reset_paths.SHAPES))
def test_reset_paths(hip_lib, panda, kind):
    reset_paths.check(_capi.Engine, hip_lib, kind, panda["table"])


def test_icub_reset_paths_on_the_lane_group_kernel(hip_lib, monkeypatch):
    monkeypatch.setenv("PBRE_ICUB_LANE", "0")
    reset_paths.check(_capi.Engine, hip_lib, "icub")
