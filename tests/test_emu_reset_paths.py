"""The shared reset() of the engines, branch by branch, on the lane emulation (tests/reset_paths.py): the emulation library executes the
same sequence text as the device library (csrc/pbre_reset_seq.hpp)."""
import pytest

import reset_paths
from pybullet_robot_envs import _capi


@pytest.mark.parametrize("kind", sorted(reset_paths.SHAPES))
def test_reset_paths(emu_lib, panda, kind):
    reset_paths.check(_capi.Engine, emu_lib, kind, panda["table"])


def test_icub_reset_paths_on_the_lane_group_kernel(emu_lib, monkeypatch):
    monkeypatch.setenv("PBRE_ICUB_LANE", "0")
    reset_paths.check(_capi.Engine, emu_lib, "icub")
