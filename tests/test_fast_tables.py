"""The per-joint packing of the Panda model constants (csrc/pbre_tables.hpp: FastTables) that the lane-per-env step code reads (CPU only).

 * pack_fast_tables() field by field, the sphere ranges and their order: a stand-alone host program built with the address and
   undefined-behaviour sanitizers (tests/fast_tables).
 * The lane-per-env code reading the packed tables against the same code reading the lane-SoA `Tables` (-DPBRE_FAST_TABLES=0): only the
   source of an operand differs between the two builds, so rows and states must agree bit for bit, step by step.  Both are built by this
   test's own recipe (tests/fast_tables/Makefile) from tests/host_emu/emu_capi.cpp with the same compiler flags; the emulation hands `Tables`
   to Fast's host-only overloads, which pack it per call in the packed build."""
import os
import subprocess

import numpy as np
import pytest

import step_batch
from pybullet_robot_envs import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "fast_tables")


def test_pack_fast_tables_under_sanitizers():
    subprocess.check_call(["make", "-s", "-C", DIR, "build/pack_check"])
    r = subprocess.run([os.path.join(DIR, "build", "pack_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout
    assert int(r.stdout.split()[1]) > 1500          # 7 cases x (9 joints x 57 fields + the scalars + the spheres)


@pytest.fixture(scope="module")
def table_libs(built):
    """(packed build, lane-SoA build) of the emulation, compiled side by side"""
    targets = ["build/libpbre_emu_tables1.so", "build/libpbre_emu_tables0.so"]
    subprocess.check_call(["make", "-s", "-j2", "-C", DIR] + targets)
    return tuple(_capi.load(os.path.join(DIR, t)) for t in targets)


@pytest.fixture(scope="module")
def crafted(panda):
    return step_batch.crafted_states(panda)


# which code steps the complex envs: the lane-per-env step_rc (the emulation's default and F_COMPLEX_LANES: the candidate lists and their
# tie-break), the row kernel + Fast::finish (F_COMPLEX_ROWS); pair: the simple envs split over a robot and an object half (PBRE_PAIR=1:
# the sphere centres parked by one half of the sweep, tested by the other)
@pytest.mark.parametrize("flags,pair", [(0, False), (_capi.F_COMPLEX_LANES, False), (_capi.F_COMPLEX_ROWS, False), (0, True)])
def test_packed_tables_bit_identical_to_lane_soa_tables(panda, table_libs, crafted, monkeypatch, flags, pair):
    monkeypatch.setenv("PBRE_PAIR", "1" if pair else "0")
    kw = dict(step_batch.KW, num_envs=step_batch.N, flags=step_batch.F_AUTO_RESET | flags)
    a = _capi.Engine(panda["table"], lib=table_libs[0], **kw)
    b = _capi.Engine(panda["table"], lib=table_libs[1], **kw)
    sa, sb = step_batch.start_state(a, crafted), step_batch.start_state(b, crafted)
    assert np.array_equal(sa, sb), "reset differs between the two table layouts"
    ra, xa = step_batch.run(a)
    rb, xb = step_batch.run(b)
    for k in range(step_batch.STEPS):
        assert np.array_equal(ra[k], rb[k]), "step %d: rows differ" % k
        assert np.array_equal(xa[k], xb[k]), "step %d: states differ" % k
    # the batch did what it is for: complex envs of both kinds, snapshot resets at step 3 and at max_steps, the split step
    ia, ib = a.kernel_info(), b.kernel_info()
    assert list(ia) == list(ib)
    assert ia[3] > 0 and ia[5] >= len(crafted) and (ia[10] > 0) == pair, ia      # [3] simple, [5] complex env-steps, [10] of them split
    done = ra[:, :, -1] != 0
    assert done[2, step_batch.SHORT[2:]].all() and done.any(0).all()
    assert (xa[-1][:, 37] >= 1).all()              # every env is in its second episode at least
    a.close(); b.close()
