"""Compound objects on the CPU: the loader (model/objects.py), the C-ABI's piece validation and the narrow phase on the lane emulation
(tests/host_emu runs the same csrc/pbre_core.hpp as the GPU kernels)."""
import os
import warnings

import numpy as np
import pytest

import compound_ref as cr
from pybullet_robot_envs.model import objects


def _write_obj(path, pieces, tag="o"):
    with open(path, "w") as f:
        for k, p in enumerate(pieces):
            if tag:
                f.write("%s piece%d\n" % (tag, k))
            for v in p:
                f.write("v %.9g %.9g %.9g\n" % tuple(v))
            f.write("f 1 2 3\n")


def _blob(seed, c, r, n=20):
    g = np.random.default_rng(seed)
    d = g.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    return np.asarray(c) + d * r


def test_read_obj_pieces_splits_at_groups(tmp_path):
    p = str(tmp_path / "m.obj")
    _write_obj(p, [_blob(k, (0.1 * k, 0, 0), 0.03) for k in range(3)], tag="g")
    pcs = objects.read_obj_pieces(p)
    assert len(pcs) == 3 and all(len(x) == 20 for x in pcs)


def test_six_pieces_merge_to_four(tmp_path):
    p = str(tmp_path / "m.obj")
    _write_obj(p, [_blob(k, (0.05 * k, 0.01 * (k % 2), 0), 0.02) for k in range(6)])
    ph = objects.compound_physics(objects.read_obj_pieces(p), 0.1, 1.0)
    pcs = objects.hull_pieces(ph["obj_hull"])
    assert len(pcs) == 4 and all(4 <= len(x) <= 32 for x in pcs)
    assert np.isnan(ph["obj_hull"]).all(axis=1).sum() == 3


def test_two_cube_mass_properties_are_analytic():
    a, d, m = 0.02, 0.03, 0.3                                        # 2 cm cubes, centres 3 cm apart along x
    ph = objects.compound_physics([cr.cube((0.1, 0.2, 0.3), a / 2), cr.cube((0.1 + d, 0.2, 0.3), a / 2)], m, 1.0)
    pcs = objects.hull_pieces(ph["obj_hull"])
    # the centre of mass is the origin of the returned frame: the pieces' centroids sit at -+ d / 2 along x
    assert np.allclose(pcs[0].mean(0), [-d / 2, 0, 0], atol=1e-12) and np.allclose(pcs[1].mean(0), [d / 2, 0, 0], atol=1e-12)
    mh = m / 2
    Ic = mh * (a * a + a * a) / 12.0
    want = [2 * Ic, 2 * (Ic + mh * (d / 2) ** 2), 2 * (Ic + mh * (d / 2) ** 2)]
    assert np.allclose(ph["obj_inertia"], want, rtol=0, atol=1e-9 * max(want) + 1e-15)
    assert abs(ph["obj_inertia"][1] - want[1]) < 1e-9 and ph["obj_h"] == pytest.approx([d / 2 + a / 2, a / 2, a / 2], abs=1e-12)


def test_urdf_scale_shrinks_the_hull(tmp_path, monkeypatch):
    big = [_blob(k, (1.0 * k, 0, 0), 0.6) for k in range(3)]          # 20x the size of duck_vhacd's table entry
    _write_obj(str(tmp_path / "duck_vhacd.obj"), big)
    monkeypatch.setenv("PBRE_OBJECT_MESH_DIR", str(tmp_path))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        unscaled = objects.object_physics("duck_vhacd")                 # no URDF: the 20x mesh as it is
    with open(str(tmp_path / "duck_vhacd.urdf"), "w") as f:
        f.write('<robot name="duck"><link name="base"><collision><origin xyz="0.01 0 0" rpy="0 0 0"/><geometry>'
                '<mesh filename="duck_vhacd.obj" scale="0.05 0.05 0.05"/></geometry></collision></link></robot>')
    ph = objects.object_physics("duck_vhacd")
    assert ph["obj_shape"] == objects.SHAPE_HULL and len(objects.hull_pieces(ph["obj_hull"])) == 3
    assert np.allclose(np.asarray(ph["obj_h"]) * 20, unscaled["obj_h"], rtol=1e-9)


def test_urdf_scale_far_off_the_table_falls_back_to_the_primitive(tmp_path, monkeypatch):
    _write_obj(str(tmp_path / "duck_vhacd.obj"), [_blob(k, (1.0 * k, 0, 0), 0.6) for k in range(2)])
    with open(str(tmp_path / "duck_vhacd.urdf"), "w") as f:
        f.write('<robot name="d"><link name="b"><collision><geometry><mesh filename="duck_vhacd.obj" scale="1 1 1"/></geometry>'
                '</collision></link></robot>')
    monkeypatch.setenv("PBRE_OBJECT_MESH_DIR", str(tmp_path))
    with pytest.warns(UserWarning, match="more than 3x off"):
        ph = objects.object_physics("duck_vhacd")
    assert ph == objects._primitive_physics("duck_vhacd")


def test_degenerate_groups_are_folded_into_a_neighbour():
    """a group with fewer than 4 points or a flat one (material groups of a visual mesh) joins the group nearest to it instead of
    sending the whole object to the primitive"""
    flat = np.array([[0.1, 0, 0], [0.12, 0, 0], [0.1, 0.02, 0], [0.12, 0.02, 0]])
    pcs = [_blob(1, (0, 0, 0), 0.03), np.array([[0.0, 0.0, 0.05], [0.01, 0.0, 0.05]]), _blob(2, (0.1, 0, 0), 0.03), flat]
    ph = objects.compound_physics(pcs, 0.1, 1.0)
    assert len(objects.hull_pieces(ph["obj_hull"])) == 2 and np.isfinite(ph["obj_inertia"]).all()


def test_greedy_merge_of_many_pieces_is_quick():
    import time
    pcs = [_blob(k, (0.03 * (k % 8), 0.03 * (k // 8), 0), 0.012, n=16) for k in range(32)]
    t0 = time.perf_counter()
    ph = objects.compound_physics(pcs, 0.1, 1.0)
    assert len(objects.hull_pieces(ph["obj_hull"])) == 4 and time.perf_counter() - t0 < 30.0


def test_one_group_mesh_is_the_plain_hull(tmp_path):
    p = str(tmp_path / "m.obj")
    v = _blob(3, (0, 0, 0), 0.04, n=40)
    _write_obj(p, [v])
    assert len(objects.read_obj_pieces(p)) == 1
    prim = objects._primitive_physics("YcbPear")
    a = objects.hull_physics(objects.read_obj_vertices(p), prim["obj_mass"], prim["obj_mu"])
    os.environ["PBRE_OBJECT_MESH_DIR"] = str(tmp_path)
    try:
        os.rename(p, str(tmp_path / "YcbPear.obj"))
        b = objects.object_physics("YcbPear")
    finally:
        del os.environ["PBRE_OBJECT_MESH_DIR"]
    assert np.array_equal(a["obj_hull"], b["obj_hull"]) and a["obj_inertia"] == b["obj_inertia"] and a["obj_h"] == b["obj_h"]


def test_select_slots_rule():
    flat = [np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1]], float), np.array([[3, 0, 0], [4, 0, 0], [3, 1, 0], [4, 1, 0]], float)]
    depth = [p[:, 2] for p in flat]
    assert cr.select_slots(flat, depth, 1e-3) == [(0, 0), (0, 3), (1, 0), (1, 3)]      # two spans
    one = cr.select_slots([flat[0], flat[1] + [0, 0, 1]], [depth[0], depth[1] + 1], 1e-3)
    assert one == [(0, 0), (0, 1), (0, 2), (0, 3)]                                        # one piece: its deepest four


def test_compound_abi_validation(emu_lib, panda):
    from pybullet_robot_envs import _capi
    cr.check_abi(_capi.Engine, emu_lib, panda["table"])


def test_single_piece_is_bit_identical_to_the_box(emu_lib, panda):
    from pybullet_robot_envs import _capi
    cr.check_single_piece_identity(_capi.Engine, emu_lib, panda["table"])


def test_dumbbell_gap_has_no_contact(emu_lib, panda):
    from pybullet_robot_envs import _capi
    cr.check_gap(_capi.Engine, emu_lib, panda["table"], panda)


def test_stem_in_touch_against_the_oracle(emu_lib, panda):
    from pybullet_robot_envs import _capi
    cr.check_stem(_capi.Engine, emu_lib, panda["table"])


def test_dumbbell_comes_to_rest_on_both_pieces(emu_lib, panda):
    from pybullet_robot_envs import _capi
    cr.check_rest_kat(_capi.Engine, emu_lib, panda["table"])


def test_multi_engine_forwards_compounds(emu_lib, panda):
    from pybullet_robot_envs import _capi
    ph = cr.dumbbell()
    one = objects.hull_physics(cr.cube((0, 0, 0), 0.025), 0.1, 1.0)
    shards = [_capi.Engine(panda["table"], task=1, num_envs=2, lib=emu_lib, phys=one) for _ in range(2)]
    me = _capi.MultiEngine.__new__(_capi.MultiEngine)          # (the shards of a MultiEngine without devices to put them on)
    me.shards = shards
    me.set_object_hull(ph["obj_hull"])
    for e in shards:
        assert list(e.get_physics().obj_h) == pytest.approx(ph["obj_h"], abs=1e-12)
        e.close()


def test_sphere_inside_each_piece_against_the_oracle(emu_lib, panda):
    from pybullet_robot_envs import _capi
    print(cr.check_sphere_on_pieces(_capi.Engine, emu_lib, panda["table"], panda))


def test_icub_sphere_inside_each_piece_against_the_oracle(emu_lib, monkeypatch):
    from pybullet_robot_envs import _capi
    monkeypatch.setenv("PBRE_ICUB_LANE", "0")
    print(cr.check_icub_sphere_on_pieces(_capi.Engine, emu_lib))


def test_kernel_slots_match_the_rule(emu_lib, panda):
    from pybullet_robot_envs import _capi
    print(cr.check_slots_against_oracle(_capi.Engine, emu_lib, panda["table"]))
