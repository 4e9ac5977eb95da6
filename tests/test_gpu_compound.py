"""Compound objects on the GPU: the Panda general row kernel (k_step, 16 lanes per env), the iCub's kw_step (32 lanes) and the hands engine
(tests/compound_ref.py holds the checks and the Python restatement of the slot selection)."""
import os
import warnings

import numpy as np
import pytest

import compound_ref as cr
import parity


@pytest.mark.gpu
def test_gpu_compound_abi_validation(hip_lib, panda):
    from pybullet_robot_envs import _capi
    cr.check_abi(_capi.Engine, hip_lib, panda["table"])


@pytest.mark.gpu
def test_gpu_single_piece_is_bit_identical_to_the_box(hip_lib, panda):
    from pybullet_robot_envs import _capi
    cr.check_single_piece_identity(_capi.Engine, hip_lib, panda["table"])


@pytest.mark.gpu
def test_gpu_dumbbell_gap_has_no_contact(hip_lib, panda):
    from pybullet_robot_envs import _capi
    cr.check_gap(_capi.Engine, hip_lib, panda["table"], panda)


@pytest.mark.gpu
def test_gpu_stem_in_touch_against_the_oracle(hip_lib, panda):
    from pybullet_robot_envs import _capi
    cr.check_stem(_capi.Engine, hip_lib, panda["table"])


@pytest.mark.gpu
def test_gpu_dumbbell_comes_to_rest_on_both_pieces(hip_lib, panda):
    from pybullet_robot_envs import _capi
    cr.check_rest_kat(_capi.Engine, hip_lib, panda["table"])


def _at_rest_on_the_table(eng, ph, s):
    """tilt, speed and both pieces' lowest points against the table top, for any engine's state layout"""
    o, v = eng.obj_off, eng.v_off + eng.obj_off
    phys = eng.get_physics()
    top = phys.table_c[2] + phys.table_h[2]
    for e in range(s.shape[0]):
        R = cr._quat_R(s[e, o + 3:o + 7])
        assert np.arccos(np.clip(R[2, 2], -1, 1)) < 1e-3, (e, s[e, o + 3:o + 7])
        assert np.linalg.norm(s[e, v:v + 3]) < 1e-3 and np.linalg.norm(s[e, v + 3:v + 6]) < 1e-3, s[e, v:v + 6]
        for p in cr.hull_pieces(ph["obj_hull"]):
            assert abs((s[e, o:o + 3] + p @ R.T)[:, 2].min() - top) <= phys.linear_slop + 1e-6


@pytest.mark.gpu
def test_gpu_icub_kw_step_compound(hip_lib, monkeypatch):
    """the iCub's lane-group kernel (kw_step) with the dumbbell: malformed compounds refused, the dumbbell rests on both pieces after a
    reset and 300 zero-action steps"""
    from pybullet_robot_envs import _capi
    monkeypatch.setenv("PBRE_ICUB_LANE", "0")
    ph = cr.dumbbell()
    eng, _, _ = parity.make_icub_pair(_capi.Engine, hip_lib, 4, use_ik=0)
    eng.set_physics(obj_mass=ph["obj_mass"], obj_mu=ph["obj_mu"], obj_inertia=ph["obj_inertia"], obj_hull=ph["obj_hull"])
    with pytest.raises(RuntimeError, match="libpbre error -1"):
        eng.set_object_hull(cr.join([cr.cube((0.05 * k, 0, 0), 0.01) for k in range(5)]))
    assert list(eng.get_physics().obj_h) == pytest.approx(ph["obj_h"], abs=1e-7)
    eng.reset()
    z = np.zeros((4, eng.act_dim), np.float32)
    for _ in range(300):
        eng.step(z)
    s = eng.get_state().astype(np.float64)
    assert np.isfinite(s).all() and eng.kernel_info()[12] == 0
    _at_rest_on_the_table(eng, ph, s)
    eng.close()


@pytest.mark.gpu
def test_gpu_hands_compound_smoke(hip_lib):
    """the hands engine (128 virtual lanes) with a compound brick: 64 envs, 20 steps, finite state"""
    from pybullet_robot_envs import _capi
    eng, _, _ = parity.make_hands_pair(_capi.Engine, hip_lib, 64)
    ph = cr.compound_physics([cr.box((-0.02, 0, 0), (0.02, 0.03, 0.025)), cr.box((0.02, 0, 0), (0.02, 0.03, 0.025))], 0.1, 1.0)
    eng.set_physics(obj_mass=ph["obj_mass"], obj_inertia=ph["obj_inertia"], obj_hull=ph["obj_hull"])
    eng.reset()
    rng = np.random.default_rng(2)
    for _ in range(20):
        eng.step(rng.uniform(-1, 1, (64, eng.act_dim)).astype(np.float32))
    assert np.isfinite(eng.get_state()).all() and eng.kernel_info()[12] == 0
    eng.close()


@pytest.mark.gpu
def test_gpu_push_env_with_a_vhacd_duck(hip_lib, tmp_path, monkeypatch):
    """pandaPushGymEnv(obj_name="duck_vhacd") with a 3-group mesh at 20x and its URDF (scale 0.05): a compound at the URDF's scale on the
    general kernel, 200 auto-reset steps finite"""
    from pybullet_robot_envs.envs import pandaPushGymEnv
    from pybullet_robot_envs.model import objects
    g = np.random.default_rng(4)
    with open(str(tmp_path / "duck_vhacd.obj"), "w") as f:
        for k in range(3):
            f.write("o part%d\n" % k)
            d = g.normal(size=(24, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
            for v in np.array([0.5 * (k - 1), 0, 0.2 * k]) + d * [0.6, 0.6, 0.5]:
                f.write("v %.7f %.7f %.7f\n" % tuple(v))
    with open(str(tmp_path / "duck_vhacd.urdf"), "w") as f:
        f.write('<robot name="duck"><link name="base"><collision><geometry><mesh filename="duck_vhacd.obj" scale="0.05 0.05 0.05"/>'
                '</geometry></collision></link></robot>')
    monkeypatch.setenv("PBRE_OBJECT_MESH_DIR", str(tmp_path))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ph = objects.object_physics("duck_vhacd")
    assert len(objects.hull_pieces(ph["obj_hull"])) == 3 and max(ph["obj_h"]) < 0.1
    n = 64
    env = pandaPushGymEnv(obj_name="duck_vhacd", num_envs=n, auto_reset=True, obj_pose_rnd_std=0.05, _lib=hip_lib)
    eng = env._client.engine
    assert eng.get_physics().obj_shape == 3 and list(eng.get_physics().obj_h) == pytest.approx(ph["obj_h"], abs=1e-6)
    env.reset()
    rng = np.random.default_rng(0)
    for _ in range(200):
        out = env.step(rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32))
        assert np.isfinite(out[0]).all()
    info = eng.kernel_info()
    assert info[3] == 0 and info[4] > 0, info                        # the general row kernel steps every env, the fast kernel none
    assert np.isfinite(eng.get_state()).all() and info[12] == 0
    env.close()


@pytest.mark.gpu
def test_gpu_sphere_inside_each_piece_against_the_oracle(hip_lib, panda):
    from pybullet_robot_envs import _capi
    print(cr.check_sphere_on_pieces(_capi.Engine, hip_lib, panda["table"], panda))


@pytest.mark.gpu
def test_gpu_icub_sphere_inside_each_piece_against_the_oracle(hip_lib, monkeypatch):
    from pybullet_robot_envs import _capi
    monkeypatch.setenv("PBRE_ICUB_LANE", "0")
    print(cr.check_icub_sphere_on_pieces(_capi.Engine, hip_lib))


@pytest.mark.gpu
def test_gpu_kernel_slots_match_the_rule(hip_lib, panda):
    from pybullet_robot_envs import _capi
    print(cr.check_slots_against_oracle(_capi.Engine, hip_lib, panda["table"]))
