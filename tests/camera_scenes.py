"""Scenes and cameras shared by the camera tests (test_camera_host.py measures the float32-vs-float64 figures of tests/camera_ref.py on
the synthetic ones here; test_gpu_camera.py renders engine states with the same cameras)."""
import types

import numpy as np

from pybullet_robot_envs import camera as pcam

FAR = 10.0      # test cameras: a floor seen at a grazing angle 50 m away is ill-conditioned in fp32 and says nothing about the kernel


def phys_like(obj_shape=0, obj_h=(0.025, 0.025, 0.025), table_c=(0.85, 0.0, 0.6)):
    return types.SimpleNamespace(table_c=table_c, table_h=(0.75, 0.5, 0.025), ground_z=0.0, obj_h=obj_h, obj_shape=obj_shape)


def task_camera(base, width, height, dyaw=0.0, dpitch=0.0, distance=1.3, far=FAR, fov=60.0):
    """the reference's camera (target the robot base, distance 1.3, yaw 180, pitch -40, fov 60, near 0.1) with far = 10, perturbed"""
    view = pcam.view_matrix_from_yaw_pitch_roll(base, distance, 180.0 + dyaw, -40.0 + dpitch, 0.0, 2)
    proj = pcam.projection_matrix_fov(fov, float(width) / height, 0.1, far)
    return view, proj


def quat_axis_angle(axis, ang):
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    return np.concatenate([a * np.sin(0.5 * ang), [np.cos(0.5 * ang)]])


HULL6 = np.array([[0.05, 0.0, -0.03], [-0.04, 0.045, -0.03], [-0.04, -0.045, -0.025], [0.0, 0.0, 0.06], [0.03, 0.035, 0.02], [-0.02, -0.01, -0.045]])
COMPOUND = np.concatenate([HULL6 * 0.8 + np.array([0.05, 0.0, 0.0]), np.full((1, 3), np.nan),
                           np.array([[-0.09, -0.03, -0.03], [-0.02, -0.03, -0.03], [-0.09, 0.03, -0.03], [-0.02, 0.03, -0.03],
                                     [-0.09, -0.03, 0.035], [-0.02, -0.03, 0.035], [-0.09, 0.03, 0.035], [-0.02, 0.03, 0.035]])])
SHAPES = {"box": (0, (0.03, 0.045, 0.02), None), "sphere": (1, (0.04, 0.04, 0.04), None), "cylinder": (2, (0.035, 0.035, 0.05), None),
          "hull": (3, None, HULL6), "compound": (3, None, COMPOUND)}


def synthetic_state(table, n, width, obj_off, rng, q0=None, spread=0.3):
    """[n, width] state records: joints q0 + noise inside the limits' reach, a tilted object above the table in front of the robot"""
    t = np.asarray(table, float)
    nd = int(t[3])
    st = np.zeros((n, width), np.float32)
    q0 = np.zeros(nd) if q0 is None else np.asarray(q0, float)
    st[:, :nd] = q0[None] + spread * rng.uniform(-1, 1, (n, nd))
    base = t[6:9]
    for e in range(n):
        st[e, obj_off:obj_off + 3] = [base[0] + 0.45 + 0.1 * rng.uniform(-1, 1), base[1] + 0.15 * rng.uniform(-1, 1), 0.625 + 0.08 + 0.05 * rng.uniform()]
        st[e, obj_off + 3:obj_off + 7] = quat_axis_angle(rng.normal(size=3), rng.uniform(0.2, 1.2))
    return st


PANDA_HOME = [0.0, -0.54, 0.0, -2.6, -0.30, 2.0, 1.0, 0.02, 0.02]


def object_before_arm(table, state, view, link_name_index=None):
    """[n, 7] object poses (position, quaternion): tilted, in the air 20 cm in front of the arm's fifth link as the camera with the view
    matrix `view` sees it, a few centimetres to the side (more per env), so that the object hides a part of the arm."""
    from pybullet_robot_envs.model.contacts import link_frames
    t = np.asarray(table, float)
    V = np.asarray(view, float).reshape(4, 4).T
    eye = -V[:3, :3].T @ V[:3, 3]
    right = V[0, :3]
    R, p = link_frames(t, np.asarray(state, float)[:, :int(t[3])])
    link = 5 if link_name_index is None else link_name_index
    out = np.zeros((len(state), 7), np.float32)
    for e in range(len(state)):
        c = p[e, link]
        to_eye = (eye - c) / np.linalg.norm(eye - c)
        out[e, :3] = c + 0.2 * to_eye + (0.02 + 0.025 * e) * right
        out[e, 3:] = quat_axis_angle([1.0, 0.4 * e - 0.3, 0.5], 0.5 + 0.3 * e)
    return out
