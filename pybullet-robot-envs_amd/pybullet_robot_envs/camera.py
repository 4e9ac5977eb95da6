"""Camera matrices for `Engine.render` (include/pbre_camera.h), in PyBullet's conventions: 16 floats, column major (OpenGL).

`view_matrix_from_yaw_pitch_roll` and `projection_matrix_fov` stand in for p.computeViewMatrixFromYawPitchRoll and
p.computeProjectionMatrixFOV, which the reference's render() calls (R/envs/panda_envs/panda_push_gym_env.py:276-286)."""
import math

import numpy as np


def _rot_ypr(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Rz = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[cr, 0.0, sr], [0.0, 1.0, 0.0], [-sr, 0.0, cr]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    return Rz @ Ry @ Rx


def look_at(eye, target, up):
    """The standard look-at view matrix, [16] float64, column major."""
    eye, target, up = (np.asarray(x, float) for x in (eye, target, up))
    f = target - eye
    f = f / np.linalg.norm(f)
    r = np.cross(f, up)
    r = r / np.linalg.norm(r)
    u = np.cross(r, f)
    M = np.eye(4)
    M[0, :3], M[1, :3], M[2, :3] = r, u, -f
    M[:3, 3] = -M[:3, :3] @ eye
    return M.T.reshape(16).copy()


def view_matrix_from_yaw_pitch_roll(target, distance, yaw, pitch, roll, up_axis=2):
    """Angles in degrees.  With z up the camera looks along f = (-cos p sin y, cos p cos y, sin p) from eye = target - distance f; its up
    vector is world z turned by the same yaw, pitch and roll (about z, the forward axis y, and x), then a standard look-at.
    [EXT-UNVERIFIED]: Bullet's construction restated without PyBullet at hand."""
    if up_axis != 2:
        raise ValueError("view_matrix_from_yaw_pitch_roll: only up_axis=2 (z up, what the reference uses)")
    R = _rot_ypr(math.radians(yaw), math.radians(pitch), math.radians(roll))
    f = R @ np.array([0.0, 1.0, 0.0])
    target = np.asarray(target, float)
    return look_at(target - distance * f, target, R @ np.array([0.0, 0.0, 1.0]))


def projection_matrix_fov(fov, aspect, near, far):
    """The standard OpenGL perspective matrix (fov: vertical, degrees; aspect = width / height), [16] float64, column major."""
    t = 1.0 / math.tan(0.5 * math.radians(fov))
    M = np.zeros((4, 4))
    M[0, 0], M[1, 1] = t / aspect, t
    M[2, 2], M[2, 3] = -(far + near) / (far - near), -2.0 * far * near / (far - near)
    M[3, 2] = -1.0
    return M.T.reshape(16).copy()


def depth_buffer(depth, near, far):
    """PyBullet's non-linear depth buffer in [0, 1] from the metric depth `Engine.render` returns."""
    depth = np.asarray(depth, np.float64)
    return far * (depth - near) / (depth * (far - near))


def depth_from_buffer(buf, near, far):
    """inverse of depth_buffer"""
    buf = np.asarray(buf, np.float64)
    return far * near / (far - (far - near) * buf)
