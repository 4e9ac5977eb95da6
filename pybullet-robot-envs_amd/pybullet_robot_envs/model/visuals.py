"""Visual primitives of a robot for the camera (include/pbre_camera.h): capsules in link frames.  The link meshes of the reference are
git-lfs pointers, so what is drawn is the RobotTable's collision spheres plus one thin capsule per parent-child link pair -- enough to
read the arm's pose in an image."""
import numpy as np

from pybullet_robot_envs.model.table import HEADER, LINK_STRIDE, SPHERE_STRIDE

PRIM_FLOATS = 12        # link | a[3] | b[3] | radius | r, g, b | reserved
MAX_PRIMS = 192
SPHERE_RGB = (0.85, 0.85, 0.88)
LINK_RGB = (0.35, 0.4, 0.55)


def default_visuals(table):
    """[n, 12] float32: the collision spheres (a == b), then per link one capsule from the link origin to each child link's origin_xyz
    (both in the link's frame); capsules shorter than 1 mm are skipped; radius = min(0.04, max(0.004, 0.25 * length))."""
    t = np.asarray(table, float)
    nl, ns = int(t[2]), int(t[5])
    out = []
    base = HEADER + nl * LINK_STRIDE
    for k in range(ns):
        s = t[base + k * SPHERE_STRIDE: base + (k + 1) * SPHERE_STRIDE]
        out.append([s[0], s[1], s[2], s[3], s[1], s[2], s[3], s[4], *SPHERE_RGB, 0.0])
    for i in range(nl):
        r = t[HEADER + i * LINK_STRIDE: HEADER + (i + 1) * LINK_STRIDE]
        par, xyz = int(r[0]), r[5:8]
        length = float(np.linalg.norm(xyz))
        if par < 0 or length < 1e-3:
            continue
        out.append([par, 0.0, 0.0, 0.0, xyz[0], xyz[1], xyz[2], min(0.04, max(0.004, 0.25 * length)), *LINK_RGB, 0.0])
    return np.asarray(out, np.float32).reshape(-1, PRIM_FLOATS)
