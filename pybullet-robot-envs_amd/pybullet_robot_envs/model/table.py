"""Generic model dict -> flat RobotTable blob (float64 array), the format
`pbre_config.robot_table` carries across the C-ABI (include/pbre.h §RobotTable).

The blob is pure data: header, one fixed-stride record per link (fixed joints
are kept as 0-DoF links exactly as PyBullet keeps them),
one record per collision sphere.  Collision spheres are a build-defined
stand-in for the reference's convex collision meshes, which are git-lfs
pointers in the checkout -- see DESIGN.md "Contact geometry".
"""
import json
import os

import numpy as np

MAGIC = 1346523717.0  # 'PBRE'
VERSION = 1.0
HEADER = 24
LINK_STRIDE = 40
SPHERE_STRIDE = 8

# (link name, centre in link frame, radius) -- Franka Panda stand-in geometry.
PANDA_SPHERES = [
    ("panda_leftfinger", (0.0, 0.0075, 0.0445), 0.0095),
    ("panda_leftfinger", (0.0, 0.0085, 0.0265), 0.0105),
    ("panda_rightfinger", (0.0, -0.0075, 0.0445), 0.0095),
    ("panda_rightfinger", (0.0, -0.0085, 0.0265), 0.0105),
    ("panda_hand", (0.0, 0.055, 0.030), 0.035),
    ("panda_hand", (0.0, -0.055, 0.030), 0.035),
    ("panda_hand", (0.0, 0.0, 0.025), 0.040),
    ("panda_link7", (0.0, 0.0, 0.070), 0.045),
    ("panda_link6", (0.045, 0.0, 0.0), 0.055),
    ("panda_link5", (0.0, 0.04, -0.12), 0.060),
    ("panda_link5", (0.0, 0.0, 0.0), 0.060),
    ("panda_link4", (-0.04, 0.04, 0.0), 0.065),
    ("panda_link3", (0.04, 0.02, -0.03), 0.065),
]

DEFAULT_LATERAL_FRICTION = 0.5  # Bullet default when the URDF has no <contact> tag [EXT-UNVERIFIED]


def build_table(model, spheres=(), ee_link=-1):
    links = model["links"]
    nl = len(links)
    names = [l["name"] for l in links]
    ndof = sum(1 for l in links if l["jtype"] != 0)
    out = np.zeros(HEADER + nl * LINK_STRIDE + len(spheres) * SPHERE_STRIDE, dtype=np.float64)
    out[0:6] = [MAGIC, VERSION, nl, ndof, ee_link, len(spheres)]
    out[6:9] = model["base_position"]
    out[9:18] = np.asarray(model["base_R"], dtype=float).reshape(9)
    out[18] = 1.0 if model.get("fixed_base", True) else 0.0
    dof = 0
    for i, l in enumerate(links):
        r = out[HEADER + i * LINK_STRIDE: HEADER + (i + 1) * LINK_STRIDE]
        r[0] = l["parent"]
        r[1] = l["jtype"]
        r[2:5] = l["axis"]
        r[5:8] = l["origin_xyz"]
        r[8:17] = np.asarray(l["origin_R"], dtype=float).reshape(9)
        r[17] = l["mass"]
        r[18:21] = l["com"]
        r[21:30] = np.asarray(l["inertia"], dtype=float).reshape(9)
        r[30] = l["lower"]
        r[31] = l["upper"]
        r[32] = l["damping"]
        if l["jtype"] != 0:
            r[33] = dof
            dof += 1
        else:
            r[33] = -1
        r[34] = l["lateral_friction"] if l.get("lateral_friction") is not None else DEFAULT_LATERAL_FRICTION
        r[35] = l.get("effort", 0.0)
        r[36] = l.get("velocity", 0.0)
        r[37] = 1.0 if l.get("ik_passive") else 0.0        # a joint the inverse kinematics must not move (float_base)
    base = HEADER + nl * LINK_STRIDE
    for k, sph in enumerate(spheres):
        lname, c, rad = sph[:3]
        li = names.index(lname)
        s = out[base + k * SPHERE_STRIDE: base + (k + 1) * SPHERE_STRIDE]
        s[0] = li
        s[1:4] = c
        s[4] = rad
        s[5] = out[HEADER + li * LINK_STRIDE + 34]
        s[6] = sph[3] if len(sph) > 3 else 0          # fingertip slot + 1
    return out


def sphere_links(table, model=None):
    """Per collision sphere of the RobotTable, in table order: its link index [ns] (int) and, with the `model` the table was built from,
    the link's name (else None).  Engine.contact_query()["nearest"] holds sphere indices: `links[nearest]` is the link that is closest."""
    t = np.asarray(table, dtype=np.float64)
    nl, ns = int(t[2]), int(t[5])
    links = t[HEADER + nl * LINK_STRIDE: HEADER + nl * LINK_STRIDE + ns * SPHERE_STRIDE].reshape(ns, SPHERE_STRIDE)[:, 0].astype(np.int64)
    names = None if model is None else [model["links"][i]["name"] for i in links]
    return links, names


def link_index(model, name):
    """Index, in the RobotTable built from `model`, of the link called `name` ("panda_link5", "l_hand"): what Engine.kin_query takes as
    `links` / `jac_link`.  An int passes through.  (A RobotTable itself holds no names: pass the model it was built from.)"""
    if isinstance(name, (int, np.integer)):
        return int(name)
    if not isinstance(model, dict) or "links" not in model:
        raise TypeError("link_index: link names need the model the RobotTable was built from (a table holds no names)")
    names = [l["name"] for l in model["links"]]
    if name not in names:
        raise KeyError("no link %r in the model (links: %s)" % (name, ", ".join(names)))
    return names.index(name)


def dof_names(model):
    """Joint name of every DoF, in the column order of Engine.kin_query()'s "jac", "mass" and "tau" (the table's dof_index order)"""
    return [l.get("joint_name", l["name"]) for l in model["links"] if l["jtype"] != 0]


def kin_args(model, kw):
    """kin_query keyword arguments with link names replaced by indices (`links`: a name, an index or a list of either; `jac_link`)"""
    kw = dict(kw)
    if kw.get("links") is not None:
        ls = kw["links"]
        ls = [ls] if isinstance(ls, (str, int, np.integer)) else list(ls)
        kw["links"] = [link_index(model, x) for x in ls]
    if kw.get("jac_link") is not None:
        kw["jac_link"] = link_index(model, kw["jac_link"])
    return kw


def hand_pose_target(pose, link_offset):
    """Hand poses [N, 6] (x, y, z, roll, pitch, yaw) or [N, 7] (x, y, z, quaternion x y z w) in the observation's convention -> (target_pos
    [N, 3], target_quat [N, 4]) of the end-effector LINK for Engine.ik_query: the orientation as given, the position moved by the constant
    ik_link_offset of the engine's config rotated into the world (zero for the Panda; the iCub's hand pose is that of the hand's centre of
    mass), which is what apply_action's inverse kinematics drives.  numpy arrays or torch tensors (the result stays where the input is)."""
    xp = np
    if not isinstance(pose, np.ndarray):
        try:
            import torch
            xp = torch if isinstance(pose, torch.Tensor) else np
        except ImportError:
            pass
        if xp is np:
            pose = np.asarray(pose, dtype=np.float64)
    if pose.ndim != 2 or pose.shape[1] not in (6, 7):
        raise ValueError("hand_pose: [N, 6] (position, Euler angles) or [N, 7] (position, quaternion) poses, got shape %r" % (tuple(pose.shape),))
    pos = pose[:, 0:3]
    if pose.shape[1] == 6:                       # pybullet.getQuaternionFromEuler
        h = pose[:, 3:6] * 0.5
        cr, sr, cp, sp, cy, sy = xp.cos(h[:, 0]), xp.sin(h[:, 0]), xp.cos(h[:, 1]), xp.sin(h[:, 1]), xp.cos(h[:, 2]), xp.sin(h[:, 2])
        quat = xp.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], 1)
    else:
        quat = pose[:, 3:7]
        quat = quat / xp.sqrt((quat * quat).sum(1))[:, None]
    ox, oy, oz = (float(v) for v in link_offset)
    x, y, z, w = quat[:, 0], quat[:, 1], quat[:, 2], quat[:, 3]
    # R(quat) offset = o + 2 w (u x o) + 2 u x (u x o), u = (x, y, z)
    cx, cy_, cz = y * oz - z * oy, z * ox - x * oz, x * oy - y * ox
    dx, dy, dz = y * cz - z * cy_, z * cx - x * cz, x * cy_ - y * cx
    off = xp.stack([ox + 2 * (w * cx + dx), oy + 2 * (w * cy_ + dy), oz + 2 * (w * cz + dz)], 1)
    return pos + off, quat


def ik_args(model, cfg, kw):
    """ik_query keyword arguments from an env-level call: `link` may be a link name; with hand_pose=True, target_pos holds hand poses
    ([N, 6] or [N, 7], hand_pose_target) of the table's end-effector link"""
    kw = dict(kw)
    if kw.get("link") is not None:
        kw["link"] = link_index(model, kw["link"])
    if kw.pop("hand_pose", False):
        if kw.get("link") is not None or kw.get("target_quat") is not None:
            raise ValueError("hand_pose=True: the pose is that of the end-effector link (leave link and target_quat unset)")
        kw["target_pos"], kw["target_quat"] = hand_pose_target(kw["target_pos"], [cfg.ik_link_offset[k] for k in range(3)])
    return kw


def save_model_json(model, path):
    with open(path, "w") as f:
        json.dump(model, f, indent=1)


def load_model_json(path):
    with open(path) as f:
        return json.load(f)


def panda_model(base_position=(0.0, 0.0, 0.625)):
    """Parsed Panda model.  Loaded from the committed JSON (generated by
    tools/compile_models.py from the reference's panda_model.urdf)."""
    from pybullet_robot_envs.robot_data import franka_panda
    m = load_model_json(os.path.join(franka_panda.get_data_path(), "panda_model.json"))
    m["base_position"] = list(map(float, base_position))
    return m


def panda_table(base_position=(0.0, 0.0, 0.625)):
    m = panda_model(base_position)
    names = [l["name"] for l in m["links"]]
    return build_table(m, PANDA_SPHERES, ee_link=names.index("panda_grasptarget")), m


def panda_arm_table(base_position=(0.0, 0.0, 0.625)):
    """RobotTable of pandaEnv used alone (robot-level interface): the same model, the finger spheres carry fingertip slots 1 (left
    finger, panda_finger_joint1) and 2 (right finger) for check_contact_fingertips (reference panda_env.py:320-361)."""
    m = panda_model(base_position)
    names = [l["name"] for l in m["links"]]
    tip = {"panda_leftfinger": 1, "panda_rightfinger": 2}
    spheres = [(ln, c, r, tip.get(ln, 0)) for ln, c, r in PANDA_SPHERES]
    return build_table(m, spheres, ee_link=names.index("panda_grasptarget")), m


# ---------------------------------------------------------------------------------------------- iCub
# initial joint positions (reference icub_env.py:19-41), by joint name
ICUB_HOME = {
    'l_knee': 0.0, 'l_ankle_pitch': 0.0, 'l_ankle_roll': 0.0, 'l_hip_pitch': 0.0, 'l_hip_roll': 0.0, 'l_hip_yaw': 0.0,
    'r_knee': 0.0, 'r_ankle_pitch': 0.0, 'r_ankle_roll': 0.0, 'r_hip_pitch': 0.0, 'r_hip_roll': 0.0, 'r_hip_yaw': 0.0,
    'neck_pitch': 0.008, 'neck_roll': 0.0, 'neck_yaw': 0.0,
    'torso_pitch': 0.0, 'torso_roll': 0.0, 'torso_yaw': 0.0,
    'l_shoulder_pitch': -0.51, 'l_shoulder_roll': 0.7, 'l_shoulder_yaw': 0.0, 'l_elbow': 1.22,
    'l_wrist_pitch': 0.0, 'l_wrist_prosup': 0.0, 'l_wrist_yaw': 0.0,
    'r_shoulder_pitch': -0.51, 'r_shoulder_roll': 0.7, 'r_shoulder_yaw': 0.0, 'r_elbow': 1.22,
    'r_wrist_pitch': 0.0, 'r_wrist_prosup': 0.0, 'r_wrist_yaw': 0.0,
}
# joint groups the reference controls (icub_env.py:43-52, 127-138): torso + the chosen arm
ICUB_TORSO = ['torso_pitch', 'torso_roll', 'torso_yaw']
ICUB_ARM = ['shoulder_pitch', 'shoulder_roll', 'shoulder_yaw', 'elbow', 'wrist_pitch', 'wrist_prosup', 'wrist_yaw']


def icub_spheres(model):
    """Stand-in collision geometry for the arms (the reference's collision meshes are git-lfs pointers):
    a sphere at the hand COM, one further out along the palm, one at the forearm COM."""
    by = {l["name"]: l for l in model["links"]}
    out = []
    for s in ("l", "r"):
        hc = by[s + "_hand"]["com"]
        out.append((s + "_hand", tuple(hc), 0.032))
        out.append((s + "_hand", tuple(1.75 * c for c in hc), 0.022))
        out.append((s + "_forearm", tuple(by[s + "_forearm"]["com"]), 0.038))
    return out


def pin_base(model):
    """The reference pins the floating base with p.createConstraint(JOINT_FIXED) whose world-side pivot is the base COM
    raised to 1.2 x its height and whose frame on the base is the base orientation itself (icub_env.py:97-103).  The
    engine idealises that constraint as its rest state [EXT-UNVERIFIED: Bullet's btMultiBodyFixedConstraint is soft and
    gets there within a few steps]: a fixed base with COM at (x, y, 1.2 z) and orientation R_base^T."""
    Rb = np.asarray(model["base_R"], dtype=float)
    pb = np.asarray(model["base_position"], dtype=float)
    com = np.asarray(model["base"]["com"], dtype=float)
    cb = pb + Rb @ com
    tgt = np.array([cb[0], cb[1], 1.2 * cb[2]])
    Rn = Rb.T
    m = dict(model)
    m["base_R"] = Rn.tolist()
    m["base_position"] = (tgt - Rn @ com).tolist()
    m["fixed_base"] = True
    return m


def prune_base_branches(model, keep_links):
    """Drop every limb rooted at the (fixed) base whose links are all outside `keep_links`' limbs.  With a fixed base the
    limbs rooted at it are independent dynamical systems: a limb without collision geometry that no env observes or drives
    (the iCub's legs) cannot influence any output, so the engine does not simulate it.  Link order is preserved."""
    links = model["links"]
    root_child = []
    for i, l in enumerate(links):
        root_child.append(i if l["parent"] < 0 else root_child[l["parent"]])
    names = [l["name"] for l in links]
    keep_roots = set(root_child[names.index(n)] for n in keep_links)
    new_index, out = {}, []
    for i, l in enumerate(links):
        if root_child[i] in keep_roots:
            new_index[i] = len(out)
            m = dict(l)
            m["parent"] = -1 if l["parent"] < 0 else new_index[l["parent"]]
            out.append(m)
    pruned = dict(model)
    pruned["links"] = out
    return pruned


def _pose_at_rest(links, i, cache):
    """(R, p) of link i's frame in the base frame with every joint at 0 (a joint's motion is the identity there)"""
    if i in cache:
        return cache[i]
    l = links[i]
    Rl, pl = np.asarray(l["origin_R"], float), np.asarray(l["origin_xyz"], float)
    if l["parent"] < 0:
        cache[i] = (Rl, pl)
    else:
        Rp, pp = _pose_at_rest(links, l["parent"], cache)
        cache[i] = (Rp @ Rl, pp + Rp @ pl)
    return cache[i]


def float_base(model, keep_links, base_force=500.0):
    """The reference's iCub is a FLOATING-base multibody whose base a soft constraint holds in place -- p.createConstraint(base, -1,
    JOINT_FIXED, ...) at (x, y, 1.2 z) (icub_env.py:95-101; SURVEY 7.2-8, 7.3 "genuinely dynamic") -- where pin_base() idealises that
    constraint as rigid.  This variant keeps the base dynamic:
      * six virtual joints world -> base (prismatic x, y, z, then revolute x, y, z; massless links) placed at the constraint's rest
        pose, so q = 0 IS the rest pose;
      * the constraint itself = the hold motors of those six joints: a Bullet constraint row drives the relative velocity to
        -erp * error / dt, which is a POSITION_CONTROL motor with positionGain = erp = 0.2 and velocityGain = 1 -- the very gains the
        reference gives every joint it does not control (icub_env.py:116-119) [EXT-UNVERIFIED: btMultiBodyFixedConstraint's erp], whose
        rows are bounded by the CONSTRAINT's maxForce instead of a motor's: `base_force` N (the reference leaves createConstraint's
        maxForce at PyBullet's default, 500 N [EXT-UNVERIFIED]; the robot's weight, 324 N, stays below it) -- link record [35] of the
        virtual joints, Tables::mforce in the engine, orc_model.max_force in the oracle (round 6);
      * the limbs rooted at the base that no env observes or drives (the legs, held at 0 by their motors) are LUMPED into the base body
        at their rest pose -- mass, centre of mass and inertia of base + legs as one rigid body -- instead of dropped: on a moving base
        their inertia matters; the kept limbs hang off the base body as before;
      * the virtual joints carry ik_passive: the inverse kinematics moves the arm, not the base.
    26 DoF instead of 20: stepped by the 64-lane engine shape (one env per wavefront)."""
    m = pin_base(model)
    links = m["links"]
    names = [l["name"] for l in links]
    root_child = []
    for i, l in enumerate(links):
        root_child.append(i if l["parent"] < 0 else root_child[l["parent"]])
    keep_roots = set(root_child[names.index(n)] for n in keep_links)
    # composite rigid body: base + every link of a dropped limb, in the base frame
    cache = {}
    bodies = [(m["base"]["mass"], np.asarray(m["base"]["com"], float), np.asarray(m["base"]["inertia"], float))]
    for i, l in enumerate(links):
        if root_child[i] in keep_roots or l["mass"] <= 0:
            continue
        R, p_ = _pose_at_rest(links, i, cache)
        bodies.append((l["mass"], p_ + R @ np.asarray(l["com"], float), R @ np.asarray(l["inertia"], float) @ R.T))
    M = sum(b[0] for b in bodies)
    C = sum(b[0] * b[1] for b in bodies) / M
    I = np.zeros((3, 3))
    for mass, c, Ic in bodies:
        d = c - C
        I += Ic + mass * ((d @ d) * np.eye(3) - np.outer(d, d))
    Rb, pb = np.asarray(m["base_R"], float), np.asarray(m["base_position"], float)
    eye = np.eye(3).tolist()
    virt = []
    for k, (jt, ax, nm) in enumerate([(2, [1, 0, 0], "base_tx"), (2, [0, 1, 0], "base_ty"), (2, [0, 0, 1], "base_tz"),
                                      (1, [1, 0, 0], "base_rx"), (1, [0, 1, 0], "base_ry"), (1, [0, 0, 1], "base_rz")]):
        virt.append({"name": "base_virtual_%d" % k, "joint_name": nm, "jtype": jt, "parent": k - 1, "axis": [float(a) for a in ax],
                     "origin_xyz": (pb.tolist() if k == 0 else [0.0, 0.0, 0.0]), "origin_R": eye, "mass": 0.0, "com": [0.0, 0.0, 0.0],
                     "inertia": np.zeros((3, 3)).tolist(), "lower": -10.0, "upper": 10.0, "damping": 0.0, "effort": float(base_force), "velocity": 0.0,
                     "lateral_friction": None, "has_collision": False, "ik_passive": True})
    base_body = {"name": m["base"]["name"], "joint_name": "base_fixed", "jtype": 0, "parent": 5, "axis": [0.0, 0.0, 0.0],
                 "origin_xyz": [0.0, 0.0, 0.0], "origin_R": Rb.tolist(), "mass": float(M), "com": C.tolist(), "inertia": I.tolist(),
                 "lower": 0.0, "upper": 0.0, "damping": 0.0, "effort": 0.0, "velocity": 0.0,
                 "lateral_friction": m["base"].get("lateral_friction"), "has_collision": False}
    out, new_index = virt + [base_body], {}
    for i, l in enumerate(links):
        if root_child[i] not in keep_roots:
            continue
        new_index[i] = len(out)
        c = dict(l)
        c["parent"] = 6 if l["parent"] < 0 else new_index[l["parent"]]
        out.append(c)
    fm = dict(m)
    fm["links"] = out
    fm["base_position"] = [0.0, 0.0, 0.0]
    fm["base_R"] = eye
    fm["fixed_base"] = True           # (the table's root is the world; the robot's base is link 6)
    fm["floating_base"] = {"lumped_mass": float(M), "virtual_joints": 6, "base_force": float(base_force)}
    return fm


def icub_model(full=False, floating_base=False, base_force=500.0):
    """The iCub as the engine simulates it: fixed base at the constraint's rest pose, legs pruned (see prune_base_branches).
    full=True keeps all 38 links / 32 DoF (the reference's joint numbering, used by iCubEnv for names and indices)."""
    from pybullet_robot_envs.robot_data import iCub
    raw = load_model_json(os.path.join(iCub.get_data_path(), "icub_model.json"))
    if floating_base:       # soft-pinned floating base (float_base): the reference's createConstraint, dynamic
        return float_base(raw, ["l_hand", "r_hand"], base_force)
    m = pin_base(raw)
    return m if full else prune_base_branches(m, ["l_hand", "r_hand"])


def icub_info(model, control_arm="l"):
    """DoF bookkeeping the reference derives by joint name (icub_env.py:107-150)."""
    dof_names = [l["joint_name"] for l in model["links"] if l["jtype"] != 0]
    ctrl_names = ICUB_TORSO + [control_arm + "_" + n for n in ICUB_ARM]
    ctrl = [i for i, n in enumerate(dof_names) if n in ctrl_names]          # traversal order, as _joints_to_control
    names = [l["name"] for l in model["links"]]
    return {"dof_names": dof_names, "controlled": ctrl, "home": [ICUB_HOME.get(n, 0.0) for n in dof_names],
            "ee_link": names.index(control_arm + "_hand")}


def icub_table(control_arm="l", full=False, floating_base=False, base_force=500.0):
    m = icub_model(full, floating_base, base_force)
    info = icub_info(m, control_arm)
    return build_table(m, icub_spheres(m), ee_link=info["ee_link"]), m, info


# ---------------------------------------------------------------------------------------------- iCub with hands
# finger joints of one hand in the reference's order (icub_env_with_hands.py:36-47): index, little, middle, ring, thumb;
# per finger the abduction joint then three flexion joints.  The fingertip is the 4th joint's link (tips_idxs, :248).
HAND_FINGERS = ['aij6', 'aij3', 'aij4', 'aij5', 'lij6', 'lij3', 'lij4', 'lij5', 'mj6', 'mj3', 'mj4', 'mj5',
                'rij6', 'rij3', 'rij4', 'rij5', 'tj2', 'tj4', 'tj5', 'tj6']
HAND_TIPS = [3, 7, 11, 15, 19]
GRASP_POS = [0, 0.75, 0.5, 0.5, 0, 0.75, 0.5, 0.5, 0, 0.75, 0.5, 0.5, 0, 0.75, 0.5, 0.5, 1.57, 0.4, 0.2, 0.07]   # _grasp_pos, :61


def hand_joint_names(side):
    return ['%s_hand::%s_%s' % (side, side, n) for n in HAND_FINGERS]


def icub_hands_model(full=False):
    """icub_model_with_hands.sdf as the engine simulates it: fixed base at the constraint's rest pose, legs pruned (60 of the
    72 DoF remain).  full=True keeps all 78 joints (the reference's numbering, used for names and indices)."""
    from pybullet_robot_envs.robot_data import iCub
    m = pin_base(load_model_json(os.path.join(iCub.get_data_path(), "icub_model_with_hands.json")))
    return m if full else prune_base_branches(m, ["l_hand::l_hand_base_link", "r_hand::r_hand_base_link"])


def icub_hands_spheres(model, control_arm="l"):
    """Stand-in collision geometry (the reference's finger / palm collision meshes are git-lfs pointers): per hand one sphere at
    the distal phalanx of every finger (the fingertip; centre = the collision mesh's origin in the link frame), one per middle
    and proximal phalanx, one for the palm; plus the forearms.  The fingertips of the controlled hand carry tip slots 1..5."""
    by = {l["name"]: l for l in model["links"]}
    jn = {l.get("joint_name"): l["name"] for l in model["links"]}
    out = []
    for s in ("l", "r"):
        names = hand_joint_names(s)
        for f in range(5):
            prox, mid, tip = (jn[names[4 * f + k]] for k in (1, 2, 3))
            out.append((tip, (0.0168, 0.0, 0.0), 0.0075, (f + 1) if s == control_arm else 0))
            out.append((mid, (0.011, 0.0, 0.0), 0.0085, 0))
            out.append((prox, (0.012, 0.0, 0.0), 0.0095, 0))
        base = s + "_hand::" + s + "_hand_base_link"
        hc = by[base]["com"]
        out.append((base, tuple(hc), 0.028, 0))
        out.append((s + "_forearm", tuple(by[s + "_forearm"]["com"]), 0.038, 0))
    return out


def icub_hands_info(model, control_arm="l"):
    """DoF bookkeeping of iCubHandsEnv.reset (icub_env_with_hands.py:104-146).  `a or b and c` in the joint selection
    (:129-136) keeps BOTH arms among the controlled joints; only the hand follows control_arm."""
    dof_names = [l["joint_name"] for l in model["links"] if l["jtype"] != 0]
    arm = lambda s: [s + "_" + n for n in ICUB_ARM]
    ctrl_names = ICUB_TORSO + arm("l") + arm("r") + hand_joint_names(control_arm)
    ctrl = [i for i, n in enumerate(dof_names) if n in ctrl_names]
    names = [l["name"] for l in model["links"]]
    fingers = [dof_names.index(n) for n in hand_joint_names(control_arm)]
    return {"dof_names": dof_names, "controlled": ctrl, "home": [ICUB_HOME.get(n, 0.0) for n in dof_names],
            "ee_link": names.index(control_arm + "_hand::" + control_arm + "_hand_base_link"), "fingers": fingers}


def icub_hands_table(control_arm="l", full=False):
    m = icub_hands_model(full)
    info = icub_hands_info(m, control_arm)
    return build_table(m, icub_hands_spheres(m, control_arm), ee_link=info["ee_link"]), m, info
