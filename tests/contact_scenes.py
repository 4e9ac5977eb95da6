"""State sets shared by the contact-query tests: test_contact_host.py measures contact_ref's float32-vs-float64 figure on them (the
GPU tolerance) and checks, on the CPU, that they satisfy what test_gpu_contact_query.py assumes of them; the GPU tests place the same
joint positions and object poses into engine records with set_state.  Nothing here needs a GPU."""
import types

import numpy as np

import camera_scenes as scn
import contact_ref as ref

SHAPE3 = np.concatenate([scn.COMPOUND, np.full((1, 3), np.nan),          # a third piece: a tetrahedron above the other two
                         np.array([[0.0, 0.0, 0.04], [0.03, 0.0, 0.04], [0.0, 0.03, 0.04], [0.01, 0.01, 0.075]])])
GAPS = (-0.002, 0.0005, 0.005)       # object against one hand sphere: penetrating, inside the 1 mm margin, outside it


def phys_like(obj_shape=0, obj_h=(0.025, 0.025, 0.025), table_c=(0.85, 0.0, 0.6), table_h=(0.75, 0.5, 0.025), margin=1e-3):
    return types.SimpleNamespace(table_c=table_c, table_h=table_h, ground_z=0.0, obj_h=obj_h, obj_shape=obj_shape, contact_margin=margin)


def hull_half(hull):
    """half extents of the bounding box about the origin (what pbre_set_object_hull writes to obj_h)"""
    v = np.asarray(hull, float)
    return tuple(np.nanmax(np.abs(v), axis=0))


def compact(q, pose):
    """[N, ndof + 7] records joints | object pose (obj_off = ndof): all contact_ref reads of a state"""
    return np.concatenate([q, pose], axis=1).astype(np.float32)


def embed(records, q, pose, obj_off):
    """the engine's records with these joints and object poses"""
    st = np.array(records, np.float32)
    st[:, :q.shape[1]] = q
    st[:, obj_off:obj_off + 7] = pose
    return st


def panda_states(panda, n_table=40, n_obj=40, n_jit=40, n_lift=11, seed=11):
    """[N, 48] Panda push records (oracle layout = engine layout): parity.contact_states' crafted table and object contacts, the settled
    arm jittered, and settled arms with the object lifted off the table (flag value 0)."""
    import orc
    import parity
    ora = orc.Oracle(panda["table"], task=1)
    ora.task.obj_pose_rnd_std, ora.task.tg_pose_rnd_std = 0.05, 0.2
    base, _ = ora.batch_reset(1)
    base = base[0]
    rng = np.random.default_rng(seed)
    S = [parity.contact_states(ora, panda, base, rng, n_table, n_obj)]
    jit = np.tile(base, (n_jit, 1))
    jit[:, :7] += rng.normal(0, 0.25, (n_jit, 7))
    S.append(jit)
    lift = np.tile(base, (n_lift, 1))
    lift[:, :7] += rng.normal(0, 0.05, (n_lift, 7))
    lift[:, 11] += rng.uniform(0.05, 0.3, n_lift)
    for e in range(n_lift):
        lift[e, 12:16] = scn.quat_axis_angle(rng.normal(size=3), rng.uniform(0.0, 1.5))
    S.append(lift)
    return np.concatenate(S).astype(np.float32)


def random_quats(rng, n, max_angle=1.2):
    return np.stack([scn.quat_axis_angle(rng.normal(size=3), rng.uniform(0.1, max_angle)) for _ in range(n)])


def place_against(table, q, k, phys, hull, gaps, rng):
    """[n, 7] object poses: rotated at random and placed along a random direction from collision sphere k so that contact_ref's float64
    distance of that sphere to the object is gaps[e] (bisection on the offset; the object's origin lies inside it)."""
    n = len(q)
    sc, sr, _, _ = ref.sphere_centres(table, np.asarray(q, np.float64))
    c, r = sc[:, k], sr[k]
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    quat = random_quats(rng, n)
    Ro = ref.mc._quat_R(quat)
    shape, oh = int(phys.obj_shape), np.array(list(phys.obj_h), float)
    pieces = ref.hull_faces(hull) if shape == 3 else None
    gaps = np.asarray(gaps, float)
    lo, hi = np.zeros(n), np.full(n, 0.6)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        f = ref.sphere_object_dist(c, r, c + d * mid[:, None], Ro, shape, oh, pieces)
        lo, hi = np.where(f < gaps, mid, lo), np.where(f < gaps, hi, mid)
    return np.concatenate([c + d * (0.5 * (lo + hi))[:, None], quat], axis=1)


def shape_set(table, q0, name, rng, n=16, spread=0.2, table_c=(0.85, 0.0, 0.6), tip_sphere=None, phys=None):
    """(q [n, ndof], pose [n, 7], phys, hull) for object shape `name` of camera_scenes.SHAPES (or "compound3"): n - 2 envs with the object
    against one of the arm's last spheres at GAPS in turn, one env with the object resting on the table and one with it hanging over the
    table's edge (some candidate points do not count).  phys: an engine's pbre_physics to place a primitive object by (then `name` and
    table_c are not used)."""
    t = np.asarray(table, float)
    nd, ns = int(t[3]), int(t[5])
    shape, oh, hull = (3, None, SHAPE3) if name == "compound3" else scn.SHAPES[name]
    oh = hull_half(hull) if hull is not None else oh
    if phys is not None:
        shape, oh, hull, table_c = int(phys.obj_shape), tuple(phys.obj_h), None, tuple(phys.table_c)
        assert shape != 3
    else:
        phys = phys_like(shape, tuple(oh), table_c=table_c)
    q = np.asarray(q0, float)[None] + spread * rng.uniform(-1, 1, (n, nd))
    k = ns - 1 - int(rng.integers(0, 3)) if tip_sphere is None else tip_sphere
    pose = place_against(t, q, k, phys, hull, [GAPS[e % 3] for e in range(n)], rng)
    top = table_c[2] + phys.table_h[2]
    x_edge = table_c[0] - phys.table_h[0]
    for e, x in ((n - 2, table_c[0] + 0.45), (n - 1, x_edge + 0.4 * oh[0])):
        pose[e, :3] = [x, table_c[1] - 0.31, top + 0.3]
        pose[e, 3:] = scn.quat_axis_angle([0.3, 0.2, 1.0], 0.4) if e == n - 2 else scn.quat_axis_angle([0.1, 1.0, 0.2], 0.3)
        r0 = ref.query(t, compact(q[e:e + 1], pose[e:e + 1]), nd, phys, hull=hull)
        pose[e, 2] -= r0["dist"][0, 0] - 0.0004          # lowest counting candidate 0.4 mm above the top: inside the margin
    return q.astype(np.float32), pose.astype(np.float32), phys, hull


def robot_sets():
    """name -> (table, ndof, q0, spread) of the engines beside the Panda task envs"""
    from pybullet_robot_envs.model.table import icub_table, icub_hands_table, panda_arm_table
    out = {"icub": (icub_table("l")[0], None, 0.2), "icub_float": (icub_table("l", floating_base=True)[0], None, 0.05),
           "hands": (icub_hands_table("r")[0], None, 0.15), "panda_arm": (panda_arm_table()[0], scn.PANDA_HOME, 0.2)}
    return {k: (np.asarray(t, float), int(t[3]), np.zeros(int(t[3])) if q0 is None else np.asarray(q0, float), s) for k, (t, q0, s) in out.items()}


def tip_spheres(table):
    """indices of the collision spheres that carry a fingertip slot"""
    t = np.asarray(table, float)
    nl, ns = int(t[2]), int(t[5])
    sph = t[24 + nl * 40: 24 + nl * 40 + ns * 8].reshape(ns, 8)
    return [k for k in range(ns) if sph[k, 6] > 0]
