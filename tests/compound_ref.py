"""Compound objects (include/pbre.h: pbre_set_object_hull with NaN-separated pieces): synthetic compounds, a Python restatement of the
object-table slot selection (csrc/pbre_core.hpp: Core::select_compound) and checks shared by the emulation and GPU tests.  Piece order
and vertex order are those of the `obj_hull` array."""
import numpy as np

import orc
import parity
import scenarios
from pybullet_robot_envs.model import contacts
from pybullet_robot_envs.model.objects import compound_physics, hull_physics, hull_pieces

NC_OT = 4
PBRE_E_ARG = -1


def cube(c, h):
    """the 8 vertices of an axis-aligned cube of half extent h about c, in the box primitive's vertex order"""
    return np.array([[c[0] + (h if v & 1 else -h), c[1] + (h if v & 2 else -h), c[2] + (h if v & 4 else -h)] for v in range(8)], float)


def box(c, h):
    return np.array([[c[0] + (h[0] if v & 1 else -h[0]), c[1] + (h[1] if v & 2 else -h[1]), c[2] + (h[2] if v & 4 else -h[2])] for v in range(8)], float)


def dumbbell(mass=0.1, mu=1.0):
    """two 2 cm cubes whose inner faces are 4 cm apart, along x"""
    return compound_physics([cube((-0.03, 0, 0), 0.01), cube((0.03, 0, 0), 0.01)], mass, mu)


def join(pieces):
    return np.concatenate([np.concatenate([p, np.full((1, 3), np.nan)]) for p in pieces])[:-1]


def select_slots(pts, depth, margin):
    """the object-table candidates a compound's slots take: pts / depth = per piece [n_i, 3] world points and their depths below the
    support surface (z - support height).  Returns the chosen (piece, vertex) pairs in candidate order."""
    cand = [[(d, i) for i, d in enumerate(dp) if d < margin] for dp in depth]
    top = [sorted(c)[:NC_OT] for c in cand]                   # (a piece's candidates beyond its NC_OT deepest can never be taken)
    chosen = set()
    touching = [p for p in range(len(top)) if top[p]]
    for p in touching:
        chosen.add((p, top[p][0][1]))                         # 1. the deepest of every piece in touch (ties: lower index)
    if len(touching) == 2:                                    # 2. two pieces in touch: each also its candidate farthest from that one
        for p in touching:
            r = pts[p][top[p][0][1]]
            rest = [(-float(np.sum((pts[p][i] - r) ** 2)), i) for _, i in top[p] if (p, i) not in chosen]
            if rest:
                chosen.add((p, min(rest)[1]))
    rest = sorted((d, p, i) for p in range(len(top)) for d, i in top[p] if (p, i) not in chosen)
    for d, p, i in rest[:max(0, NC_OT - len(chosen))]:        # 3. the deepest of the rest
        chosen.add((p, i))
    return sorted(chosen)


def _quat_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _R_quat(R):
    w = 0.5 * np.sqrt(max(1e-12, 1 + R[0, 0] + R[1, 1] + R[2, 2]))
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def check_abi(Engine, lib, table):
    """malformed compounds are refused with PBRE_E_ARG and leave the previous object in place"""
    import pytest
    ph = dumbbell()
    eng, _ = parity.make_pair(Engine, lib, table, 4, phys=ph)
    ref, _ = parity.make_pair(Engine, lib, table, 4, phys=ph)
    c = cube((0, 0, 0), 0.01)
    bad = {"five pieces": join([c + 0.05 * k for k in range(5)]),
           "empty piece": np.concatenate([c, np.full((2, 3), np.nan), c]),
           "leading separator": np.concatenate([np.full((1, 3), np.nan), c]),
           "+inf": join([c, np.where(np.arange(24).reshape(8, 3) == 5, np.inf, c)]),
           "-inf": join([c, np.where(np.arange(24).reshape(8, 3) == 7, -np.inf, c)]),
           "3-vertex piece": join([c, c[:3]]),
           "partial NaN row": np.concatenate([c, [[np.nan, 0.0, np.nan]], c])}
    h0 = list(eng.get_physics().obj_h)
    for what, v in bad.items():
        with pytest.raises(RuntimeError, match="libpbre error %d" % PBRE_E_ARG):
            eng.set_object_hull(v)
        assert list(eng.get_physics().obj_h) == h0 and eng.get_physics().obj_shape == 3, what
    eng.reset(); ref.reset()
    a = np.random.default_rng(1).uniform(-1, 1, (4, 7)).astype(np.float32)
    for _ in range(3):
        eng.step(a); ref.step(a)
    assert np.array_equal(eng.get_state(), ref.get_state()), "a refused compound changed the object"
    eng.close(); ref.close()


def check_single_piece_identity(Engine, lib, table, n=16, steps=20):
    """a one-piece list (the cube as its 8 vertices) through the compound-era table against the box primitive on the same kernel: the
    full state bit for bit over `steps` random-action steps (object out of the arm's reach, so only object-table rows differ in kind)"""
    ph = hull_physics(cube((0, 0, 0), 0.025), 0.1, 1.0)
    prim = dict(ph); prim.pop("obj_hull"); prim["obj_shape"] = 0
    eh, _ = parity.make_pair(Engine, lib, table, n, phys=ph)
    eb, _ = parity.make_pair(Engine, lib, table, n, phys=prim, flags=4)      # PBRE_F_FORCE_GENERAL: the kernel the hull takes
    eh.reset()
    s = eh.get_state().copy()
    rng = np.random.default_rng(5)
    s[:, 9] = 1.35; s[:, 10] = rng.uniform(-0.4, 0.4, n)               # (far corner of the table: the arm cannot reach it)
    s[:, 25:27] = rng.uniform(-0.2, 0.2, (n, 2)); s[:, 30] = rng.uniform(-2, 2, n)
    eh.set_state(s); eb.set_state(s)
    for _ in range(steps):
        a = rng.uniform(-1, 1, (n, 7)).astype(np.float32)
        oa, ob = eh.step(a), eb.step(a)
        assert all(np.array_equal(x, y) for x, y in zip(oa, ob))
        assert np.array_equal(eh.get_state(), eb.get_state()), "single-piece hull differs from the box primitive"
    eh.close(); eb.close()


def gap_states(ora, model, spheres, base, n):
    """dumbbell states in the air: sphere k of the hand 2 mm inside the ENVELOPE's top face, over the gap between the pieces (>= 2 mm from
    both), the dumbbell's long axis across the direction to the other finger"""
    s = np.repeat(base[None], n, 0).copy()
    s[:, 25:31] = 0
    for e in range(n):
        cen = scenarios.sphere_centres(ora, model, spheres, s[e, :9])
        k = e % len(cen)
        cs, rs = cen[k]
        other = cen[(k + 2) % len(cen)][0] if len(cen) >= 4 else cen[(k + 1) % len(cen)][0]
        d = other - cs
        z = np.array([0.0, 0.0, 1.0])
        x = np.cross(d, z); x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z], 1)
        s[e, 9:12] = cs - z * (0.01 + rs - 0.002)
        s[e, 12:16] = _R_quat(R)
    return s


def check_gap(Engine, lib, table, panda, n=8):
    """a hand sphere 2 mm inside the convex envelope of the dumbbell, over its gap: the compound has no robot-object contact and its step
    is the oracle's free flight (piece A alone as the oracle's hull, the compound's mass and inertia); the envelope hull has the contact"""
    ph = dumbbell()
    hv = ph["obj_hull"]
    pieces = hull_pieces(hv)
    env_ph = dict(ph, obj_hull=np.concatenate(pieces))
    eng, ora = parity.make_pair(Engine, lib, table, n, phys=ph)
    ene, _ = parity.make_pair(Engine, lib, table, n, phys=env_ph)
    orc.set_object(ora, dict(ph, obj_hull=pieces[0]))
    eng.reset(); ene.reset()
    st, _ = ora.batch_reset(n)
    s = gap_states(ora, panda["model"], panda["spheres"][:4], st[0], n)
    phys = eng.get_physics()
    fc = contacts.contact_flags(table, s, eng.ndof, phys, hull=hv)
    fe = contacts.contact_flags(table, s, eng.ndof, phys, hull=env_ph["obj_hull"])
    assert (fc & (contacts.ROBOT_OBJECT | contacts.OBJECT_TABLE) == 0).all(), fc
    assert (fe & contacts.ROBOT_OBJECT).all(), fe
    rng = np.random.default_rng(9)
    parity.check_single_steps(eng, ora, s, rng, steps=1, tol=parity.TOL_CONTACT)
    # the envelope: the same states and actions meet the sphere
    a = np.zeros((n, 7), np.float32)
    eng.set_state(s.astype(np.float32)); ene.set_state(s.astype(np.float32))
    eng.step(a); ene.step(a)
    sc, se = eng.get_state(), ene.get_state()
    dv = np.abs(sc[:, 25:31] - se[:, 25:31]).max(axis=1)
    assert (dv > 1e-3).all(), ("the envelope hull made no contact", dv)
    eng.close(); ene.close()
    return float(dv.min())


def stem_cap(mass=0.1, mu=1.0):
    """a 2 x 2 x 6 cm stem and a 6 x 6 x 1 cm cap beside its top, clear of the table: a T lying... standing on the stem"""
    return compound_physics([box((0, 0, 0), (0.01, 0.01, 0.03)), box((0.045, 0, 0.025), (0.03, 0.03, 0.005))], mass, mu)


def check_stem(Engine, lib, table, n=8):
    """only the stem touches the table: resting, sliding and spinning single steps against the oracle with the stem alone as its hull
    (in the compound's frame, with the compound's mass and inertia)"""
    ph = stem_cap()
    pieces = hull_pieces(ph["obj_hull"])
    eng, ora = parity.make_pair(Engine, lib, table, n, phys=ph)
    orc.set_object(ora, dict(ph, obj_hull=pieces[0]))
    eng.reset()
    st, _ = ora.batch_reset(n)
    rng = np.random.default_rng(31)
    s = st.copy()
    s[:, 9:11] = [0.75, 0.25]                                          # away from the arm
    s[:, 12:16] = [0, 0, 0, 1]
    s[:, 11] = 0.625 - pieces[0][:, 2].min() - 0.0002                  # stem 0.2 mm into the table top
    s[:, 25:31] = 0
    s[n // 3:, 25:27] = rng.uniform(-0.1, 0.1, (n - n // 3, 2))         # sliding
    s[2 * n // 3:, 30] = rng.uniform(-2, 2, n - 2 * n // 3)            # spinning
    s[:, 32:35] = [0.9, 0.9, 0.65]
    assert pieces[1][:, 2].min() + s[0, 11] - 0.625 > float(eng.get_physics().contact_margin)
    fl = contacts.contact_flags(table, s, eng.ndof, eng.get_physics(), hull=ph["obj_hull"])
    assert (fl == contacts.OBJECT_TABLE).all(), fl
    parity.check_single_steps(eng, ora, s, rng, steps=3, tol=dict(parity.TOL_CONTACT, obj_v=5e-4))
    eng.close()


def check_rest_kat(Engine, lib, table, n=4, steps=300):
    """the dumbbell after pbre_reset and `steps` zero-action steps: flat, both pieces on the table top, at rest; every piece holds a
    table slot (select_slots on the final state, consistent with contact_flags)"""
    ph = dumbbell()
    pieces = hull_pieces(ph["obj_hull"])
    eng, _ = parity.make_pair(Engine, lib, table, n, phys=ph)
    eng.reset()
    z = np.zeros((n, 7), np.float32)
    for _ in range(steps):
        eng.step(z)
    s = eng.get_state().astype(np.float64)
    phys = eng.get_physics()
    top = phys.table_c[2] + phys.table_h[2]
    for e in range(n):
        R = _quat_R(s[e, 12:16])
        tilt = np.arccos(np.clip(R[2, 2], -1, 1))
        assert tilt < 1e-3, (e, tilt)
        pts = [s[e, 9:12] + p @ R.T for p in pieces]
        for p in pts:
            assert abs(p[:, 2].min() - top) <= phys.linear_slop + 1e-6, (e, p[:, 2].min() - top)
        assert np.linalg.norm(s[e, 25:28]) < 1e-3 and np.linalg.norm(s[e, 28:31]) < 1e-3, s[e, 25:31]
        ch = select_slots(pts, [p[:, 2] - top for p in pts], phys.contact_margin)
        assert {p for p, _ in ch} == {0, 1} and len(ch) == NC_OT, ch
    assert (contacts.contact_flags(table, s, eng.ndof, phys, hull=ph["obj_hull"]) & contacts.OBJECT_TABLE).all()
    eng.close()
    return s


# ------------------------------------------------------------------------------------- robot spheres against one piece of a compound
def twin_cubes(h, gap, mass=0.1, mu=1.0):
    """two cubes of half extent h whose centres are `gap` apart along x"""
    return compound_physics([cube((-gap / 2, 0, 0), h), cube((gap / 2, 0, 0), h)], mass, mu)


def _box_symmetries(h):
    """the rotations (signed permutations, det +1) that map the box of half extents h onto itself"""
    import itertools
    out = []
    for perm in itertools.permutations(range(3)):
        for sg in itertools.product((1.0, -1.0), repeat=3):
            S = np.zeros((3, 3))
            for i in range(3):
                S[perm[i], i] = sg[i]
            if np.linalg.det(S) > 0 and np.allclose(np.abs(S) @ h, h):
                out.append(S)
    return out


def onto_piece(table, states, off, phys, ph, k, h):
    """box states (a box of half extents h at Q[off..off+7), a robot sphere in it) -> states of the compound `ph` whose piece k takes the
    box's place exactly (a symmetry of the box turns the compound so that its other pieces touch nothing: contact_flags).  Returns the
    states that have such a turn, and the object-frame centre of piece k."""
    from scipy.spatial.transform import Rotation
    pieces = hull_pieces(ph["obj_hull"])
    ck = 0.5 * (pieces[k].min(0) + pieces[k].max(0))
    others = [p for i, p in enumerate(pieces) if i != k]
    out = []
    for s in states:
        Rb = _quat_R(s[off + 3:off + 7])
        for S in _box_symmetries(np.asarray(h, float)):
            t = s.copy()
            Rc = Rb @ S
            t[off:off + 3] = s[off:off + 3] - Rc @ ck
            t[off + 3:off + 7] = Rotation.from_matrix(Rc).as_quat()
            if all(contacts.contact_flags(table, t[None], off, phys, hull=p)[0] == 0 for p in others):
                out.append(t)
                break
    return np.array(out), ck


def check_sphere_on_pieces(Engine, lib, table, panda, n=16):
    """Panda (k_step): a hand sphere ~2 mm inside piece 0, then inside piece 1 (non-zero vertex / face offsets in the table's directory)
    of a two-cube compound, the other piece clear of everything: ROBOT_OBJECT with the compound's geometry, and one step against the
    oracle with that piece alone as its hull (the compound's frame, mass and inertia), per quantity"""
    h = 0.025                                                           # (scenarios.object_contact_states: the 5 cm cube)
    ph = twin_cubes(h, 0.16)
    out = {}
    for k in (0, 1):
        eng, ora = parity.make_pair(Engine, lib, table, n, phys=ph)
        pieces = hull_pieces(ph["obj_hull"])
        orc.set_object(ora, dict(ph, obj_hull=pieces[k]))
        ora32 = orc.Oracle(table, f32=True, task=1)
        ora32.task.obj_pose_rnd_std, ora32.task.tg_pose_rnd_std = ora.task.obj_pose_rnd_std, ora.task.tg_pose_rnd_std
        orc.set_object(ora32, dict(ph, obj_hull=pieces[k]))
        eng.reset()
        st, _ = ora.batch_reset(n)
        rng = np.random.default_rng(40 + k)
        box_ora = orc.Oracle(table, task=1)                             # (the state generator's filter: the 5 cm cube primitive)
        cand = scenarios.object_contact_states(box_ora, panda["model"], panda["spheres"], st[0], 2 * n, rng)
        s, _ = onto_piece(table, cand, 9, eng.get_physics(), ph, k, [h, h, h])
        assert len(s) >= n, ("too few states with the other piece clear", len(s))
        s = s[:n]
        fl = contacts.contact_flags(table, s, eng.ndof, eng.get_physics(), hull=ph["obj_hull"])
        assert (fl & contacts.ROBOT_OBJECT).all(), fl
        r = parity.check_single_steps(eng, ora, s, rng, steps=1, tol=parity.TOL_CONTACT, skip_ambiguous=True, max_skip=0.5, ora32=ora32,
                                      max_outliers=0.1)
        out[k] = r["compared"]
        eng.close()
    return out


def check_icub_sphere_on_pieces(Engine, lib, n_each=12):
    """the same on the iCub's lane-group kernel kw_step (32 lanes): an arm sphere ~2 mm inside piece 0, then piece 1, against the
    oracle holding that piece alone; states whose contact set flips under a +-3 um nudge of the margin are skipped and counted"""
    h = 0.025
    ph = twin_cubes(h, 0.16)
    pieces = hull_pieces(ph["obj_hull"])
    box = {"obj_shape": 0, "obj_h": [h, h, h], "obj_mass": ph["obj_mass"], "obj_mu": ph["obj_mu"], "obj_inertia": ph["obj_inertia"]}
    eng0, ora0, info = parity.make_icub_pair(Engine, lib, 1, task=1, use_ik=0, obj_std=0.0, tg_std=0.2)
    orc.set_object(ora0, box)
    base, _ = ora0.batch_reset(1)
    eng0.close()
    rep = {}
    for k in (0, 1):
        rng = np.random.default_rng(60 + k)
        S, _ = parity.icub_contact_states(ora0, info, base[0], rng, 2 * n_each, 0, 0, 0)
        eng, ora, info = parity.make_icub_pair(Engine, lib, 1, task=1, use_ik=0, obj_std=0.0, tg_std=0.2, max_steps=10 ** 6, phys=ph)
        s, _ = onto_piece(_icub_table(), S, eng.obj_off, eng.get_physics(), ph, k, [h, h, h])
        eng.close()
        assert len(s) >= n_each, ("too few states with the other piece clear", len(s))
        s = s[:n_each]
        n = len(s)
        eng, ora, info = parity.make_icub_pair(Engine, lib, n, task=1, use_ik=0, obj_std=0.0, tg_std=0.2, max_steps=10 ** 6, phys=ph)
        orc.set_object(ora, dict(ph, obj_hull=pieces[k]))
        ora.task.max_steps = 10 ** 6
        assert eng.get_physics().obj_shape == 3 and ora.params.obj_shape == 3
        fl = contacts.contact_flags(_icub_table(), s, eng.obj_off, eng.get_physics(), hull=ph["obj_hull"])
        assert (fl & contacts.ROBOT_OBJECT).all(), fl
        eng.reset()
        a = rng.uniform(-1, 1, (n, eng.act_dim)).astype(np.float32)
        s32 = s.astype(np.float32)
        eng.set_state(s32)
        ob, rw, dn = eng.step(a)
        se = eng.get_state()
        so, out = ora.batch_step(s32.astype(np.float64), a)
        ok = ~parity.ambiguous_envs(ora, s32.astype(np.float64), a)
        assert ok.sum() >= n // 2, ("ambiguous", int((~ok).sum()), n)
        w = parity.group_quantities(eng, se[ok], so[ok], ob[ok], out[ok])
        parity.assert_within(w, parity.TOL_ICUB_CONTACT, "(iCub: sphere in piece %d of a compound)" % k)
        rep[k] = {"compared": int(ok.sum()), "worst": dict((q, float("%.3g" % v)) for q, v in w.items())}
        eng.close()
    return rep


def _icub_table(control_arm="l"):
    from pybullet_robot_envs.model.table import icub_table
    return icub_table(control_arm)[0]


def check_slots_against_oracle(Engine, lib, table, n=6):
    """The object-table slots the kernel takes for a compound resting tilted on the table, against select_slots: per env, an oracle whose
    hull is exactly the 4 vertices select_slots picks (in candidate order) plus an apex far above the margin, so that the oracle's
    contact points are those 4; one step from identical states, per quantity.  Two pieces in touch (select_compound's step 2: the two
    spans) and three pieces in touch (step 1 and the deepest of the rest); another choice of 4 points moves the object differently."""
    from scipy.spatial.transform import Rotation
    cases = {"two": compound_physics([cube((-0.03, 0, 0), 0.015), cube((0.03, 0, 0), 0.015)], 0.1, 1.0),
             "three": compound_physics([cube((-0.03, 0, 0), 0.012), cube((0.03, 0, 0), 0.012), cube((0, 0.04, 0), 0.012)], 0.1, 1.0)}
    rep = {}
    for name, ph in cases.items():
        pieces = hull_pieces(ph["obj_hull"])
        eng, _ = parity.make_pair(Engine, lib, table, n, phys=ph)
        eng.reset()
        base = eng.get_state().astype(np.float64)
        phys = eng.get_physics()
        top = phys.table_c[2] + phys.table_h[2]
        rng = np.random.default_rng(77)
        s = base.copy()
        ora_hulls = []
        for e in range(n):
            ax = rng.normal(size=3); ax[2] = 0; ax /= np.linalg.norm(ax)
            R = (Rotation.from_rotvec(ax * rng.uniform(0.004, 0.008)) * Rotation.from_rotvec([0, 0, rng.uniform(-3, 3)])).as_matrix()
            low = min((p @ R.T)[:, 2].min() for p in pieces)
            s[e, 9:12] = [1.3, rng.uniform(-0.35, 0.35), top - low - rng.uniform(1e-4, 3e-4)]     # out of the arm's reach
            s[e, 12:16] = Rotation.from_matrix(R).as_quat()
            s[e, 25:31] = 0
            s[e, 25:27] = rng.uniform(-0.05, 0.05, 2); s[e, 30] = rng.uniform(-0.5, 0.5)
            pts = [s[e, 9:12] + p @ R.T for p in pieces]
            ch = select_slots(pts, [p[:, 2] - top for p in pts], phys.contact_margin)
            assert len(ch) == NC_OT and len({p for p, _ in ch}) == len(pieces), ch
            hv = np.array([pieces[p][i] for p, i in ch] + [[0.0, 0.0, 0.08]])
            ora_hulls.append(hv)
        s32 = s.astype(np.float32)
        a = rng.uniform(-1, 1, (n, 7)).astype(np.float32)
        eng.set_state(s32)
        ob, rw, dn = eng.step(a)
        se = eng.get_state()
        worst = {}
        for e in range(n):
            ora = orc.Oracle(table, task=1)
            orc.set_object(ora, dict(ph, obj_hull=ora_hulls[e]))
            so, out = ora.batch_step(s32[e:e + 1].astype(np.float64), a[e:e + 1])
            parity.merge_worst(worst, parity.panda_quantities(se[e:e + 1], so, ob[e:e + 1], out))
        parity.assert_within(worst, parity.TOL_CONTACT, "(compound slots, %s pieces in touch)" % name)
        rep[name] = dict((q, float("%.3g" % v)) for q, v in worst.items())
        eng.close()
    return rep
