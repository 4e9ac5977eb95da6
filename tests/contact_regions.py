"""Robot-object contacts region by region at arbitrary object poses (tests only).

Every step kernel turns "collision sphere against the object" into a contact row through a hand-written narrow phase -- the lane form
Core::sphere_box / sphere_round / sphere_hull (csrc/pbre_core.hpp) or the scalar form Fast::sphere_box / Shapes::sphere_round
(csrc/pbre_fast.hpp, pbre_objstep.hpp).  This module places ONE collision sphere of the Panda's hand in a NAMED region of an object --
a face, an edge, a vertex of a box or a hull, the cap, the lateral surface, the rim of a can, the inside of any of them -- at a uniformly
random orientation of the object, and keeps the state only if the fp64 oracle (a) lists exactly that one robot-object contact and nothing
else, (b) reports the normal, the signed distance and the point on the object that the region's closed form gives, and (c) calls the
state well conditioned (row_paths.flagged).  Everything here runs on the CPU from the oracle alone; tests/test_emu_contact_regions.py and
tests/test_gpu_contact_regions.py replay the same batches through the engines.

The closed forms are written per region (the face's plane, the edge's line, the vertex, the rim's circle), never through a classifier
of the point: that is what the narrow phases under test are.  They are evaluated in float64 on the float32-rounded state, in the
object frame R^T (c - x) of the rotation matrix the oracle builds from the (rounded, hence not exactly unit) quaternion.

One select cannot be reached through a state record: the cylinder's on-axis one (`rho <= 1e-12`).  The sphere centre comes out of the
forward kinematics and the object's position is a float32, so the smallest radial coordinate a state can have is the rounding of that
position, ~3e-8 m.  The "axis" region places the centre there: the radial unit vector is then the direction of a rounding residue, which
the cap's normal must not depend on.
"""
import functools

import numpy as np

import orc
import row_paths
import scenarios

NJ = 9
SEED = 20241103
DEPTH = 0.002                 # how far the sphere's SURFACE is inside the object (regions on the outside)
MIN_PER_REGION = 6
FAR_TARGET = (0.9, 0.9, 0.65)
SPHERES = (0, 1, 2, 3, 4, 5)  # PANDA_SPHERES: the four finger spheres, the two 35 mm hand spheres
# velocities of the moving sets: N(0, QD_STD) on the joints, N(0, TWIST_STD) on the object's twist (scenarios.object_contact_states).  The
# values the issue names; they did not have to be lowered (no batch needed more than a few rounds of re-drawing).
QD_STD, TWIST_STD = 0.3, 0.15
# bounds of the oracle against the closed form (both float64 on the same rounded state)
TOL_N, TOL_DIST, TOL_PB = 1e-6, 1e-8, 1e-7


def quat_R(q):
    """the oracle's quat_to_R (x, y, z, w; local -> world), without normalising"""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _unit(v):
    return v / np.linalg.norm(v)


# ---------------------------------------------------------------------------------------------------------------- regions
# A region draw returns (p, form): p = the sphere CENTRE in the object frame for a sphere of radius rs, form = the closed form of the
# region, a function p -> (n, d, pb): outward unit normal, signed distance of the CENTRE to the surface, point on the surface -- all in
# the object frame.  form is evaluated again on the rounded state.
def _plane_form(a, n):
    def form(p):
        d = float(n @ (p - a))
        return n.copy(), d, p - n * d
    return form


def _point_form(v):
    def form(p):
        e = p - v
        d = np.linalg.norm(e)
        return e / d, float(d), v.copy()
    return form


def _line_form(a, u):
    """closest point on the line a + t u (u a unit vector); the draw keeps t inside the edge"""
    def form(p):
        q = a + u * float(u @ (p - a))
        e = p - q
        d = np.linalg.norm(e)
        return e / d, float(d), q
    return form


class Box:
    kind = "box"

    def __init__(self, h):
        self.h = np.asarray(h, np.float64)
        self.regions = (["face%s%s" % (s, a) for a in "xyz" for s in "+-"] + ["edge_%s" % a for a in "xyz"] + ["vertex"] + ["in_%s" % a for a in "xyz"])

    def draw(self, region, rs, rng, k):
        h = self.h
        out = rs - DEPTH
        if region.startswith("face"):
            s, a = (1.0 if region[4] == "+" else -1.0), "xyz".index(region[5])
            p = rng.uniform(-1, 1, 3) * (h - 0.003)
            p[a] = s * (h[a] + out)
            n = np.zeros(3); n[a] = s
            return p, _plane_form(n * h[a], n)
        if region.startswith("edge"):
            a = "xyz".index(region[5])
            b, c = (a + 1) % 3, (a + 2) % 3
            sb, sc = rng.choice([-1.0, 1.0], 2)
            th = np.deg2rad(rng.uniform(10, 80))
            e = np.zeros(3); e[a] = rng.uniform(-1, 1) * (h[a] - 0.003); e[b] = sb * h[b]; e[c] = sc * h[c]
            m = np.zeros(3); m[b] = sb * np.cos(th); m[c] = sc * np.sin(th)
            u = np.zeros(3); u[a] = 1.0
            return e + m * out, _line_form(e, u)
        if region == "vertex":
            sg = rng.choice([-1.0, 1.0], 3)
            m = _unit(rng.uniform(0.25, 1.0, 3)) * sg
            return sg * h + m * out, _point_form(sg * h)
        a = "xyz".index(region[3])                                   # in_<a>: the centre 1 - 4 mm behind a face of axis a, farther from the others
        s = rng.choice([-1.0, 1.0])
        dep = rng.uniform(0.001, 0.004)
        p = rng.uniform(-1, 1, 3) * (h - dep - 0.003)
        p[a] = s * (h[a] - dep)
        n = np.zeros(3); n[a] = s
        return p, _plane_form(n * h[a], n)


class Ball:
    kind = "ball"
    regions = ["surface"]

    def __init__(self, r):
        self.r = float(r)

    def draw(self, region, rs, rng, k):
        m = _unit(rng.normal(size=3))
        r = self.r

        def form(p):
            d = np.linalg.norm(p)
            return p / d, float(d - r), p / d * r
        return m * (r + rs - DEPTH), form


class Cylinder:
    kind = "cylinder"
    RIM_ELEVATIONS = (8.0, 22.0, 36.0, 50.0, 64.0, 78.0, 86.0)         # degrees above the cap's plane, across (0, 90)

    def __init__(self, r, hh):
        self.r, self.hh = float(r), float(hh)
        self.regions = ["cap+", "cap-", "lateral", "rim+", "rim-", "axis", "in_lat", "in_cap"]

    def _cap_form(self, s):
        return _plane_form(np.array([0.0, 0.0, s * self.hh]), np.array([0.0, 0.0, s]))

    def _lat_form(self):
        r = self.r

        def form(p):
            rho = np.hypot(p[0], p[1])
            u = np.array([p[0] / rho, p[1] / rho, 0.0])
            return u, float(rho - r), np.array([u[0] * r, u[1] * r, p[2]])
        return form

    def _rim_form(self, s):
        r, hh = self.r, self.hh

        def form(p):
            rho = np.hypot(p[0], p[1])
            q = np.array([p[0] / rho * r, p[1] / rho * r, s * hh])
            e = p - q
            d = np.linalg.norm(e)
            return e / d, float(d), q
        return form

    def draw(self, region, rs, rng, k):
        r, hh = self.r, self.hh
        out = rs - DEPTH
        ph = rng.uniform(0, 2 * np.pi)
        u = np.array([np.cos(ph), np.sin(ph), 0.0])
        ez = np.array([0.0, 0.0, 1.0])
        if region in ("cap+", "cap-"):
            s = 1.0 if region[3] == "+" else -1.0
            return u * rng.uniform(0.001, r - 0.003) + ez * s * (hh + out), self._cap_form(s)
        if region == "lateral":
            return u * (r + out) + ez * rng.uniform(-1, 1) * (hh - 0.003), self._lat_form()
        if region in ("rim+", "rim-"):
            s = 1.0 if region[3] == "+" else -1.0
            el = np.deg2rad(self.RIM_ELEVATIONS[k % len(self.RIM_ELEVATIONS)])
            return u * r + ez * s * hh + (u * np.cos(el) + ez * s * np.sin(el)) * out, self._rim_form(s)
        if region == "axis":                                         # radial coordinate: whatever the rounding of the object's position leaves
            s = 1.0 if k % 2 == 0 else -1.0
            return ez * s * (hh + out), self._cap_form(s)
        dep = rng.uniform(0.001, 0.004)
        if region == "in_lat":                                       # inside, nearer the lateral surface; radial coordinate > 0.016 m
            rho = r - dep
            assert rho > 0.016
            return u * rho + ez * rng.uniform(-1, 1) * (hh - dep - 0.003), self._lat_form()
        s = rng.choice([-1.0, 1.0])                                  # in_cap: inside, nearer a cap
        return u * rng.uniform(0.001, r - dep - 0.003) + ez * s * (hh - dep), self._cap_form(s)


class Hull:
    kind = "hull"

    def __init__(self, verts, all_edges=False):
        from scipy.spatial import ConvexHull
        self.v = np.asarray(verts, np.float64)
        H = ConvexHull(self.v)
        self.tri = H.simplices
        self.nrm = H.equations[:, :3].copy()
        self.off = -H.equations[:, 3].copy()                         # face f: nrm[f] . x = off[f]
        edges = {}
        for f, t in enumerate(self.tri):
            for i in range(3):
                edges.setdefault(tuple(sorted((int(t[i]), int(t[(i + 1) % 3])))), []).append(f)
        self.edges = sorted((e, fs) for e, fs in edges.items() if len(fs) == 2)
        self.all_edges = all_edges                                   # draw k of "edge" takes edge k % len(edges): every edge comes up
        self.regions = ["face", "edge", "vertex", "inside"]

    def draw(self, region, rs, rng, k):
        v, out = self.v, rs - DEPTH
        if region == "face":
            f = int(rng.integers(len(self.tri)))
            w = 0.15 + 0.55 * rng.dirichlet([1.0, 1.0, 1.0])
            a = w @ v[self.tri[f]]
            return a + self.nrm[f] * out, _plane_form(a, self.nrm[f])
        if region == "edge":
            (i, j), (f1, f2) = self.edges[k % len(self.edges)] if self.all_edges else self.edges[int(rng.integers(len(self.edges)))]
            e = v[i] + rng.uniform(0.25, 0.75) * (v[j] - v[i])
            m = _unit(self.nrm[f1] + self.nrm[f2])
            return e + m * out, _line_form(v[i], _unit(v[j] - v[i]))
        if region == "vertex":
            i = int(rng.integers(len(v)))
            m = _unit(self.nrm[[f for f, t in enumerate(self.tri) if i in t]].mean(0))
            return v[i] + m * out, _point_form(v[i])
        for _ in range(1000):                                        # inside: 1 - 3 mm behind a face, at least 1 mm farther from every other
            f = int(rng.integers(len(self.tri)))
            w = 0.2 + 0.4 * rng.dirichlet([1.0, 1.0, 1.0])
            dep = rng.uniform(0.001, 0.003)
            p = w @ v[self.tri[f]] - self.nrm[f] * dep
            sd = self.nrm @ p - self.off
            same = np.abs(self.nrm @ self.nrm[f] - 1.0) < 1e-9        # (coplanar triangles of one face)
            if (sd[~same] < -dep - 0.001).all():
                return p, _plane_form(v[self.tri[f][0]], self.nrm[f])
        raise AssertionError("no point 1 - 3 mm behind exactly one face")


# ---------------------------------------------------------------------------------------------------------------- objects
def objects():
    """name -> (physics dict of the engine, shape with the regions).  The can twice (the slim soup can and the squat MasterChef can), a
    non-cube box, the ball, two hulls; and the 5 cm cube, the one object whose complex envs the lane-per-env robot-contact kernel
    steps (Fast::sphere_box -- every other primitive's go to the row kernel: pbre_panda.hpp, launch_step_t)."""
    from pybullet_robot_envs.model.objects import object_physics, hull_physics
    import parity
    out = {}
    for name in ("YcbCrackerBox", "cube_small"):
        ph = object_physics(name, use_mesh=False)
        out[name] = (ph, Box(ph["obj_h"]))
    ph = object_physics("YcbTennisBall", use_mesh=False)
    out["YcbTennisBall"] = (ph, Ball(ph["obj_h"][0]))
    for name in ("YcbTomatoSoupCan", "YcbMasterChefCan"):
        ph = object_physics(name, use_mesh=False)
        out[name] = (ph, Cylinder(ph["obj_h"][0], ph["obj_h"][2]))
    for name in ("tetra", "blob20"):
        verts, mass, mu = parity.hull_test_objects()[name]
        ph = hull_physics(verts, mass, mu)
        out[name] = (ph, Hull(ph["obj_hull"], all_edges=name == "tetra"))
    return out


OBJECTS = ("YcbCrackerBox", "cube_small", "YcbTennisBall", "YcbTomatoSoupCan", "YcbMasterChefCan", "tetra", "blob20")
HULLS = ("tetra", "blob20")


class Batch:
    """S [n, STATE] float32, A [n, 7] float32, region[e], sphere[e]; so / out: the fp64 oracle's step of (S, A), computed once"""

    def __init__(self, name, moving, lab, S, A, region, sphere, tries):
        self.name, self.moving, self.lab, self.S, self.A, self.region, self.sphere, self.tries = name, moving, lab, S, A, region, sphere, tries
        self.so, self.out = lab.ora.batch_step(S.astype(np.float64), A)

    @property
    def n(self):
        return len(self.S)


def object_lab(panda, ph):
    lab = row_paths.Lab(panda, False)
    lab.phys = dict(ph)
    for o in (lab.ora, lab.ora32):
        orc.set_object(o, ph)
    return lab


def closed_form_world(lab, s, sphere, form):
    """(n, dist, pB) in world axes of the region's closed form on the fp32 state s: float64 throughout"""
    s = np.asarray(s, np.float32).astype(np.float64)
    P = lab.panda
    c, rs = scenarios.sphere_centres(lab.ora, P["model"], P["spheres"], s[:NJ])[sphere]
    R = quat_R(s[12:16])
    n, d, pb = form(R.T @ (c - s[9:12]))
    return R @ n, d - rs, s[9:12] + R @ pb


def accept(lab, s, sphere, form):
    """the oracle-only rule: exactly one contact, the chosen sphere's against the object, equal to the closed form.  Returns None or the
    differences (n, dist, pB)."""
    s64 = np.asarray(s, np.float32).astype(np.float64)
    _, info = lab.ora.sim_step(s64, s64[:NJ].copy(), np.full(NJ, 0.1), np.full(NJ, 1.0))
    if info.ncontacts != 1 or info.type[0] != 1 or info.idx[0] != sphere:
        return None
    n, d, pb = closed_form_world(lab, s, sphere, form)
    err = (float(np.linalg.norm(np.array(info.n[0][:]) - n)), abs(float(info.dist[0]) - d), float(np.linalg.norm(np.array(info.pB[0][:]) - pb)))
    assert err[0] <= TOL_N and err[1] <= TOL_DIST and err[2] <= TOL_PB, \
        "the oracle's contact differs from the closed form of the region (n, dist, pB): %r, bounds %r" % (err, (TOL_N, TOL_DIST, TOL_PB))
    return err


def _candidate(lab, shape, region, rng, k, moving):
    P = lab.panda
    s = lab.base.copy()
    q = scenarios.HOME + rng.normal(0, 0.2, NJ)
    q[7:] = 0.035
    q = np.clip(q, lab.lo + 0.05 * (lab.hi - lab.lo), lab.hi - 0.05 * (lab.hi - lab.lo)).astype(np.float32).astype(np.float64)
    sphere = int(rng.choice(SPHERES[:4])) if rng.random() < 0.75 else int(rng.choice(SPHERES[4:]))
    c, rs = scenarios.sphere_centres(lab.ora, P["model"], P["spheres"], q)[sphere]
    p, form = shape.draw(region, rs, rng, k)
    quat = _unit(rng.normal(size=4))                                 # uniform on the rotation group
    R = quat_R(quat.astype(np.float32).astype(np.float64))
    s[:NJ] = q
    s[12:16] = quat
    s[9:12] = c - R @ p
    s[16:31] = 0.0
    if moving:
        s[16:25] = rng.normal(0, QD_STD, NJ)
        s[25:31] = rng.normal(0, TWIST_STD, 6)
    s[32:35] = FAR_TARGET
    return np.asarray(s, np.float32), sphere, form


def _draw(lab, shape, region, rng, k, moving, counter):
    for _ in range(20000):
        counter[0] += 1
        s, sphere, form = _candidate(lab, shape, region, rng, k, moving)
        if accept(lab, s, sphere, form) is not None:
            return s, rng.uniform(-1, 1, 7).astype(np.float32), sphere, form
    raise AssertionError("region %r: no single-contact state in 20000 placements" % region)


def _count(shape, region):
    if shape.kind == "cylinder" and region.startswith("rim"):
        return len(shape.RIM_ELEVATIONS)                             # every elevation on both caps
    if shape.kind == "ball":
        return 2 * MIN_PER_REGION
    if shape.kind == "hull" and region == "edge" and shape.all_edges:
        return max(MIN_PER_REGION, len(shape.edges))
    return MIN_PER_REGION


def build(panda, name, moving):
    ph, shape = objects()[name]
    lab = object_lab(panda, ph)
    rng = np.random.default_rng(SEED + 2 * OBJECTS.index(name) + int(moving))
    slots = [(r, k) for r in shape.regions for k in range(_count(shape, r))]
    counter = [0]
    cur = [_draw(lab, shape, r, rng, k, moving, counter) for r, k in slots]
    for rnd in range(40):                                            # as row_paths._build: re-draw what the oracle calls ill conditioned
        S = np.array([c[0] for c in cur]); A = np.array([c[1] for c in cur])
        bad = np.nonzero(row_paths.flagged(lab, S, A))[0]
        if not len(bad):
            break
        for e in bad:
            cur[e] = _draw(lab, shape, slots[e][0], rng, slots[e][1], moving, counter)
    else:
        raise AssertionError("%s (%s): still ill-conditioned states after 40 rounds of re-drawing" % (name, "moving" if moving else "at rest"))
    b = Batch(name, moving, lab, S, A, [r for r, _ in slots], np.array([c[2] for c in cur]), {"placements": counter[0], "rounds": rnd})
    b.forms = [c[3] for c in cur]
    b.shape = shape
    assert_coverage(b)
    return b


def assert_coverage(b):
    """every region of the object's list with at least MIN_PER_REGION states; the tetrahedron's six edges each; the rim at every
    elevation on both caps; in_lat beyond the radius at which fp32 leaves a residue above 1e-9"""
    have = dict((r, b.region.count(r)) for r in b.shape.regions)
    assert all(v >= MIN_PER_REGION for v in have.values()) and set(b.region) == set(b.shape.regions), have
    if b.shape.kind == "hull" and b.shape.all_edges:
        seen = set()
        for e in range(b.n):
            if b.region[e] == "edge":
                _, _, pb = b.forms[e](object_frame(b, e))
                seen.add(min(range(len(b.shape.edges)), key=lambda i: _seg_dist(b.shape.v, b.shape.edges[i][0], pb)))
        assert len(seen) == len(b.shape.edges) == 6, seen
    if b.shape.kind == "cylinder":
        for e in range(b.n):
            p = object_frame(b, e)
            rho = float(np.hypot(p[0], p[1]))
            if b.region[e] == "in_lat":
                assert rho > 0.016 and rho < b.shape.r and abs(p[2]) < b.shape.hh
            if b.region[e] == "axis":
                assert rho < 2e-7, rho


def _seg_dist(v, e, p):
    a, d = v[e[0]], v[e[1]] - v[e[0]]
    t = min(1.0, max(0.0, float(d @ (p - a)) / float(d @ d)))
    return float(np.linalg.norm(p - a - t * d))


def object_frame(b, e):
    """the chosen sphere's centre in the object frame of state e (float64 on the rounded state)"""
    s = b.S[e].astype(np.float64)
    P = b.lab.panda
    c, _ = scenarios.sphere_centres(b.lab.ora, P["model"], P["spheres"], s[:NJ])[int(b.sphere[e])]
    return quat_R(s[12:16]).T @ (c - s[9:12])


_PANDA = {}


@functools.lru_cache(maxsize=None)
def _batch(panda_key, name, moving):
    return build(_PANDA[panda_key], name, moving)


def batch(panda, name, moving):
    """cached: the states and the oracle's verdicts are computed once per process"""
    _PANDA[id(panda)] = panda
    return _batch(id(panda), name, bool(moving))


# ---------------------------------------------------------------------------------------------------------------- the comparison
def compare(b, eng, tol=None, tag=""):
    """one step of the batch from its fp32 states with its own actions against the fp64 oracle: every env is compared (nothing is skipped,
    there is no outlier allowance), every quantity of tol (parity.TOL_CONTACT).  Returns {region: {quantity: worst}}; raises with the
    failing regions named.  tag: the kernel's name for the record PBRE_PARITY_MEASURE=1 prints (profiles/r12_contact_regions.json)."""
    import parity
    tol = parity.TOL_CONTACT if tol is None else tol
    eng.set_state(b.S)
    ob, rw, dn = eng.step(b.A)
    se = np.asarray(eng.get_state(), np.float64)
    q = row_paths.quantities_per_env(se, b.so, np.asarray(ob, np.float64), b.out)
    q["reward"] = parity.rel(rw, b.out[:, -2])
    worst, bad = {}, {}
    for r in sorted(set(b.region)):
        m = np.array([x == r for x in b.region])
        worst[r] = dict((k, float(v[m].max())) for k, v in q.items())
        over = dict((k, (float("%.3g" % v), tol[k])) for k, v in worst[r].items() if k in tol and not v <= tol[k])
        if over:
            bad[r] = over
    if parity.MEASURE:
        import json
        print("CONTACT_REGIONS " + json.dumps({"object": b.name, "moving": b.moving, "kernel": tag, "envs": b.n,
                                               "worst": dict((r, dict((k, float("%.3g" % x)) for k, x in w.items())) for r, w in worst.items())}))
    assert np.array_equal(np.asarray(dn, np.float64), b.out[:, -1]), "done flags differ"
    assert not bad, "%s (%s), regions beyond the bounds (measured, bound): %r" % (b.name, "moving" if b.moving else "at rest", bad)
    return worst


# ---------------------------------------------------------------------------------------------------------------- iCub push with the can
# The same placement on the 20-DoF iCub (joint control, left arm): a hand sphere of the controlled arm in a region of the soup can.  This
# drives Core::sphere_round at 32 lanes (the lane-group kernel, PBRE_ICUB_LANE=0) and whatever the lane-per-env pipeline does with an env
# in robot-object contact (PBRE_ICUB_LANE=1).  State record: Q[32] | V[32] | X[16], the object's pose behind the 20 joints.
ICUB_OBJECT = "YcbTomatoSoupCan"
ICUB_REGIONS = ("cap+", "lateral", "rim+", "in_lat")
ICUB_PER_REGION = 4
ICUB_HAND_SPHERES = (0, 1)      # model/table.py: icub_spheres -- the two spheres of l_hand (radius 32 mm and 22 mm)


class _Dims:
    def __init__(self, ndof, v_off):
        self.ndof, self.v_off = ndof, v_off


class ICubLab:
    def __init__(self):
        from pybullet_robot_envs.model.objects import object_physics
        from pybullet_robot_envs.model.table import icub_model, icub_spheres
        self.phys = object_physics(ICUB_OBJECT, use_mesh=False)
        self.ora, self.table, self.info = orc.icub_oracle("l", task=1, use_ik=0)
        self.ora32, _, _ = orc.icub_oracle("l", task=1, use_ik=0, f32=True)
        for o in (self.ora, self.ora32):                             # as parity.make_icub_pair + check_icub_contact_states
            o.task.reward_type, o.task.obj_pose_rnd_std, o.task.tg_pose_rnd_std, o.task.max_steps = 1, 0.0, 0.2, 10 ** 6
            orc.set_object(o, self.phys)
        self.nd = self.ora.ndof
        self.base = self.ora.batch_reset(1)[0][0]
        self.vo = (len(self.base) - 16) // 2
        self.dims = _Dims(self.nd, self.vo)
        m = icub_model()
        names = [l["name"] for l in m["links"]]
        self.spheres = [(names.index(ln), np.array(c), r) for ln, c, r in icub_spheres(m)]
        self.lo = np.array([self.ora.model.lower[self.ora.model.link_of_dof[k]] for k in range(self.nd)])
        self.hi = np.array([self.ora.model.upper[self.ora.model.link_of_dof[k]] for k in range(self.nd)])

    def engine(self, Engine, lib, n):
        import parity
        eng, _, _ = parity.make_icub_pair(Engine, lib, n, task=1, control_arm="l", use_ik=0, obj_std=0.0, tg_std=0.2, max_steps=10 ** 6, phys=self.phys)
        return eng

    def centre(self, q, sphere):
        R, p = self.ora.fk(q)
        i, c, r = self.spheres[sphere]
        return p[i] + R[i] @ c, r

    def accept(self, s, sphere, form):
        nd = self.nd
        s64 = np.asarray(s, np.float32).astype(np.float64)
        _, info = self.ora.sim_step(s64, s64[:nd].copy(), np.full(nd, 0.1), np.full(nd, 1.0))
        if info.ncontacts != 1 or info.type[0] != 1 or info.idx[0] != sphere:
            return None
        c, rs = self.centre(s64[:nd], sphere)
        R = quat_R(s64[nd + 3:nd + 7])
        n, d, pb = form(R.T @ (c - s64[nd:nd + 3]))
        err = (float(np.linalg.norm(np.array(info.n[0][:]) - R @ n)), abs(float(info.dist[0]) - (d - rs)),
               float(np.linalg.norm(np.array(info.pB[0][:]) - (s64[nd:nd + 3] + R @ pb))))
        assert err[0] <= TOL_N and err[1] <= TOL_DIST and err[2] <= TOL_PB, ("the oracle's contact differs from the region's closed form", err)
        return err

    def quantities(self, se, so, ob, out):
        """parity.group_quantities env by env"""
        import parity
        rows = [parity.group_quantities(self.dims, se[e:e + 1], so[e:e + 1], ob[e:e + 1], out[e:e + 1]) for e in range(len(se))]
        return dict((k, np.array([r[k] for r in rows])) for k in rows[0])

    def flagged(self, S, A, tol):
        """row_paths.flagged for the lane-group layout: a contact candidate within 3 um of the margin, or a result that moves by more than
        half the bounds when the fp64 oracle's input is perturbed at the fp32 rounding level or its fp32 build runs instead"""
        import parity
        nd, vo = self.nd, self.vo
        s32 = np.asarray(S, np.float32)
        s64 = s32.astype(np.float64)
        n = len(s32)
        bad = parity.ambiguous_envs(self.ora, s64, A)
        so, out = self.ora.batch_step(s64, A)
        prng = np.random.default_rng(12345)
        trials = [self.ora32.batch_step(s32, A)]
        cols = np.r_[0:nd + 7, vo:vo + nd + 6]
        for _ in range(4):
            sp = s64.copy()
            sp[:, cols] *= 1.0 + prng.uniform(-2e-7, 2e-7, (n, len(cols)))
            trials.append(self.ora.batch_step(sp, A))
        for s_f, o_f in trials:
            qf = self.quantities(np.asarray(s_f, np.float64), so, np.asarray(o_f[:, :-2], np.float64), out)
            for k, v in qf.items():
                if k in tol:
                    bad |= v > 0.5 * tol[k]
        return bad


def _icub_draw(lab, shape, region, rng, k, counter):
    nd, vo = lab.nd, lab.vo
    ctrl = np.array(lab.info["controlled"])
    for _ in range(20000):
        counter[0] += 1
        s = np.array(lab.base, np.float64)
        q = s[:nd].copy()
        q[ctrl] += rng.normal(0, 0.3, len(ctrl))
        q = np.clip(q, lab.lo + 2e-3, lab.hi - 2e-3).astype(np.float32).astype(np.float64)
        sphere = int(rng.choice(ICUB_HAND_SPHERES))
        c, rs = lab.centre(q, sphere)
        p, form = shape.draw(region, rs, rng, k)
        quat = _unit(rng.normal(size=4))
        s[:nd] = q
        s[nd + 3:nd + 7] = quat
        s[nd:nd + 3] = c - quat_R(quat.astype(np.float32).astype(np.float64)) @ p
        s[vo:vo + nd + 6] = 0.0
        s = np.asarray(s, np.float32)
        if lab.accept(s, sphere, form) is not None:
            return s, rng.uniform(-1, 1, len(ctrl)).astype(np.float32), sphere, form
    raise AssertionError("iCub, region %r: no single-contact state in 20000 placements" % region)


@functools.lru_cache(maxsize=None)
def icub_batch():
    """the can against a hand sphere of the iCub's left arm, ICUB_PER_REGION states per region, everything at rest; accepted by the same
    oracle-only rule as the Panda's"""
    import parity
    lab = ICubLab()
    shape = Cylinder(lab.phys["obj_h"][0], lab.phys["obj_h"][2])
    rng = np.random.default_rng(SEED + 100)
    slots = [(r, k) for r in ICUB_REGIONS for k in range(ICUB_PER_REGION)]
    counter = [0]
    cur = [_icub_draw(lab, shape, r, rng, k, counter) for r, k in slots]
    for rnd in range(40):
        S = np.array([c[0] for c in cur]); A = np.array([c[1] for c in cur])
        bad = np.nonzero(lab.flagged(S, A, parity.TOL_ICUB_CONTACT))[0]
        if not len(bad):
            break
        for e in bad:
            cur[e] = _icub_draw(lab, shape, slots[e][0], rng, slots[e][1], counter)
    else:
        raise AssertionError("iCub: still ill-conditioned states after 40 rounds of re-drawing")
    b = Batch.__new__(Batch)
    b.name, b.moving, b.lab, b.S, b.A, b.region, b.sphere = "icub/" + ICUB_OBJECT, False, lab, S, A, [r for r, _ in slots], np.array([c[2] for c in cur])
    b.tries = {"placements": counter[0], "rounds": rnd}
    b.forms, b.shape = [c[3] for c in cur], shape
    b.so, b.out = lab.ora.batch_step(S.astype(np.float64), A)
    assert all(b.region.count(r) >= ICUB_PER_REGION for r in ICUB_REGIONS)
    return b


def icub_compare(b, eng, tol=None, tag=""):
    """compare() for the lane-group layout, parity.TOL_ICUB_CONTACT"""
    import parity
    tol = parity.TOL_ICUB_CONTACT if tol is None else tol
    eng.set_state(b.S)
    ob, rw, dn = eng.step(b.A)
    se = np.asarray(eng.get_state(), np.float64)
    q = b.lab.quantities(se, b.so, np.asarray(ob, np.float64), b.out)
    worst, bad = {}, {}
    for r in sorted(set(b.region)):
        m = np.array([x == r for x in b.region])
        worst[r] = dict((k, float(v[m].max())) for k, v in q.items())
        over = dict((k, (float("%.3g" % v), tol[k])) for k, v in worst[r].items() if k in tol and not v <= tol[k])
        if over:
            bad[r] = over
    if parity.MEASURE:
        import json
        print("CONTACT_REGIONS " + json.dumps({"object": b.name, "moving": b.moving, "kernel": tag, "envs": b.n,
                                               "worst": dict((r, dict((k, float("%.3g" % x)) for k, x in w.items())) for r, w in worst.items())}))
    assert np.array_equal(np.asarray(dn, np.float64), b.out[:, -1]), "done flags differ"
    assert np.abs(rw - b.out[:, -2]).max() < 1e-3 * max(1.0, np.abs(b.out[:, -2]).max())          # (as parity.check_icub)
    assert not bad, "%s, regions beyond the bounds (measured, bound): %r" % (b.name, bad)
    return worst
