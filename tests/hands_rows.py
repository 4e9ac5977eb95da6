"""States that put every row kind of the hands engine's solve to work, joint by joint (tests only).

The 60-DoF iCub with hands, robot-level interface, right arm, joint control (pbre_hands.hip: Core<DevLanes128, Shape128>::step).  One env per
wave of 64 lanes (128 virtual lanes), four waves per block:

    env = block * 4 + thread / 64

so envs 4 k .. 4 k + 3 share a block and with it the LDS that DevLanes128::RowStore<72> cuts into one private region per wave.  Whoever
remaps envs to waves and blocks in this kernel updates tests/hands_rows.py knowingly: the block-mate check (b) relies on this rule.

Everything here comes from the oracle alone: single-env states by ROW SIGNATURE (joints at a limit by the oracle's own test; robot-object,
robot-table, object-table contact counts from orc.sim_step's StepInfo.type), pools of them, the assertion that every pool is full after the
oracle's own conditioning probe has dropped what it objects to -- so the engine-side checks skip nothing.  Physics variants:

  U   the defaults (PyBullet's default force is an impulse bound of 417, which no pool state comes near): the clamp-free attempt runs through
  B   max_motor_impulse = 0.004 (as parity.check_hands_force_limited_reset): the clamp-free attempt is made, goes over the bound and hands
      back to the clamping rows
  B2  max_motor_impulse = 1e-4: the bound of the finger joints' limit pools (below)
  F   the defaults, every joint of the env force-limited through set_motors / hands_set_motors (force F_FORCE = 10 N, the reference's grasp
      force): fscale < 1, so the attempt is skipped and the clamping loops run directly.  (The step's own command gives the 37 controlled
      joints their full force back; the 23 others -- head, left hand -- stay limited, which is what the skip tests.)  U and F share the
      default physics: check (a) steps them in ONE engine per brick kind, every state twice, the F copies through set_motors(mask=...)
  M   max_motor_impulse = 30, for check (c): a bound that the motors of the pool states stay under and those of a fast state exceed

A limit row of this model is invisible under U: the position motor of the same joint undoes its impulse within the sweep.  With bounded
motors the row decides where the joint goes, but only where the motor alone does not stop the joint; so a `lim` state is accepted only if
the ORACLE's step with and without limit rows (limit_max_impulse at its default and at 0) differs by >= LIM_EFFECT in that joint's velocity.
Under B that holds for every state drawn for the 20 torso / head / arm joints; a 10 g finger link is often stopped by a motor of 0.004 N m s
alone, so a state that fails the rule under B is tried under B2, a bound forty times smaller (15 of the 160 finger states end up there, on
14 joints).  Every limit-type state carries the variant it was found under and is stepped under that variant.  No pool state's step ends
faster than QD_MAX = 12 rad/s in any joint or has a contact deeper than 4 mm: violent steps are what the fast states of check (c) are for.

After 150 sweeps a row that is missing from every second half-sweep has converged to the same impulse regardless, so check (a) also runs
at solver_iters = 1 and 2 (FEW_SWEEPS): the backward half-sweep alone, then backward and forward.
"""
import ctypes
import functools
import json
import time

import numpy as np

import orc
import parity
from row_paths import step_bits

ND, W, LC = 60, 128, 60                # DoF, velocity offset, object offset of the 272-float state record (Q[128] | V[128] | X[16])
MD = orc.MAXD                          # the oracle's motor record: target | kp | force scale | max velocity, MD each
SEED = 20250417
PHYS = {"U": {}, "B": {"max_motor_impulse": 0.004}, "B2": {"max_motor_impulse": 1e-4}, "F": {}, "M": {"max_motor_impulse": 30.0}}
BOUNDED = ("B", "B2")
F_FORCE = 10.0
LIM_EFFECT = 0.05                      # rad/s
PEN = (0.002, 0.03)                    # rad past the limit -- never ON it: fp32 rounding of the limit would flip the row
INTO = (0.1, 5.0)                      # rad/s into the limit
SPREAD = 0.15                          # rad: the other joints about home
CLAMP_MARGIN = 0.05                    # no |qd| of a limit state's result within 5 % of the step's velocity clamp
QD_MAX = 12.0                          # rad/s: no pool state's step ends faster than this in any joint (from rest: 2900 rad/s^2)
N_LIM, N_OTHER = 2, 8
BLOCK = 10                             # Core::step's limit rows are skipped per block of 10 joints (pbre_core.hpp: LB)
MAX_LEFT_OUT = 8
NC_RO, NC_RT = 6, 2                    # robot-object and robot-table contact slots of this shape (oracle/pbre_oracle.h: ORC_NC_RO_HANDS, ORC_NC_RT)
MAX_DEPTH = 0.004                      # m: no contact deeper than this (the crafted scenes aim at 0.5 - 3 mm; deeper ones are collisions, not rows)

RO_K = ["ro1", "ro2", "ro3", "ro4", "ro5"]
PLAIN_POOLS = ["free"] + RO_K + ["rt1", "rt2", "ro+rt"]                  # stepped under U, B and F
LIM_OTHER = ["lim2:same", "lim2:cross", "lim2:ends", "lim+ro", "lim+rt"]  # stepped under the variant they were found under
HULL_POOLS = ["ot_hull", "ot_hull+lim"]                                   # engines of their own (the hull is a batch-uniform setting)
ALL_JS = [(j, side) for j in range(ND) for side in (0, 1)]


def lim_name(j, side):
    return "lim:%d:%d" % (j, side)


class _Shape:                          # what parity.group_quantities reads of an engine
    ndof, v_off = ND, W


F_TAG = " [F]"                         # group names of the F envs of an engine that U and F envs share


def tol_of(pool):
    return parity.TOL_HANDS if pool in ("free", "free" + F_TAG) else parity.TOL_HANDS_CONTACT


def brick_hull(P):
    """the demo's brick as a hull object: its 8 vertices"""
    from pybullet_robot_envs.model.objects import hull_physics
    h = [P.obj_h[k] for k in range(3)]
    v = np.array([[(h[0] if i & 1 else -h[0]), (h[1] if i & 2 else -h[1]), (h[2] if i & 4 else -h[2])] for i in range(8)], float)
    return hull_physics(v, P.obj_mass, P.obj_mu)


class Item:
    """one pool state: fp32 state record, action (absolute targets of the 37 controlled joints), signature, the variant a limit-type state
    was found under (None: any), finger command (None or the 20 targets of set_motors(fingers, ., 0.1, 10))"""

    def __init__(self, s, a, sig, variant=None, fingers=None):
        self.s, self.a, self.sig, self.variant, self.fingers = np.asarray(s, np.float32), np.asarray(a, np.float32), sig, variant, fingers


class Lab:
    """fp64 and fp32 oracle with the same settings (a variant, box or hull brick), the joint limits, the engine to match"""

    def __init__(self, variant, hull, Engine, lib):
        self.variant, self.hull, self.phys = variant, hull, dict(PHYS[variant])
        eng, self.ora, self.info = parity.make_hands_pair(Engine, lib, 1, "r", 0)      # the scene's numbers: the engine's defaults
        eng.close()
        self.ora32, self.tbl, _ = orc.hands_oracle("r", f32=True)
        ctypes.memmove(ctypes.byref(self.ora32.params), ctypes.byref(self.ora.params), ctypes.sizeof(orc.Params))
        ctypes.memmove(ctypes.byref(self.ora32.task), ctypes.byref(self.ora.task), ctypes.sizeof(orc.Task))
        self.hull_ph = brick_hull(self.ora.params) if hull else None
        for o in (self.ora, self.ora32):
            for k, v in self.phys.items():
                setattr(o.params, k, v)
            if hull:
                orc.set_object(o, self.hull_ph)
            assert o.ndof == ND and o.state_floats == 2 * W + 16
        m = self.ora.model
        self.lo = np.array([m.lower[m.link_of_dof[k]] for k in range(ND)])
        self.hi = np.array([m.upper[m.link_of_dof[k]] for k in range(ND)])
        self.home = np.asarray(self.info["home"], float)
        self.ctrl, self.fing = list(self.info["controlled"]), list(self.info["fingers"])
        self.vclamp = float(self.ora.params.max_coord_vel)

    def engine(self, Engine, lib, n):
        ph = dict(self.phys)
        if self.hull:
            ph.update(self.hull_ph)
        eng, _, _ = parity.make_hands_pair(Engine, lib, n, "r", 0, **({"phys": ph} if ph else {}))
        if self.hull:
            assert eng.get_physics().obj_shape == 3
        return eng

    # ---- motor records
    def forced_of(self, items, forced=None):
        """per env: every joint force-limited (F)?  Default: all envs of an F lab, none of any other"""
        return np.full(len(items), self.variant == "F") if forced is None else np.asarray(forced, bool)

    def mrec_of(self, items, ora=None, forced=None):
        """the oracle's motor record of every env: the reset's hold command, the env's finger command, and in F envs every joint force-limited"""
        ora = ora or self.ora
        n = len(items)
        forced = self.forced_of(items, forced)
        mrec = np.zeros((n, 4 * MD), ora.np_real)
        mrec[:, :ND], mrec[:, MD:2 * MD], mrec[:, 2 * MD:3 * MD] = self.home, ora.task.kp_hold, 1.0
        if forced.any():
            mrec = ora.hands_set_motors(mrec, list(range(ND)), self.home, ora.task.kp_hold, F_FORCE, mask=forced)
        for key in sorted(set(it.fingers for it in items if it.fingers is not None)):
            mrec = ora.hands_set_motors(mrec, self.fing, list(key), 0.1, F_FORCE, mask=[it.fingers == key for it in items])
        return mrec

    def reset_record(self):
        """[4, W]: the motor record a reset leaves (kw_mrec_init: hold command, force scale 1 on ALL lanes -- a lane with a smaller one, a dead
        lane included, counts as a force-limited motor and switches the clamp-free attempt off); check_reset_record holds it to a real reset"""
        m = np.zeros((4, W), np.float32)
        m[0, :ND], m[1, :ND], m[2, :] = self.home, self.ora.task.kp_hold, 1.0
        return m

    def command(self, eng, items, forced=None):
        """the same through the engine's interface: set_motors(mask=...) per command; the two records must then agree, lane by lane"""
        n = len(items)
        forced = self.forced_of(items, forced)
        eng.set_motor_state(np.repeat(self.reset_record()[None], n, 0))
        if forced.any():
            eng.set_motors(list(range(ND)), self.home, self.ora.task.kp_hold, F_FORCE, mask=forced)
        for key in sorted(set(it.fingers for it in items if it.fingers is not None)):
            eng.set_motors(self.fing, list(key), 0.1, F_FORCE, mask=[it.fingers == key for it in items])
        got, want = eng.get_motor_state()[:, :, :ND], self.mrec_of(items, forced=forced).reshape(n, 4, MD)[:, :, :ND].astype(np.float32)
        assert np.array_equal(got, want), "motor records of the engine and the oracle differ after the same commands"
        assert (got[forced, 2] < 1.0).all() and (got[~forced, 2][:, [j for j in range(ND) if j not in self.fing]] == 1.0).all()

    def step(self, items, f32=False, forced=None):
        """one oracle step of the items -> state records, output rows, sweeps used"""
        ora = self.ora32 if f32 else self.ora
        S = np.array([it.s for it in items])
        so, _, out = ora.hands_step(S.astype(ora.np_real), self.mrec_of(items, ora, forced), np.array([it.a for it in items]))
        return np.asarray(so, np.float64), np.asarray(out, np.float64), ora.last_sweeps.copy()

    def signature(self, s):
        """(joints at a limit, robot-object contacts, robot-table contacts, object-table contacts) of the fp32 state s"""
        s = np.asarray(s, np.float32).astype(np.float64)
        _, info = self.ora.sim_step(s, s[:ND].copy(), np.full(ND, 0.1), np.full(ND, 1.0))
        t = [info.type[k] for k in range(info.ncontacts)]
        # fingertip slots (1 .. 5) of the spheres on the object, as a bit mask: what the contact query reports as `tips` (slot s: bit s - 1)
        self.tips = 0
        for k in range(info.ncontacts):
            if info.type[k] == 1 and self.ora.model.s_tip[info.idx[k]] > 0:
                self.tips |= 1 << (int(self.ora.model.s_tip[info.idx[k]]) - 1)
        lim = frozenset(j for j in range(ND) if s[j] - self.lo[j] <= 0 or self.hi[j] - s[j] <= 0)        # the oracle's own test (limit rows)
        self.deepest = min([info.dist[k] for k in range(info.ncontacts)] + [0.0])
        return lim, t.count(1), t.count(2), t.count(0)

    def limit_effect(self, items):
        """[n, ND]: how far the oracle's joint velocities after one step move when its limit rows are taken away; and whether the fp64 and
        fp32 results (with the rows) stay clear of the step's velocity clamp"""
        so, _, _ = self.step(items)
        s32, _, _ = self.step(items, f32=True)
        keep = self.ora.params.limit_max_impulse
        self.ora.params.limit_max_impulse = 0.0
        try:
            s0, _, _ = self.step(items)
        finally:
            self.ora.params.limit_max_impulse = keep
        top = (1.0 - CLAMP_MARGIN) * self.vclamp
        clear = (np.abs(so[:, W:W + ND]).max(1) < top) & (np.abs(s32[:, W:W + ND]).max(1) < top)
        return np.abs(so[:, W:W + ND] - s0[:, W:W + ND]), clear


_BIND = {}


def bind(Engine, lib):
    """the engine class and library the scene's constants are read from (the first caller's; they are the same numbers in every library)"""
    _BIND.setdefault("e", (Engine, lib))


@functools.lru_cache(maxsize=None)
def lab_of(variant, hull=False):
    return Lab(variant, hull, *_BIND["e"])


@functools.lru_cache(maxsize=None)
def base_state():
    """the settled reset state of the default physics: every crafted state is a copy of it with other joints / another brick pose"""
    return lab_of("U").ora.hands_reset(1)[0][0]


def flagged(lab, items, names):
    """Envs of the batch that the oracle itself calls ill conditioned under lab's variant: a contact candidate within 3 um of the margin, or a
    result that moves by more than half the pool's bounds when the fp64 oracle's input is perturbed at the fp32 rounding level or its fp32
    build runs instead (the probe of icub_rows.flagged on this record: 272 floats, W = 128, LC = 60).  No engine is involved."""
    n = len(items)
    s32 = np.array([it.s for it in items])
    bad = np.zeros(n, bool)
    so, out, _ = lab.step(items)
    m0 = lab.ora.params.contact_margin       # (parity.ambiguous_envs' test, through hands_step: this oracle steps with a motor record)
    try:
        for m in (m0 + 3e-6, m0 - 3e-6):
            lab.ora.params.contact_margin = m
            bad |= np.abs(lab.step(items)[0] - so).max(1) > 1e-9
    finally:
        lab.ora.params.contact_margin = m0
    prng = np.random.default_rng(12345)
    trials = [lab.step(items, f32=True)[:2]]
    cols = np.r_[0:ND + 7, W:W + ND + 6]
    # (one rounding, 2^-24, in every pool: TOL_HANDS_CONTACT's obj_pos bound of 2e-7 m is 3 fp32 roundings of the brick's height, so
    # icub_rows' 2e-7 would move the INPUT by 0.65 of that bound, whatever the state)
    size = 2.0 ** -24
    top = (1.0 - CLAMP_MARGIN) * lab.vclamp
    bad |= ~(np.abs(so[:, W:W + ND]).max(1) < min(top, QD_MAX))
    for _ in range(4):
        sp = s32.astype(np.float64)
        sp[:, cols] *= 1.0 + size * prng.uniform(-1.0, 1.0, (n, len(cols)))
        ora = lab.ora
        st, _, o = ora.hands_step(sp, lab.mrec_of(items), np.array([it.a for it in items]))
        trials.append((st, o))
    for s_f, o_f in trials:
        s_f, o_f = np.asarray(s_f, np.float64), np.asarray(o_f, np.float64)
        for e in range(n):
            tt = tol_of(names[e])
            q = parity.group_quantities(_Shape, s_f[e:e + 1], so[e:e + 1], o_f[e:e + 1, :-2], out[e:e + 1], tail=7)
            bad[e] |= any(v > 0.5 * tt[k] for k, v in q.items())
            bad[e] |= not np.array_equal(o_f[e, -4:-2], out[e, -4:-2])          # tips in contact, contact points
            bad[e] |= not np.abs(s_f[e, W:W + ND]).max() < top                  # a joint at the step's velocity clamp
    return bad


def _quat_of(R):
    """unit quaternion (x, y, z, w) of a rotation matrix"""
    w = 0.5 * np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2]))
    if w > 1e-3:
        return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    k = int(np.argmax(np.diag(R)))
    i, j = (k + 1) % 3, (k + 2) % 3
    v = np.zeros(4)
    v[k] = 0.5 * np.sqrt(max(0.0, 1.0 + R[k, k] - R[i, i] - R[j, j]))
    v[i], v[j], v[3] = (R[i, k] + R[k, i]) / (4 * v[k]), (R[j, k] + R[k, j]) / (4 * v[k]), (R[j, i] - R[i, j]) / (4 * v[k])
    return v


def _rot(axis, ang):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


FIVE_POSE = tuple([0.0] * 16 + [1.1775, 1.37375, 0.785, 0.0])      # parity.check_hands_five_fingertips: the thumb in the plane of the four tips


class Pools:
    """pool name -> states with that row signature (and, for the limit-type pools, with limit rows the oracle's result depends on)"""

    def __init__(self, seed=SEED):
        from pybullet_robot_envs.model.table import icub_hands_model, icub_hands_spheres, hand_joint_names
        self.rng = np.random.default_rng(seed)
        self.lab = lab_of("U")
        self.base = np.array(base_state(), float)
        m = icub_hands_model()
        links = [l["name"] for l in m["links"]]
        by_joint = {l.get("joint_name"): i for i, l in enumerate(m["links"])}
        self.sph = [(links.index(ln), np.array(c), r) for ln, c, r, _ in icub_hands_spheres(m, "r")]
        self.hand_r = [k for k, (ln, _, _, _) in enumerate(icub_hands_spheres(m, "r")) if ln.startswith("r_hand")]
        self.tips = [by_joint[hand_joint_names("r")[k]] for k in (3, 7, 11, 15, 19)]
        self.pool, self.used, self.drawn = {}, {}, {}
        P = self.lab.ora.params
        self.ztop, self.tc, self.th = P.table_c[2] + P.table_h[2], np.array(list(P.table_c)), np.array(list(P.table_h))
        self.oh = np.array([P.obj_h[k] for k in range(3)])
        self.arm_r = [j for j in self.lab.ctrl if 30 <= j < 40] + [0, 1, 2]       # right arm and torso
        self.passive = [j for j in range(ND) if j not in self.lab.ctrl]

    # ---- pieces
    def _inside(self, q):
        lab = self.lab
        return np.clip(q, lab.lo + 0.05 * (lab.hi - lab.lo), lab.hi - 0.05 * (lab.hi - lab.lo))

    def _state(self, q, qd, base=None):
        s = (self.base if base is None else base).copy()
        s[:ND], s[W:W + ND] = q, qd
        return s

    def _joints(self, spread=SPREAD, vel=0.3):
        """all 60 joints spread about home, inside their ranges (none AT a limit: the resting fingers sit on theirs), random velocities.
        The 23 joints the step does not command (head, left hand) are pulled home by their hold motors at kp / dt = 48 rad/s per rad: they
        get a third of the spread, so that the step stays an ordinary one (QD_MAX)"""
        sig = np.full(ND, spread)
        sig[self.passive] = spread / 3.0
        q = self._inside(self.lab.home + self.rng.normal(0, 1.0, ND) * sig)
        return q, self.rng.normal(0, vel, ND)

    def _past(self, q, qd, j, side):
        """joint j PAST its limit, moving into it"""
        pen, v = self.rng.uniform(*PEN), self.rng.uniform(*INTO)
        q[j], qd[j] = (self.lab.lo[j] - pen, -v) if side == 0 else (self.lab.hi[j] + pen, v)

    def _action(self, q):
        """absolute targets of the controlled joints near where they are (the command clips them to the joint ranges)"""
        return (np.asarray(q)[self.lab.ctrl] + self.rng.uniform(-0.02, 0.02, len(self.lab.ctrl))).astype(np.float32)      # (kp_act / dt = 120 rad/s per rad)

    def _centres(self, q):
        R, p = self.lab.ora.fk(q)
        return [(p[i] + R[i] @ c, r) for i, c, r in self.sph]

    def _table_gap(self, q):
        """lowest point of the robot's spheres over the table top, relative to it"""
        ds = [c[2] - r - self.ztop for c, r in self._centres(q) if abs(c[0] - self.tc[0]) < self.th[0] and abs(c[1] - self.tc[1]) < self.th[1]]
        return min(ds) if ds else 1.0

    def _hand_on_table(self, lim=None):
        """joints between home and a random right-arm pose, at the point where the lowest sphere is 0.5 - 3 mm inside the table (bisection
        along the line; lim = (j, side): joint j past its limit all along)"""
        rng, lab = self.rng, self.lab
        for _ in range(400):
            q0, qd = self._joints()
            q1 = q0.copy()
            q1[self.arm_r] = self._inside(lab.home + rng.normal(0, 0.7, ND))[self.arm_r]
            if lim is not None:
                self._past(q0, qd, *lim)
                q1[lim[0]] = q0[lim[0]]
            target = -rng.uniform(0.0005, 0.003)
            if self._table_gap(q0) <= target or self._table_gap(q1) >= target:
                continue
            a, b = 0.0, 1.0
            for _ in range(30):
                t = 0.5 * (a + b)
                if self._table_gap(q0 + t * (q1 - q0)) > target:
                    a = t
                else:
                    b = t
            return q0 + b * (q1 - q0), qd
        raise RuntimeError("no pose with a hand sphere on the table")

    def _brick_on_a_sphere(self, s, pen=0.002):
        """the brick, axis-aligned, one face `pen` deep in one sphere of the right hand from above / beside"""
        rng = self.rng
        c, r = self._centres(s[:ND])[self.hand_r[rng.integers(0, len(self.hand_r))]]
        d = rng.normal(size=3); d[2] = abs(d[2])
        dd = np.zeros(3); k = int(np.argmax(np.abs(d))); dd[k] = np.sign(d[k])
        s[LC:LC + 3] = c + dd * (r + self.oh[k] - pen)
        s[LC + 3:LC + 7] = [0, 0, 0, 1]
        s[W + LC:W + LC + 6] = rng.normal(0, 0.05, 6)

    def _tips_scene(self):
        """the five-fingertip scene with the brick shifted in its plane and tilted about an in-plane axis: one to five tips stay on it"""
        rng = self.rng
        q, qd = self._joints(spread=0.05, vel=0.1)
        q[self.lab.fing] = FIVE_POSE
        qd[self.lab.fing] = rng.normal(0, 0.05, 20)
        centre, _, Rb, (ex, ey, nrm) = parity.five_fingertip_brick(self.lab.ora, self.lab.info, q, self.tips, self.oh[2])
        s = self._state(q, qd)
        mode = rng.integers(0, 3)
        shift = ex * rng.uniform(-0.06, 0.06) + ey * rng.uniform(-0.05, 0.05) if mode else np.zeros(3)
        ax = ex * rng.normal() + ey * rng.normal()
        ang = rng.uniform(-0.12, 0.12) if mode == 2 else rng.uniform(-0.01, 0.01)
        T = _rot(ax, ang)
        face = centre - nrm * self.oh[2]                          # tilt about the face's centre, so that some tip stays inside
        s[LC:LC + 3] = face + shift + T @ (centre - face) + nrm * rng.uniform(-0.0008, 0.0003)
        s[LC + 3:LC + 7] = _quat_of(T @ Rb)
        s[W + LC:W + LC + 6] = rng.normal(0, 0.02, 6)
        a = np.asarray(q, np.float32)[self.lab.ctrl]
        return Item(s, a, None, fingers=FIVE_POSE)

    # ---- candidates of a pool (not yet checked against its signature)
    def _make(self, name):
        rng, lab = self.rng, self.lab
        parts = name.split(":")
        kind = parts[0]
        if kind == "free":
            out = []
            for _ in range(8):
                q, qd = self._joints()
                out.append(Item(self._state(q, qd), self._action(q), None))
            return out
        if kind == "lim":                       # lim:<j>:<side>
            out = []
            for _ in range(10):
                q, qd = self._joints()
                self._past(q, qd, int(parts[1]), int(parts[2]))
                out.append(Item(self._state(q, qd), self._action(q), None))
            return out
        if kind == "lim2":                      # two joints of one env: in one block of 10, in two, joints 0 and 59
            out = []
            for _ in range(16):
                q, qd = self._joints()
                j1 = int(rng.integers(0, ND))
                if parts[1] == "same":
                    j2 = BLOCK * (j1 // BLOCK) + (j1 % BLOCK + int(rng.integers(1, BLOCK))) % BLOCK
                elif parts[1] == "cross":
                    j2 = (j1 + BLOCK * int(rng.integers(1, ND // BLOCK))) % ND
                    j2 = BLOCK * (j2 // BLOCK) + int(rng.integers(0, BLOCK))
                else:
                    j1, j2 = 0, ND - 1
                self._past(q, qd, j1, int(rng.integers(0, 2)))
                self._past(q, qd, j2, int(rng.integers(0, 2)))
                out.append(Item(self._state(q, qd), self._action(q), None))
            return out
        if kind in RO_K:
            return [self._tips_scene() for _ in range(16)]
        if kind in ("rt1", "rt2"):
            out = []
            for _ in range(8):
                q, qd = self._hand_on_table()
                out.append(Item(self._state(q, 0.3 * qd), self._action(q), None))
            return out
        if kind == "ro+rt":                     # a hand sphere on the table, the brick on a sphere of that hand
            out = []
            for _ in range(8):
                q, qd = self._hand_on_table()
                s = self._state(q, 0.3 * qd)
                self._brick_on_a_sphere(s)
                out.append(Item(s, self._action(q), None))
            return out
        if kind == "lim+ro":                    # a finger joint of the right hand past its limit, the brick on a sphere of that hand
            out = []
            for _ in range(12):
                q, qd = self._joints()
                self._past(q, qd, int(rng.integers(40, 60)), int(rng.integers(0, 2)))
                s = self._state(q, qd)
                self._brick_on_a_sphere(s)
                out.append(Item(s, self._action(q), None))
            return out
        if kind == "lim+rt":                    # a joint of the right arm or hand past its limit, a hand sphere on the table
            out = []
            for _ in range(6):
                q, qd = self._hand_on_table(lim=(int(rng.integers(33, 60)), int(rng.integers(0, 2))))
                out.append(Item(self._state(q, qd), self._action(q), None))
            return out
        if kind == "ot_hull":                   # the hull brick at rest on the table (the reset state's): four object-table slots, no robot contact
            out = []
            for _ in range(8):
                q, qd = self._joints()
                s = self._state(q, qd)
                s[LC:LC + 2] += rng.uniform(-0.02, 0.02, 2)
                s[LC + 3:LC + 7] = _quat_of(_rot([0, 0, 1], rng.uniform(-1, 1)))
                s[W + LC:W + LC + 2] = rng.normal(0, 0.05, 2)
                out.append(Item(s, self._action(q), None))
            return out
        if kind == "ot_hull+lim":
            out = []
            for _ in range(10):
                q, qd = self._joints()
                self._past(q, qd, int(rng.integers(0, ND)), int(rng.integers(0, 2)))
                out.append(Item(self._state(q, qd), self._action(q), None))
            return out
        raise KeyError(name)

    def _fits(self, name, sig):
        lim, nro, nrt, not_ = sig
        parts = name.split(":")
        kind = parts[0]
        if kind == "free":
            return not lim and nro == 0 and nrt == 0
        if kind == "lim":
            return lim == {int(parts[1])} and nro == 0 and nrt == 0
        if kind == "lim2":
            if len(lim) != 2 or nro or nrt:
                return False
            a, b = sorted(lim)
            if parts[1] == "ends":
                return (a, b) == (0, ND - 1)
            return (a // BLOCK == b // BLOCK) == (parts[1] == "same")
        if kind in RO_K:                        # the brick in the air, on the fingertips (the straight fingers sit ON their lower limits, 0)
            return nro == int(kind[2]) and nrt == 0 and not_ == 0
        if kind in ("rt1", "rt2"):
            return not lim and nro == 0 and nrt == int(kind[2])
        if kind == "ro+rt":                     # (the brick in the air)
            return not lim and nro >= 1 and nrt >= 1 and not_ == 0
        if kind == "lim+ro":
            return len(lim) == 1 and 40 <= min(lim) < 60 and nro >= 1 and nrt == 0 and not_ == 0
        if kind == "lim+rt":
            return len(lim) == 1 and nro == 0 and nrt >= 1
        if kind == "ot_hull":
            return not lim and nro == 0 and nrt == 0 and not_ == 4
        if kind == "ot_hull+lim":
            return len(lim) == 1 and nro == 0 and nrt == 0 and not_ == 4
        raise KeyError(name)

    def _effective(self, name, cand):
        """limit-type pools: the first bounded variant under which the oracle's result depends on every limit row of the state"""
        hull = name.startswith("ot_hull")
        verdict = [None] * len(cand)
        for v in (BOUNDED[:1] if hull else BOUNDED):      # (the hull engines: one bound, so that every engine of check (a) has states)
            todo = [e for e in range(len(cand)) if verdict[e] is None]
            if not todo:
                break
            eff, clear = lab_of(v, hull).limit_effect([cand[e] for e in todo])
            for k, e in enumerate(todo):
                if clear[k] and all(eff[k, j] >= LIM_EFFECT for j in cand[e].sig[0]):
                    verdict[e] = v
        return verdict

    def take(self, name, tries_max=12):
        """the next unused item of pool `name` (None once a limit pool has given up: its joint-side is left out)"""
        lst = self.pool.setdefault(name, [])
        k = self.used.get(name, 0)
        tries = 0
        sig_lab = lab_of("U", name.startswith("ot_hull"))
        while k >= len(lst):
            tries += 1
            if tries > tries_max:
                assert name.startswith("lim:"), "no state with the signature of pool %r" % name
                return None
            cand = self._make(name)
            self.drawn[name] = self.drawn.get(name, 0) + len(cand)
            for it in cand:
                it.sig = sig_lab.signature(it.s)
                it.deepest, it.tips = sig_lab.deepest, sig_lab.tips
            cand = [it for it in cand if it.deepest > -MAX_DEPTH]
            if name in RO_K:                    # one generator, five pools: keep what fits the others
                for it in cand:
                    for other in RO_K:
                        if other != name and self._fits(other, it.sig):
                            self.pool.setdefault(other, []).append(it)
            cand = [it for it in cand if self._fits(name, it.sig)]
            if "lim" in name:
                for it, v in zip(cand, self._effective(name, cand)):
                    if v is not None:
                        it.variant = v
                        lst.append(it)
            else:
                lst += cand
        self.used[name] = k + 1
        return lst[k]


def variants_of(name, it):
    """the variants a pool's states are stepped (and probed) under"""
    if "lim" in name:
        return [it.variant]
    return ["U", "F"] if name.startswith("ot_hull") else ["U", "B", "F"]


class Rows:
    """the filled pools: by[name] = list of Items, all of them well conditioned under every variant they are stepped under"""

    def __init__(self):
        t0 = time.process_time()
        pools = Pools()
        want = [(lim_name(j, side), N_LIM) for j, side in ALL_JS] + [(nm, N_OTHER) for nm in PLAIN_POOLS + LIM_OTHER + HULL_POOLS]
        cur = []
        self.left_out = []
        for nm, k in want:
            got = [pools.take(nm) for _ in range(k)]
            if any(g is None for g in got):
                self.left_out.append(nm)
                continue
            cur += [(nm, g) for g in got]
        self.redrawn = 0
        for rnd in range(40):
            bad = np.zeros(len(cur), bool)
            groups = {}
            for e, (nm, it) in enumerate(cur):
                for v in variants_of(nm, it):
                    groups.setdefault((v, nm.startswith("ot_hull")), []).append(e)
            for (v, hull), idx in groups.items():
                bad[idx] |= flagged(lab_of(v, hull), [cur[e][1] for e in idx], [cur[e][0] for e in idx])
            if not bad.any():
                break
            for e in np.nonzero(bad)[0]:
                nm = cur[e][0]
                if nm in self.left_out:
                    continue
                g = pools.take(nm)
                self.redrawn += 1
                if g is None:
                    self.left_out.append(nm)
                else:
                    cur[e] = (nm, g)
            cur = [(nm, it) for nm, it in cur if nm not in self.left_out]
        else:
            raise AssertionError("still ill-conditioned states after 40 rounds of re-drawing")
        self.by, self.drawn = {}, dict(pools.drawn)
        for nm, it in cur:
            self.by.setdefault(nm, []).append(it)
        for nm, k in want:       # every pool is full: nothing is skipped downstream
            assert nm in self.left_out or len(self.by[nm]) == k, (nm, len(self.by.get(nm, [])))
        self.lim_pools = [lim_name(j, side) for j, side in ALL_JS if lim_name(j, side) not in self.left_out]
        self.seconds = time.process_time() - t0

    def items(self, names):
        return [(nm, it) for nm in names for it in self.by[nm]]


_ROWS = []


def rows(Engine, lib):
    """cached: the states and the oracle's verdicts are computed once per process"""
    bind(Engine, lib)
    if not _ROWS:
        _ROWS.append(Rows())
    return _ROWS[0]


def assert_pools(R):
    """the generator's own promises, re-checked from the finished pools"""
    assert all(nm.startswith("lim:") for nm in R.left_out) and len(R.left_out) <= MAX_LEFT_OUT, R.left_out
    have = {(j, side) for j, side in ALL_JS if lim_name(j, side) in R.by}
    for j in range(ND):
        assert (j, 0) in have or (j, 1) in have, "joint %d has no limit pool" % j
    for b in range(0, ND, BLOCK):       # the ends of every block of 10: where a wrong block bound shows
        for j in (b, b + BLOCK - 1):
            assert (j, 0) in have or (j, 1) in have
    for j, side in sorted(have):
        nm = lim_name(j, side)
        assert len(R.by[nm]) == N_LIM
        for it in R.by[nm]:
            lab = lab_of(it.variant)
            eff, clear = lab.limit_effect([it])
            assert eff[0, j] >= LIM_EFFECT and clear[0], (nm, eff[0, j])
            assert lab.signature(it.s)[:3] == (frozenset([j]), 0, 0)
            gap = (lab.lo[j] - it.s[j]) if side == 0 else (it.s[j] - lab.hi[j])
            assert PEN[0] - 1e-6 <= gap <= PEN[1] + 1e-6 and (it.s[W + j] < 0) == (side == 0)
    for nm in PLAIN_POOLS + LIM_OTHER + HULL_POOLS:
        assert len(R.by[nm]) == N_OTHER, nm
    for nm in LIM_OTHER + ["ot_hull+lim"]:
        for it in R.by[nm]:
            eff, clear = lab_of(it.variant, nm.startswith("ot_hull")).limit_effect([it])
            assert clear[0] and all(eff[0, j] >= LIM_EFFECT for j in it.sig[0]), nm
    for it in R.by["lim2:same"]:
        a, b = sorted(it.sig[0]); assert a // BLOCK == b // BLOCK
    for it in R.by["lim2:cross"]:
        a, b = sorted(it.sig[0]); assert a // BLOCK != b // BLOCK
    for it in R.by["lim2:ends"]:
        assert it.sig[0] == {0, ND - 1}
    for k, nm in enumerate(RO_K):
        assert set(it.sig[1:] for it in R.by[nm]) == {(k + 1, 0, 0)}
    assert set(it.sig[3] for it in R.by["ot_hull"] + R.by["ot_hull+lim"]) == {4}
    assert all(40 <= min(it.sig[0]) < 60 for it in R.by["lim+ro"])
    for v, hull, names in engines_of(R):
        for v1 in (("U", "F") if v == "UF" else (v,)):
            its = [(nm, it) for nm, it in R.items(names) if v1 in variants_of(nm, it)]
            assert not flagged(lab_of(v1, hull), [it for _, it in its], [nm for nm, _ in its]).any()


# ---------------------------------------------------------------------------------------------- (a) one step against the oracle, per pool
def engines_of(R):
    """(variant, hull, pools): the engines of check (a), as few as the variants allow.  UF: U and F share the default physics, so one engine
    holds every state twice, the second copy with all 60 joints force-limited through set_motors(mask=...) (its groups carry F_TAG)"""
    return [("UF", False, PLAIN_POOLS), ("B", False, PLAIN_POOLS + R.lim_pools + LIM_OTHER), ("B2", False, R.lim_pools + LIM_OTHER),
            ("UF", True, ["ot_hull"]), ("B", True, ["ot_hull+lim"])]
ENGINES = [("UF", False), ("B", False), ("B2", False), ("UF", True), ("B", True)]
MAX_ENVS = 336                         # "about 320": the B engine holds 332


def groups_of(names):
    """report groups: every pool; the limit pools together and joint by joint (so that a failure names the joint)"""
    g = {}
    for e, nm in enumerate(names):
        if nm.startswith("lim:"):
            j = int(nm.split(":")[1])
            g.setdefault("lim", []).append(e)
            g.setdefault("lim:joint %d" % j, []).append(e)
        else:
            g.setdefault(nm, []).append(e)
    return g


def force_bound(tail_o):
    """today's bound on the five reported fingertip forces (parity.check_hands_contacts)"""
    return 2e-2 * (1.0 + np.abs(tail_o[:, :5]).max())


def compare(names, se, ob, so, out, s_f, o_f, shape=_Shape, tol=tol_of, groups=groups_of, tail=7):
    """per group and quantity: the engine against the fp64 oracle, bound = TOL or, where the oracle's own fp32 build misses TOL on the same
    states, max(TOL, 4 x d32); the observation tail: counts equal, forces within 4 x d32 but never looser than force_bound.
    shape, tol, groups, tail: another lane-group engine's record, tables, report groups and observation tail (tests/arm_rows.py; tail 0:
    an engine that reports no fingertip forces).  -> report, failures"""
    rep, bad = {}, {}
    for g, idx in groups(names).items():
        tt = tol(g)
        d32 = parity.group_quantities(shape, s_f[idx], so[idx], o_f[idx, :-2], out[idx], tail=tail)
        w = parity.group_quantities(shape, se[idx], so[idx], ob[idx], out[idx], tail=tail)
        rep[g] = {}
        for k in tt:
            bound = float(tt[k] if d32[k] <= tt[k] else max(tt[k], 4.0 * d32[k]))
            rep[g][k] = {"engine": float("%.3g" % w[k]), "d32": float("%.3g" % d32[k]), "bound": float("%.3g" % bound)}
            if not w[k] <= bound:
                bad.setdefault(g, {})[k] = (float("%.3g" % w[k]), bound)
        if not tail:
            continue
        te, to, tf = ob[idx, -7:], out[idx, -9:-2], o_f[idx, -9:-2]
        if not np.array_equal(te[:, 5:], to[:, 5:]):
            bad.setdefault(g, {})["tips in contact, contact points"] = (te[:, 5:].tolist(), to[:, 5:].tolist())
        f_e, f_32 = float(np.abs(te[:, :5] - to[:, :5]).max()), float(np.abs(tf[:, :5] - to[:, :5]).max())
        fb = min(4.0 * f_32, force_bound(to))       # (no tip on the brick: the oracle's forces are 0 in both builds, and so must the engine's be)
        rep[g]["tip_force"] = {"engine": float("%.3g" % f_e), "d32": float("%.3g" % f_32), "bound": float("%.3g" % fb)}
        if not f_e <= fb:
            bad.setdefault(g, {})["tip_force"] = (f_e, fb)
    return rep, bad


def contact_sets_equal(eng, items):
    """The engine's own contact query, from the state as set, against the oracle's signature: the three classes of pairs in contact (flags),
    the fingertip slots on the brick (tips), and the numbers of spheres on the brick and on the table (count) -- the oracle keeps at most 6
    and 2 of those, so a full class is compared as `at least`.  Device libraries only: the host emulation has no contact query, there the
    observation tail's tips-in-contact and contact-point counts (compare()) are the whole of this check."""
    if not hasattr(eng.lib, "pbre_contact_query"):
        return
    from pybullet_robot_envs.model import contacts
    got = eng.contact_query(dist=False, nearest=False)
    want = np.array([(contacts.OBJECT_TABLE if it.sig[3] else 0) | (contacts.ROBOT_OBJECT if it.sig[1] else 0) | (contacts.ROBOT_TABLE if it.sig[2] else 0)
                     for it in items], np.int32)
    assert np.array_equal(got["flags"], want), "contact classes differ from the oracle's in envs %r" % np.nonzero(got["flags"] != want)[0].tolist()
    tips = np.array([it.tips for it in items], np.int32)
    assert np.array_equal(got["tips"], tips), "fingertip slots on the brick differ from the oracle's in envs %r" % np.nonzero(got["tips"] != tips)[0].tolist()
    for col, k, cap in ((0, 1, NC_RO), (1, 2, NC_RT)):
        want_n = np.array([it.sig[k] for it in items])
        ok = np.where(want_n < cap, got["count"][:, col] == want_n, got["count"][:, col] >= cap)
        assert ok.all(), "sphere counts (%s) differ from the oracle's in envs %r" % ("object" if col == 0 else "table", np.nonzero(~ok)[0].tolist())


def check_reset_record(Engine, lib):
    """the motor record the checks start every engine from is, lane by lane, what a real reset leaves (the checks skip the reset: 202 settle
    steps per env)"""
    bind(Engine, lib)
    lab = lab_of("U")
    eng = lab.engine(Engine, lib, 1)
    try:
        eng.reset()
        got = eng.get_motor_state()[0]
    finally:
        eng.close()
    want = lab.reset_record()
    assert np.array_equal(got[:, :ND], want[:, :ND]) and np.array_equal(got[2], want[2]), (got[:, ND - 2:ND + 6], want[:, ND - 2:ND + 6])
    assert np.array_equal(got[3], want[3])


FEW_SWEEPS = (1, 2)
FEW_ENGINES = [("B", False), ("B2", False), ("UF", True), ("B", True)]      # the limit-type pools and the hull brick


def check_rows_against_oracle(Engine, lib, variant, hull=False, kernel="", sweeps=None):
    """One engine of all pool states of the variant, one step with the states' fixed actions, per-quantity comparison with the fp64 oracle
    pool by pool: TOL_HANDS_CONTACT (TOL_HANDS for `free`), nothing skipped.  Returns the report {group: {quantity: ...}}.
    sweeps: the same at solver_iters = 1 or 2 instead of 150, for the limit-type pools and the hull brick.  After 150 sweeps a row that is
    left out of every second half-sweep has converged to the same impulse all the same (a scratch build that skips a block of limits_bwd,
    or the object-table rows of the odd sweeps, passes everything at 150).  One sweep is the backward half-sweep alone (motors 59 .. 0,
    limits_bwd, contact rows), two add the forward one (limits_fwd, motors 0 .. 59, contact rows): each loop body is seen on its own, and
    the oracle's result still depends on every limit row (asserted here for one state of every joint, as the pools assert it at 150)."""
    R = rows(Engine, lib)
    names_all = [p for v, h, p in engines_of(R) if (v, h) == (variant, hull)][0]
    if sweeps is not None:
        names_all = [nm for nm in names_all if "lim" in nm or nm.startswith("ot_hull")]
    pairs = [(nm, it) for nm, it in R.items(names_all) if ("U" if variant == "UF" else variant) in variants_of(nm, it)]
    names, items = [nm for nm, _ in pairs], [it for _, it in pairs]
    forced = None
    if variant == "UF":
        forced = [False] * len(items) + [True] * len(items)
        names, items = names + [nm + F_TAG for nm in names], items + items
    lab = lab_of("U" if variant == "UF" else variant, hull)
    n = len(items)
    assert 0 < n <= MAX_ENVS
    S, A = np.array([it.s for it in items]), np.array([it.a for it in items])
    iters = int(lab.ora.params.solver_iters)
    eng = lab.engine(Engine, lib, n)
    try:
        if sweeps is not None:
            parity.set_solver_iters(eng, sweeps, lab.ora, lab.ora32)
        lab.command(eng, items, forced)
        eng.set_state(S)
        contact_sets_equal(eng, items)
        ob, rw, dn = eng.step(A)
        se = np.asarray(eng.get_state(), np.float64)
        so, out, _ = lab.step(items, forced=forced)
        s_f, o_f, _ = lab.step(items, f32=True, forced=forced)
        if sweeps is not None:
            eff, _ = lab.limit_effect(items)
            seen = {}
            for e, it in enumerate(items):
                for j in it.sig[0]:
                    seen[j] = max(seen.get(j, 0.0), eff[e, j])
            weak = sorted(j for j, v in seen.items() if v < LIM_EFFECT)
            assert not weak, "after %d sweep(s) the oracle's result does not depend on the limit rows of joints %r" % (sweeps, weak)
    finally:
        eng.close()
        lab.ora.params.solver_iters = lab.ora32.params.solver_iters = iters
    ob = np.asarray(ob, np.float64)
    rep, bad = compare(names, se, ob, so, out, s_f, o_f)
    print("HANDS_ROWS " + json.dumps({"check": "a" if sweeps is None else "a, %d sweep(s)" % sweeps, "variant": variant, "hull": hull, "kernel": kernel, "envs": n, "groups": rep}))
    assert not bad, "variant %s%s, %s sweeps, %s: per-quantity bound exceeded (measured, bound) in %r" % (variant, " (hull)" if hull else "", sweeps or iters, kernel, bad)
    assert (np.asarray(dn) == out[:, -1]).all() and np.abs(np.asarray(rw) - out[:, -2]).max() < 1e-3 * max(1.0, np.abs(out[:, -2]).max())
    return rep


# ---------------------------------------------------------------------------------------------- (b) block-mates must not matter, bit for bit
def _bits(lab, eng, items):
    lab.command(eng, items)
    return step_bits(eng, np.array([it.s for it in items]), np.array([it.a for it in items]))


def finger_lim_pool(R):
    """the first limit pool of a finger joint of the right hand"""
    return [nm for nm in R.lim_pools if 40 <= int(nm.split(":")[1]) < 60][0]


def check_block_mates(Engine, lib, variant):
    """env = block * 4 + thread / 64: a probe (free, a finger joint at its limit, two fingertips on the brick) alone in an engine, at each of
    the four positions of a block whose three other envs are `ro5` states (every row slot of the LDS row store written), and as the last env
    of a ragged batch of five -- state record and output row bit for bit.  The wave's region of RowStore<72> is private to it."""
    R = rows(Engine, lib)
    lab = lab_of(variant)
    mates = R.by["ro5"][:3]
    e1, e4, e5 = (lab.engine(Engine, lib, n) for n in (1, 4, 5))
    try:
        for nm in ("free", finger_lim_pool(R), "ro2"):
            probe = R.by[nm][-1]
            ref = _bits(lab, e1, [probe])
            assert not np.array_equal(ref[0][0, :ND], probe.s[:ND].view(np.uint32)), "the probe did not move: nothing tested"
            for p in range(4):
                batch = mates[:p] + [probe] + mates[p:]
                st, row = _bits(lab, e4, batch)
                ctx = "probe %s at position %d of a block of ro5 states, variant %s" % (nm, p, variant)
                assert np.array_equal(st[p], ref[0][0]), "state record differs from the env alone: " + ctx
                assert np.array_equal(row[p], ref[1][0]), "output row differs from the env alone: " + ctx
            st, row = _bits(lab, e5, mates + [R.by["free"][0], probe])
            assert np.array_equal(st[4], ref[0][0]) and np.array_equal(row[4], ref[1][0]), "probe %s as the last env of a ragged batch, variant %s" % (nm, variant)
    finally:
        for e in (e1, e4, e5):
            e.close()


# ---------------------------------------------------------------------------------------------- (c) same value whichever loop
def _fast(it):
    """the state with every joint at 50 rad/s: under M its motors leave the bound, so the clamp-free attempt hands back to the clamping rows"""
    s = it.s.copy()
    s[W:W + ND] = 50.0
    return Item(s, it.a, it.sig, it.variant, it.fingers)


def loop_probes(R):
    """free states and one limit state per block of 10 joints"""
    names = ["free", "free"] + [[nm for nm in R.lim_pools if int(nm.split(":")[1]) // BLOCK == b][0] for b in range(ND // BLOCK)]
    return names, [R.by[nm][k] for k, nm in zip([0, 1] + [0] * (ND // BLOCK), names)]


def check_same_value_whichever_loop(Engine, lib):
    """Under M (max_motor_impulse = 30) the clamp-free attempt of a pool state runs through, as under U: the engine's results under M are the
    oracle's within the pool's bounds and, bit for bit, those of an engine created under U -- asserted first from the oracle: lifting the
    bound from 30 to the default changes nothing for these states.  The same states with every joint at 50 rad/s leave the bound (from the
    oracle: their results under M and U differ), so their attempt hands back -- dv, m_app, l_app and the contact impulses start from zero
    again -- and the result is held to the oracle under M and must differ from the engine's under U."""
    R = rows(Engine, lib)
    M, U = lab_of("M"), lab_of("U")
    names, probes = loop_probes(R)
    # fast: the first state of EVERY limit pool.  A stale l_app only shows where the clamping solve ends with that limit row at zero (a row
    # that pushes converges to the same total from any start), which a handful of them do: a scratch build without `R.l_app = zeroR` is
    # 0.035 .. 0.64 rad/s off in 6 of the 120 and bit-identical or within rounding in the others
    fast = [_fast(R.by[nm][0]) for nm in R.lim_pools]
    items, labels = probes + fast, names + ["fast"] * len(fast)
    n, k = len(items), len(probes)
    so_m, out_m, _ = M.step(items)
    so_u, _, _ = U.step(items)
    assert np.abs(so_m[:, W:W + ND]).max() < (1.0 - CLAMP_MARGIN) * M.vclamp, "a fast state ends at the step's velocity clamp"
    assert (so_m[:k] == so_u[:k]).all(), "a pool state's motors reach the bound of 30: M would not end on the clamp-free rows"
    assert (so_m[k:] != so_u[k:]).any(1).all(), "a fast state's motors stay under the bound of 30: no hand-back"
    eng_m, eng_u = M.engine(Engine, lib, n), U.engine(Engine, lib, n)
    try:
        st_m, row_m = _bits(M, eng_m, items)
        se, ob = np.asarray(eng_m.get_state(), np.float64), row_m.view(np.float32)[:, :-2].astype(np.float64)
        st_u, row_u = _bits(U, eng_u, items)
    finally:
        eng_m.close(); eng_u.close()
    for e in range(k):
        assert np.array_equal(st_m[e], st_u[e]) and np.array_equal(row_m[e], row_u[e]), "probe %s: the engine's result under M differs from that under U" % names[e]
    for e in range(k, n):
        assert not np.array_equal(st_m[e], st_u[e]), "fast %s: the same result under M and U" % R.lim_pools[e - k]
    s_f, o_f, _ = M.step(items, f32=True)
    # (the fast states are a group like any other: TOL_HANDS_CONTACT or, where the oracle's own fp32 build misses it, 4 x d32 over the group)
    rep, bad = compare(names=labels, se=se, ob=ob, so=so_m, out=out_m, s_f=s_f, o_f=o_f)
    print("HANDS_ROWS " + json.dumps({"check": "c", "variant": "M", "envs": n, "groups": rep}))
    assert not bad, "variant M: per-quantity bound exceeded (measured, bound) in %r" % bad
    return rep


# ---------------------------------------------------------------------------------------------- (d) the residual exit
RT_THRESHOLD = 1e-7
RT_ENGINES = [("U", False, ["free", "ro2", "ro5"]), ("B", False, ["lim+ro"]), ("B2", False, ["lim+ro"]), ("U", True, ["ot_hull"])]


def check_residual_exit(Engine, lib):
    """solver_residual_threshold = 1e-7 (Core::step<RT>): sweep counts against the oracle's, flips counted (at most 10 %, at most 2 sweeps
    apart, held to TOL_RT_FLIP_GROUP -- the rule of parity.check_hands_residual_threshold); envs with equal counts are held to the bounds
    of check (a), the reported fingertip forces included: an env that leaves early reports the normal impulses of ITS exit sweep (rt_an)."""
    R = rows(Engine, lib)
    total = flips = ro_early = ro_n = 0
    report = {}
    for variant, hull, pools in RT_ENGINES:
        lab = lab_of(variant, hull)
        pairs = [(nm, it) for nm, it in R.items(pools) if variant in variants_of(nm, it)]
        if not pairs:
            continue
        names, items = [nm for nm, _ in pairs], [it for _, it in pairs]
        iters = int(lab.ora.params.solver_iters)
        eng = lab.engine(Engine, lib, len(items))
        try:
            eng.set_physics(solver_residual_threshold=RT_THRESHOLD)
            lab.ora.params.solver_residual_threshold = lab.ora32.params.solver_residual_threshold = RT_THRESHOLD
            st, row = _bits(lab, eng, items)
            sw = eng.get_sweeps().astype(int)
            se, ob = np.asarray(eng.get_state(), np.float64), row.view(np.float32)[:, :-2].astype(np.float64)
            so, out, used = lab.step(items)
            s_f, o_f, _ = lab.step(items, f32=True)
        finally:
            lab.ora.params.solver_residual_threshold = lab.ora32.params.solver_residual_threshold = 0.0
            eng.close()
        same = sw == used
        total += len(items); flips += int((~same).sum())
        ro = np.array([nm in ("ro2", "ro5", "lim+ro") for nm in names])
        ro_n += int(ro.sum()); ro_early += int((ro & (used < iters)).sum())
        assert np.abs(sw - used).max() <= 2, (variant, names, sw.tolist(), used.tolist())
        idx = np.nonzero(same)[0]
        rep, bad = compare([names[e] for e in idx], se[idx], ob[idx], so[idx], out[idx], s_f[idx], o_f[idx])
        report["%s%s" % (variant, " hull" if hull else "")] = {"groups": rep, "sweeps": used.tolist(), "flips": int((~same).sum())}
        assert not bad, "residual exit, variant %s: per-quantity bound exceeded (measured, bound) in %r" % (variant, bad)
        if (~same).any():
            f = np.nonzero(~same)[0]
            parity.assert_within(parity.group_quantities(_Shape, se[f], so[f], ob[f], out[f], tail=7), parity.TOL_RT_FLIP_GROUP, "(hands rows, sweep-count flips)")
    print("HANDS_ROWS " + json.dumps({"check": "d", "variant": "RT", "engines": report, "envs": total, "flips": flips, "ro_early": ro_early, "ro": ro_n}))
    assert 2 * ro_early >= ro_n, "only %d of %d envs with robot-object rows leave before the cap: the snapshot is not exercised" % (ro_early, ro_n)
    assert flips <= max(1, total // 10), "exit sweeps differ in %d of %d envs" % (flips, total)
    return report
