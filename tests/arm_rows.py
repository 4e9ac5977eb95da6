"""States that put every row kind of the robot-level Panda and iCub solves to work, joint by joint (tests only).

pandaEnv and iCubEnv used alone: WideImpl<ShapePA, DevLanes32> (9 DoF, 4 robot-object slots, two fingertip slots whose forces go into
the state record) and WideImpl<ShapeIA, DevLanes32> (pbre_icub_arm.hip, 20 DoF), joint control (use_ik = 0: no IK flips anywhere here).
Both keep a per-env motor record target | kp | force scale | max velocity and put two envs into one wave (pbre_wide_impl.hpp):

    env = block * EPB + thread / 32

so envs 2 k and 2 k + 1 share a wave, and Core::step decides PER WAVE whether the clamp-free motor attempt is made (no contact row but the
object-table ones, no force-limited motor anywhere in the wave), whether it hands back (`over`), which contact loop runs and which limit
rows run.  Whoever remaps envs to waves in kw_step updates tests/arm_rows.py knowingly: the wave-mate check (b) relies on this rule.

Everything here comes from the oracle alone: single-env states by ROW SIGNATURE (joints at a limit by the oracle's own test; robot-object,
robot-table, object-table contact counts from orc.sim_step's StepInfo.type), pools of them, the assertion that every pool is full after the
oracle's own conditioning probe has dropped what it objects to -- so the engine-side checks skip nothing.  Two ways to step:

  C   command + step: set_state, set_motor_state, eng.step(a) against ora.hands_step (the fused command gives every commanded joint -- all 9
      of the Panda, the 10 controlled ones of the iCub -- full force and no velocity bound before the step reads the record)
  S   step from a motor record: set_state, set_motor_state, eng.settle(1) (kw_step's K_SETTLE_TGT instantiation) against
      ora.hands_settle(st, mrec, 1); the record is used as given, so force scale and max velocity reach the solve.  The record is the one
      the same command would have written (ora.hands_apply_action), then the env's own finger / force / velocity commands

and the physics variants

  U   the defaults (PyBullet's default force is an impulse bound of 417): the clamp-free attempt runs through          C and S
  B   max_motor_impulse = 0.004: the attempt is made, goes over the bound and hands back to the clamping rows             C
  B2  max_motor_impulse = 1e-4: for a limit state that B leaves without effect                                            C
  F   the defaults, joints force-limited in the record (set_motors / hands_set_motors, force 10 on every joint; the Panda's contact pools:
      the reference's grasp, force 10 and maxVelocity 1 on the two fingers): fscale < 1, the attempt is skipped             S (and C)
  V   the defaults, maxVelocity in the record: the clamp of the motor row's target velocity                                S (and C)
      (F and V with C: the fused command must hand every commanded joint its full force and unbounded velocity back)
  M   max_motor_impulse = 30, for check (c): a bound the pool states stay under and a state at 50 rad/s exceeds            C

A limit row of these models is invisible under U: the position motor of the same joint undoes its impulse within the sweep.  With bounded
motors the row decides where the joint goes, but only where the motor alone does not stop the joint; so a `lim` state is accepted only if
the ORACLE's step with and without limit rows (limit_max_impulse at its default and at 0) differs by >= LIM_EFFECT in that joint's velocity
(rad/s; m/s for the Panda's prismatic fingers), first under B, then under B2.  A `vel` state likewise only if the oracle's result for its
joint moves by >= LIM_EFFECT when the velocity bound is taken out of the record.  No pool state's step ends faster than QD_MAX in any joint
or has a contact deeper than MAX_DEPTH.

One more rule, found on the MI355X with the first version of the `ot` pool (cubes sliding at 5 cm/s): no pool state ends the oracle's step
with an object-table contact that is unloaded (normal impulse 0) and still carries friction impulse.  Bullet solves a contact's friction
rows only while its normal impulse is positive (btMultiBodyConstraintSolver: `if (totalImpulse > 0)`), and so do the oracle and the engine
(pbre_objstep.hpp: `dd = hi > 0 ? dd : 0`); a vertex that a braking, tipping box lifts off the table keeps the friction impulse it had in
the sweep it unloaded in.  How much that is depends on the rounding of the sweeps before, not on the state: for one such state the object
step compiled with contraction (kw_obj on the device; the same header built with clang and FMA on the CPU gives the device's bits) ends
6.0e-4 m/s from the one compiled without (the emulation) and from the oracle, after 150 sweeps and after 1000, both of them fixed points
of the same iteration.  Such states test rounding, not rows; Lab.signature calls them `stale` and the generator drops them.
"""
import ctypes
import functools
import json
import time

import numpy as np

import orc
import parity

W = 32                                 # lanes per env: velocity offset of the 80-float state record Q[32] | V[32] | X[16], width of the motor record
MD = orc.MAXD                          # the oracle's motor record: target | kp | force scale | max velocity, MD each
SEED = 20250612
PHYS = {"U": {}, "B": {"max_motor_impulse": 0.004}, "B2": {"max_motor_impulse": 1e-4}, "F": {}, "V": {}, "M": {"max_motor_impulse": 30.0}}
BOUNDED = ("B", "B2")
F_FORCE = 10.0                         # N: the reference's grasp force (panda_env.py:218-225)
V_BOUND = 0.5                          # rad/s (m/s): maxVelocity of the `vel` pools
LIM_EFFECT = 0.05                      # rad/s (m/s for the prismatic fingers): the rule and value of icub_rows / hands_rows
PEN, INTO = (0.005, 0.02), (0.5, 4.0)  # rad past the limit (never ON it: fp32 rounding of the limit would flip the row), rad/s into it
PEN_LIN, INTO_LIN = (0.001, 0.004), (0.02, 0.2)      # the same for the Panda's fingers: mm past the limit, cm/s into it
SPREAD = 0.25                          # rad: the joints about home
CLAMP_MARGIN = 0.05                    # no |qd| of a result within 5 % of the step's velocity clamp
QD_MAX = 12.0                          # rad/s: no pool state's step ends faster than this in any joint
MAX_DEPTH = 0.004                      # m: no contact deeper than this
N_LIM, N_VEL, N_OTHER = 2, 2, 4


class _Shape:                          # what parity.group_quantities reads of an engine
    def __init__(self, nd):
        self.ndof, self.v_off = nd, W


class Robot:
    """what differs between the two engines: DoF, tolerances, oracle and engine factories, collision spheres, pool names"""

    def __init__(self, name):
        self.name, self.panda = name, name == "panda"
        self.nd = 9 if self.panda else 20
        self.lc = self.nd                                  # object pose: Q[nd .. nd + 6]
        self.tail = 7 if self.panda else 0                 # observation tail: 5 fingertip force slots (2 used), fingers in contact, contact points
        self.lin = (7, 8) if self.panda else ()            # prismatic joints
        self.nc_ro, self.nc_rt = (4, 2) if self.panda else (2, 2)
        self.shape = _Shape(self.nd)
        self.kernel = "kw_step<ShapePA>" if self.panda else "kw_step<ShapeIA>"
        self.tol_free = parity.TOL_PANDA_ARM if self.panda else parity.TOL_ICUB_ARM
        self.tol_contact = parity.TOL_PANDA_ARM_CONTACT if self.panda else parity.TOL_ICUB_CONTACT
        ro = ["ro1", "ro2", "ro3", "ro4"] if self.panda else ["ro1"]
        self.ro_pools = ro
        self.contact_pools = ro + (["rt1", "rt2", "ro+ot"] if self.panda else ["rt1"])
        self.plain_pools = ["free", "ot"] + self.contact_pools if self.panda else ["free"] + self.contact_pools
        self.lim_other = ["lim2:same-env"] + (["lim+ro"] if self.panda else [])
        self.lim_pools = ["lim:%d:%d" % (j, side) for j in range(self.nd) for side in (0, 1)]
        self.vel_pools = ["vel:%d:%d" % (j, sign) for j in range(self.nd) for sign in (0, 1)] + ["vel:slack"]

    def oracle(self, f32=False):
        """-> oracle, {"home", "controlled"}"""
        if self.panda:
            o, _ = orc.panda_arm_oracle(0, 1, f32=f32)
            return o, {"home": [o.task.home[k] for k in range(9)], "controlled": list(range(9))}
        o, _, info = orc.icub_arm_oracle("l", 0, 1, f32=f32)
        return o, info

    def pair(self, Engine, lib, n, reset=False):
        """parity.make_panda_arm_pair / make_icub_arm_pair -> engine, oracle, close().  Without `reset` the engine starts from what its
        constructor leaves (the drop-in iCubEnv resets the engine it builds: 202 settle steps per env, which the checks do without)"""
        if self.panda:
            eng, ora = parity.make_panda_arm_pair(Engine, lib, n, 0, 1)
            if reset:
                eng.reset()
            return eng, ora, eng.close
        from pybullet_robot_envs import _client
        robot, eng, ora, cid = parity.make_icub_arm_pair(Engine, lib, n, "l", 0, 1, reset=reset)
        return eng, ora, lambda: _client.disconnect(cid)

    def spheres(self):
        """[(link, centre in the link's frame, radius)] of the robot's collision spheres"""
        if self.panda:
            from pybullet_robot_envs.model.table import panda_model, PANDA_SPHERES
            m = panda_model((0.0, 0.0, 0.625))
            links = [l["name"] for l in m["links"]]
            return [(links.index(ln), np.array(c), r) for ln, c, r in PANDA_SPHERES]
        from pybullet_robot_envs.model.table import icub_model, icub_spheres
        m = icub_model()
        links = [l["name"] for l in m["links"]]
        return [(links.index(ln), np.array(c), r) for ln, c, r in icub_spheres(m)]


ROBOTS = {"panda": Robot("panda"), "icub": Robot("icub")}
GRASP = ([7, 8], [0.0, 0.0], 0.1, F_FORCE, 1.0)          # pandaEnv.grasp: apply_action_fingers([0, 0], force 10), maxVelocity 1


class Item:
    """one pool state: fp32 state record, action (absolute joint targets of the controlled joints), signature, the variant a limit-type
    state was found under (None: any), vel = (joint, target) of a `vel` state (`vel:slack`: (None, None)), grasp: a Panda state whose F
    variant is the reference's grasp command"""

    def __init__(self, s, a, sig=None, variant=None, vel=None, grasp=False):
        self.s, self.a, self.sig, self.variant, self.vel, self.grasp = np.asarray(s, np.float32), np.asarray(a, np.float32), sig, variant, vel, grasp
        self.deepest, self.tips, self.stale = 0.0, 0, False

    def fast(self, nd):
        """the state with every joint at 50 rad/s: under M its motors leave the bound"""
        it = Item(self.s.copy(), self.a, self.sig, self.variant, self.vel, self.grasp)
        it.s[W:W + nd] = 50.0
        return it


class Lab:
    """fp64 and fp32 oracle with the same settings (a variant), the joint limits, the engine to match"""

    def __init__(self, robot, variant, Engine, lib):
        self.rb, self.variant, self.phys = ROBOTS[robot], variant, dict(PHYS[variant])
        rb = self.rb
        eng, self.ora, close = rb.pair(Engine, lib, 1)                # the scene's numbers: the engine's defaults
        close()
        _, self.info = rb.oracle()
        self.ora32, _ = rb.oracle(f32=True)
        ctypes.memmove(ctypes.byref(self.ora32.params), ctypes.byref(self.ora.params), ctypes.sizeof(orc.Params))
        ctypes.memmove(ctypes.byref(self.ora32.task), ctypes.byref(self.ora.task), ctypes.sizeof(orc.Task))
        for o in (self.ora, self.ora32):
            for k, v in self.phys.items():
                setattr(o.params, k, v)
            assert o.ndof == rb.nd and o.state_floats == 2 * W + 16 and o.task.use_ik == 0
        m = self.ora.model
        nd = rb.nd
        self.lo = np.array([m.lower[m.link_of_dof[k]] for k in range(nd)])
        self.hi = np.array([m.upper[m.link_of_dof[k]] for k in range(nd)])
        self.home = np.asarray(self.info["home"], float)[:nd]
        self.ctrl = list(self.info["controlled"])
        self.others = [j for j in range(nd) if j not in self.ctrl]
        self.vclamp = float(self.ora.params.max_coord_vel)
        self.kp_act, self.kp_hold = float(self.ora.task.kp_act), float(self.ora.task.kp_hold)
        self.rec0 = np.zeros(4 * MD)                                  # the reset's hold command (orc_hands_reset writes the same)
        self.rec0[:nd], self.rec0[MD:MD + nd], self.rec0[2 * MD:2 * MD + nd] = self.home, self.kp_hold, 1.0

    def engine(self, Engine, lib, n):
        """-> engine (not reset), close()"""
        eng, _, close = self.rb.pair(Engine, lib, n)
        if self.phys:
            eng.set_physics(**self.phys)
        return eng, close

    # ---- motor records
    def cmds_of(self, item, role, rec):
        """the commands an env's role adds to its record `rec`: F every joint force-limited (a grasp state: the grasp), V the state's velocity bound"""
        nd = self.rb.nd
        if role == "F":
            if item.grasp:
                return [GRASP]
            out = [(self.ctrl, rec[self.ctrl], rec[MD + self.ctrl[0]], F_FORCE, 0.0)]
            if self.others:
                out.append((self.others, rec[self.others], rec[MD + self.others[0]], F_FORCE, 0.0))
            return out
        if role == "V" and item.vel is not None:
            j, tgt = item.vel
            if j is None:                                             # vel:slack: a bound on every controlled joint, none binding
                return [(self.ctrl, rec[self.ctrl], rec[MD + self.ctrl[0]], 0.0, V_BOUND)]
            return [([j], [tgt], rec[MD + j], 0.0, V_BOUND)]
        assert role in (None, "F", "V"), role
        return []

    def mrec_of(self, items, mode, roles=None, ora=None, unbound=False):
        """[n, 4 MD]: the oracle's motor record of every env before the step: the reset's hold command; S: the command the C step would
        give, written by ora.hands_apply_action; then the commands of the env's role (unbound: V without its velocity bound)"""
        ora = ora or self.ora
        n = len(items)
        roles = roles or [None] * n
        mr = np.repeat(self.rec0[None], n, 0).astype(ora.np_real)
        if mode == "S":
            _, mr = ora.hands_apply_action(np.array([it.s for it in items]).astype(ora.np_real), mr, np.array([it.a for it in items]))
        for e, (it, role) in enumerate(zip(items, roles)):
            for dofs, tgt, kp, force, mv in self.cmds_of(it, role, np.asarray(mr[e], np.float64)):
                mr[e:e + 1] = ora.hands_set_motors(mr[e:e + 1], dofs, np.asarray(tgt, ora.np_real), float(kp), force, max_vel=0.0 if unbound else mv)
        return mr

    def reset_record(self):
        """[4, W]: the motor record a reset leaves (kw_mrec_init: hold command, force scale 1 on ALL lanes -- a lane with a smaller one, a dead
        lane included, counts as a force-limited motor and switches the clamp-free attempt off); check_reset_record holds it to a real reset"""
        m = np.zeros((4, W), np.float32)
        nd = self.rb.nd
        m[0, :nd], m[1, :nd], m[2, :] = self.home, self.kp_hold, 1.0
        return m

    def record32(self, items, mode, roles=None):
        """[n, 4, W] float32: the same records as the engine takes them (set_motor_state)"""
        nd = self.rb.nd
        mr = self.mrec_of(items, mode, roles)
        m32 = np.repeat(self.reset_record()[None], len(items), 0)
        for c in range(4):
            m32[:, c, :nd] = mr[:, c * MD:c * MD + nd]
        return m32

    # ---- the oracle's step
    def step(self, items, mode, roles=None, f32=False, unbound=False):
        """one oracle step of the items (C: hands_step, S: hands_settle from the record) -> state records, output rows (S: observation | 0 | 0),
        sweeps used"""
        ora = self.ora32 if f32 else self.ora
        S = np.array([it.s for it in items]).astype(ora.np_real)
        mr = self.mrec_of(items, mode, roles, ora, unbound)
        if mode == "C":
            so, _, out = ora.hands_step(S, mr, np.array([it.a for it in items]))
            return np.asarray(so, np.float64), np.asarray(out, np.float64), ora.last_sweeps.copy()
        so, used = np.zeros_like(S), np.zeros(len(items), np.int32)
        sw2 = (ctypes.c_int * 2)()
        for e in range(len(items)):
            so[e] = ora.hands_settle(S[e:e + 1], mr[e:e + 1], 1)[0]
            ora.lib.orc_last_sweeps(sw2)
            used[e] = sw2[0]
        out = np.array([np.r_[ora.observation(s), 0.0, 0.0] for s in so])
        return np.asarray(so, np.float64), np.asarray(out, np.float64), used

    def signature(self, s):
        """(joints at a limit, robot-object contacts, robot-table contacts, object-table contacts) of the fp32 state s; sets .tips (fingertip
        slots on the object as a bit mask, slot s: bit s - 1) and .deepest (the deepest contact's distance)"""
        nd = self.rb.nd
        s = np.asarray(s, np.float32).astype(np.float64)
        _, info = self.ora.sim_step(s, s[:nd].copy(), np.full(nd, 0.1), np.full(nd, 1.0))
        t = [info.type[k] for k in range(info.ncontacts)]
        self.tips = 0
        for k in range(info.ncontacts):
            if info.type[k] == 1 and self.ora.model.s_tip[info.idx[k]] > 0:
                self.tips |= 1 << (int(self.ora.model.s_tip[info.idx[k]]) - 1)
        lim = frozenset(j for j in range(nd) if s[j] - self.lo[j] <= 0 or self.hi[j] - s[j] <= 0)        # the oracle's own test (limit rows)
        self.deepest = min([info.dist[k] for k in range(info.ncontacts)] + [0.0])
        # an object-table contact that ends the step unloaded but still carries friction impulse: Bullet (and with it oracle and engine)
        # skips the friction rows of a contact whose normal impulse is 0, so the friction such a contact keeps is whatever it had in the
        # sweep it unloaded in -- the result depends on the path there, not on the state alone (module docstring)
        self.stale = any(info.type[k] == 0 and info.lambda_n[k] == 0 and (info.lambda_f1[k] != 0 or info.lambda_f2[k] != 0) for k in range(info.ncontacts))
        return lim, t.count(1), t.count(2), t.count(0)

    def limit_effect(self, items):
        """[n, nd]: how far the oracle's joint velocities after one C step move when its limit rows are taken away; and whether the fp64 and
        fp32 results (with the rows) stay clear of the step's velocity clamp"""
        nd = self.rb.nd
        so, _, _ = self.step(items, "C")
        s32, _, _ = self.step(items, "C", f32=True)
        keep = self.ora.params.limit_max_impulse
        self.ora.params.limit_max_impulse = 0.0
        try:
            s0, _, _ = self.step(items, "C")
        finally:
            self.ora.params.limit_max_impulse = keep
        top = (1.0 - CLAMP_MARGIN) * self.vclamp
        clear = (np.abs(so[:, W:W + nd]).max(1) < top) & (np.abs(s32[:, W:W + nd]).max(1) < top)
        return np.abs(so[:, W:W + nd] - s0[:, W:W + nd]), clear

    def bound_effect(self, items):
        """[n, nd]: how far the oracle's joint velocities after one S step under V move when the velocity bounds are taken out of the records"""
        nd = self.rb.nd
        roles = ["V"] * len(items)
        so, _, _ = self.step(items, "S", roles)
        s0, _, _ = self.step(items, "S", roles, unbound=True)
        return np.abs(so[:, W:W + nd] - s0[:, W:W + nd])


_BIND = {}


def bind(Engine, lib):
    """the engine class and library the scene's constants are read from (the first caller's; they are the same numbers in every library)"""
    _BIND.setdefault("e", (Engine, lib))


@functools.lru_cache(maxsize=None)
def lab_of(robot, variant):
    return Lab(robot, variant, *_BIND["e"])


def tol_of(rb, pool):
    """the table of a pool: the contact table where the robot touches something"""
    return rb.tol_contact if any(k in pool for k in ("ro", "rt")) or pool == "fast" else rb.tol_free


def role_of(variant):
    return variant if variant in ("F", "V") else None


def flagged(lab, items, names, mode, role=None):
    """Envs of the batch that the oracle itself calls ill conditioned under lab's variant and this way of stepping: a contact candidate
    within 3 um of the margin, a result that moves by more than half the pool's bounds when the fp64 oracle's input is perturbed by one fp32
    rounding or its fp32 build runs instead, a result at the velocity clamp or beyond QD_MAX (the probe of hands_rows.flagged on this
    record).  No engine is involved."""
    rb = lab.rb
    nd, lc, tail = rb.nd, rb.lc, rb.tail
    n = len(items)
    roles = [role] * n
    bad = np.zeros(n, bool)
    so, out, _ = lab.step(items, mode, roles)
    m0 = lab.ora.params.contact_margin
    try:
        for m in (m0 + 3e-6, m0 - 3e-6):
            lab.ora.params.contact_margin = m
            bad |= np.abs(lab.step(items, mode, roles)[0] - so).max(1) > 1e-9
    finally:
        lab.ora.params.contact_margin = m0
    prng = np.random.default_rng(12345)
    trials = [lab.step(items, mode, roles, f32=True)[:2]]
    cols = np.r_[0:nd + 7, W:W + nd + 6]
    top = (1.0 - CLAMP_MARGIN) * lab.vclamp
    bad |= ~(np.abs(so[:, W:W + nd]).max(1) < min(top, QD_MAX))
    for _ in range(4):
        pert = []
        for it in items:
            sp = it.s.astype(np.float64)
            sp[cols] *= 1.0 + 2.0 ** -24 * prng.uniform(-1.0, 1.0, len(cols))
            p = Item(it.s, it.a, it.sig, it.variant, it.vel, it.grasp)
            p.s = sp                                                   # (kept in fp64: the perturbation is below fp32's resolution)
            pert.append(p)
        trials.append(lab.step(pert, mode, roles)[:2])
    for s_f, o_f in trials:
        for e in range(n):
            tt = tol_of(rb, names[e])
            q = parity.group_quantities(rb.shape, s_f[e:e + 1], so[e:e + 1], o_f[e:e + 1, :-2], out[e:e + 1], tail=tail)
            bad[e] |= any(v > 0.5 * tt[k] for k, v in q.items() if k in tt)
            if tail:
                bad[e] |= not np.array_equal(o_f[e, -4:-2], out[e, -4:-2])          # fingers in contact, contact points
            bad[e] |= not np.abs(s_f[e, W:W + nd]).max() < top
    return bad


def _rot(axis, ang):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


class Pools:
    """pool name -> states with that row signature (and, for the limit-type and `vel` pools, with a row the oracle's result depends on)"""

    def __init__(self, robot, seed=SEED):
        from hands_rows import _quat_of
        self.quat_of = _quat_of
        self.rb = ROBOTS[robot]
        self.rng = np.random.default_rng(seed + self.rb.nd)
        self.lab = lab_of(robot, "U")
        self.base = np.array(self.lab.ora.hands_reset(1)[0][0], float)   # the settled reset state: every crafted state is a copy with other joints / another object pose
        self.sph = self.rb.spheres()
        self.pool, self.used, self.drawn = {}, {}, {}
        P = self.lab.ora.params
        self.ztop, self.tc, self.th = P.table_c[2] + P.table_h[2], np.array(list(P.table_c)), np.array(list(P.table_h))
        self.oh = np.array([P.obj_h[k] for k in range(3)])
        self.arm = list(range(7)) if self.rb.panda else list(self.lab.ctrl)
        if self.rb.panda:
            self.ik_ora, _ = orc.panda_arm_oracle(1, 1)                # (the oracle's own IK, to put the hand over the table: a tool of the generator only)

    # ---- pieces
    def _inside(self, q):
        lab = self.lab
        return np.clip(q, lab.lo + 0.05 * (lab.hi - lab.lo), lab.hi - 0.05 * (lab.hi - lab.lo))

    def _state(self, q, qd):
        nd = self.rb.nd
        s = self.base.copy()
        s[:nd], s[W:W + nd] = q, qd
        return s

    def _joints(self, spread=SPREAD, vel=0.3):
        """all joints spread about home, inside their ranges (none AT a limit), random velocities.  The joints the step does not command (the
        iCub's head and right arm) are pulled home by their hold motors: they get a third of the spread.  Fingers: mm and cm/s"""
        lab, nd = self.lab, self.rb.nd
        sig, vs = np.full(nd, spread), np.full(nd, vel)
        sig[lab.others] = spread / 3.0
        for j in self.rb.lin:
            sig[j], vs[j] = 0.008, 0.02
        q = self._inside(lab.home + self.rng.normal(0, 1.0, nd) * sig)
        return q, self.rng.normal(0, 1.0, nd) * vs

    def _past(self, q, qd, j, side):
        """joint j PAST its limit, moving into it"""
        lin = j in self.rb.lin
        pen, v = self.rng.uniform(*(PEN_LIN if lin else PEN)), self.rng.uniform(*(INTO_LIN if lin else INTO))
        q[j], qd[j] = (self.lab.lo[j] - pen, -v) if side == 0 else (self.lab.hi[j] + pen, v)

    def _action(self, q, past=None):
        """absolute targets of the controlled joints near where they are (kp_act / dt = 120 rad/s per rad; the command clips them to the joint
        ranges); past = (j, side): joint j's target beyond that limit, so that the motor of a state past the limit keeps pushing into it"""
        lab = self.lab
        d = self.rng.uniform(-0.02, 0.02, len(lab.ctrl))
        for k, j in enumerate(lab.ctrl):
            if j in self.rb.lin:
                d[k] *= 0.05
        a = np.asarray(q)[lab.ctrl] + d
        if past is not None and past[0] in lab.ctrl:
            j, side = past
            a[lab.ctrl.index(j)] = (lab.lo[j] - 0.5) if side == 0 else (lab.hi[j] + 0.5)
        return a.astype(np.float32)

    def _centres(self, q):
        R, p = self.lab.ora.fk(q)
        return [(p[i] + R[i] @ c, r) for i, c, r in self.sph]

    def _table_gap(self, q):
        """lowest point of the robot's spheres over the table top, relative to it"""
        ds = [c[2] - r - self.ztop for c, r in self._centres(q) if abs(c[0] - self.tc[0]) < self.th[0] and abs(c[1] - self.tc[1]) < self.th[1]]
        return min(ds) if ds else 1.0

    def _pose_over_table(self):
        """arm joints of a pose whose lowest sphere would be well inside the table: the end of a line of poses"""
        rng, lab = self.rng, self.lab
        if self.rb.panda:      # the hand pointing down at a spot of the table away from the cube, tilted so that one finger is lower or both are level
            pos = [rng.uniform(0.3, 0.6), rng.choice([-1, 1]) * rng.uniform(0.12, 0.3), 0.64]
            eul = [np.pi + rng.choice([0.0, 1.0]) * rng.uniform(-0.2, 0.2), rng.uniform(-0.05, 0.05), rng.uniform(-1.0, 1.0)]
            q, _ = self.ik_ora.ik(self.base[:9], pos, eul)
            return np.asarray(q, float)
        return self._inside(lab.home + rng.normal(0, 0.7, self.rb.nd))

    def _on_table(self, lim=None):
        """joints between a pose about home and one reaching into the table, at the point where the lowest sphere is 0.5 - 3 mm inside the
        table (bisection along the line; lim = (j, side): joint j past its limit all along)"""
        rng = self.rng
        for _ in range(400):
            q0, qd = self._joints()
            q1 = q0.copy()
            q1[self.arm] = self._pose_over_table()[self.arm]
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
        raise RuntimeError("no pose with a sphere on the table")

    def _cube_on_a_sphere(self, s, which, axes=None, pen=None):
        """the cube, aligned with `axes` (default: the world's), one face `pen` deep in one of the spheres `which`"""
        rng, lc = self.rng, self.rb.lc
        pen = rng.uniform(0.0005, 0.003) if pen is None else pen
        A = np.eye(3) if axes is None else axes
        c, r = self._centres(s[:self.rb.nd])[which[rng.integers(0, len(which))]]
        k, sg = int(rng.integers(0, 3)), rng.choice([-1.0, 1.0])
        s[lc:lc + 3] = c + sg * A[:, k] * (r + self.oh[k] - pen)
        s[lc + 3:lc + 7] = self.quat_of(A)
        s[W + lc:W + lc + 6] = rng.normal(0, 0.05, 6)

    def _grasp_scene(self, z, resting=False):
        """Panda: the hand pointing down at height z over the cube's place, the fingers closed on the cube to 0.5 - 2 mm; the cube shifted
        along and across the fingers and tilted, so that one to four of the finger spheres stay on it (in the air; resting: on the table,
        upright)"""
        rng, lc = self.rng, self.rb.lc
        q, qd = self._joints(spread=0.0, vel=0.1)
        qa, _ = self.ik_ora.ik(self.base[:9], [0.5 + rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), z], [np.pi, 0.0, rng.uniform(-0.3, 0.3)])
        q[:7] = np.asarray(qa, float)[:7]
        q[7:9] = self.oh[1] + 0.002 - rng.uniform(0.0005, 0.002, 2)      # (the finger spheres' inner surfaces are 2 mm inside the joint coordinate)
        R, p = self.lab.ora.fk(q)
        hand = self.sph[4][0]
        Rh = R[hand]
        cs = self._centres(q)[:4]
        mid = np.mean([c for c, _ in cs], 0)
        s = self._state(q, qd)
        if resting:
            yaw = np.arctan2(Rh[1, 0], Rh[0, 0])
            A = _rot([0, 0, 1], yaw)
            s[lc:lc + 3] = [mid[0], mid[1], self.base[lc + 2]]
            s[lc:lc + 2] += A[:2, 1] * rng.choice([0.0, 1.0]) * rng.uniform(-0.003, 0.003)
            s[W + lc:W + lc + 6] = 0.0
        else:
            mode = rng.integers(0, 4)
            sh = np.array([rng.uniform(-0.02, 0.02), 0.0, 0.0])
            if mode in (1, 3):
                sh[1] = rng.uniform(-0.003, 0.003)                       # across: frees one finger
            if mode in (2, 3):
                sh[2] = rng.uniform(-0.04, 0.04)                         # along the fingers: frees the tips or the second spheres
            A = Rh @ _rot([1, 0, 0], rng.uniform(-0.15, 0.15) if mode == 3 else rng.uniform(-0.01, 0.01))
            s[lc:lc + 3] = mid + Rh @ sh
            s[W + lc:W + lc + 6] = rng.normal(0, 0.02, 6)
        s[lc + 3:lc + 7] = self.quat_of(A)
        return Item(s, self._action(q), grasp=True)

    # ---- candidates of a pool (not yet checked against its signature)
    def _make(self, name):
        rng, lab, rb = self.rng, self.lab, self.rb
        nd, lc = rb.nd, rb.lc
        parts = name.split(":")
        kind = parts[0]
        if kind == "free":                      # the scene as the reset leaves it: the cube at rest where it was put
            out = []
            for _ in range(8):
                q, qd = self._joints()
                out.append(Item(self._state(q, qd), self._action(q)))
            return out
        if kind == "ot":                        # the cube at rest elsewhere, turned, sliding: four object-table slots, no robot contact
            out = []
            for _ in range(8):
                q, qd = self._joints()
                s = self._state(q, qd)
                s[lc:lc + 2] += rng.uniform(-0.05, 0.05, 2)
                s[lc + 3:lc + 7] = self.quat_of(_rot([0, 0, 1], rng.uniform(-1, 1)))
                s[W + lc:W + lc + 2] = rng.normal(0, 0.02, 2)       # (faster, and the slender box tips enough to unload its rear vertices: `stale`)
                out.append(Item(s, self._action(q)))
            return out
        if kind == "lim":                       # lim:<j>:<side>
            j, side = int(parts[1]), int(parts[2])
            out = []
            for k in range(12):
                q, qd = self._joints(spread=SPREAD if k % 3 else 2 * SPREAD)
                self._past(q, qd, j, side)
                out.append(Item(self._state(q, qd), self._action(q, past=(j, side) if k % 2 else None)))
            return out
        if kind == "lim2":                      # two joints of one env
            out = []
            for _ in range(16):
                q, qd = self._joints()
                j1 = int(rng.integers(0, nd))
                j2 = (j1 + int(rng.integers(1, nd))) % nd
                self._past(q, qd, j1, int(rng.integers(0, 2)))
                self._past(q, qd, j2, int(rng.integers(0, 2)))
                out.append(Item(self._state(q, qd), self._action(q)))
            return out
        if kind == "vel":
            out = []
            if parts[1] == "slack":             # a bound on every controlled joint, targets close by and joints slow: none binds
                for _ in range(8):
                    q, qd = self._joints(vel=0.03)
                    a = (q[lab.ctrl] + rng.uniform(-0.001, 0.001, len(lab.ctrl)) * np.array([0.05 if j in rb.lin else 1.0 for j in lab.ctrl])).astype(np.float32)
                    out.append(Item(self._state(q, qd), a, vel=(None, None)))
                return out
            j, sign = int(parts[1]), (-1.0, 1.0)[int(parts[2])]
            d = 0.01 if j in rb.lin else 0.1    # kp d / dt = 1.2 m/s, 12 rad/s at kp_act; 4.8 rad/s at the hold gain of an uncommanded joint
            for _ in range(8):
                q, qd = self._joints()
                m = 0.1 * (lab.hi[j] - lab.lo[j])
                q[j] = rng.uniform(lab.lo[j] + m + (d if sign < 0 else 0.0), lab.hi[j] - m - (d if sign > 0 else 0.0))
                out.append(Item(self._state(q, qd), self._action(q), vel=(j, float(np.float32(q[j] + sign * d)))))
            return out
        if kind in ("rt1", "rt2"):
            if not rb.panda:                    # parity.icub_contact_states' table search, as icub_rows
                S, _ = parity.icub_contact_states(lab.ora, lab.info, self.base, rng, control_arm="l", n_obj=0, n_table=8, n_both=0, n_limit=0)
                return [Item(s, self._action(s[:nd])) for s in S]
            out = []
            for _ in range(8):
                q, qd = self._on_table()
                out.append(Item(self._state(q, 0.3 * qd), self._action(q)))
            return out
        if kind in rb.ro_pools:
            if not rb.panda:                    # parity.icub_contact_states' cube on a sphere of the left arm, as icub_rows
                S, _ = parity.icub_contact_states(lab.ora, lab.info, self.base, rng, control_arm="l", n_obj=12, n_table=0, n_both=0, n_limit=0)
                return [Item(s, self._action(s[:nd])) for s in S]
            return [self._grasp_scene(0.75) for _ in range(16)]
        if kind == "ro+ot":
            return [self._grasp_scene(0.67, resting=True) for _ in range(8)]
        if kind == "lim+ro":                    # a finger joint past its limit, the cube (in the air, aligned with the hand) on a sphere of that finger
            out = []
            for _ in range(12):
                q, qd = self._joints(spread=0.0, vel=0.1)
                qa, _ = self.ik_ora.ik(self.base[:9], [0.5, 0.0, 0.78], [np.pi, 0.0, 0.0])
                q[:7] = np.asarray(qa, float)[:7]
                j, side = int(rng.integers(7, 9)), int(rng.integers(0, 2))
                self._past(q, qd, j, side)
                s = self._state(q, qd)
                R, _ = lab.ora.fk(q)
                self._cube_on_a_sphere(s, [0, 1] if j == 7 else [2, 3], axes=R[self.sph[4][0]])
                out.append(Item(s, self._action(q), grasp=False))
            return out
        raise KeyError(name)

    def _fits(self, name, sig):
        lim, nro, nrt, not_ = sig
        parts = name.split(":")
        kind = parts[0]
        if kind == "free":
            return not lim and nro == 0 and nrt == 0
        if kind == "ot":
            return not lim and nro == 0 and nrt == 0 and not_ == 4
        if kind == "lim":
            return lim == {int(parts[1])} and nro == 0 and nrt == 0
        if kind == "lim2":
            return len(lim) == 2 and nro == 0 and nrt == 0
        if kind == "vel":
            return not lim and nro == 0 and nrt == 0
        if kind in ("rt1", "rt2"):
            return not lim and nro == 0 and nrt == int(kind[2])
        if kind in self.rb.ro_pools:            # the cube in the air
            return not lim and nro == int(kind[2]) and nrt == 0 and not_ == 0
        if kind == "ro+ot":
            return not lim and nro >= 1 and nrt == 0 and not_ == 4
        if kind == "lim+ro":
            return len(lim) == 1 and min(lim) in (7, 8) and nro >= 1 and nrt == 0 and not_ == 0
        raise KeyError(name)

    def _effective(self, cand):
        """limit-type pools: the first bounded variant under which the oracle's result depends on every limit row of the state"""
        verdict = [None] * len(cand)
        for v in BOUNDED:
            todo = [e for e in range(len(cand)) if verdict[e] is None]
            if not todo:
                break
            eff, clear = lab_of(self.rb.name, v).limit_effect([cand[e] for e in todo])
            for k, e in enumerate(todo):
                if clear[k] and all(eff[k, j] >= LIM_EFFECT for j in cand[e].sig[0]):
                    verdict[e] = v
        return verdict

    def take(self, name, tries_max=40):
        """the next unused item of pool `name`"""
        lst = self.pool.setdefault(name, [])
        k = self.used.get(name, 0)
        tries = 0
        while k >= len(lst):
            tries += 1
            assert tries <= tries_max, "no state with the signature of pool %r" % name
            cand = self._make(name)
            self.drawn[name] = self.drawn.get(name, 0) + len(cand)
            for it in cand:
                it.sig = self.lab.signature(it.s)
                it.deepest, it.tips, it.stale = self.lab.deepest, self.lab.tips, self.lab.stale
            cand = [it for it in cand if it.deepest > -MAX_DEPTH and not it.stale]
            if name in self.rb.ro_pools and self.rb.panda:      # one generator, four pools: keep what fits the others
                for it in cand:
                    for other in self.rb.ro_pools:
                        if other != name and self._fits(other, it.sig):
                            self.pool.setdefault(other, []).append(it)
            cand = [it for it in cand if self._fits(name, it.sig)]
            if "lim" in name:
                for it, v in zip(cand, self._effective(cand)):
                    if v is not None:
                        it.variant = v
                        lst.append(it)
            elif name.startswith("vel:") and name != "vel:slack":
                eff = self.lab.bound_effect(cand) if cand else []
                lst += [it for e, it in enumerate(cand) if eff[e, it.vel[0]] >= LIM_EFFECT]
            elif name == "vel:slack":
                eff = self.lab.bound_effect(cand) if cand else []
                lst += [it for e, it in enumerate(cand) if eff[e].max() < 1e-7]
            else:
                lst += cand
        self.used[name] = k + 1
        return lst[k]


def cases_of(rb, name, it):
    """the (variant, way of stepping) pairs a pool's states are stepped (and probed) under"""
    if "lim" in name:
        return [(it.variant, "C")]
    if name.startswith("vel"):
        return [("V", "S"), ("V", "C")]
    return [("U", "C"), ("U", "S"), ("B", "C"), ("F", "S"), ("F", "C")]


# F / V with C: the record is force-limited / velocity-bounded when eng.step(a) is called, and the fused command must give every commanded
# joint its full force and unbounded velocity back before the step reads the record (the iCub's 10 uncommanded joints keep theirs)
CASES = [("U", "C"), ("U", "S"), ("B", "C"), ("B2", "C"), ("F", "S"), ("V", "S"), ("F", "C"), ("V", "C")]


class Rows:
    """the filled pools of a robot: by[name] = list of Items, all of them well conditioned under every case they are stepped under"""

    def __init__(self, robot):
        t0 = time.process_time()
        self.rb = rb = ROBOTS[robot]
        pools = Pools(robot)
        self.want = ([(nm, N_LIM) for nm in rb.lim_pools] + [(nm, N_VEL) for nm in rb.vel_pools]
                     + [(nm, N_OTHER) for nm in rb.plain_pools + rb.lim_other])
        cur = [(nm, pools.take(nm)) for nm, k in self.want for _ in range(k)]
        self.redrawn = 0
        for rnd in range(40):
            bad = np.zeros(len(cur), bool)
            groups = {}
            for e, (nm, it) in enumerate(cur):
                for case in cases_of(rb, nm, it):
                    groups.setdefault(case, []).append(e)
            for (v, mode), idx in groups.items():
                bad[idx] |= flagged(lab_of(robot, v), [cur[e][1] for e in idx], [cur[e][0] for e in idx], mode, role_of(v))
            if not bad.any():
                break
            for e in np.nonzero(bad)[0]:
                cur[e] = (cur[e][0], pools.take(cur[e][0]))
                self.redrawn += 1
        else:
            raise AssertionError("still ill-conditioned states after 40 rounds of re-drawing")
        self.by, self.drawn = {}, dict(pools.drawn)
        for nm, it in cur:
            self.by.setdefault(nm, []).append(it)
        for nm, k in self.want:       # every pool is full: nothing is skipped downstream
            assert len(self.by[nm]) == k, (nm, len(self.by.get(nm, [])))
        self.seconds = time.process_time() - t0

    def items(self, names):
        return [(nm, it) for nm in names for it in self.by[nm]]

    def case(self, variant, mode, only=None):
        """(pool name, item) of every state stepped under this case"""
        rb = self.rb
        return [(nm, it) for nm, it in self.items([nm for nm, _ in self.want]) if (variant, mode) in cases_of(rb, nm, it)
                and (only is None or any(nm.startswith(p) for p in only))]


@functools.lru_cache(maxsize=None)
def _rows(robot):
    return Rows(robot)


def rows(Engine, lib, robot):
    """cached: the states and the oracle's verdicts are computed once per process"""
    bind(Engine, lib)
    return _rows(robot)


def assert_pools(R):
    """the generator's own promises, re-checked from the finished pools"""
    rb = R.rb
    nd = rb.nd
    assert len(rb.lim_pools) == 2 * nd and len(rb.vel_pools) == 2 * nd + 1
    for nm in rb.lim_pools:
        j, side = int(nm.split(":")[1]), int(nm.split(":")[2])
        assert len(R.by[nm]) == N_LIM
        for it in R.by[nm]:
            lab = lab_of(rb.name, it.variant)
            eff, clear = lab.limit_effect([it])
            assert it.variant in BOUNDED and eff[0, j] >= LIM_EFFECT and clear[0], (nm, eff[0, j])
            assert lab.signature(it.s)[:3] == (frozenset([j]), 0, 0)
            pen = PEN_LIN if j in rb.lin else PEN
            gap = (lab.lo[j] - it.s[j]) if side == 0 else (it.s[j] - lab.hi[j])
            assert pen[0] - 1e-6 <= gap <= pen[1] + 1e-6 and (it.s[W + j] < 0) == (side == 0)
    V = lab_of(rb.name, "V")
    for nm in rb.vel_pools:
        assert len(R.by[nm]) == N_VEL
        eff = V.bound_effect(R.by[nm])
        for e, it in enumerate(R.by[nm]):
            assert V.signature(it.s)[:3] == (frozenset(), 0, 0)
            if nm == "vel:slack":
                assert it.vel == (None, None) and eff[e].max() < 1e-7
                continue
            j, sign = int(nm.split(":")[1]), (-1.0, 1.0)[int(nm.split(":")[2])]
            assert it.vel[0] == j and (it.vel[1] - it.s[j]) * sign > 0 and V.lo[j] < it.vel[1] < V.hi[j] and eff[e, j] >= LIM_EFFECT, (nm, eff[e, j])
            m32 = V.record32([it], "S", ["V"])[0]
            assert m32[3, j] == np.float32(V_BOUND) and (np.delete(m32[3], j) == 0).all() and (m32[2] == 1).all()
    for nm in rb.plain_pools + rb.lim_other:
        assert len(R.by[nm]) == N_OTHER, nm
    for nm, _ in R.want:
        for it in R.by[nm]:
            lab_of(rb.name, "U").signature(it.s)
            assert not lab_of(rb.name, "U").stale and lab_of(rb.name, "U").deepest > -MAX_DEPTH, nm
    if rb.panda:
        assert any(np.abs(it.s[W + rb.lc:W + rb.lc + 2]).max() > 0.01 for it in R.by["ot"]), "no sliding cube in `ot`"
    for nm in rb.lim_other:
        for it in R.by[nm]:
            eff, clear = lab_of(rb.name, it.variant).limit_effect([it])
            assert clear[0] and all(eff[0, j] >= LIM_EFFECT for j in it.sig[0]), nm
    assert all(len(it.sig[0]) == 2 for it in R.by["lim2:same-env"])
    for k, nm in enumerate(rb.ro_pools):       # ro3 / ro4: slots 2 / 3 of ShapePA are in use
        assert set(it.sig[1:] for it in R.by[nm]) == {(k + 1, 0, 0)}, nm
    assert all(it.sig[2] == int(nm[2]) for nm in rb.contact_pools if nm.startswith("rt") for it in R.by[nm])
    if rb.panda:
        assert all(it.sig[3] == 4 for nm in ("free", "ot", "ro+ot") for it in R.by[nm]) and all(it.sig[1] >= 1 for it in R.by["ro+ot"])
        assert all(min(it.sig[0]) in (7, 8) and it.sig[1] >= 1 for it in R.by["lim+ro"])
    for v, mode in CASES:
        its = R.case(v, mode)
        if its:
            assert not flagged(lab_of(rb.name, v), [it for _, it in its], [nm for nm, _ in its], mode, role_of(v)).any()


# ---------------------------------------------------------------------------------------------- the engine's side of a step
def run_engine(lab, eng, items, mode, roles=None):
    """set_state, set_motor_state, then C: eng.step(a) -> observation, reward, done; S: eng.settle(1), eng.observe() -> observation, 0, 0.
    -> state records [n, 80] float32, output rows [n, obs + 2] float32"""
    n = len(items)
    eng.set_motor_state(lab.record32(items, mode, roles))
    eng.set_state(np.array([it.s for it in items]))
    if mode == "C":
        ob, rw, dn = eng.step(np.array([it.a for it in items]))
    else:
        eng.settle(1)
        ob, rw, dn = eng.observe(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    row = np.concatenate([np.asarray(ob, np.float32), np.asarray(rw, np.float32).reshape(n, -1), np.asarray(dn, np.float32).reshape(n, -1)], 1)
    return np.ascontiguousarray(eng.get_state(), np.float32), np.ascontiguousarray(row)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_reset_record(Engine, lib, robot):
    """the motor record the checks start every engine from is, lane by lane and on all 32 lanes, what a real reset leaves (the checks skip the
    reset's settle steps)"""
    bind(Engine, lib)
    lab = lab_of(robot, "U")
    eng, _, close = lab.rb.pair(Engine, lib, 2, reset=True)
    try:
        got = eng.get_motor_state()
    finally:
        close()
    want = lab.reset_record()
    assert got.shape == (2, 4, W)
    for e in range(2):
        assert np.array_equal(got[e], want), (got[e], want)
    assert (want[2] == 1.0).all()
    # and the oracle's reset writes the same hold command
    mrec = lab.ora.hands_reset(1)[1][0]
    nd = lab.rb.nd
    assert all(np.array_equal(mrec[c * MD:c * MD + nd], lab.rec0[c * MD:c * MD + nd]) for c in range(4))


def check_records_agree(Engine, lib, robot):
    """the records the checks hand to set_motor_state are the oracle's (hands_apply_action, hands_set_motors); the engine's own commands
    (apply_action, set_motors with a mask) write the same numbers, lane by lane: an F env, a V env, a plain one, and on the Panda the grasp"""
    R = rows(Engine, lib, robot)
    lab = lab_of(robot, "U")
    rb = lab.rb
    nd = rb.nd
    free, vel = R.by["free"][0], R.by["vel:%d:1" % (nd - 1)][0]
    items, roles = [free, free, vel], [None, "F", "V"]
    if rb.panda:
        items, roles = items + [R.by["ro4"][0]], roles + ["F"]
    n = len(items)
    eng, close = lab.engine(Engine, lib, n)
    try:
        eng.set_motor_state(np.repeat(lab.reset_record()[None], n, 0))
        eng.set_state(np.array([it.s for it in items]))
        eng.apply_action(np.array([it.a for it in items]))
        rec = lab.mrec_of(items, "S")
        for e, (it, role) in enumerate(zip(items, roles)):
            for dofs, tgt, kp, force, mv in lab.cmds_of(it, role, rec[e]):
                eng.set_motors(list(dofs), np.asarray(tgt, np.float32), float(kp), force, mask=np.arange(n) == e, max_vel=mv)
        got = eng.get_motor_state()
    finally:
        close()
    want = lab.record32(items, "S", roles)
    assert np.array_equal(got, want), "motor records of the engine and the oracle differ after the same commands"
    assert (got[1, 2, :nd] < 1.0).all() and (got[1, 2, nd:] == 1.0).all() and (got[0, 2] == 1.0).all() and got[2, 3, nd - 1] == np.float32(V_BOUND)
    if rb.panda:
        assert (got[3, 2, 7:9] < 1.0).all() and (got[3, 3, 7:9] == 1.0).all() and (got[3, 2, :7] == 1.0).all()


# ---------------------------------------------------------------------------------------------- (a) one step against the oracle, per pool
def groups_of(names):
    """report groups: every pool; the limit and `vel` pools together and joint by joint (so that a failure names the joint)"""
    g = {}
    for e, nm in enumerate(names):
        kind = nm.split(":")[0]
        if kind in ("lim", "vel") and nm != "vel:slack":
            g.setdefault(kind, []).append(e)
            g.setdefault("%s:joint %d" % (kind, int(nm.split(":")[1])), []).append(e)
        else:
            g.setdefault(nm, []).append(e)
    return g


def compare(rb, names, se, ob, so, out, s_f, o_f):
    """hands_rows.compare on this robot's record, tables and report groups: per group and quantity the engine against the fp64 oracle,
    bound = the pool's table or, where the oracle's own fp32 build misses an entry on the same states, max(entry, 4 x d32); the Panda's
    fingertip tail: counts equal, forces within 4 x d32 of the forces over the pool's own states and never looser than 2 % of the pool's
    largest force (hands_rows.force_bound) -- round 16's rule, pool by pool.  On top of it the counts in the state record's copy of the
    tail, Q[21 .. 22], must be the oracle's (its forces are the observation's to the bit: check_rows_against_oracle).  -> report, failures"""
    import hands_rows
    nd, tail = rb.nd, rb.tail
    rep, bad = hands_rows.compare(names, se, ob, so, out, s_f, o_f, shape=rb.shape, tol=lambda g: tol_of(rb, g), groups=groups_of, tail=tail)
    if tail:
        for g, idx in groups_of(names).items():
            qe, qo = se[idx, nd + 7:nd + 7 + tail], so[idx, nd + 7:nd + 7 + tail]
            if not np.array_equal(qe[:, 5:], qo[:, 5:]):
                bad.setdefault(g, {})["fingers in contact, contact points (state record)"] = (qe[:, 5:].tolist(), qo[:, 5:].tolist())
    return rep, bad


def contact_sets_equal(rb, eng, items):
    """The engine's own contact query, from the state as set, against the oracle's signature: the three classes of pairs in contact (flags),
    the fingertip slots on the object (tips), and the numbers of spheres on the object and on the table (count) -- the oracle keeps at most
    nc_ro and nc_rt of those, so a full class is compared as `at least`.  Device libraries only: the host emulation has no contact query,
    there the observation tail's counts (compare()) are this check."""
    if not hasattr(eng.lib, "pbre_contact_query"):
        return
    from pybullet_robot_envs.model import contacts
    got = eng.contact_query(dist=False, nearest=False)
    want = np.array([(contacts.OBJECT_TABLE if it.sig[3] else 0) | (contacts.ROBOT_OBJECT if it.sig[1] else 0) | (contacts.ROBOT_TABLE if it.sig[2] else 0)
                     for it in items], np.int32)
    assert np.array_equal(got["flags"], want), "contact classes differ from the oracle's in envs %r" % np.nonzero(got["flags"] != want)[0].tolist()
    tips = np.array([it.tips for it in items], np.int32)
    assert np.array_equal(got["tips"], tips), "fingertip slots on the object differ from the oracle's in envs %r" % np.nonzero(got["tips"] != tips)[0].tolist()
    for col, k, cap in ((0, 1, rb.nc_ro), (1, 2, rb.nc_rt)):
        want_n = np.array([it.sig[k] for it in items])
        ok = np.where(want_n < cap, got["count"][:, col] == want_n, got["count"][:, col] >= cap)
        assert ok.all(), "sphere counts (%s) differ from the oracle's in envs %r" % ("object" if col == 0 else "table", np.nonzero(~ok)[0].tolist())


FEW_SWEEPS = (1, 2)
FEW_POOLS = ("lim", "ot", "vel", "free")       # (`free` with PBRE_OBJ_SPLIT=0 is an `ot` state as well: the cube rests where the reset put it)


def engines_of(robot):
    """(variant, way of stepping, sweeps) of check (a): every case at 150 sweeps; the cases that hold limit, `vel` or resting-cube states
    also at 1 and 2"""
    out = [(v, m, None) for v, m in CASES]
    few = [("B", "C"), ("B2", "C"), ("V", "S")] + ([("U", "C"), ("U", "S"), ("F", "S")] if robot == "panda" else [])
    return out + [(v, m, k) for v, m in few for k in FEW_SWEEPS]


def a_cases():
    """(robot, variant, way of stepping, sweeps, PBRE_OBJ_SPLIT) of check (a): the Panda with the knob unset and "0" (the resting cube's rows
    stay in kw_step: both only_ot loops, U the free one, F / B the clamping one); the iCub with it unset"""
    return [(r, v, m, k, sp) for r, splits in (("panda", (None, "0")), ("icub", (None,))) for v, m, k in engines_of(r) for sp in splits]


def check_rows_against_oracle(Engine, lib, robot, variant, mode, sweeps=None, split=None, kernel=""):
    """One engine of all pool states of the case, one step, per-quantity comparison with the fp64 oracle pool by pool and, for the limit and
    `vel` pools, joint by joint; nothing skipped (a case without states -- B2 where B sufficed for every limit state -- says so).
    sweeps: solver_iters = 1 or 2 instead of 150, for the limit, `vel` and resting-cube pools: after 150 sweeps a row that is missing from
    every second half-sweep has converged to the same impulse all the same.  One sweep is the backward half-sweep alone, two add the
    forward one; the oracle's result still depends on every limit row and velocity bound there (asserted).
    split: what PBRE_OBJ_SPLIT was set to before this call (None: unset; "0": the resting cube's rows stay in kw_step)."""
    R = rows(Engine, lib, robot)
    rb, lab = R.rb, lab_of(robot, variant)
    pairs = R.case(variant, mode, only=FEW_POOLS if sweeps is not None else None)
    if not pairs:
        assert variant == "B2", "no state is stepped under %s / %s" % (variant, mode)
        print("ARM_ROWS " + json.dumps({"check": "a", "robot": robot, "variant": variant, "envs": 0, "note": "B sufficed for every limit state"}))
        return {}
    names, items = [nm for nm, _ in pairs], [it for _, it in pairs]
    n = len(items)
    roles = [role_of(variant)] * n
    iters = int(lab.ora.params.solver_iters)
    eng, close = lab.engine(Engine, lib, n)
    try:
        if sweeps is not None:
            parity.set_solver_iters(eng, sweeps, lab.ora, lab.ora32)
        eng.set_state(np.array([it.s for it in items]))
        contact_sets_equal(rb, eng, items)
        se, row = run_engine(lab, eng, items, mode, roles)
        so, out, _ = lab.step(items, mode, roles)
        s_f, o_f, _ = lab.step(items, mode, roles, f32=True)
        if sweeps is not None:
            seen = {}
            if variant in BOUNDED:
                eff, _ = lab.limit_effect(items)
            elif variant == "V":
                eff = lab.bound_effect(items)
            else:
                eff = None
            for e, it in enumerate(items):
                for j in (it.sig[0] if variant in BOUNDED else ([it.vel[0]] if variant == "V" and it.vel[0] is not None else [])):
                    seen[j] = max(seen.get(j, 0.0), eff[e, j])
            weak = sorted(j for j, v in seen.items() if v < LIM_EFFECT)
            assert not weak, "after %d sweep(s) the oracle's result does not depend on the rows of joints %r" % (sweeps, weak)
    finally:
        close()
        lab.ora.params.solver_iters = lab.ora32.params.solver_iters = iters
    se, ob = np.asarray(se, np.float64), row[:, :-2].astype(np.float64)
    rep, bad = compare(rb, names, se, ob, so, out, s_f, o_f)
    print("ARM_ROWS " + json.dumps({"check": "a" if sweeps is None else "a, %d sweep(s)" % sweeps, "robot": robot, "variant": variant, "stepping": mode,
                                    "obj_split": split, "kernel": kernel, "envs": n, "groups": rep}))
    assert not bad, "%s, variant %s (%s), %s sweeps, split %s, %s: per-quantity bound exceeded (measured, bound) in %r" % (robot, variant, mode, sweeps or iters, split, kernel, bad)
    if mode == "C":
        assert (row[:, -1] == out[:, -1]).all() and np.abs(row[:, -2] - out[:, -2]).max() < 1e-3 * max(1.0, np.abs(out[:, -2]).max())
    if rb.tail:       # the state record carries what the observation reports
        assert np.array_equal(bits(se[:, rb.nd + 7:rb.nd + 7 + rb.tail]), bits(row[:, -rb.tail - 2:-2]))
    return rep


# ---------------------------------------------------------------------------------------------- (b), (c) wave-mates must not matter, bit for bit
def wave_probes(R):
    """(label, item, role): free, a limit state, the resting / held cube (Panda), a sphere on the table, a `vel` state with its bound"""
    rb = R.rb
    lim = "lim:%d:0" % (3 if rb.panda else 6)
    p = [("free", R.by["free"][-1], None), (lim, R.by[lim][-1], None)]
    if rb.panda:
        p += [("ot", R.by["ot"][-1], None), ("ro2", R.by["ro2"][-1], None)]
    return p + [("rt1", R.by["rt1"][-1], None), ("vel", R.by["vel:%d:1" % (1 if rb.panda else 4)][-1], "V")]


def wave_mates(R, variant):
    """(label, item, role): pair 0 is the reference (a free mate); a state with joint j at its lower limit for every j (the row then runs for
    the probe as an exact no-op); robot contacts; a force-limited mate (F: the whole wave skips the clamp-free attempt, the probe takes
    motor_x instead of motor_free); a velocity-bounded mate; a fast mate, every joint at 50 rad/s (under M its motors leave the bound and
    the wave repeats the solve with clamping rows: check (c))"""
    rb = R.rb
    free = R.by["free"]
    m = [("free", free[0], None)] + [("lim:%d:0" % j, R.by["lim:%d:0" % j][0], None) for j in range(rb.nd)]
    m += [(nm, R.by[nm][0], None) for nm in (("ro1", "ro4", "rt2") if rb.panda else ("ro1", "rt1"))]
    return m + [("F", free[1], "F"), ("V", R.by["vel:0:0"][0], "V"), ("fast", free[2].fast(rb.nd), None)]


def assert_only_the_fast_mate_exceeds_the_bound(lab, items, roles, labels, mode, p, probe_too=True):
    """variant M, from the oracle alone: lifting the motor bound to the default changes no pool env and does change the fast mate, so that only
    the wave that holds the fast mate repeats its solve with clamping rows (an F mate's force limit is a fraction of the bound: it moves
    with it and is left out)"""
    so, _, _ = lab.step(items, mode, roles)
    keep = lab.ora.params.max_motor_impulse
    lab.ora.params.max_motor_impulse = lab_of(lab.rb.name, "U").ora.params.max_motor_impulse
    try:
        s0, _, _ = lab.step(items, mode, roles)
    finally:
        lab.ora.params.max_motor_impulse = keep
    same = (so == s0).all(1)
    for w, label in enumerate(labels):
        mate = 2 * w + 1 - p
        if label == "fast":
            assert not same[mate], "the fast mate's motors stay under the bound: its wave would not repeat the solve"
        elif label != "F":
            assert same[mate], "a pool env's motors reach the bound (mate %s)" % label
        assert same[2 * w + p] or not probe_too, "the probe's motors reach the bound"


def check_wave_mates(Engine, lib, robot, variant, mode, split=None):
    """env = block * EPB + thread / 32: pair w of the batch is the probe beside mate w, the probe in the lower (p = 0) and in the upper (p = 1)
    half-wave; its state record and output row are bit-identical to those of the same probe beside a free mate, whatever the mate makes
    the wave do.  Under M this is check (c): the premise comes from the oracle, the probe beside the fast mate went through the hand-back."""
    R = rows(Engine, lib, robot)
    rb, lab = R.rb, lab_of(robot, variant)
    mates = wave_mates(R, variant)
    nv = len(mates)
    eng, close = lab.engine(Engine, lib, 2 * nv)
    moved = 0
    try:
        for label, probe, prole in wave_probes(R):
            for p in (0, 1):
                items, roles = [], []
                for _, mate, mrole in mates:
                    pair, prl = [None, None], [None, None]
                    pair[p], pair[1 - p], prl[p], prl[1 - p] = probe, mate, prole, mrole
                    items += pair; roles += prl
                if variant == "M":
                    # (a probe with robot contact rows: its wave makes no clamp-free attempt whatever the mate -- Core::step tries it only
                    # where the wave has no contact row but the object-table ones -- so there is no hand-back to force and the probe's own
                    # motors may bind, as the squeezing fingers' of `ro2` do; the mates' half of the premise is asserted all the same)
                    assert_only_the_fast_mate_exceeds_the_bound(lab, items, roles, [m[0] for m in mates], mode, p,
                                                                probe_too=not any(k in label for k in ("ro", "rt")))
                st, row = run_engine(lab, eng, items, mode, roles)
                st, row = bits(st), bits(row)
                moved += not np.array_equal(st[p, :rb.nd], bits(probe.s[:rb.nd]))
                diff = [mates[w][0] for w in range(1, nv) if not (np.array_equal(st[p], st[2 * w + p]) and np.array_equal(row[p], row[2 * w + p]))]
                assert not diff, ("%s, probe %s in half-wave %d, variant %s (%s), split %s: state record or output row differs from the probe beside a free mate "
                                  "beside the mates %r" % (robot, label, p, variant, mode, split, diff))
    finally:
        close()
    assert moved == 2 * len(wave_probes(R)), "a probe did not move: nothing tested"


# ---------------------------------------------------------------------------------------------- (d) the residual exit with fingertip forces
RT_THRESHOLD = 1e-7
RT_CASES = [("U", "C"), ("U", "S"), ("F", "S")]


def check_residual_exit(Engine, lib, variant, mode):
    """Panda, solver_residual_threshold = 1e-7 (Core::step<RT>) on the `ro` pools: sweep counts against the oracle's, with the allowance of
    hands_rows check (d) and parity.check_hands_residual_threshold (flips in at most 10 % of the envs, at most 2 sweeps apart, held to
    TOL_RT_FLIP_GROUP); envs with equal counts are held to the bounds of check (a), fingertip forces included.  The envs are ordered so
    that the two envs of a wave leave the loop at different sweeps (from the oracle): each must report the normal impulses of ITS exit
    sweep (the rt_an snapshot)."""
    robot = "panda"
    R = rows(Engine, lib, robot)
    rb, lab = R.rb, lab_of(robot, variant)
    pairs = R.items(rb.ro_pools + ["ro+ot"])
    names, items = [nm for nm, _ in pairs], [it for _, it in pairs]
    n = len(items)
    roles = [role_of(variant)] * n
    iters = int(lab.ora.params.solver_iters)
    eng, close = lab.engine(Engine, lib, n)
    try:
        eng.set_physics(solver_residual_threshold=RT_THRESHOLD)
        lab.ora.params.solver_residual_threshold = lab.ora32.params.solver_residual_threshold = RT_THRESHOLD
        _, _, used = lab.step(items, mode, roles)
        order = np.argsort(used, kind="stable")
        order = np.stack([order[:n // 2], order[n - n // 2:]], 1).ravel() if n % 2 == 0 else order      # wave k: the k-th earliest beside the k-th of the later half
        names, items = [names[e] for e in order], [items[e] for e in order]
        so, out, used = lab.step(items, mode, roles)
        s_f, o_f, _ = lab.step(items, mode, roles, f32=True)
        se, row = run_engine(lab, eng, items, mode, roles)
        sw = eng.get_sweeps().astype(int)
    finally:
        lab.ora.params.solver_residual_threshold = lab.ora32.params.solver_residual_threshold = 0.0
        close()
    se, ob = np.asarray(se, np.float64), row[:, :-2].astype(np.float64)
    apart = int(sum(used[2 * k] != used[2 * k + 1] for k in range(n // 2)))
    early = int((used < iters).sum())
    same = sw == used
    flips = int((~same).sum())
    assert np.abs(sw - used).max() <= 2, (variant, names, sw.tolist(), used.tolist())
    idx = np.nonzero(same)[0]
    rep, bad = compare(rb, [names[e] for e in idx], se[idx], ob[idx], so[idx], out[idx], s_f[idx], o_f[idx])
    print("ARM_ROWS " + json.dumps({"check": "d", "robot": robot, "variant": variant, "stepping": mode, "envs": n, "sweeps": used.tolist(), "flips": flips,
                                    "early": early, "waves apart": apart, "groups": rep}))
    assert not bad, "residual exit, variant %s (%s): per-quantity bound exceeded (measured, bound) in %r" % (variant, mode, bad)
    if flips:
        f = np.nonzero(~same)[0]
        parity.assert_within(parity.group_quantities(rb.shape, se[f], so[f], ob[f], out[f], tail=rb.tail), parity.TOL_RT_FLIP_GROUP, "(arm rows, sweep-count flips)")
    assert 2 * early >= n, "only %d of %d envs with robot-object rows leave before the cap: the snapshot is not exercised" % (early, n)
    assert apart >= 1, "no wave whose two envs leave the loop at different sweeps"
    assert flips <= max(1, n // 10), "exit sweeps differ in %d of %d envs" % (flips, n)
    return rep
