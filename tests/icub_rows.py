"""States that put every row kind of the 20-DoF iCub solve kernels to work, joint by joint (tests only).

The iCub push task, left arm, joint control (no IK flips), no auto-reset.  Two engines step it:

  the lane-per-env pipeline (csrc/pbre_lane.hip: kw_dyn -> kw_quad / kw_quad_rc -> kw_fin; PBRE_ICUB_LANE=1, the default from 16384 envs on).
      Its solve, quad_step, exists on the GPU only -- the emulation runs Lane::step in its place -- and works with wave-level shortcuts:
      limit row j runs if ANY env of the wave has joint j at a limit (a ballot mask; the row is owned by quad lane j / 5), contact slot c
      if any env uses it (__any), the clamp-free motor attempt is made per wave and repeated with clamping rows if any env's motor
      exceeded its bound.
      kw_quad     global lane gl serves env gl >> 2: wave w holds envs 16 w .. 16 w + 15, in natural order
      kw_quad_rc  the envs with robot-object contact, from a compacted list: with at most 16 of them in the batch (and PBRE_QUAD_RC_EPW at
                  its default of 16) they share wave 0 whatever order the atomics produce
  the lane-group kernel (kw_step, pbre_wide_impl.hpp; PBRE_ICUB_LANE=0): one env per 32 lanes, so envs 2 k and 2 k + 1 share a wave.

Whoever remaps envs to waves in these kernels updates this module knowingly: the wave-mate checks below rely on the three rules.

Everything here comes from the oracle alone: single-env states by ROW SIGNATURE (joints at a limit by the oracle's own test; robot-object,
robot-table, object-table contact counts from orc.sim_step's StepInfo.type), pools of them, the assertion that every pool is full after the
oracle's own conditioning probe has dropped what it objects to -- so the engine-side checks skip nothing.  Two physics variants:

  B  bounded motors, max_motor_impulse = 0.004 (as parity.check_icub_force_limited and the Panda families with bounded motors)
  U  the defaults (unbounded: PyBullet's default force is an impulse bound of 417, which no state here comes near)
  M  max_motor_impulse = 30, for the wave-mate check of kw_quad only: a bound that the motors of the pool states stay under and those of a
     state with every joint at 50 rad/s exceed, so that such a wave-mate makes the wave repeat its clamp-free attempt with clamping rows

With unbounded motors a limit row is invisible in the result: the position motor of the same joint undoes its impulse within the sweep (the
oracle's step with and without limit rows differs by < 1e-7 rad/s, 1 cm past any of the 40 limits).  With bounded motors the row decides
where the joint goes, but only in states where the motor alone does not stop the joint; so a `lim` state is accepted only if the ORACLE's
step with and without limit rows (limit_max_impulse at its default and at 0) differs by >= LIM_EFFECT in that joint's velocity.
"""
import functools
import json

import numpy as np

import orc
import parity
from row_paths import step_bits

ND, W, LC = 20, 32, 20                 # DoF, velocity offset, object offset of the 80-float state record (Q[32] | V[32] | X[16])
SEED = 20250311
PHYS = {"B": {"max_motor_impulse": 0.004}, "U": {}, "M": {"max_motor_impulse": 30.0}}
LIM_EFFECT = 0.05                      # rad/s: 50 x TOL_ICUB_CONTACT["qd"]
PEN = (0.005, 0.02)                    # rad past the limit -- never ON it: fp32 rounding of the limit would flip the row
INTO = (0.5, 4.0)                      # rad/s into the limit
ARM_L = (3, 4, 5, 6, 7, 8, 9)          # the controlled left-arm joints
N_LIM, N_OTHER = 2, 8

OTHER_POOLS = ["free", "lim2:same", "lim2:cross", "rt1", "rt2", "ro1", "ro2", "ro1+rt1", "lim+rt1", "lim+ro1"]
LIM_POOLS = ["lim:%d:%d" % (j, side) for j in range(ND) for side in (0, 1)]
CONTACT_POOLS = ["rt1", "rt2", "ro1", "ro2", "ro1+rt1", "lim+rt1", "lim+ro1"]
RO_POOLS = ["ro1", "ro2", "ro1+rt1", "lim+ro1"]


class _Shape:                          # what parity.group_quantities reads of an engine
    ndof, v_off = ND, W


def tol_of(pool):
    return parity.TOL_ICUB if pool == "free" else parity.TOL_ICUB_CONTACT


class Lab:
    """fp64 and fp32 oracle with the same settings (variant "B" or "U"), the joint limits, the engine to match"""

    def __init__(self, variant):
        self.variant, self.phys = variant, dict(PHYS[variant])
        (self.ora, self.tbl, self.info), (self.ora32, _, _) = (self._oracle(f32) for f32 in (False, True))
        m = self.ora.model
        self.lo = np.array([m.lower[m.link_of_dof[k]] for k in range(ND)])
        self.hi = np.array([m.upper[m.link_of_dof[k]] for k in range(ND)])
        self.home = np.asarray(self.info["home"], float)
        self.ctrl = list(self.info["controlled"])

    def _oracle(self, f32):
        o, tbl, info = orc.icub_oracle("l", task=1, use_ik=0, control_orientation=0, f32=f32)
        o.task.reward_type, o.task.obj_pose_rnd_std, o.task.tg_pose_rnd_std, o.task.max_steps = 1, 0.0, 0.2, 10 ** 6
        for k, v in self.phys.items():
            setattr(o.params, k, v)
        assert o.ndof == ND and o.state_floats == 2 * W + 16
        return o, tbl, info

    def engine(self, Engine, lib, n):
        from pybullet_robot_envs import _capi
        ov = parity.icub_overrides(self.info, "l", 0, 0, 1)
        return Engine(self.tbl, task=1, num_envs=n, lib=lib, robot=_capi.ROBOT_ICUB, obj_pose_rnd_std=0.0, tg_pose_rnd_std=0.2, max_steps=10 ** 6,
                      **({"phys": self.phys} if self.phys else {}), **ov)

    def signature(self, s):
        """(joints at a limit, robot-object contacts, robot-table contacts, object-table contacts) of the fp32 state s"""
        s = np.asarray(s, np.float32).astype(np.float64)
        _, info = self.ora.sim_step(s, s[:ND].copy(), np.full(ND, 0.1), np.full(ND, 1.0))
        t = [info.type[k] for k in range(info.ncontacts)]
        lim = frozenset(j for j in range(ND) if s[j] - self.lo[j] <= 0 or self.hi[j] - s[j] <= 0)        # the oracle's own test (limit rows)
        return lim, t.count(1), t.count(2), t.count(0)

    def limit_effect(self, S, A):
        """[n, ND]: how far the oracle's joint velocities after one step move when its limit rows are taken away"""
        s64 = np.asarray(S, np.float32).astype(np.float64)
        so, _ = self.ora.batch_step(s64, A)
        keep = self.ora.params.limit_max_impulse
        self.ora.params.limit_max_impulse = 0.0
        try:
            s0, _ = self.ora.batch_step(s64, A)
        finally:
            self.ora.params.limit_max_impulse = keep
        return np.abs(so[:, W:W + ND] - s0[:, W:W + ND])


@functools.lru_cache(maxsize=None)
def lab_of(variant):
    return Lab(variant)


@functools.lru_cache(maxsize=None)
def base_state():
    """the settled reset state of the default physics: every crafted state is a copy of it with other joints / another cube pose"""
    return lab_of("U").ora.batch_reset(1)[0][0]


def flagged(lab, S, A, names):
    """Envs of the batch (S, A; names[e] = pool of env e) that the oracle itself calls ill conditioned: a contact candidate within 3 um of the
    margin (parity.ambiguous_envs), or a result that moves by more than half the pool's bounds when the fp64 oracle's input is perturbed at
    the fp32 rounding level or its fp32 build runs instead (the probe of row_paths.flagged on the iCub's record).  No engine is involved."""
    s32 = np.asarray(S, np.float32)
    s64 = s32.astype(np.float64)
    n = len(s32)
    bad = parity.ambiguous_envs(lab.ora, s64, A)
    so, out = lab.ora.batch_step(s64, A)
    prng = np.random.default_rng(12345)
    trials = [lab.ora32.batch_step(s32, A)]
    cols = np.r_[0:ND + 7, W:W + ND + 6]
    # (`free` is held to TOL_ICUB, whose obj_pos bound of 3e-7 m is 2.3 fp32 roundings of the resting cube's height: row_paths' 2e-7 would
    # move the INPUT by 0.43 of that bound, whatever the state.  One rounding, 2^-24, there.)
    size = np.array([2.0 ** -24 if nm == "free" else 2e-7 for nm in names])[:, None]
    for _ in range(4):
        sp = s32.astype(np.float64)
        sp[:, cols] *= 1.0 + size * prng.uniform(-1.0, 1.0, (n, len(cols)))
        trials.append(lab.ora.batch_step(sp, A))
    for s_f, o_f in trials:
        s_f, o_f = np.asarray(s_f, np.float64), np.asarray(o_f, np.float64)
        for e in range(n):
            tt = tol_of(names[e])
            q = parity.group_quantities(_Shape, s_f[e:e + 1], so[e:e + 1], o_f[e:e + 1, :-2], out[e:e + 1])
            bad[e] |= any(v > 0.5 * tt[k] for k, v in q.items())
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


class Pools:
    """pool name -> states with that row signature (and, for the limit pools, with limit rows the oracle's result depends on)"""

    def __init__(self, seed=SEED):
        from pybullet_robot_envs.model.table import icub_model, icub_spheres
        self.lab, self.rng = lab_of("B"), np.random.default_rng(seed)       # (B: the sensitivity rule is about bounded motors)
        self.base = np.array(base_state(), float)
        m = icub_model()
        links = [l["name"] for l in m["links"]]
        self.sph = [(links.index(ln), np.array(c), r) for ln, c, r in icub_spheres(m) if ln.startswith("l_")]      # hand, hand, forearm
        self.pool, self.used, self.drawn = {}, {}, {}
        P = self.lab.ora.params
        self.ztop, self.tc, self.th = P.table_c[2] + P.table_h[2], np.array(list(P.table_c)), np.array(list(P.table_h))
        self.oh = float(P.obj_h[0])

    # ---- pieces
    def _inside(self, q):
        lab = self.lab
        return np.clip(q, lab.lo + 0.05 * (lab.hi - lab.lo), lab.hi - 0.05 * (lab.hi - lab.lo))

    def _state(self, q, qd):
        s = self.base.copy()
        s[:ND], s[W:W + ND] = q, qd
        return s

    def _arm(self, spread, every=True):
        """joints spread about home (every: all 20 DoF, else the 10 controlled ones) inside their ranges, random velocities"""
        lab, rng = self.lab, self.rng
        q = lab.home.copy()
        idx = np.arange(ND) if every else np.array(lab.ctrl)
        q[idx] += rng.normal(0, spread, len(idx))
        qd = np.zeros(ND)
        qd[idx] = rng.normal(0, 0.3, len(idx))
        return self._inside(q), qd

    def _past(self, q, qd, j, side):
        """joint j PAST its limit, moving into it"""
        pen, v = self.rng.uniform(*PEN), self.rng.uniform(*INTO)
        q[j], qd[j] = (self.lab.lo[j] - pen, -v) if side == 0 else (self.lab.hi[j] + pen, v)

    def _centres(self, q):
        R, p = self.lab.ora.fk(q)
        return [(p[i] + R[i] @ c, r) for i, c, r in self.sph]

    def _cube_on_a_sphere(self, s, pen=0.002):
        """the cube, axis-aligned, one face `pen` deep in one left-arm sphere from below / beside"""
        rng = self.rng
        c, r = self._centres(s[:ND])[rng.integers(0, len(self.sph))]
        d = rng.normal(size=3); d[2] = -abs(d[2])
        dd = np.zeros(3); k = int(np.argmax(np.abs(d))); dd[k] = np.sign(d[k])
        s[LC:LC + 3] = c + dd * (r + self.oh - pen)
        s[LC + 3:LC + 7] = [0, 0, 0, 1]
        s[W + LC:W + LC + 6] = rng.normal(0, 0.1, 6)

    def _cube_across_the_hand(self, s, pen=0.002):
        """the cube's face diagonal laid across the two l_hand spheres (radii 32 and 22 mm, centres 5.2 cm apart: less than the 7.1 cm
        diagonal), the face `pen` deep in both: two robot-object contacts"""
        rng = self.rng
        (c1, r1), (c2, r2) = self._centres(s[:ND])[:2]
        u = c2 - c1; L = np.linalg.norm(u); u /= L
        v = rng.normal(size=3); v[2] = abs(v[2]) + 0.5            # (the face looks up at the hand, the cube hangs below / beside it)
        v -= (v @ u) * u; v /= np.linalg.norm(v)
        a = (r2 - r1) / L                                         # the face's normal n: n . (c2 - c1) = r2 - r1, both spheres equally deep
        n = a * u + np.sqrt(1.0 - a * a) * v
        p1, p2 = c1 - n * (r1 - pen), c2 - n * (r2 - pen)
        t = (p2 - p1) / np.linalg.norm(p2 - p1)
        b = np.cross(n, t)
        R = np.stack([(t + b) / np.sqrt(2.0), (b - t) / np.sqrt(2.0), n], 1)      # face axes at 45 degrees to the line of the spheres
        s[LC:LC + 3] = 0.5 * (p1 + p2) + rng.uniform(-0.004, 0.004) * t - n * self.oh
        s[LC + 3:LC + 7] = _quat_of(R)
        s[W + LC:W + LC + 6] = rng.normal(0, 0.1, 6)

    def _on_table(self, q):
        ds = [c[2] - r - self.ztop for c, r in self._centres(q) if abs(c[0] - self.tc[0]) < self.th[0] and abs(c[1] - self.tc[1]) < self.th[1]]
        return bool(ds) and -0.004 < min(ds) < 0.0008

    def _crafted(self, **cnt):
        kw = dict(n_obj=0, n_table=0, n_both=0, n_limit=0)
        kw.update(cnt)
        S, _ = parity.icub_contact_states(self.lab.ora, self.lab.info, self.base, self.rng, control_arm="l", **kw)
        return list(S)

    # ---- candidates of a pool (not yet checked against its signature)
    def _make(self, name):
        rng, lab = self.rng, self.lab
        parts = name.split(":")
        kind = parts[0]
        if kind == "free":
            return [self._state(*self._arm(0.25)) for _ in range(8)]
        if kind == "lim":                       # lim:<j>:<side>
            out = []
            for _ in range(12):
                q, qd = self._arm(0.3)
                self._past(q, qd, int(parts[1]), int(parts[2]))
                out.append(self._state(q, qd))
            return out
        if kind == "lim2":                      # lim2:same / lim2:cross: two joints of one env, owned by one quad lane (j // 5) or by two
            out = []
            for _ in range(24):
                q, qd = self._arm(0.3)
                j1 = int(rng.integers(0, ND))
                if parts[1] == "same":
                    j2 = 5 * (j1 // 5) + (j1 % 5 + int(rng.integers(1, 5))) % 5
                else:
                    j2 = (j1 + 5 * int(rng.integers(1, 4))) % ND
                    j2 = 5 * (j2 // 5) + int(rng.integers(0, 5))
                self._past(q, qd, j1, int(rng.integers(0, 2)))
                self._past(q, qd, j2, int(rng.integers(0, 2)))
                out.append(self._state(q, qd))
            return out
        if kind in ("rt1", "rt2"):              # parity.icub_contact_states' table search
            return self._crafted(n_table=8)
        if kind == "ro1":
            return self._crafted(n_obj=12)
        if kind == "ro2":
            out = []
            for _ in range(8):
                s = self._state(*self._arm(0.3, every=False))
                self._cube_across_the_hand(s)
                out.append(s)
            return out
        if kind == "ro1+rt1":
            return self._crafted(n_both=8)
        if kind == "lim+rt1":                   # a controlled left-arm joint past its limit, a sphere of that arm on the table
            out = []
            for _ in range(4):
                j, side = ARM_L[int(rng.integers(0, len(ARM_L)))], int(rng.integers(0, 2))
                for _ in range(20000):
                    q, qd = self._arm(0.5, every=False)
                    self._past(q, qd, j, side)
                    if self._on_table(q):
                        break
                else:
                    raise RuntimeError("no table-contact configuration with joint %d at its limit" % j)
                out.append(self._state(q, qd))
            return out
        if kind == "lim+ro1":                   # lim+ro1[:<j>]: joint j (default: a controlled left-arm joint) past its limit, the cube on that arm
            out = []
            for _ in range(8):
                q, qd = self._arm(0.3, every=False)
                j = int(parts[1]) if len(parts) > 1 else ARM_L[int(rng.integers(0, len(ARM_L)))]
                self._past(q, qd, j, int(rng.integers(0, 2)))
                s = self._state(q, qd)
                self._cube_on_a_sphere(s)
                out.append(s)
            return out
        raise KeyError(name)

    def _fits(self, name, s, sig):
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
            return (a // 5 == b // 5) == (parts[1] == "same")
        if kind in ("rt1", "rt2"):
            return not lim and nro == 0 and nrt == int(kind[2])
        if kind in ("ro1", "ro2"):              # the cube in the air
            return not lim and nro == int(kind[2]) and nrt == 0 and not_ == 0
        if kind == "ro1+rt1":
            return not lim and nro == 1 and nrt == 1
        if kind == "lim+rt1":
            return len(lim) == 1 and min(lim) in ARM_L and nro == 0 and nrt == 1
        if kind == "lim+ro1":
            return len(lim) == 1 and (min(lim) == int(parts[1]) if len(parts) > 1 else min(lim) in ARM_L) and nro == 1 and nrt == 0 and not_ == 0
        raise KeyError(name)

    def take(self, name):
        """the next unused (state, action, signature) of pool `name`"""
        lst = self.pool.setdefault(name, [])
        k = self.used.get(name, 0)
        tries = 0
        while k >= len(lst):
            tries += 1
            assert tries < 200, "no state with the signature of pool %r" % name
            cand = [np.asarray(s, np.float32) for s in self._make(name)]
            self.drawn[name] = self.drawn.get(name, 0) + len(cand)
            acts = self.rng.uniform(-1, 1, (len(cand), len(self.lab.ctrl))).astype(np.float32)
            sigs = [self.lab.signature(s) for s in cand]
            eff = self.lab.limit_effect(np.array(cand), acts) if name.startswith("lim") else None
            for e, (s, sig) in enumerate(zip(cand, sigs)):
                if not self._fits(name, s, sig):
                    continue
                if eff is not None and not all(eff[e, j] >= LIM_EFFECT for j in sig[0]):      # the sensitivity rule, per state
                    continue
                lst.append((s, acts[e], sig))
        self.used[name] = k + 1
        return lst[k]


class Rows:
    """the filled pools: by[name] = list of (state, action, signature), all of them well conditioned under both physics variants"""

    def __init__(self, extra=()):
        pools = Pools()
        want = [(nm, N_LIM) for nm in LIM_POOLS] + [(nm, N_OTHER) for nm in OTHER_POOLS] + [(nm, 1) for nm in extra]
        cur = [(nm, pools.take(nm)) for nm, k in want for _ in range(k)]
        self.redrawn = 0
        for rnd in range(40):
            S, A, names = np.array([c[0] for _, c in cur]), np.array([c[1] for _, c in cur]), [nm for nm, _ in cur]
            bad = flagged(lab_of("B"), S, A, names) | flagged(lab_of("U"), S, A, names)
            if not bad.any():
                break
            for e in np.nonzero(bad)[0]:
                cur[e] = (names[e], pools.take(names[e]))
                self.redrawn += 1
        else:
            raise AssertionError("still ill-conditioned states after 40 rounds of re-drawing")
        self.by, self.drawn = {}, dict(pools.drawn)
        for nm, c in cur:
            self.by.setdefault(nm, []).append(c)
        for nm, k in want:       # every pool is full: nothing is skipped downstream
            assert len(self.by[nm]) == k, (nm, len(self.by[nm]))

    def batch(self, names):
        """all states of the pools `names` as one batch: S [n, 80] float32, A [n, 10] float32, pool name per env"""
        items = [(nm, c) for nm in names for c in self.by[nm]]
        return np.array([c[0] for _, c in items]), np.array([c[1] for _, c in items]), [nm for nm, _ in items]


MATE_POOLS = ["lim+ro1:%d" % j for j in (3, 8, 11, 16)]        # a joint of each quad lane at its limit in an env of kw_quad_rc's wave


@functools.lru_cache(maxsize=None)
def rows():
    """cached: the states and the oracle's verdicts are computed once per process"""
    return Rows(extra=MATE_POOLS)


def assert_pools(R):
    """the generator's own promises, re-checked from the finished pools"""
    B = lab_of("B")
    for j in range(ND):
        for side in (0, 1):
            nm = "lim:%d:%d" % (j, side)
            S, A, _ = R.batch([nm])
            assert len(S) == N_LIM
            eff = B.limit_effect(S, A)[:, j]
            assert (eff >= LIM_EFFECT).all(), (nm, eff)
            for s in S:
                assert B.signature(s)[:3] == (frozenset([j]), 0, 0)
                gap = (B.lo[j] - s[j]) if side == 0 else (s[j] - B.hi[j])
                assert PEN[0] - 1e-6 <= gap <= PEN[1] + 1e-6 and (s[W + j] < 0) == (side == 0)
    for nm in OTHER_POOLS:
        assert len(R.by[nm]) == N_OTHER
    for nm, same in (("lim2:same", True), ("lim2:cross", False)):
        S, A, _ = R.batch([nm])
        eff = B.limit_effect(S, A)
        for e, (_, _, sig) in enumerate(R.by[nm]):
            a, b = sorted(sig[0])
            assert (a // 5 == b // 5) == same and eff[e, a] >= LIM_EFFECT and eff[e, b] >= LIM_EFFECT
    assert set(sig[1:3] for _, _, sig in R.by["ro2"]) == {(2, 0)} and set(sig[1:3] for _, _, sig in R.by["rt2"]) == {(0, 2)}
    S, A, names = R.batch(LIM_POOLS + OTHER_POOLS + MATE_POOLS)
    assert S.dtype == np.float32 and len(S) == 2 * ND * N_LIM + len(OTHER_POOLS) * N_OTHER + len(MATE_POOLS)
    for v in ("B", "U"):
        assert not flagged(lab_of(v), S, A, names).any()


# ---------------------------------------------------------------------------------------------- (a) one step against the oracle, per pool
def pools_of(variant):
    """B: every pool.  U: the contact pools -- there the limit pools are redundant (the motor undoes the row), and a wave with contact rows
    skips the clamp-free attempt"""
    return (LIM_POOLS + OTHER_POOLS) if variant == "B" else CONTACT_POOLS


def groups_of(names):
    """report groups: every pool; the limit pools together and joint by joint (so that a failure names the joint)"""
    g = {}
    for e, nm in enumerate(names):
        if nm.startswith("lim:"):
            g.setdefault("lim", []).append(e)
            g.setdefault("lim:joint %d" % int(nm.split(":")[1]), []).append(e)
        else:
            g.setdefault(nm, []).append(e)
    return g


def check_rows_against_oracle(Engine, lib, variant, lane, device=True, kernel=""):
    """One engine of all pool states of the variant, one step with the states' fixed actions, per-quantity comparison with the fp64 oracle
    (parity.group_quantities) pool by pool: TOL_ICUB_CONTACT (TOL_ICUB for `free`), nothing skipped.  The bound is not the engine's: where
    the oracle's own fp32 build misses a bound on a pool, that pool's bound is max(TOL, 4 x d32), d32 taken over the same states and actions
    (the rule and margin of tests/test_gpu_kin_query.py and tests/sweep_counts.py).  lane: what PBRE_ICUB_LANE was set to when this is called.
    device: the engine classes a batch when its state is set (the emulation counts complex env-steps as it takes them).
    Returns {group: {quantity: {"engine", "d32", "bound"}}}."""
    lab, R = lab_of(variant), rows()
    S, A, names = R.batch(pools_of(variant))
    n = len(S)
    n_ro = sum(nm in RO_POOLS for nm in names)
    eng = lab.engine(Engine, lib, n)
    try:
        eng.set_state(S)
        info0 = eng.kernel_info()
        ob, rw, dn = eng.step(A)
        se = np.asarray(eng.get_state(), np.float64)
        info1 = eng.kernel_info()
    finally:
        eng.close()
    assert info0[2] == lane, info0
    if lane:       # the envs with robot-object contact are the complex class (kw_quad_rc / the emulation's complex path): as many as the oracle says
        assert n_ro > 0 and (info0[5] if device else info1[5] - info0[5]) == n_ro, (info0, info1, n_ro)
    s64 = S.astype(np.float64)
    so, out = lab.ora.batch_step(s64, A)
    s_f, o_f = (np.asarray(x, np.float64) for x in lab.ora32.batch_step(S, A))
    ob = np.asarray(ob, np.float64)
    rep, bad = {}, {}
    for g, idx in groups_of(names).items():
        tt = tol_of(g)
        d32 = parity.group_quantities(_Shape, s_f[idx], so[idx], o_f[idx, :-2], out[idx])
        w = parity.group_quantities(_Shape, se[idx], so[idx], ob[idx], out[idx])
        rep[g] = {}
        for k in tt:
            bound = tt[k] if d32[k] <= tt[k] else max(tt[k], 4.0 * d32[k])
            rep[g][k] = {"engine": float("%.3g" % w[k]), "d32": float("%.3g" % d32[k]), "bound": float("%.3g" % bound)}
            if not w[k] <= bound:
                bad.setdefault(g, {})[k] = (float("%.3g" % w[k]), bound)
    print("ICUB_ROWS " + json.dumps({"check": "a", "variant": variant, "kernel": kernel, "envs": n, "groups": rep}))
    assert not bad, "variant %s, %s: per-quantity bound exceeded (measured, bound) in %r" % (variant, kernel, bad)
    assert (np.asarray(dn) == out[:, -1]).all() and np.abs(np.asarray(rw) - out[:, -2]).max() < 1e-3 * max(1.0, np.abs(out[:, -2]).max())
    return rep


# ---------------------------------------------------------------------------------------------- (b) wave-mates must not matter, bit for bit
def _fast(c):
    """the state with every joint at 50 rad/s.  Under M its motors exceed the bound, so its wave repeats the clamp-free attempt with clamping
    rows (under U they do not: 417 is out of reach, the mate is merely fast)"""
    s = c[0].copy()
    s[W:W + ND] = 50.0
    return s, c[1], c[2]


QUAD_PROBES = ["free", "lim:3:1", "lim:8:0", "lim:12:1", "lim:17:0", "rt1"]      # a limit probe per quad lane (joint // 5)
QUAD_POSITIONS = (0, 6, 15)


def quad_variants(variant):
    """kw_quad: what the probe's 15 wave-mates are, wave by wave"""
    v = [("free", None)] + [("lim:%d:0" % j, "lim:%d:0" % j) for j in range(ND)] + [("rt1", "rt1"), ("rt2", "rt2")]
    return v + ([("fast", "fast")] if variant in ("U", "M") else [])


def assert_fast_mate_alone_exceeds_the_bound(S, A, labels):
    """variant M, from the oracle alone: lifting the motor bound to the default changes nothing in the envs of the waves whose mates are free or
    at a limit (their motors stay under the bound; waves with robot-table rows make no clamp-free attempt anyway) and does change the fast
    mate's result (its motors are clamped)"""
    lab = lab_of("M")
    s64 = S.astype(np.float64)
    so, _ = lab.ora.batch_step(s64, A)
    lab.ora.params.max_motor_impulse = lab_of("U").ora.params.max_motor_impulse
    try:
        s0, _ = lab.ora.batch_step(s64, A)
    finally:
        lab.ora.params.max_motor_impulse = PHYS["M"]["max_motor_impulse"]
    same = (so == s0).all(1)
    for w, label in enumerate(labels):
        if label == "fast":
            assert (~same[16 * w:16 * w + 16]).sum() == 1, "the fast mate's motors stay under the bound: its wave would not repeat the attempt"
        elif not label.startswith("rt"):
            assert same[16 * w:16 * w + 16].all(), "an ordinary env's motors reach the bound (wave %d, mates %s)" % (w, label)


def quad_batch(variant, probe, p):
    """16 x V envs, one variant per wave of kw_quad: env 16 w + p is the probe (pool `probe`, its second state where the pool has as many, so
    that a `lim:j:0` mate is another state), one mate of wave w is the variant's, the others are free.  -> S, A, labels"""
    R = rows()
    free = R.by["free"]
    pc = R.by[probe][-1]
    S, A, labels = [], [], []
    for w, (label, mate) in enumerate(quad_variants(variant)):
        wave = [free[(w + i) % (len(free) - 1)] for i in range(16)]        # (free[-1] is the free probe)
        if mate is not None:
            at = (p + 1 + 5 * w) % 16
            at = at if at != p else (p + 1) % 16
            wave[at] = _fast(free[0]) if mate == "fast" else R.by[mate][0]
        wave[p] = pc
        S += [c[0] for c in wave]; A += [c[1] for c in wave]; labels.append(label)
    return np.array(S), np.array(A), labels


def _same_probe(st, row, e0, e, ctx):
    assert np.array_equal(st[e0], st[e]), "state record differs with the wave-mates: " + ctx
    assert np.array_equal(row[e0], row[e]), "output row differs with the wave-mates: " + ctx


def check_quad_wave_mates(Engine, lib, variant, lane=1, probes=QUAD_PROBES, positions=QUAD_POSITIONS):
    """kw_quad: the probe's state record and output row are bit-identical in every wave, whatever its mates make the wave do"""
    lab = lab_of(variant)
    nv = len(quad_variants(variant))
    eng = lab.engine(Engine, lib, 16 * nv)
    try:
        for probe in probes:
            for p in positions:
                S, A, labels = quad_batch(variant, probe, p)
                if variant == "M" and p == positions[0] and not probe.startswith("rt"):
                    assert_fast_mate_alone_exceeds_the_bound(S, A, labels)
                eng.set_state(S)
                info = eng.kernel_info()
                assert info[2] == lane and info[5] == 0, info      # (no env is in the complex class: kw_quad steps them all)
                st, row = step_bits(eng, S, A)
                assert not np.array_equal(st[p, :ND], S[p, :ND].view(np.uint32)), "the probe did not move: nothing tested"
                diff = [labels[w] for w in range(1, nv) if not (np.array_equal(st[p], st[16 * w + p]) and np.array_equal(row[p], row[16 * w + p]))]
                assert not diff, "probe %s at position %d, variant %s: state record or output row differs from the wave with free mates beside the mates %r" % (probe, p, variant, diff)
    finally:
        eng.close()


def quad_rc_variants(variant):
    v = [[], ["ro2"]] + [[nm] for nm in MATE_POOLS] + [["ro1+rt1"], ["ro2", "ro1+rt1"] + MATE_POOLS]
    return v + ([["fast"]] if variant == "U" else [])


RC_PROBE, RC_MATES = 5, (0, 3, 8, 9, 12, 14, 15)


def quad_rc_batch(variant, mates):
    """16 envs: env 5 is the probe (an `ro1` state), the mates -- further envs with robot-object contact, i.e. of kw_quad_rc's one wave --
    at other positions, everything else free (simple envs: kw_quad's)"""
    R = rows()
    free = R.by["free"]
    wave = [free[i % len(free)] for i in range(16)]
    wave[RC_PROBE] = R.by["ro1"][0]
    for pos, nm in zip(RC_MATES, mates):
        wave[pos] = _fast(R.by["ro1"][1]) if nm == "fast" else R.by[nm][0 if nm != "ro1+rt1" else 1]
    return np.array([c[0] for c in wave]), np.array([c[1] for c in wave])


def check_quad_rc_wave_mates(Engine, lib, variant, lane=1, device=True):
    """kw_quad_rc: at most 16 complex envs share wave 0; the `ro1` probe is bit-identical whoever shares it"""
    lab = lab_of(variant)
    eng = lab.engine(Engine, lib, 16)
    ref = None
    try:
        for mates in quad_rc_variants(variant):
            S, A = quad_rc_batch(variant, mates)
            eng.set_state(S)
            info = eng.kernel_info()
            assert info[2] == lane and (not (lane and device) or info[5] == 1 + len(mates)), (info, mates)
            st, row = step_bits(eng, S, A)
            if ref is None:
                ref = (st, row)
                assert not np.array_equal(st[RC_PROBE, :ND], S[RC_PROBE, :ND].view(np.uint32))
                continue
            ctx = "the ro1 probe, variant %s, beside %r against alone" % (variant, mates)
            assert np.array_equal(ref[0][RC_PROBE], st[RC_PROBE]), "state record differs with the wave-mates: " + ctx
            assert np.array_equal(ref[1][RC_PROBE], row[RC_PROBE]), "output row differs with the wave-mates: " + ctx
    finally:
        eng.close()


def check_quad_rc_epw(Engine, lib, variant, setenv, delenv):
    """the whole `ro` batch with every env alone in its wave (PBRE_QUAD_RC_EPW=1) against the default of 16 per wave: records and rows bit for
    bit ("What an env computes does not depend on epw", pbre_lane.hip)"""
    lab = lab_of(variant)
    S, A, names = rows().batch(RO_POOLS + MATE_POOLS)
    bits = []
    for epw in (None, "1"):
        if epw is None:
            delenv("PBRE_QUAD_RC_EPW", raising=False)
        else:
            setenv("PBRE_QUAD_RC_EPW", epw)
        eng = lab.engine(Engine, lib, len(S))
        try:
            eng.set_state(S)
            info = eng.kernel_info()
            assert info[2] == 1 and info[5] == len(S), info
            bits.append(step_bits(eng, S, A))
        finally:
            eng.close()
    delenv("PBRE_QUAD_RC_EPW", raising=False)
    for e in range(len(S)):
        assert np.array_equal(bits[0][0][e], bits[1][0][e]) and np.array_equal(bits[0][1][e], bits[1][1][e]), "env %d (%s) depends on the envs per wave" % (e, names[e])
    assert not np.array_equal(bits[0][0][:, :ND], S[:, :ND].view(np.uint32))


GROUP_PROBES = ["free", "lim:8:0", "lim:12:1", "rt1", "ro1"]
GROUP_MATES = ["free", "lim:8:0", "lim:12:0", "lim:3:0", "rt2", "ro2"]


def check_group_wave_mates(Engine, lib, variant):
    """kw_step (PBRE_ICUB_LANE=0): env = block * 8 + thread / 32, so envs 2 k and 2 k + 1 share a wave.  Pair w of the batch is the probe
    beside mate w, the probe in the lower and in the upper half-wave."""
    lab, R = lab_of(variant), rows()
    nv = len(GROUP_MATES)
    eng = lab.engine(Engine, lib, 2 * nv)
    try:
        for probe in GROUP_PROBES:
            for p in (0, 1):
                pc = R.by[probe][-1]
                pairs = []
                for nm in GROUP_MATES:
                    pair = [None, None]
                    pair[p], pair[1 - p] = pc, R.by[nm][0]
                    pairs += pair
                S, A = np.array([c[0] for c in pairs]), np.array([c[1] for c in pairs])
                eng.set_state(S)
                assert eng.kernel_info()[2] == 0
                st, row = step_bits(eng, S, A)
                assert not np.array_equal(st[p, :ND], S[p, :ND].view(np.uint32))
                for w in range(1, nv):
                    _same_probe(st, row, p, 2 * w + p, "probe %s in half-wave %d, variant %s, beside %s against beside free" % (probe, p, variant, GROUP_MATES[w]))
    finally:
        eng.close()
